"""GPU tier of Flow.matrix / get_flow_matrix (ofl_matrix.hip): the reference's own recovery, noise and mask cases
(test/test_flow_class.py:1903-2006, its tolerances), the kernels against the oracle (tests/matrix_oracle.py: n_valid, the
winner and the inlier count EQUAL, the matrices within the bar derived from the measured float64 summation-order deviation),
batch independence and run-to-run identity bit for bit, the from_matrix round trip at 1080p."""
import numpy as np
import pytest
import torch

import matrix_oracle as mo

pytestmark = pytest.mark.gpu

PAIRS = [(4, 'ransac'), (4, 'lmeds'), (6, 'ransac'), (6, 'lmeds'), (8, 'lms'), (8, 'ransac'), (8, 'lmeds')]
TRANSFORMS = [['translation', 2, 1], ['rotation', 20, 20, 30], ['scaling', 10, 10, 1.1]]
# Largest deviation of a kernel matrix from the oracle's (math.fsum sums), relative to the matrix' largest entry, measured on the
# MI355X over the 73 cases of the test_against_oracle_* tests below: 1.47e-14.  The bar is 16 x that figure: the
# summation order changes with the grid, other shapes need room.
MEASURED_DEVIATION = 1.47e-14
ORACLE_BAR = 16 * MEASURED_DEVIATION


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


def _true_matrix():
    from oflibpytorch_amd.utils import matrix_from_transforms
    return matrix_from_transforms(TRANSFORMS)


def _tol(ref, dof):
    if dof == 8:
        return dict(rtol=1e-6, atol=1e-4)
    return dict(rtol=1e-6) if ref == 's' else dict(rtol=1e-3)


# ---- the reference's test_matrix on the device ----------------------------------------------------------------------------
@pytest.mark.parametrize("ref", ['s', 't'])
@pytest.mark.parametrize("dof,method", PAIRS)
def test_recovers_known_matrix(dof, method, ref, dev):
    import oflibpytorch_amd as ofl
    matrix = _true_matrix()
    flow = ofl.Flow.from_matrix(matrix.unsqueeze(0), (100, 200), ref, device=dev)
    got = flow.matrix(dof=dof, method=method)
    assert got.dtype == torch.float64 and got.shape == (1, 3, 3) and got.device.type == 'cuda'
    err = np.abs(got.cpu().numpy()[0] - matrix.numpy().astype(np.float64))
    print("recover", dof, method, ref, "max abs err %.3e" % err.max())
    np.testing.assert_allclose(got.cpu().numpy()[0], matrix.numpy(), **_tol(ref, dof))


def test_recovers_batched_matrices(dev):
    import oflibpytorch_amd as ofl
    from oflibpytorch_amd.utils import matrix_from_transforms
    m1, m2 = matrix_from_transforms(TRANSFORMS[:2]), matrix_from_transforms(TRANSFORMS[1:])
    flow = ofl.batch_flows((ofl.Flow.from_matrix(m1, (100, 200), 's', device=dev),
                            ofl.Flow.from_matrix(m2, (100, 200), 's', device=dev)))
    got = flow.matrix(dof=4, method='ransac').cpu().numpy()
    np.testing.assert_allclose(got[0], m1.numpy(), rtol=1e-6)
    np.testing.assert_allclose(got[1], m2.numpy(), rtol=1e-6)


@pytest.mark.parametrize("dof,method", PAIRS)
def test_noise_case(dof, method, dev):
    import oflibpytorch_amd as ofl
    matrix = _true_matrix()
    noise = ((np.random.RandomState(7).rand(100, 200, 2) - .5) * 5).astype(np.float32)
    flow = ofl.Flow.from_matrix(matrix, (100, 200), 's', device=dev) + noise
    got = flow.matrix(dof, method)[0].cpu().numpy()
    print("noise", dof, method, "max abs err [:2,:2] %.3e" % np.abs(got[:2, :2] - matrix.numpy()[:2, :2]).max())
    np.testing.assert_allclose(got[:2, :2], matrix.numpy()[:2, :2], atol=1e-2, rtol=1e-1)


def test_mask_case(dev):
    """The true flow in [:50, :50], uniform +-100 px elsewhere, the mask True on the corner only.  The reference compares at
    assert_allclose's default 1e-7 on OpenCV's output; a float64 fit of an fp32 flow reaches about 1.4e-7 on 100 x 200, so the
    bar is the 1e-6 of the unmasked case."""
    import oflibpytorch_amd as ofl
    matrix = _true_matrix()
    mask = np.zeros((100, 200), 'bool')
    mask[:50, :50] = 1
    true_vecs = ofl.Flow.from_matrix(matrix, (100, 200), 's', device=dev).vecs.cpu().numpy()
    vecs = ((np.random.RandomState(11).rand(1, 2, 100, 200) - 0.5) * 200).astype(np.float32)
    vecs[:, :, :50, :50] = true_vecs[:, :, :50, :50]
    flow = ofl.Flow(torch.tensor(vecs, device=dev), 's', torch.tensor(mask, device=dev))
    with pytest.raises(AssertionError):
        np.testing.assert_allclose(flow.matrix(4, 'lmeds', False)[0].cpu().numpy(), matrix.numpy(), rtol=1e-3)
    np.testing.assert_allclose(flow.matrix(4, 'lmeds', True)[0].cpu().numpy(), matrix.numpy(), rtol=1e-6)


def test_lms_falls_back_to_ransac_and_too_few_points(dev):
    import oflibpytorch_amd as ofl
    flow = ofl.Flow.from_matrix(_true_matrix(), (100, 200), 's', device=dev)
    with pytest.warns(UserWarning, match="defaulting to 'ransac'"):
        a = flow.matrix(dof=4, method='lms')
    assert torch.equal(a, flow.matrix(dof=4, method='ransac'))
    m = torch.zeros(2, 6, 7, dtype=torch.bool, device=dev)
    m[0] = True                                                   # image 0 is all valid, image 1 has no valid pixel
    few = ofl.Flow(torch.zeros(2, 2, 6, 7, device=dev), 't', m)
    for dof, method in PAIRS:                                     # rejected by status codes: no kernel runs on nothing
        with pytest.raises(ValueError, match="batch element 1"):
            few.matrix(dof, method)
    assert few.matrix(8, 'lms', masked=False).shape == (2, 3, 3)


# ---- against the oracle ---------------------------------------------------------------------------------------------------
def _inputs(kind, n, h, w, ref, dev, seed):
    """exact flows of n different matrices; 'outliers': 30 % of the pixels replaced by uniform +-100 px vectors; 'noise': +-2.5 px"""
    import oflibpytorch_amd as ofl
    from oflibpytorch_amd.utils import matrix_from_transforms
    rs = np.random.RandomState(seed)
    mats = torch.stack([matrix_from_transforms([['translation', 2 + i, 1 - i], ['rotation', w / 5, h / 5, 30 - 7 * i],
                                                ['scaling', w / 20, h / 10, 1.1 - 0.05 * i]]) for i in range(n)])
    vecs = ofl.Flow.from_matrix(mats, (h, w), ref, device=dev).vecs.cpu().numpy().astype(np.float32)
    if kind == 'outliers':
        bad = rs.rand(n, 1, h, w) < 0.3
        vecs = np.where(bad, ((rs.rand(n, 2, h, w) - 0.5) * 200).astype(np.float32), vecs)
    elif kind == 'noise':
        vecs = vecs + ((rs.rand(n, 2, h, w) - 0.5) * 5).astype(np.float32)
    return np.ascontiguousarray(vecs, np.float32)


def _compare(vecs, ref, mask, dof, method, dev, half=False):
    from oflibpytorch_amd import _native
    import oflibpytorch_amd as ofl
    t = torch.tensor(vecs, device=dev)
    if half:
        t = t.half()
        vecs = t.cpu().numpy()                                   # (the oracle reads the same fp16 values)
    tm = None if mask is None else torch.tensor(mask, device=dev)
    fl = ofl.Flow(t, ref, tm)
    if half:
        assert fl._half is not None
    got, info = _native.matrix_fit(fl._fv, ref, tm, dof, method)
    got, info = got.cpu().numpy(), info.cpu().numpy()
    exp, einfo = mo.fit(vecs, ref, mask, dof, method)
    dev_rel = max(float(np.abs(got[i] - exp[i]).max() / np.abs(exp[i]).max()) for i in range(len(exp)))
    print("oracle", vecs.shape, ref, dof, method, "masked" if mask is not None else "-", "fp16" if half else "-",
          "info", info.tolist(), "deviation %.3e" % dev_rel)
    assert np.array_equal(info, einfo), (info.tolist(), einfo.tolist())
    assert np.all(einfo[:, 3] == 0)
    assert dev_rel <= ORACLE_BAR, dev_rel
    return dev_rel


@pytest.mark.parametrize("kind", ['exact', 'outliers', 'noise'])
@pytest.mark.parametrize("h,w", [(100, 200), (93, 131)])
def test_against_oracle_small(h, w, kind, dev):
    for i, (dof, method) in enumerate(PAIRS):
        ref = 's' if (i + h) % 2 == 0 else 't'
        _compare(_inputs(kind, 2, h, w, ref, dev, 3 + i), ref, None, dof, method, dev)


@pytest.mark.parametrize("h,w", [(100, 200), (93, 131)])
def test_against_oracle_masked_and_fp16(h, w, dev):
    rs = np.random.RandomState(h)
    mask = rs.rand(2, h, w) > 0.35
    mask[:, h // 4: h // 2, w // 3: w // 2] = False
    mask[1, 5] = False                                            # an empty row
    for i, (dof, method) in enumerate(PAIRS):
        ref = 't' if i % 2 == 0 else 's'
        _compare(_inputs('outliers', 2, h, w, ref, dev, 20 + i), ref, mask, dof, method, dev)
        _compare(_inputs('noise', 2, h, w, ref, dev, 40 + i), ref, mask if i % 3 == 0 else None, dof, method, dev, half=True)


@pytest.mark.parametrize("kind,ref,dof,method", [('outliers', 's', 4, 'ransac'), ('noise', 't', 8, 'lmeds'), ('exact', 's', 8, 'lms')])
def test_against_oracle_1080p(kind, ref, dof, method, dev):
    _compare(_inputs(kind, 2, 1080, 1920, ref, dev, 60), ref, None, dof, method, dev)


# ---- batch independence, reproducibility -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dof,method", PAIRS)
def test_batch_independent_and_reproducible(dof, method, dev):
    import oflibpytorch_amd as ofl
    h, w = 181, 333
    vecs = _inputs('outliers', 5, h, w, 's', dev, 77)
    mask = np.random.RandomState(5).rand(5, h, w) > 0.2
    tv, tm = torch.tensor(vecs, device=dev), torch.tensor(mask, device=dev)
    fl = ofl.Flow(tv, 's', tm)
    a, b = fl.matrix(dof, method), fl.matrix(dof, method)
    assert torch.equal(a, b)
    for i in range(5):
        alone = ofl.Flow(tv[i:i + 1].clone(), 's', tm[i:i + 1].clone()).matrix(dof, method)     # image i alone
        assert alone.shape == (1, 3, 3)
        assert torch.equal(alone[0], a[i]), (i, (alone[0] - a[i]).abs().max().item())
    assert not torch.equal(a[0], a[1])                            # (different matrices per image did come back)


# ---- from_matrix round trip at 1080p ---------------------------------------------------------------------------------------
def test_from_matrix_round_trip_1080p(dev):
    """A similarity, a sheared affine map, a mild homography and the identity, one per image, through the project's own
    generator.  Each is checked with the reference's tolerances for every model family that holds it.  The identity gives
    a zero flow: src == dst exactly, so dof 4 / 6 return eye(3)'s last row exactly, and 'lms' dof 8 the identity within 1e-4."""
    import oflibpytorch_amd as ofl
    from oflibpytorch_amd.utils import matrix_from_transforms
    sim = matrix_from_transforms([['translation', -12, 7], ['rotation', 960, 540, -8], ['scaling', 900, 500, 0.93]])
    aff = sim.clone()
    aff[0, 1] += 0.04                                            # a shear
    hom = aff.clone()
    hom[2, 0], hom[2, 1] = 2e-5, -1e-5
    mats = torch.stack([sim, aff, hom, torch.eye(3)])
    for ref in ('s', 't'):
        flow = ofl.Flow.from_matrix(mats, (1080, 1920), ref, device=dev)
        for dof, method in PAIRS:
            got = flow.matrix(dof, method).cpu().numpy()
            holds = [True, dof >= 6, dof == 8]
            for i in range(3):
                if holds[i]:
                    err = np.abs(got[i] - mats[i].numpy().astype(np.float64))
                    print("round trip", ref, dof, method, i, "max abs err %.3e" % err.max())
                    np.testing.assert_allclose(got[i], mats[i].numpy(), **_tol(ref, dof))
            if dof == 8:
                if method == 'lms':
                    np.testing.assert_allclose(got[3], np.eye(3), atol=1e-4, rtol=0)
            else:
                assert np.array_equal(got[3][2], np.eye(3)[2])


def test_get_flow_matrix_on_device(dev):
    import oflibpytorch_amd as ofl
    matrix = _true_matrix()
    flow = ofl.Flow.from_matrix(matrix, (100, 200), 's', device=dev)
    m3 = ofl.get_flow_matrix(flow.vecs[0], 's', dof=6, method='lmeds')
    assert m3.shape == (3, 3) and m3.dtype == torch.float64 and m3.device.type == 'cuda'
    m4 = ofl.get_flow_matrix(flow.vecs.cpu().numpy(), 's', dof=6, method='lmeds')
    assert m4.shape == (1, 3, 3)
    np.testing.assert_allclose(m3.cpu().numpy(), matrix.numpy(), rtol=1e-6)
    assert np.array_equal(m4[0].cpu().numpy(), m3.cpu().numpy())
