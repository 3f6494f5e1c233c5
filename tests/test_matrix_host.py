"""CPU tier of Flow.matrix / get_flow_matrix: the oracle (tests/matrix_oracle.py) on the cases and with the
tolerances of the reference's own test (test/test_flow_class.py:1903-2006), the host logic of the API with the native call
served by the oracle, and the C ABI's argument checks."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import matrix_oracle as mo

PAIRS = [(4, 'ransac'), (4, 'lmeds'), (6, 'ransac'), (6, 'lmeds'), (8, 'lms'), (8, 'ransac'), (8, 'lmeds')]
TRANSFORMS = [['translation', 2, 1], ['rotation', 20, 20, 30], ['scaling', 10, 10, 1.1]]


def _fake_matrix_fit(vecs, ref, mask, dof, method):
    v = vecs.detach().cpu().numpy()
    m = None if mask is None else mask.detach().cpu().numpy()
    if m is not None and m.shape[0] != v.shape[0]:
        m = np.broadcast_to(m, (v.shape[0],) + m.shape[1:])
    mats, info = mo.fit(v if v.dtype == np.float16 else v.astype(np.float32), ref, m, dof, method)
    return torch.from_numpy(mats), torch.from_numpy(info)


@pytest.fixture
def matrix_native(oracle_native, monkeypatch):
    from oflibpytorch_amd import _native
    monkeypatch.setattr(_native, "matrix_fit", _fake_matrix_fit)
    return _native


def _true_matrix():
    from oflibpytorch_amd.utils import matrix_from_transforms
    return matrix_from_transforms(TRANSFORMS)


def _tol(ref, dof):
    if dof == 8:
        return dict(rtol=1e-6, atol=1e-4)
    return dict(rtol=1e-6) if ref == 's' else dict(rtol=1e-3)


# ---- the oracle on the reference's cases (input flows from oracle_backend.flow_from_matrix, through Flow.from_matrix) ----------
@pytest.mark.parametrize("ref", ['s', 't'])
@pytest.mark.parametrize("dof,method", PAIRS)
def test_oracle_recovers_known_matrix(dof, method, ref, matrix_native):
    import oflibpytorch_amd as ofl
    matrix = _true_matrix()
    flow = ofl.Flow.from_matrix(matrix.unsqueeze(0), (100, 200), ref)
    got, info = mo.fit(flow.vecs.numpy(), ref, None, dof, method)
    assert info[0, 3] == 0 and info[0, 0] == 20000
    np.testing.assert_allclose(got[0], matrix.numpy(), **_tol(ref, dof))


def test_oracle_recovers_batched_matrices(matrix_native):
    import oflibpytorch_amd as ofl
    from oflibpytorch_amd.utils import matrix_from_transforms
    m1, m2 = matrix_from_transforms(TRANSFORMS[:2]), matrix_from_transforms(TRANSFORMS[1:])
    flow = ofl.batch_flows((ofl.Flow.from_matrix(m1, (100, 200), 's'), ofl.Flow.from_matrix(m2, (100, 200), 's')))
    got = flow.matrix(dof=4, method='ransac').numpy()
    np.testing.assert_allclose(got[0], m1.numpy(), rtol=1e-6)
    np.testing.assert_allclose(got[1], m2.numpy(), rtol=1e-6)


@pytest.mark.parametrize("dof,method", PAIRS)
def test_oracle_noise_case(dof, method, matrix_native):
    import oflibpytorch_amd as ofl
    matrix = _true_matrix()
    noise = ((np.random.RandomState(7).rand(100, 200, 2) - .5) * 5).astype(np.float32)
    flow = ofl.Flow.from_matrix(matrix, (100, 200), 's') + noise
    got = flow.matrix(dof, method)[0].numpy()
    np.testing.assert_allclose(got[:2, :2], matrix.numpy()[:2, :2], atol=1e-2, rtol=1e-1)


def test_oracle_mask_case(matrix_native):
    """As the reference's: the true flow in [:50, :50], +-100 px elsewhere, the mask True on the corner only.  The reference
    compares at 1e-7 on OpenCV's output; a float64 fit of an fp32 flow reaches about 1.4e-7, so the bar is the 1e-6 of the
    unmasked case.  Unmasked, 'lmeds' must miss (87.5 % outliers): the reference asserts that it fails."""
    import oflibpytorch_amd as ofl
    matrix = _true_matrix()
    mask = np.zeros((100, 200), 'bool')
    mask[:50, :50] = 1
    true_vecs = ofl.Flow.from_matrix(matrix, (100, 200), 's').vecs.numpy()
    vecs = ((np.random.RandomState(11).rand(1, 2, 100, 200) - 0.5) * 200).astype(np.float32)
    vecs[:, :, :50, :50] = true_vecs[:, :, :50, :50]
    flow = ofl.Flow(vecs, 's', mask)
    with pytest.raises(AssertionError):
        np.testing.assert_allclose(flow.matrix(4, 'lmeds', False)[0].numpy(), matrix.numpy(), rtol=1e-3)
    np.testing.assert_allclose(flow.matrix(4, 'lmeds', True)[0].numpy(), matrix.numpy(), rtol=1e-6)


def test_oracle_pieces():
    """The draw hash is splitmix64; the elimination solves what numpy solves; a repeated or collinear sample is invalid."""
    assert mo.draw_hash(0, 0) == mo.draw_hash(0, 0) and mo.draw_hash(0, 0) != mo.draw_hash(0, 1) != mo.draw_hash(1, 0)
    assert all(0 <= mo.draw_hash(k, j) < 2 ** 64 for k in range(4) for j in range(4))
    rs = np.random.RandomState(3)
    a, b = rs.randn(8, 8), rs.randn(8, 2)
    x = np.array(mo.gauss_solve(a.tolist(), b.tolist()))
    np.testing.assert_allclose(x, np.linalg.solve(a, b), rtol=1e-9)
    assert mo.gauss_solve([[1.0, 2.0], [2.0, 4.0]], [[1.0], [2.0]]) is None
    pts = np.array([[0.0, 0.0], [1.0, 1.0], [2.0, 2.0], [5.0, 1.0]])
    assert mo._collinear(pts[0], pts[1], pts[2]) and not mo._collinear(pts[0], pts[1], pts[3])
    r = np.array([3.0, 1.0, 2.0, 8.0], np.float32)
    assert mo.median_f32(r) == np.float32(2.5) and mo.median_f32(r[:3]) == np.float32(2.0)


# ---- host logic: the API with the native call served by the oracle -------------------------------------------------------
def test_host_argument_checks_in_reference_order(matrix_native):
    import oflibpytorch_amd as ofl
    flow = ofl.Flow.zero([10, 10])
    with pytest.raises(ValueError, match="Dof needs to be 4, 6 or 8"):
        flow.matrix(dof='test')
    with pytest.raises(ValueError, match="Dof needs to be 4, 6 or 8"):
        flow.matrix(dof=5)
    with pytest.raises(ValueError, match="Method needs to be 'lms', 'ransac', or 'lmeds'"):
        flow.matrix(dof=4, method='test')
    with pytest.raises(TypeError, match="Masked needs to be boolean"):
        flow.matrix(dof=4, method='lms', masked='test')
    # order: dof, then method, then masked
    with pytest.raises(ValueError, match="Dof needs"):
        flow.matrix(dof=5, method='test', masked='test')
    with pytest.raises(ValueError, match="Method needs"):
        flow.matrix(dof=4, method='test', masked='test')


def test_host_lms_warning_and_fallback(matrix_native):
    import oflibpytorch_amd as ofl
    flow = ofl.Flow.from_matrix(_true_matrix(), (40, 60), 's')
    for dof in (4, 6):
        with pytest.warns(UserWarning, match="Method 'lms' .* defaulting to 'ransac'"):
            a = flow.matrix(dof=dof, method='lms')
        assert torch.equal(a, flow.matrix(dof=dof, method='ransac'))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        flow.matrix(dof=8, method='lms')
        flow.matrix()                                            # defaults: 8, 'ransac', True


def test_host_too_few_points_raise_value_error(matrix_native):
    import oflibpytorch_amd as ofl
    m = torch.zeros(2, 6, 7, dtype=torch.bool)
    m[0] = True
    few = ofl.Flow(torch.zeros(2, 2, 6, 7), 't', m)
    for dof, method in PAIRS:
        with pytest.raises(ValueError, match="batch element 1"):
            few.matrix(dof, method)
    assert few.matrix(8, 'lms', masked=False).shape == (2, 3, 3)
    m[1, 0, :3] = True                                            # three pixels: enough for dof 4 and 6 counts, collinear
    few = ofl.Flow(torch.zeros(2, 2, 6, 7), 't', m)
    assert few.matrix(4, 'ransac').shape == (2, 3, 3)
    for dof in (6, 8):
        with pytest.raises(ValueError, match="batch element 1"):
            few.matrix(dof, 'ransac')


def test_host_return_types_and_squeeze(matrix_native):
    import oflibpytorch_amd as ofl
    matrix = _true_matrix()
    fl = ofl.Flow.from_matrix(matrix, (30, 40), 's')
    got = fl.matrix(6, 'lmeds')
    assert isinstance(got, torch.Tensor) and got.dtype == torch.float64 and got.shape == (1, 3, 3)
    assert got.device == fl.vecs.device and not got.requires_grad
    v = fl.vecs                                                   # 1-2-H-W
    assert torch.equal(ofl.get_flow_matrix(v, 's', 6, 'lmeds'), got)
    assert torch.equal(ofl.get_flow_matrix(v[0], 's', 6, 'lmeds'), got[0])                        # 3-D in -> 3 x 3 out
    assert torch.equal(ofl.get_flow_matrix(v[0].numpy(), 's', 6, 'lmeds'), got[0])
    assert torch.equal(ofl.get_flow_matrix(v.permute(0, 2, 3, 1).contiguous(), 's', 6, 'lmeds'), got)     # channels last
    assert torch.equal(ofl.get_flow_matrix(np.moveaxis(v[0].numpy(), 0, -1), 's', 6, 'lmeds'), got[0])
    assert ofl.get_flow_matrix(v[0], 's').shape == (3, 3)                                         # defaults 8 / 'ransac'
    assert torch.equal(ofl.get_flow_matrix(v, 's'), fl.matrix())


# ---- C ABI -------------------------------------------------------------------------------------------------------------
def test_cabi_matrix_rejects_bad_arguments():
    from oflibpytorch_amd import _native
    lib = _native.load_library()
    assert lib.ofl_version() == 36 == _native.ABI_VERSION
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(16)    # (never dereferenced: rejected before any launch)
    wb = lib.ofl_matrix_workspace_bytes
    assert wb(0, 4, 4, 8, 1) == -2 and wb(1, 0, 4, 8, 1) == -2 and wb(70000, 4, 4, 8, 1) == -2
    assert wb(1, 4, 4, 5, 1) == -3 and wb(1, 4, 4, 8, 3) == -3 and wb(1, 4, 4, 8, -1) == -3
    assert wb(1, 4, 4, 8, 0) > 0 and wb(1, 4, 4, 8, 0) % 8 == 0
    assert wb(2, 1080, 1920, 8, 2) > wb(2, 1080, 1920, 8, 1) > wb(2, 1080, 1920, 8, 0)
    fit = lib.ofl_matrix_fit_f64
    assert fit(null, 0, 0, 0, null, 0, 1, 4, 4, 8, 1, one, one, one, null) == -1
    assert fit(one, 0, 0, 0, null, 0, 1, 4, 4, 8, 1, null, one, one, null) == -1
    assert fit(one, 0, 0, 0, null, 0, 1, 4, 4, 8, 1, one, null, one, null) == -1
    assert fit(one, 0, 0, 0, null, 0, 1, 4, 4, 8, 1, one, one, null, null) == -1
    assert fit(one, 0, 0, 0, null, 0, 0, 4, 4, 8, 1, one, one, one, null) == -2
    assert fit(one, 0, 0, 0, null, 0, 1, 4, -1, 8, 1, one, one, one, null) == -2
    assert fit(one, 0, 0, 0, null, 0, 1, 4, 4, 7, 1, one, one, one, null) == -3
    assert fit(one, 0, 0, 0, null, 0, 1, 4, 4, 8, 3, one, one, one, null) == -3
    assert fit(one, 0, 2, 0, null, 0, 1, 4, 4, 8, 1, one, one, one, null) == -3
    assert fit(one, 0, 0, 2, null, 0, 1, 4, 4, 8, 1, one, one, one, null) == -3
    assert fit(one, -8, 0, 0, null, 0, 1, 4, 4, 8, 1, one, one, one, null) == -3
    assert fit(one, 0, 0, 0, null, -1, 1, 4, 4, 8, 1, one, one, one, null) == -3
    assert fit(one, 0, 0, 0, null, 0, 1, 4, 4, 8, 1, ctypes.c_void_p(12), one, one, null) == -3      # workspace not 8-byte aligned
