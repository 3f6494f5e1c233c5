"""CPU tier of Flow.error_stats / epe_map / epe: the oracle (tests/flow_error_oracle.py) on hand-computed cases, the
host logic of the API with the two native calls served by the oracle, and the C ABI's declarations and argument checks."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import flow_error_oracle as feo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# 2 x 3 pixels, row-major.  Ground truth speeds g = 0, 10, 40 / 5, 50, 100 (the vectors (6, 8) and (24, 32) sit exactly on the bin edges);
# errors e = 1, 3, 5 / 0, 10, 5 (exactly on the thresholds 1, 3, 5: NOT over under the strict >).
GT = np.array([[[0, 6, 24], [3, 30, 60]], [[0, 8, 32], [4, 40, 80]]], np.float32)[None]
D = np.array([[[1, 0, 3], [0, 6, 3]], [[0, 3, 4], [0, 8, 4]]], np.float32)[None]
EST = GT + D


@pytest.fixture
def error_native(oracle_native, monkeypatch):
    from oflibpytorch_amd import _native
    monkeypatch.setattr(_native, "flow_error", feo.fake_flow_error)
    monkeypatch.setattr(_native, "flow_epe_grad", feo.fake_flow_epe_grad)
    return _native


# ---- the oracle on hand-computed cases ---------------------------------------------------------------------------------------
def test_oracle_hand_case_all_valid():
    r = feo.score(EST, GT)
    assert r['map'].dtype == np.float32 and r['map'].tolist() == [[[1, 3, 5], [0, 10, 5]]]
    assert r['count'].tolist() == [6] and r['sum'].tolist() == [24.0] and r['max'].tolist() == [10.0]
    # e exactly 1, 3 and 5 are not over 1, 3 and 5
    assert r['n_over'].tolist() == [[4, 3, 1]]
    # Fl: e = 5 at g = 40 (5 > 2) and e = 10 at g = 50 (10 > 2.5) are outliers; e = 5 at g = 100 is not (5 > 5 fails), e = 3 is not
    assert r['n_fl'].tolist() == [2]
    # g exactly 10 belongs to [10, 40), g exactly 40 to [40, inf); g = 0 to [0, 10)
    assert r['speed_count'].tolist() == [[2, 1, 3]] and r['speed_sum'].tolist() == [[1.0, 3.0, 20.0]]
    assert r['records'].tolist() == [[6, 24, 10, 4, 3, 1, 0, 2, 2, 1, 3, 1, 3, 20, 0, 0]]


def test_oracle_hand_case_masks_and_zero_speed():
    em = np.array([[[1, 1, 1], [1, 0, 1]]], bool)
    gm = np.array([[[0, 1, 1], [1, 1, 1]]], bool)
    r = feo.score(EST, GT, em, gm)
    assert r['map'].tolist() == [[[0, 3, 5], [0, 0, 5]]]
    assert r['count'].tolist() == [4] and r['sum'].tolist() == [13.0] and r['max'].tolist() == [5.0]
    assert r['n_over'].tolist() == [[3, 2, 0]] and r['n_fl'].tolist() == [1]
    assert r['speed_count'].tolist() == [[1, 1, 2]] and r['speed_sum'].tolist() == [[0.0, 3.0, 10.0]]
    # g = 0 everywhere: the product form needs no division -- an outlier is simply e > 3
    z = np.zeros_like(GT)
    r = feo.score(D, z, thresholds=(3,))
    assert r['n_fl'].tolist() == [3] and r['n_over'].tolist() == [[3]] and r['speed_count'].tolist() == [[6, 0, 0]]
    # no valid pixel at all
    r = feo.score(EST, GT, np.zeros((1, 2, 3), bool), None)
    assert r['count'].tolist() == [0] and r['sum'].tolist() == [0.0] and r['max'].tolist() == [0.0] and not r['records'].any()


def test_oracle_steps_are_float32_and_sums_exact():
    est = np.array([0.1, 0.2], np.float32).reshape(1, 2, 1, 1)
    gt = np.zeros((1, 2, 1, 1), np.float32)
    a, b = np.float32(0.1), np.float32(0.2)
    want = np.sqrt(np.float32(a * a) + np.float32(b * b))
    assert feo.score(est, gt)['map'][0, 0, 0] == want and want.dtype == np.float32
    # fsum: 2^30 + 4096 x 2^-24 is exact in float64, a float32 running sum would lose every small term
    e = np.full((1, 1, 4097), 2.0 ** -24, np.float32)
    e[0, 0, 0] = 2.0 ** 30
    est = np.stack([e, np.zeros_like(e)], axis=1)
    assert feo.score(est, np.zeros_like(est))['sum'][0] == 2.0 ** 30 + 4096 * 2.0 ** -24
    # fp16 storage is up-converted exactly
    h = np.array([1.5, -2.25], np.float16).reshape(1, 2, 1, 1)
    assert feo.score(h, gt)['map'][0, 0, 0] == feo.score(h.astype(np.float32), gt)['map'][0, 0, 0]


def test_oracle_gradient_hand_case():
    g = feo.epe_grad(EST, GT, None, np.array([[[1, 1, 0], [1, 1, 1]]], bool), np.array([0.5], np.float32))
    assert g.dtype == np.float64 and g.shape == (1, 2, 2, 3)
    assert g[0, :, 0, 0].tolist() == [0.5, 0.0] and g[0, :, 0, 1].tolist() == [0.0, 0.5]
    assert g[0, :, 0, 2].tolist() == [0.0, 0.0]                       # not valid
    assert g[0, :, 1, 0].tolist() == [0.0, 0.0]                       # e = 0: the subgradient 0
    np.testing.assert_allclose(g[0, :, 1, 1], [0.3, 0.4], rtol=1e-15)


# ---- host logic: the API with the native calls served by the oracle -----------------------------------------------------------
def _flows(n=2, h=6, w=7, seed=0, masks=True):
    import oflibpytorch_amd as ofl
    rs = np.random.RandomState(seed)
    gt = (rs.randn(n, 2, h, w) * 20).astype(np.float32)
    est = gt + (rs.randn(n, 2, h, w) * 2.5).astype(np.float32)
    em = torch.from_numpy(rs.rand(n, h, w) > 0.2) if masks else None
    gm = torch.from_numpy(rs.rand(n, h, w) > 0.2) if masks else None
    return ofl.Flow(torch.from_numpy(est), 't', em), ofl.Flow(torch.from_numpy(gt), 't', gm)


def test_error_stats_keys_dtypes_shapes(error_native):
    est, gt = _flows()
    s = est.error_stats(gt)
    assert sorted(s) == ['count', 'epe', 'fl', 'max', 'outliers', 'speed_count', 'speed_epe']
    assert s['count'].dtype == torch.int64 and s['count'].shape == (2,)
    assert s['speed_count'].dtype == torch.int64 and s['speed_count'].shape == (2, 3)
    for k, shape in (('epe', (2,)), ('max', (2,)), ('fl', (2,)), ('outliers', (2, 3)), ('speed_epe', (2, 3))):
        assert s[k].dtype == torch.float64 and s[k].shape == shape, k
    ref = feo.score(est.vecs.numpy(), gt.vecs.numpy(), est.mask.numpy(), gt.mask.numpy())
    assert s['count'].tolist() == ref['count'].tolist() and s['speed_count'].tolist() == ref['speed_count'].tolist()
    assert s['epe'].tolist() == (ref['sum'] / ref['count']).tolist() and s['max'].tolist() == ref['max'].tolist()
    assert s['outliers'].tolist() == (ref['n_over'] / ref['count'][:, None]).tolist()
    assert s['fl'].tolist() == (ref['n_fl'] / ref['count']).tolist()
    assert est.error_stats(gt, thresholds=[2.5])['outliers'].shape == (2, 1)
    assert est.error_stats(gt, thresholds=(0, 1, 2, 3))['outliers'].shape == (2, 4)
    assert all(not v.requires_grad for v in s.values())


def test_hand_case_through_the_api(error_native):
    import oflibpytorch_amd as ofl
    s = ofl.Flow(EST, 's').error_stats(ofl.Flow(GT, 's'))
    assert s['count'].tolist() == [6] and s['epe'].tolist() == [4.0] and s['max'].tolist() == [10.0]
    assert s['outliers'].tolist() == [[4 / 6, 3 / 6, 1 / 6]] and s['fl'].tolist() == [2 / 6]
    assert s['speed_count'].tolist() == [[2, 1, 3]] and s['speed_epe'].tolist() == [[0.5, 3.0, 20 / 3]]
    assert ofl.Flow(EST, 's').epe_map(ofl.Flow(GT, 's')).tolist() == [[[1, 3, 5], [0, 10, 5]]]
    assert ofl.Flow(EST, 's').epe(ofl.Flow(GT, 's')).tolist() == [4.0]


def test_nan_at_count_zero_and_consider_mask(error_native):
    import oflibpytorch_amd as ofl
    est, gt = _flows()
    m = est.mask.clone()
    m[1] = False
    est0 = ofl.Flow(est.vecs, 't', m)
    s = est0.error_stats(gt)
    assert s['count'][1] == 0 and math.isnan(s['epe'][1]) and not math.isnan(s['epe'][0])
    assert torch.isnan(s['outliers'][1]).all() and math.isnan(s['fl'][1]) and torch.isnan(s['speed_epe'][1]).all()
    assert s['max'][1] == 0 and s['speed_count'][1].tolist() == [0, 0, 0]
    e = est0.epe(gt)
    assert e.dtype == torch.float32 and e.shape == (2,) and math.isnan(e[1]) and not math.isnan(e[0])
    assert not est0.epe_map(gt)[1].any()
    # consider_mask=False: every pixel, whatever the masks say
    s = est0.error_stats(gt, consider_mask=False)
    assert s['count'].tolist() == [42, 42]
    ref = feo.score(est.vecs.numpy(), gt.vecs.numpy())
    assert s['epe'].tolist() == (ref['sum'] / 42).tolist()
    assert np.array_equal(est0.epe_map(gt, consider_mask=False).numpy(), ref['map'])
    assert est0.epe(gt, False).tolist() == (ref['sum'] / 42).astype(np.float32).tolist()
    # the default (None) is True
    assert torch.equal(est0.epe_map(gt), est0.epe_map(gt, consider_mask=True))


def test_epe_map_and_epe_types(error_native):
    est, gt = _flows()
    m = est.epe_map(gt)
    assert m.dtype == torch.float32 and m.shape == (2, 6, 7) and not m.requires_grad
    ref = feo.score(est.vecs.numpy(), gt.vecs.numpy(), est.mask.numpy(), gt.mask.numpy())
    assert np.array_equal(m.numpy(), ref['map'])
    assert not m[~(est.mask & gt.mask)].any()
    e = est.epe(gt)
    assert e.dtype == torch.float32 and e.grad_fn is None
    assert e.tolist() == (ref['sum'] / ref['count']).astype(np.float32).tolist()


def test_argument_checks(error_native):
    import oflibpytorch_amd as ofl
    est, gt = _flows()
    for call in (est.error_stats, est.epe_map, est.epe):
        with pytest.raises(TypeError, match="Error scoring flow: Gt needs to be of type 'Flow'"):
            call(gt.vecs)
        with pytest.raises(ValueError, match="Error scoring flow: Flow fields need to have the same shape, including batch size"):
            call(ofl.Flow(gt.vecs[:1], 't'))
        with pytest.raises(ValueError, match="same shape"):
            call(ofl.Flow(gt.vecs[:, :, :5], 't'))
        with pytest.raises(ValueError, match="Error scoring flow: Flow fields need to have the same reference"):
            call(ofl.Flow(gt.vecs, 's'))
        with pytest.raises(TypeError, match="Error scoring flow: Consider_mask needs to be boolean"):
            call(gt, consider_mask=1)
        # order: type of gt, shape, reference, consider_mask
        with pytest.raises(ValueError, match="same shape"):
            call(ofl.Flow(gt.vecs[:1], 's'), consider_mask='yes')
    with pytest.raises(TypeError, match="Error scoring flow: Thresholds needs to be a list or a tuple"):
        est.error_stats(gt, thresholds=3.0)
    with pytest.raises(ValueError, match="Error scoring flow: Thresholds list or tuple needs to have length 1 to 4"):
        est.error_stats(gt, thresholds=[])
    with pytest.raises(ValueError, match="length 1 to 4"):
        est.error_stats(gt, thresholds=(1, 2, 3, 4, 5))
    with pytest.raises(TypeError, match="Error scoring flow: Thresholds needs to hold integers or floats"):
        est.error_stats(gt, thresholds=(1, '3'))
    with pytest.raises(TypeError, match="integers or floats"):
        est.error_stats(gt, thresholds=(True,))
    for bad in (-1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match="Error scoring flow: Thresholds need to be finite and not negative"):
            est.error_stats(gt, thresholds=(1, bad))


def test_wrappers_equal_the_methods(error_native):
    import oflibpytorch_amd as ofl
    est, gt = _flows()
    assert callable(ofl.flow_error_stats) and callable(ofl.flow_epe)
    want = est.error_stats(gt, thresholds=(2, 4))
    got = ofl.flow_error_stats(est.vecs, gt.vecs, est.mask, gt.mask, thresholds=(2, 4))
    assert sorted(got) == sorted(want) and all(torch.equal(got[k], want[k]) for k in want if k not in ('epe', 'fl', 'outliers', 'speed_epe'))
    assert all(torch.equal(got[k].nan_to_num(-1), want[k].nan_to_num(-1)) for k in want)
    assert torch.equal(ofl.flow_epe(est.vecs, gt.vecs, est.mask, gt.mask), est.epe(gt))
    # NumPy arrays, channels last, no masks, 3-D in -> no batch dimension out
    e0, g0 = est.vecs[0].numpy(), gt.vecs[0].numpy()
    want = ofl.Flow(e0).error_stats(ofl.Flow(g0))
    got = ofl.flow_error_stats(np.moveaxis(e0, 0, -1), g0)
    assert got['count'].shape == () and got['outliers'].shape == (3,) and got['speed_epe'].shape == (3,)
    assert all(torch.equal(got[k].nan_to_num(-1), want[k][0].nan_to_num(-1)) for k in want)
    one = ofl.flow_epe(e0, g0)
    assert one.shape == () and one == ofl.Flow(e0).epe(ofl.Flow(g0))[0]
    assert ofl.flow_epe(e0, g0, est.mask[0].numpy(), gt.mask[0]) == est.epe(gt)[0]


@pytest.mark.parametrize("which", ["est", "gt", "both"])
def test_epe_gradient_equals_torch_autograd(which, error_native):
    import oflibpytorch_amd as ofl
    from oflibpytorch_amd import _autograd
    est, gt = _flows(seed=3)
    m = est.mask.clone()
    m[1, :3] = False
    valid = (m & gt.mask)
    upstream = torch.tensor([0.75, -2.0])
    a, b = est.vecs.clone(), gt.vecs.clone()
    a[0, :, 2, 3] = b[0, :, 2, 3]                                   # e = 0 on a valid pixel: gradient 0, as torch's norm
    valid[0, 2, 3] = True
    m[0, 2, 3] = True
    gm = gt.mask.clone()
    gm[0, 2, 3] = True
    leaves = []
    for t, wanted in ((a, which in ("est", "both")), (b, which in ("gt", "both"))):
        leaves.append(t.clone().requires_grad_(wanted))
    out = ofl.Flow(leaves[0], 't', m).epe(ofl.Flow(leaves[1], 't', gm))
    assert out.grad_fn is not None and type(out.grad_fn).__name__.startswith(_autograd.EpeFn.__name__)
    out.backward(upstream)
    # the expression a user writes today, on the CPU
    ref_leaves = [t.detach().clone().requires_grad_(t.requires_grad) for t in leaves]
    e = torch.linalg.vector_norm(ref_leaves[0] - ref_leaves[1], dim=1)
    mean = torch.stack([e[i][valid[i]].mean() for i in range(2)])
    torch.testing.assert_close(out.detach(), mean.detach(), rtol=1e-6, atol=0)
    mean.backward(upstream)
    for got, want in zip(leaves, ref_leaves):
        if not want.requires_grad:
            assert got.grad is None
            continue
        torch.testing.assert_close(got.grad, want.grad, rtol=1e-5, atol=1e-12)
        assert not got.grad[:, 0][~valid].any() and not got.grad[:, 1][~valid].any()
        assert got.grad[0, :, 2, 3].tolist() == [0.0, 0.0]
    if which == "both":
        assert torch.equal(leaves[0].grad, -leaves[1].grad)


def test_epe_gradient_of_an_image_without_valid_pixels_is_zero(error_native):
    import oflibpytorch_amd as ofl
    est, gt = _flows()
    m = est.mask.clone()
    m[0] = False
    v = est.vecs.clone().requires_grad_()
    out = ofl.Flow(v, 't', m).epe(gt)
    assert math.isnan(out[0].item())
    out.backward(torch.ones(2))
    assert not v.grad[0].any() and v.grad[1].any() and torch.isfinite(v.grad).all()


# ---- C ABI ------------------------------------------------------------------------------------------------------------------
FLOW_ARGS = ['const void*', 'int64_t', 'int32_t', 'const void*', 'int64_t', 'int32_t', 'const uint8_t*', 'int64_t', 'const uint8_t*', 'int64_t']
DECLARED = {
    'ofl_flow_error_workspace_bytes': ('int64_t', ['int32_t', 'int32_t', 'int32_t']),
    'ofl_flow_error_f64': ('int', FLOW_ARGS + ['int32_t', 'float', 'float', 'float', 'float', 'void*', 'float*', 'double*', 'int32_t', 'int32_t',
                                               'int32_t', 'void*']),
    'ofl_flow_epe_grad_f32': ('int', FLOW_ARGS + ['const float*', 'float*', 'float*', 'int32_t', 'int32_t', 'int32_t', 'void*']),
}


def test_header_declares_and_library_exports_the_entry_points():
    from oflibpytorch_amd import _build, _native
    header = open(os.path.join(ROOT, 'include', 'oflib_hip.h')).read()
    lib = _native.load_library()
    raw = ctypes.CDLL(_build.LIB_PATH)
    for name, (ret, args) in DECLARED.items():
        m = re.search(r'^(int|int64_t) %s\(([^;]*)\);' % name, header, flags=re.M)
        assert m is not None, name
        assert m.group(1) == ret
        types = [re.sub(r'\s*\w+$', '', a.strip()).replace(' *', '*') for a in m.group(2).replace('\n', ' ').split(',')]
        assert types == args, name
        assert hasattr(raw, name) and name in _native.exported_symbols()
        assert len(getattr(lib, name).argtypes) == len(args)
    assert re.search(r'^#define OFL_FLOW_ERROR_RECORD 16$', header, flags=re.M) and _native.ERROR_RECORD == 16
    assert lib.ofl_version() == 36 == _native.ABI_VERSION


def test_cabi_rejects_bad_arguments_without_a_device():
    from oflibpytorch_amd import _native
    lib = _native.load_library()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(16)          # (never dereferenced: rejected before any launch)
    wb = lib.ofl_flow_error_workspace_bytes
    assert wb(0, 4, 4) == -2 and wb(1, 0, 4) == -2 and wb(1, 4, -1) == -2 and wb(65536, 4, 4) == -2
    assert wb(1, 65536, 32768) == -2 and wb(1, 46341, 46341) == -2                 # h * w >= 2^31
    assert wb(1, 2, 2) == 128 and wb(3, 2, 2) == 3 * 128
    # the blocks of an image are a function of h * w alone: the bytes are linear in n
    assert wb(7, 1080, 1920) == 7 * wb(1, 1080, 1920) and wb(1, 1080, 1920) == wb(1, 1920, 1080) > wb(1, 96, 136) > 128
    thr = (3, 1.0, 3.0, 5.0, 0.0)
    err = lib.ofl_flow_error_f64
    ok = lambda **kw: [kw.get('est', one), 0, 0, kw.get('gt', one), 0, 0, null, 0, null, 0, *kw.get('thr', thr), kw.get('ws', one), null,
                       kw.get('rec', one), kw.get('n', 1), kw.get('h', 4), kw.get('w', 4), null]
    for key in ('est', 'gt', 'ws', 'rec'):
        assert err(*ok(**{key: null})) == -1, key
    assert err(*ok(n=0)) == -2 and err(*ok(n=65536)) == -2 and err(*ok(h=0)) == -2
    assert err(*ok(h=65536, w=32768)) == -2                                           # h * w = 2^31
    assert err(*ok(thr=(5, 1.0, 2.0, 3.0, 4.0))) == -3 and err(*ok(thr=(-1, 0.0, 0.0, 0.0, 0.0))) == -3
    assert err(*ok(thr=(2, 1.0, -1.0, 0.0, 0.0))) == -3 and err(*ok(thr=(1, float('nan'), 0.0, 0.0, 0.0))) == -3
    assert err(*ok(thr=(1, float('inf'), 0.0, 0.0, 0.0))) == -3
    assert err(*ok(ws=ctypes.c_void_p(12))) == -3 and err(*ok(est=ctypes.c_void_p(18))) == -3
    assert err(one, -4, 0, one, 0, 0, null, 0, null, 0, *thr, one, null, one, 1, 4, 4, null) == -3
    assert err(one, 0, 2, one, 0, 0, null, 0, null, 0, *thr, one, null, one, 1, 4, 4, null) == -3
    grad = lib.ofl_flow_epe_grad_f32
    gk = lambda **kw: [kw.get('est', one), 0, 0, kw.get('gt', one), 0, 0, null, 0, null, 0, kw.get('scale', one), kw.get('ge', one),
                       kw.get('gg', null), kw.get('n', 1), kw.get('h', 4), kw.get('w', 4), null]
    for key in ('est', 'gt', 'scale'):
        assert grad(*gk(**{key: null})) == -1, key
    assert grad(*gk(ge=null, gg=null)) == -1                                          # no output wanted
    assert grad(*gk(n=0)) == -2 and grad(*gk(w=0)) == -2 and grad(*gk(h=65536, w=32768)) == -2
    assert grad(*gk(ge=ctypes.c_void_p(18))) == -3
    assert grad(one, 0, 0, one, 0, 3, null, 0, null, 0, one, one, null, 1, 4, 4, null) == -3
