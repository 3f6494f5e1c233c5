"""CPU tier of Flow.visualise / visualise_flow: the oracle (tests/vis_oracle.py) against the reference's own output
(tests/golden/vis.npz) and its unit tests' known answers, the exact pieces the kernels restate (fmaf, the fp32 percentile), the
host logic of the API with the two native calls served by the oracle, and the C ABI's argument checks."""
import ctypes
import ctypes.util
import math

import numpy as np
import pytest
import torch

import vis_cases
import vis_oracle as vo


# ---- the oracle against the reference ---------------------------------------------------------------------------------
@pytest.mark.parametrize("k", vis_cases.case_ids())
def test_oracle_equals_reference_fixture(k):
    meta, flow, mask, expected = vis_cases.case(k)
    out, err = vis_cases.run_oracle(meta, flow, mask)
    if meta['error'] is not None:
        assert err is not None and list(err) == meta['error']
        return
    assert err is None
    assert out.dtype == np.uint8 and out.shape == expected.shape
    assert np.array_equal(out, expected)


def _translation(n, h, w, dx, dy, mask=None):
    f = np.zeros((n, 2, h, w), np.float32)
    f[:, 0], f[:, 1] = np.float32(dx), np.float32(dy)
    return f


def test_oracle_reference_kats():
    """test/test_flow_class.py:1681-1762 (test_visualise) of the reference, through the oracle"""
    f = np.zeros((1, 2, 200, 300), np.float32)
    f[0, 0, 0, 0] = 1
    img = vo.visualise(f, 'bgr')
    img[0, 0, 0] = 255
    assert np.all(img == 255)
    h, w = 200, 300
    cases = [((1, 0), [0, 0, 255], 0), ((-1, math.sqrt(3)), [0, 255, 0], 60), ((-1, -math.sqrt(3)), [255, 0, 0], 120)]
    for (dx, dy), bgr, hue in cases:
        fl = _translation(1, h, w, dx, dy)
        assert np.array_equal(vo.visualise(fl, 'bgr')[0], np.broadcast_to(np.array(bgr, np.uint8), (h, w, 3)))
        assert np.array_equal(vo.visualise(fl, 'rgb')[0], np.broadcast_to(np.array(bgr[::-1], np.uint8), (h, w, 3)))
        hsv = vo.visualise(fl, 'hsv')[0]
        assert np.all(hsv[..., 0] == hue) and np.all(hsv[..., 1] == 255) and np.all(hsv[..., 2] == 255)
    batch = np.concatenate([_translation(1, h, w, dx, dy) for (dx, dy), _, _ in cases])
    vis = vo.visualise(batch, 'bgr')
    for i, (_, bgr, _) in enumerate(cases):
        assert np.array_equal(vis[i], np.broadcast_to(np.array(bgr, np.uint8), (h, w, 3)))
    mask = np.zeros((1, h, w), bool)
    mask[:, 30:-30, 40:-40] = True
    fl = _translation(1, h, w, 1, 0)
    assert list(vo.visualise(fl, 'bgr', mask, True)[0, 10, 10]) == [0, 0, 180]
    assert list(vo.visualise(fl, 'rgb', mask, True)[0, 10, 10]) == [180, 0, 0]
    hsv = vo.visualise(fl, 'hsv', mask, True)[0]
    assert np.all(hsv[..., 0] == 0) and np.all(hsv[..., 1] == 255) and hsv[10, 10, 2] == 180 and hsv[100, 100, 2] == 255
    assert list(vo.visualise(fl, 'bgr', mask, True, True)[0, 30, 40]) == [0, 0, 0]
    assert list(vo.visualise(fl, 'rgb', mask, True, True)[0, 30, 40]) == [0, 0, 0]
    hsv = vo.visualise(fl, 'hsv', mask, True, True)[0]
    assert np.all(hsv[..., 0] == 0) and hsv[30, 40, 1] == 0 and hsv[30, 40, 2] == 0


def test_fmaf_emulation_equals_libm():
    libm = ctypes.CDLL(ctypes.util.find_library('m'))
    libm.fmaf.argtypes = [ctypes.c_float] * 3
    libm.fmaf.restype = ctypes.c_float
    rs = np.random.RandomState(5)
    n = 100000
    # mixed magnitudes and signs, plus products that nearly cancel the addend (where a non-fused form differs)
    a = (rs.randn(n) * np.exp2(rs.randint(-20, 20, n))).astype(np.float32)
    b = (rs.randn(n) * np.exp2(rs.randint(-20, 20, n))).astype(np.float32)
    c = (rs.randn(n) * np.exp2(rs.randint(-30, 30, n))).astype(np.float32)
    near = rs.rand(n) < 0.3
    c[near] = -(a[near] * b[near])
    got = vo.fmaf(a, b, c)
    ref = np.array([libm.fmaf(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], np.float32)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    assert not np.array_equal(got, (a * b + c).astype(np.float32))       # (the draws do exercise the fusion)


def test_fp32_percentile_lerp_equals_numpy():
    rs = np.random.RandomState(9)
    sizes = [1, 2, 3, 101, 201, 301, 1001, 10001] + list(rs.randint(1, 5000, 9992))
    for n in sizes:
        kind = rs.randint(4)
        if kind == 0:
            v = rs.rand(n).astype(np.float32) * 10
        elif kind == 1:
            v = rs.randint(0, 4, n).astype(np.float32) * np.float32(0.37)          # ties
        elif kind == 2:
            v = np.abs(rs.randn(n) * np.exp2(rs.randint(-10, 10, n))).astype(np.float32)
        else:
            v = np.full(n, np.float32(rs.rand() * 5))
        ref = np.percentile(v, 99)
        got = vo.percentile_lerp(v)
        assert ref.dtype == np.float32 and got.view(np.uint32) == ref.view(np.uint32), (n, kind)


# ---- host logic: the API with the two native calls served by the oracle ----------------------------------------------
def _fake_range(vecs, mask=None):
    v = vecs.detach().cpu().float().numpy()
    mag, _ = vo.cart_to_polar(vo.threshold(v[:, 0]), vo.threshold(v[:, 1]))
    m = None if mask is None else mask.detach().cpu().numpy()
    rng, counts = [], []
    for i in range(v.shape[0]):
        sel = mag[i].ravel() if m is None else mag[i][m[i]]
        counts.append(sel.size)
        rng.append(vo.default_range(sel[None, :])[0] if sel.size else 1.0)
    return torch.tensor(rng, dtype=torch.float64), torch.tensor(counts, dtype=torch.int32)


def _fake_visualise(vecs, range_max, mode, mask=None, show_mask=False, show_mask_borders=False, layout=0):
    v = vecs.detach().cpu().float().numpy()
    m = None if mask is None else mask.detach().cpu().numpy()
    out = vo.visualise(v, mode, m, show_mask, show_mask_borders, torch.as_tensor(range_max, dtype=torch.float64).numpy())
    return torch.from_numpy(out if layout == 1 else np.ascontiguousarray(np.moveaxis(out, -1, 1)))


@pytest.fixture
def vis_native(oracle_native, monkeypatch):
    from oflibpytorch_amd import _native
    monkeypatch.setattr(_native, "visualise_range", _fake_range)
    monkeypatch.setattr(_native, "visualise", _fake_visualise)
    return _native


@pytest.mark.parametrize("k", vis_cases.case_ids())
def test_host_logic_against_reference_fixture(k, vis_native):
    import oflibpytorch_amd as ofl
    meta, flow, mask, expected = vis_cases.case(k)
    out, err = vis_cases.run_api(ofl, meta, flow, mask, torch.device('cpu'))
    if meta['error'] is not None:
        assert err is not None and list(err) == meta['error']
        return
    assert err is None
    assert (isinstance(out, torch.Tensor) and meta['returned'] == 'tensor') or \
        (isinstance(out, np.ndarray) and meta['returned'] == 'ndarray')
    got = out.numpy() if isinstance(out, torch.Tensor) else out
    assert got.dtype == np.uint8 and got.shape == expected.shape
    assert np.array_equal(got, expected)


def test_host_argument_checks_in_reference_order(vis_native):
    """test/test_flow_class.py:1765-1783 of the reference, and the order of its checks"""
    import oflibpytorch_amd as ofl
    flow = ofl.Flow.zero([10, 10])
    with pytest.raises(ValueError, match="Mode needs to be"):
        flow.visualise(mode=3)
    with pytest.raises(ValueError, match="Mode needs to be"):
        flow.visualise(mode='test')
    with pytest.raises(TypeError, match="Show_mask needs"):
        flow.visualise('rgb', show_mask=2)
    with pytest.raises(TypeError, match="Show_mask_borders needs"):
        flow.visualise('rgb', show_mask_borders=2)
    with pytest.raises(TypeError, match="Return_tensor needs"):
        flow.visualise('rgb', return_tensor=2)
    with pytest.raises(TypeError, match="Range_max needs to be an integer"):
        flow.visualise('rgb', range_max='2')
    with pytest.raises(TypeError, match=r"length \(2\) needs to match the flow batch size \(1\)"):
        flow.visualise('rgb', range_max=(1, 2))
    with pytest.raises(ValueError, match="larger than zero"):
        flow.visualise('rgb', range_max=[0])
    with pytest.raises(ValueError, match="larger than zero"):
        flow.visualise('rgb', range_max=-1)
    # order: the type checks first (show_mask before return_tensor), range_max before the mode, the empty mask's IndexError
    # before the mode
    with pytest.raises(TypeError, match="Show_mask needs"):
        flow.visualise('nope', show_mask=1, return_tensor=3)
    with pytest.raises(TypeError, match="Range_max"):
        flow.visualise('nope', range_max='x')
    empty = ofl.Flow(torch.zeros(2, 2, 5, 6), 't', torch.zeros(2, 5, 6, dtype=torch.bool))
    with pytest.raises(IndexError, match="index -1 is out of bounds for axis 0 with size 0"):
        empty.visualise('nope', show_mask=True)
    with pytest.raises(ValueError, match="Mode needs to be"):
        empty.visualise('nope', show_mask=False)


def test_host_return_types_and_squeeze(vis_native):
    import oflibpytorch_amd as ofl
    f = torch.randn(2, 7, 9, 2)          # channel-last, as the reference accepts
    fl = ofl.Flow(f)
    assert isinstance(fl.visualise('bgr'), torch.Tensor) and fl.visualise('bgr').shape == (2, 3, 7, 9)
    assert fl.visualise('bgr').dtype == torch.uint8
    assert isinstance(fl.visualise('rgb', return_tensor=False), np.ndarray) and fl.visualise('rgb', return_tensor=False).shape == (2, 7, 9, 3)
    assert isinstance(fl.visualise('hsv', return_tensor=True), np.ndarray)      # the reference's 'hsv' quirk
    assert ofl.visualise_flow(f[0], 'bgr').shape == (3, 7, 9)
    assert ofl.visualise_flow(f[0].numpy(), 'hsv').shape == (7, 9, 3)
    assert ofl.visualise_flow(f, 'rgb', return_tensor=False).shape == (2, 7, 9, 3)
    assert np.array_equal(ofl.visualise_flow(f, 'bgr', range_max=[1, 2]).numpy(),
                          fl.visualise('bgr', range_max=[1.0, 2.0]).numpy())


# ---- C ABI -------------------------------------------------------------------------------------------------------------
def test_cabi_visualise_rejects_bad_arguments():
    from oflibpytorch_amd import _native
    lib = _native.load_library()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(16)    # (never dereferenced: rejected before any launch)
    assert lib.ofl_visualise_workspace_ints(0) == -2
    assert lib.ofl_visualise_workspace_ints(3) > 3 * 2048
    assert lib.ofl_visualise_range_f32(null, 0, 0, null, 0, one, one, null, 1, 4, 4, null) == -1
    assert lib.ofl_visualise_range_f32(one, 0, 0, null, 0, null, one, null, 1, 4, 4, null) == -1
    assert lib.ofl_visualise_range_f32(one, 0, 0, null, 0, one, null, null, 1, 4, 4, null) == -1
    assert lib.ofl_visualise_range_f32(one, 0, 0, null, 0, one, one, null, 0, 4, 4, null) == -2
    assert lib.ofl_visualise_range_f32(one, 0, 0, null, 0, one, one, null, 1, 0, 4, null) == -2
    assert lib.ofl_visualise_range_f32(one, 0, 2, null, 0, one, one, null, 1, 4, 4, null) == -3
    assert lib.ofl_visualise_range_f32(one, -8, 0, null, 0, one, one, null, 1, 4, 4, null) == -3
    u8 = lib.ofl_visualise_u8
    assert u8(null, 0, 0, null, 0, 0, 0, one, 2, 0, one, 1, 4, 4, null) == -1
    assert u8(one, 0, 0, null, 0, 0, 0, null, 2, 0, one, 1, 4, 4, null) == -1
    assert u8(one, 0, 0, null, 0, 0, 0, one, 2, 0, null, 1, 4, 4, null) == -1
    assert u8(one, 0, 0, null, 0, 0, 0, one, 2, 0, one, 1, 4, -1, null) == -2
    assert u8(one, 0, 0, null, 0, 0, 0, one, 2, 0, one, 70000, 4, 4, null) == -2
    assert u8(one, 0, 0, null, 0, 0, 0, one, 3, 0, one, 1, 4, 4, null) == -3
    assert u8(one, 0, 0, null, 0, 0, 0, one, 2, 2, one, 1, 4, 4, null) == -3
    assert u8(one, 0, 0, null, 0, 2, 0, one, 2, 0, one, 1, 4, 4, null) == -3
    assert u8(one, 0, 3, null, 0, 0, 0, one, 2, 0, one, 1, 4, 4, null) == -3
