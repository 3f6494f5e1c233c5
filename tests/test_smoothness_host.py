"""CPU tier of Flow.smoothness / smoothness_map / smoothness_stats: the oracle (tests/smoothness_oracle.py) against
torch's float64 autograd and on cases written out by hand, the host logic of the API with the native call served by the oracle, every
argument check that needs no device, and the C ABI's argument checks.  No device."""
import ctypes
import math

import numpy as np
import pytest
import torch

import smoothness_oracle as so


@pytest.fixture
def smoothness_native(oracle_native, monkeypatch):
    from oflibpytorch_amd import _smoothness
    monkeypatch.setattr(_smoothness, "flow_smoothness", so.fake_flow_smoothness)
    return _smoothness


# ---- the oracle's gradient is the derivative ------------------------------------------------------------------------------------------
def _torch_loss(f, valid, img, order, alpha, eps):
    """The definition as one differentiable float64 torch expression: per image the mean of the valid terms."""
    total, count = 0.0, 0.0
    for axis in (3, 2):
        n = f.shape[axis]
        if n < order + 1:
            continue
        nar = lambda t, a, b, ax=axis: t.narrow(ax if t.dim() == 4 else ax - 1, a, b)
        if order == 1:
            d = nar(f, 1, n - 1) - nar(f, 0, n - 1)
            ok = nar(valid, 1, n - 1) & nar(valid, 0, n - 1)
            g = None if img is None else (nar(img, 1, n - 1) - nar(img, 0, n - 1)).abs().mean(1)
        else:
            d = nar(f, 0, n - 2) - 2 * nar(f, 1, n - 2) + nar(f, 2, n - 2)
            ok = nar(valid, 0, n - 2) & nar(valid, 1, n - 2) & nar(valid, 2, n - 2)
            g = None if img is None else (nar(img, 2, n - 2) - nar(img, 0, n - 2)).abs().mean(1) * 0.5
        r = d.abs().sum(1) if eps == 0 else torch.sqrt(d * d + eps * eps).sum(1)      # (|d|: the subgradient 0 at d = 0)
        t = r if g is None else torch.exp(-alpha * g) * r
        total = total + (t * ok).sum((1, 2))
        count = count + ok.sum((1, 2))
    return total / count


@pytest.mark.parametrize("with_img", [False, True], ids=["plain", "img"])
@pytest.mark.parametrize("eps", [0.0, 1e-3])
@pytest.mark.parametrize("order", [1, 2])
def test_oracle_gradient_is_the_float64_derivative(order, eps, with_img):
    """Vectors on a grid of 2^-10, so that the float32 differences of the definition are exact and only its float32 weight and roots
    differ from the float64 expression: the oracle's gradient is within 1e-6 of the gradient's scale."""
    n, h, w = 3, 9, 11
    rng = np.random.RandomState(5)
    f = (np.round(rng.normal(0, 1.5, (n, 2, h, w)) * 1024) / 1024).astype(np.float32)
    f[:, :, 2:5, 3:7] = 0.5                                   # d = 0 occurs
    mask = rng.uniform(size=(n, h, w)) >= 0.2
    img = rng.uniform(size=(n, 3, h, w)).astype(np.float32) if with_img else None
    alpha = 4.0
    got, a, read = so.grad(f, mask, img, order, alpha, eps, so.UPSTREAM)
    ft = torch.from_numpy(f).double().requires_grad_(True)
    loss = _torch_loss(ft, torch.from_numpy(mask), None if img is None else torch.from_numpy(img).double(), order, alpha,
                       float(np.float32(eps)))
    (loss * torch.tensor(so.UPSTREAM, dtype=torch.float64)).sum().backward()
    want = ft.grad.numpy()
    scale = np.abs(want).max()
    err = np.abs(got.astype(np.float64) - want).max()
    print("order %d eps %g img %s: max |oracle - autograd| = %.3e of a gradient scale %.3e" % (order, eps, with_img, err, scale))
    assert scale > 1e-3 and err <= 1e-6 * scale
    assert not got[~np.broadcast_to(read[:, None], got.shape)].any() and not want[~np.broadcast_to(read[:, None], want.shape)].any()
    assert np.all(np.abs(got) <= a * (1 + 1e-6) + 1e-30)


# ---- the oracle on hand-computed cases -------------------------------------------------------------------------------------------
def _frame23():
    f = np.zeros((1, 2, 2, 3), np.float32)
    f[0, 0, 0] = [0, 1, 3]
    return f


def test_hand_computed_records_of_a_2_by_3_frame():
    f = _frame23()
    r = so.compute(f, None, None, 1, 10.0, 0.0)
    # x: |1| + |2| in row 0, 0 + 0 in row 1; y: 0 + 1 + 3
    assert r['records'].tolist() == [[4, 3, 3, 4, 3, 0, 0, 0]] and r['smoothness'].tolist() == [1.0]
    assert r['map'].tolist() == [[[1, 3, 3], [0, 0, 0]]]                     # attributed to the left / upper pixel
    r = so.compute(f, None, None, 2, 10.0, 0.0)
    # x: the centre column, (0 - 2) + 3 = 1 and 0; y: no term in two rows
    assert r['records'].tolist() == [[2, 0, 1, 0, 1, 0, 0, 0]] and r['smoothness'].tolist() == [0.5]
    assert r['map'].tolist() == [[[0, 1, 0], [0, 0, 0]]]
    mask = np.ones((1, 2, 3), bool)
    mask[0, 0, 2] = False
    r = so.compute(f, mask, None, 1, 10.0, 0.0)
    assert r['records'].tolist() == [[3, 2, 1, 1, 1, 0, 0, 0]] and r['map'].tolist() == [[[1, 1, 0], [0, 0, 0]]]
    assert so.compute(f, mask, None, 2, 10.0, 0.0)['records'].tolist() == [[1, 0, 0, 0, 0, 0, 0, 0]]       # row 1's centre: 0, valid
    mask[:] = False
    r = so.compute(f, mask, None, 1, 10.0, 0.0)
    assert not r['records'].any() and math.isnan(r['smoothness'][0]) and not r['map'].any()
    # eps: every step float32
    eps = np.float32(0.5)
    r = so.compute(f, None, None, 1, 10.0, 0.5)
    one = np.sqrt(np.float32(1) + eps * eps) + np.sqrt(eps * eps)
    assert r['x']['t'][0, 0, 0] == one and r['x']['t'].dtype == np.float32 and r['x']['t'][0, 1, 0] == np.float32(1.0)


def test_hand_computed_weights():
    f = _frame23()
    img = np.zeros((1, 2, 2, 3), np.float32)
    img[0, 0, :, 1:] = 1.0                                     # channel 0 steps by 1 between columns 0 and 1; channel 1 is flat
    r = so.compute(f, None, img, 1, 2.0, 0.0)
    w = np.float32(math.exp(-1.0))                             # g = (1 + 0) / 2, alpha g = 1
    assert r['x']['w'][0].tolist() == [[w, 1, 1], [w, 1, 1]] and r['y']['w'][0, 0].tolist() == [1, 1, 1]
    assert r['map'][0, 0].tolist() == [w * np.float32(1), 3, 3]
    r2 = so.compute(f, None, img, 2, 2.0, 0.0)                 # g = ((1 + 0) / 2) * 0.5
    assert r2['x']['w'][0, 0, 1] == np.float32(math.exp(-0.5)) and r2['records'][0, 0] == 2
    # uint8: s / 255; a C-H-W image broadcasts; a constant image weighs 1
    u8 = (img * 255).astype(np.uint8)
    assert np.array_equal(so.compute(f, None, u8, 1, 2.0, 0.0)['map'], r['map'])
    assert np.array_equal(so.compute(np.concatenate([f, f]), None, img[0], 1, 2.0, 0.0)['map'][1], r['map'][0])
    assert np.array_equal(so.compute(f, None, img * 0 + 0.3, 1, 2.0, 0.0)['map'], so.compute(f, None, None, 1, 2.0, 0.0)['map'])
    # fp16 storage is up-converted exactly
    assert np.array_equal(so.compute(f.astype(np.float16), None, img, 1, 2.0, 0.0)['map'], r['map'])


def test_hand_computed_gradient():
    f = _frame23()
    g, a, read = so.grad(f, None, None, 1, 10.0, 0.0, (7.0,))
    # 7 terms, scale 1, q = sign(d): row 0 takes (-1, +1 - 1, +1) from its x terms and (0 at d = 0, +1, +1) from the y terms below it
    assert g[0, 0].tolist() == [[-1, 1, 2], [0, -1, -1]] and not g[0, 1].any() and read.all()
    assert a[0, 0].tolist() == [[1, 3, 2], [0, 1, 1]]
    one = np.zeros((1, 2, 1, 1), np.float32)
    g, a, read = so.grad(one, None, None, 1, 10.0, 0.001, (1.0,))
    assert not g.any() and not a.any() and not read.any() and g.dtype == np.float32


# ---- host logic: the API with the native call served by the oracle -------------------------------------------------------------------
def _flow(n=2, h=6, w=7, mask=True):
    import oflibpytorch_amd as ofl
    f, m = so.case(n, h, w)
    return ofl.Flow(torch.from_numpy(f.copy()), 't', torch.from_numpy(m.copy()) if mask else None)


def test_stats_keys_dtypes_shapes_and_values(smoothness_native):
    flow = _flow()
    f, m = so.case(2, 6, 7)
    img = so.image(2, 6, 7)
    res = flow.smoothness_stats(torch.from_numpy(img.copy()))
    assert sorted(res) == ['count_x', 'count_y', 'max', 'smoothness', 'sum_x', 'sum_y']
    for k in ('count_x', 'count_y'):
        assert res[k].dtype == torch.int64 and res[k].shape == (2,)
    for k in ('sum_x', 'sum_y', 'max', 'smoothness'):
        assert res[k].dtype == torch.float64 and res[k].shape == (2,)
    want = so.compute(f, m, img)                               # the defaults: order 1, alpha 10, eps 0.001
    rec = want['records']
    assert res['count_x'].tolist() == rec[:, 0].tolist() and res['count_y'].tolist() == rec[:, 1].tolist()
    assert res['sum_x'].tolist() == rec[:, 2].tolist() and res['max'].tolist() == rec[:, 4].tolist()
    assert res['smoothness'].tolist() == ((rec[:, 2] + rec[:, 3]) / (rec[:, 0] + rec[:, 1])).tolist()
    assert flow.smoothness(img.copy()).tolist() == want['smoothness'].tolist() and flow.smoothness(img.copy()).dtype == torch.float32
    smap = flow.smoothness_map(img.copy(), order=2, alpha=3, eps=0)
    assert smap.dtype == torch.float32 and np.array_equal(smap.numpy(), so.compute(f, m, img, 2, 3.0, 0.0)['map'])
    # consider_mask=False drops the mask; a C-H-W image, a uint8 image and a non-contiguous one are taken
    assert flow.smoothness_stats(consider_mask=False)['count_x'].tolist() == [36, 36]
    assert flow.smoothness(img[0].copy()).tolist() == so.compute(f, m, img[0])['smoothness'].tolist()
    u8 = so.image(2, 6, 7, 3, True)
    assert flow.smoothness(u8.copy()).tolist() == so.compute(f, m, u8)['smoothness'].tolist()
    nhwc = torch.from_numpy(img.copy()).contiguous(memory_format=torch.channels_last)
    assert flow.smoothness(nhwc).tolist() == want['smoothness'].tolist()


def test_adapters_on_tensors_and_arrays(smoothness_native):
    import oflibpytorch_amd as ofl
    f, m = so.case(2, 6, 7)
    img = so.image(2, 6, 7)
    want = so.compute(f, m, img, 2, 10.0, 0.001)
    got = ofl.flow_smoothness(f.copy(), img.copy(), m.copy(), order=2)
    assert got.shape == (2,) and got.tolist() == want['smoothness'].tolist()
    one = ofl.flow_smoothness(torch.from_numpy(f[1].copy()), torch.from_numpy(img[1].copy()), torch.from_numpy(m[1].copy()), order=2)
    assert one.shape == () and float(one) == float(want['smoothness'][1])
    stats = ofl.flow_smoothness_stats(f[1].copy(), img[1].copy(), m[1].copy(), order=2)
    assert stats['count_x'].shape == () and int(stats['count_x']) == want['records'][1, 0]
    stats = ofl.flow_smoothness_stats(f.copy(), order=1, eps=0)
    assert stats['count_y'].tolist() == [35, 35]


# ---- the checks of the API, none of which needs a device ------------------------------------------------------------------------------
def test_api_checks_and_their_messages(oracle_native, monkeypatch):
    import oflibpytorch_amd as ofl
    from oflibpytorch_amd import _smoothness

    def never(*args, **kw):
        raise AssertionError("the checks come before the kernel")
    monkeypatch.setattr(_smoothness, "flow_smoothness", never)
    monkeypatch.setattr(_smoothness, "smoothness", never)
    flow = _flow()
    pre = r"Error computing flow smoothness: "
    good = torch.zeros(2, 3, 6, 7)
    for call in (flow.smoothness, flow.smoothness_map, flow.smoothness_stats):
        for bad in ("img", [1.0], 3):
            with pytest.raises(TypeError, match=pre + "Img needs to be a torch tensor or a numpy array"):
                call(bad)
        for bad in (good.double(), good.half(), good.to(torch.int32), np.zeros((2, 3, 6, 7)), np.zeros((2, 3, 6, 7), np.int8)):
            with pytest.raises(TypeError, match=pre + "Img needs to be of dtype float32 or uint8"):
                call(bad)
        for bad in (torch.zeros(6, 7), torch.zeros(1, 2, 3, 6, 7)):
            with pytest.raises(ValueError, match=pre + "Img needs to have 3 or 4 dimensions"):
                call(bad)
        for bad in (torch.zeros(2, 5, 6, 7), torch.zeros(0, 6, 7)):
            with pytest.raises(ValueError, match=pre + "Img needs to have 1 to 4 channels"):
                call(bad)
        for bad in (torch.zeros(2, 3, 7, 6), torch.zeros(3, 6, 8)):
            with pytest.raises(ValueError, match=pre + "Img needs to have the H-W shape of the flow"):
                call(bad)
        for bad in (torch.zeros(1, 3, 6, 7), torch.zeros(3, 3, 6, 7)):
            with pytest.raises(ValueError, match=pre + "Img needs to have the batch size of the flow"):
                call(bad)
        for bad in (1.0, True, "1", [1]):
            with pytest.raises(TypeError, match=pre + "Order needs to be an integer"):
                call(good, order=bad)
        for bad in (0, 3, -1):
            with pytest.raises(ValueError, match=pre + "Order needs to be 1 or 2"):
                call(good, order=bad)
        for name, key in (("Alpha", "alpha"), ("Eps", "eps")):
            for bad in (True, "1", [0.1], torch.tensor(0.1), np.ones(1)):
                with pytest.raises(TypeError, match=pre + name + " needs to be an integer or a float"):
                    call(good, **{key: bad})
            for bad in (-1, -1e-9, float('nan'), float('inf'), -float('inf')):
                with pytest.raises(ValueError, match=pre + name + " needs to be finite and not negative"):
                    call(good, **{key: bad})
        for bad in (1, 0, "True", 1.0):
            with pytest.raises(TypeError, match=pre + "Consider_mask needs to be boolean"):
                call(good, consider_mask=bad)
    # the order: img, order, alpha, eps, consider_mask
    with pytest.raises(ValueError, match="channels"):
        flow.smoothness(torch.zeros(2, 9, 6, 7), order="x", alpha=-1)
    with pytest.raises(TypeError, match="Order"):
        flow.smoothness(good, order="x", alpha=-1, consider_mask=1)
    with pytest.raises(ValueError, match="Alpha"):
        flow.smoothness(good, order=2, alpha=-1, eps="x")
    with pytest.raises(TypeError, match="Eps"):
        flow.smoothness(good, order=2, alpha=1, eps="x", consider_mask=1)
    with pytest.raises(ValueError, match=pre):
        ofl.flow_smoothness(flow.vecs, good, order=5)
    with pytest.raises(TypeError, match=pre):
        ofl.flow_smoothness_stats(flow.vecs, good.double())


def test_integers_and_zero_are_valid_parameters(smoothness_native):
    flow = _flow()
    f, m = so.case(2, 6, 7)
    img = so.image(2, 6, 7)
    for alpha, eps in ((0, 0), (1, 2), (0.0, 1e30)):
        got = flow.smoothness(img.copy(), alpha=alpha, eps=eps)
        assert got.tolist() == so.compute(f, m, img, 1, alpha, eps)['smoothness'].tolist()


def test_the_methods_and_adapters_are_exported():
    import oflibpytorch_amd as ofl
    for name in ("smoothness", "smoothness_map", "smoothness_stats"):
        assert callable(getattr(ofl.Flow, name))
    assert callable(ofl.flow_smoothness) and callable(ofl.flow_smoothness_stats)
    assert "carries no gradient" in ofl.Flow.smoothness.__doc__


# ---- the C ABI: declared, exported, and every rejected argument is rejected before any launch --------------------------------------
def test_c_abi_argument_checks_need_no_gpu():
    from oflibpytorch_amd import _native, _smoothness
    names = {"ofl_flow_smoothness_workspace_bytes", "ofl_flow_smoothness_f64", "ofl_flow_smoothness_grad_f32"}
    assert names <= set(_native.exported_symbols())
    header = open(_native._build.HEADERS[0]).read()
    for name in names:
        assert (" %s(" % name) in header
    lib = _smoothness._library()
    assert lib.ofl_version() == _native.ABI_VERSION == 36               # names were added, no signature changed
    ws = lib.ofl_flow_smoothness_workspace_bytes
    # one block per tile of 8 x 128, 256 at most; 64 bytes per block record
    assert ws(1, 1, 1) == 64 and ws(3, 8, 128) == 3 * 64 and ws(3, 9, 129) == 3 * 4 * 64 and ws(2, 37, 53) == 2 * 5 * 64
    assert ws(1, 1080, 1920) == 256 * 64 and ws(65535, 2, 2) == 65535 * 64 and ws(1, 32768, 65535) == 256 * 64
    for bad in ((0, 4, 4), (-1, 4, 4), (65536, 4, 4), (1, 0, 4), (1, 4, 0), (1, 65536, 32768), (1, 46341, 46341)):
        assert ws(*bad) == -3, bad
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(4096)      # never dereferenced: every call below is rejected first

    def fwd(flow=one, flow_bs=0, half=0, mask=null, mask_bs=0, img=null, img_bs=0, chan=0, u8=0, order=1, alpha=10.0, eps=0.001,
            wsp=one, smap=one, rec=one, n=1, h=4, w=4):
        return lib.ofl_flow_smoothness_f64(flow, flow_bs, half, mask, mask_bs, img, img_bs, chan, u8, order, alpha, eps, wsp, smap,
                                           rec, n, h, w, null)

    def bwd(flow=one, flow_bs=0, half=0, mask=null, mask_bs=0, img=null, img_bs=0, chan=0, u8=0, order=1, alpha=10.0, eps=0.001,
            scale=one, grad=one, n=1, h=4, w=4):
        return lib.ofl_flow_smoothness_grad_f32(flow, flow_bs, half, mask, mask_bs, img, img_bs, chan, u8, order, alpha, eps, scale,
                                                grad, n, h, w, null)
    shared = (dict(n=0), dict(n=65536), dict(n=-3), dict(h=0), dict(w=0), dict(h=65536, w=32768), dict(h=46341, w=46341),
              dict(order=0), dict(order=3), dict(order=-1),
              dict(img=one, chan=0), dict(img=one, chan=5), dict(img=one, chan=-1), dict(img=one, chan=3, u8=2),
              dict(img=one, chan=3, img_bs=-1), dict(img=ctypes.c_void_p(4098), chan=3),
              dict(alpha=-1.0), dict(alpha=float('nan')), dict(alpha=float('inf')), dict(eps=-1e-9), dict(eps=float('nan')),
              dict(eps=float('inf')), dict(flow=null), dict(flow_bs=-1), dict(mask_bs=-32), dict(half=2), dict(half=-1),
              dict(flow=ctypes.c_void_p(4098)), dict(flow=ctypes.c_void_p(4097), half=1))
    for kw in shared + (dict(wsp=null), dict(rec=null), dict(wsp=ctypes.c_void_p(4100)), dict(rec=ctypes.c_void_p(4100)),
                        dict(smap=ctypes.c_void_p(4098))):
        assert fwd(**kw) == -3, kw
    for kw in shared + (dict(scale=null), dict(grad=null), dict(scale=ctypes.c_void_p(4098)), dict(grad=ctypes.c_void_p(4098))):
        assert bwd(**kw) == -3, kw
