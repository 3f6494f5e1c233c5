"""CPU tier of Flow.photometric / photometric_map / photometric_stats: the oracle (tests/photometric_oracle.py) on
frames written out by hand and against torch's float64 autograd, the host logic of the API with the native call served by the oracle,
every argument check that needs no device, the C ABI's argument checks, and the coverage condition of the GPU tier's inputs.  No
device."""
import ctypes
import math

import numpy as np
import pytest
import torch

import grad_oracle64 as go
import photometric_oracle as po


@pytest.fixture
def photometric_native(oracle_native, monkeypatch):
    from oflibpytorch_amd import _photometric
    monkeypatch.setattr(_photometric, "flow_photometric", po.fake_flow_photometric)
    return _photometric


# ---- the oracle on hand-computed cases -------------------------------------------------------------------------------------------
def _ramp():
    """other(y, x) = x / 4 on a 3 x 5 frame (w - 1 = 4: positions are exact), img = 0"""
    other = np.tile(np.arange(5, dtype=np.float32) / 4, (1, 1, 3, 1))
    return np.zeros((1, 1, 3, 5), np.float32), other


def test_hand_computed_records_of_a_3_by_5_frame():
    img, other = _ramp()
    a = np.zeros((1, 2, 3, 5), np.float32)
    a[0, 0] = 1.5                                             # 's': the sample of pixel x lies at x + 1.5
    r = po.compute(a, None, img, other, 's', 0.0)
    # x = 0, 1, 2 sample 0.375, 0.625, 0.875; x = 3 (4.5: the east tap leaves the frame) and x = 4 are not known
    assert r['known'][0].tolist() == [[True, True, True, False, False]] * 3
    assert r['map'][0].tolist() == [[0.375, 0.625, 0.875, 0, 0]] * 3 and r['map'].dtype == np.float32
    assert r['records'].tolist() == [[9, 3 * 1.875, 0.875, 0, 0, 0, 0, 0]] and r['photometric'].tolist() == [0.625]
    # 't': the sample lies at x - 1.5; x = 0, 1 are not known; x = 2, 3, 4 sample 0.125, 0.375, 0.625
    r = po.compute(a, None, img, other, 't', 0.0)
    assert r['map'][0].tolist() == [[0, 0, 0.125, 0.375, 0.625]] * 3 and r['records'][0, :3].tolist() == [9, 3 * 1.125, 0.625]
    # the mask takes pixels out; an all-False mask leaves nothing: NaN, and a map of +0
    mask = np.ones((1, 3, 5), bool)
    mask[0, :, 2] = False
    r = po.compute(a, mask, img, other, 's', 0.0)
    assert r['records'][0, :3].tolist() == [6, 3.0, 0.625] and r['map'][0, 1].tolist() == [0.375, 0.625, 0, 0, 0]
    r = po.compute(a, ~np.ones((1, 3, 5), bool), img, other, 's', 0.0)
    assert not r['records'].any() and math.isnan(r['photometric'][0]) and not r['map'].view(np.uint32).any()
    # eps: every step float32; channels are averaged in float32
    eps = np.float32(0.5)
    r = po.compute(a, None, img, other, 's', 0.5)
    assert r['map'][0, 0, 0] == np.sqrt(np.float32(0.375) * np.float32(0.375) + eps * eps)
    img3, other3 = np.repeat(img, 3, 1), np.concatenate([other, 2 * other, 0 * other], 1)
    r3 = po.compute(a, None, img3, other3, 's', 0.0)
    assert r3['map'][0, 0, 0] == ((np.float32(0.375) + np.float32(0.75)) + np.float32(0)) / np.float32(3)
    # uint8 is s / 255; C-H-W broadcasts; fp16 storage is up-converted exactly
    u8 = (other * 4 * 60).astype(np.uint8)                    # 0, 60, 120, 180, 240
    ru = po.compute(a, None, np.zeros_like(u8), u8, 's', 0.0)
    as_f32 = u8.astype(np.float32) / np.float32(255)
    assert np.array_equal(ru['map'], po.compute(a, None, img, as_f32, 's', 0.0)['map']) and ru['map'][0, 0, 1] > 0.35
    base = po.compute(a, None, img, other, 's', 0.0)['map']
    two = po.compute(np.concatenate([a, a]), None, img[0], other[0], 's', 0.0)
    assert np.array_equal(two['map'][1], base[0])
    assert np.array_equal(po.compute(a.astype(np.float16), None, img, other, 's', 0.0)['map'], base)


def test_hand_computed_gradient():
    img, other = _ramp()
    a = np.zeros((1, 2, 3, 5), np.float32)
    a[0, 0] = 1.5
    # d > 0 everywhere known, eps = 0: q = 1; d Iw / d sx = 1/4; 's': d sx / d u = +1; count 9, upstream 9: scale 1
    want, big_a = po.grad(a, None, img, other, 's', 0.0, (9.0,))
    assert want[0, 0].tolist() == [[0.25, 0.25, 0.25, 0, 0]] * 3
    # along y the north and the south taps cancel -- except in the last row, whose south taps (weight 0) lie outside the frame and
    # are no terms: the one-sided derivative of the taps inside, as the grid sampler's backward gives it
    assert not want[0, 1, :2].any() and want[0, 1, 2].tolist() == [-0.375, -0.625, -0.875, 0, 0]
    # A: |s v_w| + |s v_e| with s = 1 (the row fraction is 0): x = 0 reads 0.25 and 0.5
    assert big_a[0, 0, 0].tolist() == [0.75, 1.25, 1.75, 0, 0]
    assert big_a[0, 1, 0, :3].tolist() == [0.75, 1.25, 1.75] and big_a[0, 1, 2, :3].tolist() == [0.375, 0.625, 0.875]
    want, _ = po.grad(a, None, img, other, 't', 0.0, (9.0,))
    assert want[0, 0].tolist() == [[0, 0, -0.25, -0.25, -0.25]] * 3
    # d = 0 with eps = 0: the gradient is 0, not NaN; an image without a known pixel has gradient 0
    want, big_a = po.grad(a, None, img, 0 * other, 's', 0.0, (9.0,))
    assert not want.any() and not big_a.any() and not np.isnan(want).any()
    want, _ = po.grad(a, ~np.ones((1, 3, 5), bool), img, other, 's', 1e-3, (1.0,))
    assert not want.any() and not np.isnan(want).any()


# ---- the oracle's gradient is the derivative ------------------------------------------------------------------------------------------
def _torch_loss(u, known, img, other, sign, eps):
    """The definition as one differentiable float64 torch expression: explicit bilinear sample, masked mean per image."""
    n, c, h, w = other.shape
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing='ij')
    sx, sy = xs - sign * u[:, 0], ys - sign * u[:, 1]
    x0, y0 = torch.floor(sx.detach()), torch.floor(sy.detach())
    ww, nn = sx - x0, sy - y0
    iw = 0.0
    for dy, wy in ((0, 1 - nn), (1, nn)):
        for dx, wx in ((0, 1 - ww), (1, ww)):
            xi, yi = x0 + dx, y0 + dy
            ok = (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)
            idx = (yi.clamp(0, h - 1) * w + xi.clamp(0, w - 1)).long()
            v = torch.gather(other.reshape(n, c, h * w), 2, idx.reshape(n, 1, -1).expand(n, c, -1)).reshape(n, c, h, w)
            iw = iw + (wy * wx * ok)[:, None] * v
    d = iw - img
    r = d.abs() if eps == 0 else torch.sqrt(d * d + eps * eps)      # (|d|: the subgradient 0 at d = 0)
    rho = r.sum(1) / c
    return (rho * known).sum((1, 2)) / known.sum((1, 2))


@pytest.mark.parametrize("eps", [0.0, 1e-3])
@pytest.mark.parametrize("ref", po.REFS)
def test_oracle_gradient_is_the_float64_derivative(ref, eps):
    """A 9 x 17 frame (h - 1 and w - 1 powers of two) with vectors on a grid of 2^-6, |a| < 4: every float32 sample position is exact.
    Images on a grid of 2^-8, so that the float32 Iw and d of the definition are exact too and only the float32 scale differs from
    the float64 expression: the oracle's gradient is within 1e-6 of the gradient's scale."""
    n, h, w = 3, 9, 17
    rng = np.random.RandomState(11)
    a = (rng.randint(-255, 256, (n, 2, h, w)) / 64.0).astype(np.float32)
    assert np.abs(a).max() < 4
    mask = rng.uniform(size=(n, h, w)) >= 0.2
    img = (rng.randint(0, 256, (n, 3, h, w)) / 256.0).astype(np.float32)
    other = (rng.randint(0, 256, (n, 3, h, w)) / 256.0).astype(np.float32)
    sign = po.sign_of(ref)
    sx, sy = go.warp_positions(a, n, sign)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    assert np.array_equal(sx.astype(np.float64), xs - sign * a[:, 0].astype(np.float64))          # the float32 positions are exact
    assert np.array_equal(sy.astype(np.float64), ys - sign * a[:, 1].astype(np.float64))
    res = po.compute(a, mask, img, other, ref, eps)
    assert 0.2 < res['known'].mean() < 0.8 and res['known'].any((1, 2)).all()
    got, big_a = po.grad(a, mask, img, other, ref, eps, po.UPSTREAM)
    u = torch.from_numpy(a).double().requires_grad_(True)
    loss = _torch_loss(u, torch.from_numpy(res['known']), torch.from_numpy(img).double(), torch.from_numpy(other).double(), sign,
                       float(np.float32(eps)))
    assert np.allclose(loss.detach().numpy(), res['records'][:, 1] / res['records'][:, 0], rtol=1e-6)
    (loss * torch.tensor(po.UPSTREAM, dtype=torch.float64)).sum().backward()
    want = u.grad.numpy()
    scale = np.abs(want).max()
    err = np.abs(got - want).max()
    print("ref %s eps %g: max |oracle - autograd| = %.3e of a gradient scale %.3e" % (ref, eps, err, scale))
    assert got.dtype == np.float64 and big_a.dtype == np.float64
    assert scale > 1e-4 and err <= 1e-6 * scale
    unknown = ~np.broadcast_to(res['known'][:, None], got.shape)
    assert not got[unknown].any() and not want[unknown].any() and not big_a[unknown].any()
    assert np.all(np.abs(got) <= big_a * (1 + 1e-12) + 1e-300)


# ---- the coverage condition of the GPU tier's inputs ----------------------------------------------------------------------------------
def test_every_frame_of_the_gpu_table_shows_every_category():
    """No GPU test can pass on an empty set: in every frame of 8 x 12 and larger, for both refs, at least 25 % of the pixels are known,
    at least 5 % are unknown because the sample leaves the frame and at least 5 % by the mask alone; every frame has a known pixel,
    the small ones at least 0.15 of theirs."""
    for n, h, w in po.FRAMES:
        for ref in po.REFS:
            known, leaves, masked = (float(s.mean()) for s in po.categories(n, h, w, ref))
            print("%d x %d x %d '%s': known %.1f %%, leaves the frame %.1f %%, masked %.1f %%" % (n, h, w, ref, 100 * known,
                                                                                                 100 * leaves, 100 * masked))
            assert abs(known + leaves + masked - 1) < 1e-12
            if h * w >= 8 * 12:
                assert known >= 0.25 and leaves >= 0.05 and masked >= 0.05, (n, h, w, ref)
            else:
                assert known >= 0.15 - 1e-12, (n, h, w, ref)
            assert known * n * h * w >= 1


# ---- host logic: the API with the native call served by the oracle -------------------------------------------------------------------
def _flow(ref='s', n=2, h=20, w=28, mask=True):
    import oflibpytorch_amd as ofl
    a, m = po.case(n, h, w, ref)[:2]
    return ofl.Flow(torch.from_numpy(a.copy()), ref, torch.from_numpy(m.copy()) if mask else None)


@pytest.mark.parametrize("ref", po.REFS)
def test_stats_keys_dtypes_shapes_and_values(photometric_native, ref):
    n, h, w = 2, 20, 28
    flow = _flow(ref)
    a, m, img, other, img_u8, other_u8 = po.case(n, h, w, ref)
    res = flow.photometric_stats(torch.from_numpy(img.copy()), torch.from_numpy(other.copy()))
    assert sorted(res) == ['count', 'max', 'photometric', 'sum']
    assert res['count'].dtype == torch.int64 and res['count'].shape == (n,)
    for k in ('sum', 'max', 'photometric'):
        assert res[k].dtype == torch.float64 and res[k].shape == (n,)
    want = po.compute(a, m, img, other, ref)                  # the default: eps 0.001
    rec = want['records']
    assert res['count'].tolist() == rec[:, 0].tolist() and res['sum'].tolist() == rec[:, 1].tolist()
    assert res['max'].tolist() == rec[:, 2].tolist() and res['photometric'].tolist() == (rec[:, 1] / rec[:, 0]).tolist()
    loss = flow.photometric(img.copy(), other.copy())
    assert loss.tolist() == want['photometric'].tolist() and loss.dtype == torch.float32 and loss.shape == (n,)
    pmap = flow.photometric_map(img.copy(), other.copy(), eps=0)
    assert pmap.dtype == torch.float32 and np.array_equal(pmap.numpy(), po.compute(a, m, img, other, ref, 0.0)['map'])
    # consider_mask=False drops the mask; C-H-W images, uint8 images and non-contiguous ones are taken
    assert flow.photometric_stats(img.copy(), other.copy(), consider_mask=False)['count'].tolist() == \
        po.compute(a, None, img, other, ref)['records'][:, 0].tolist()
    assert flow.photometric(img[0].copy(), other[0].copy()).tolist() == po.compute(a, m, img[0], other[0], ref)['photometric'].tolist()
    assert flow.photometric(img_u8.copy(), other_u8.copy()).tolist() == po.compute(a, m, img_u8, other_u8, ref)['photometric'].tolist()
    nhwc = [torch.from_numpy(x.copy()).contiguous(memory_format=torch.channels_last) for x in (img, other)]
    assert flow.photometric(*nhwc).tolist() == want['photometric'].tolist()
    for eps in (0, 2, 1e30):                                   # integers and zero are valid; eps * eps may overflow to inf
        assert flow.photometric(img.copy(), other.copy(), eps=eps).tolist() == po.compute(a, m, img, other, ref, eps)['photometric'].tolist()


def test_adapters_on_tensors_and_arrays(photometric_native):
    import oflibpytorch_amd as ofl
    n, h, w = 2, 20, 28
    a, m, img, other, _, _ = po.case(n, h, w, 't')
    want = po.compute(a, m, img, other, 't', 0.001)
    got = ofl.flow_photometric(a.copy(), img.copy(), other.copy(), 't', m.copy())
    assert got.shape == (n,) and got.tolist() == want['photometric'].tolist()
    one = ofl.flow_photometric(torch.from_numpy(a[1].copy()), torch.from_numpy(img[1].copy()), torch.from_numpy(other[1].copy()), 't',
                               torch.from_numpy(m[1].copy()))
    assert one.shape == () and float(one) == float(want['photometric'][1])
    stats = ofl.flow_photometric_stats(a[1].copy(), img[1].copy(), other[1].copy(), 't', m[1].copy())
    assert stats['count'].shape == () and int(stats['count']) == want['records'][1, 0]
    stats = ofl.flow_photometric_stats(a.copy(), img.copy(), other.copy(), 's', eps=0)
    assert stats['count'].tolist() == po.compute(a, None, img, other, 's', 0.0)['records'][:, 0].tolist()


# ---- the checks of the API, none of which needs a device ------------------------------------------------------------------------------
def test_api_checks_and_their_messages(oracle_native, monkeypatch):
    import oflibpytorch_amd as ofl
    from oflibpytorch_amd import _photometric

    def never(*args, **kw):
        raise AssertionError("the checks come before the kernel")
    monkeypatch.setattr(_photometric, "flow_photometric", never)
    monkeypatch.setattr(_photometric, "photometric", never)
    flow = _flow(n=2, h=6, w=7)
    pre = r"Error computing photometric loss: "
    good = torch.zeros(2, 3, 6, 7)
    for call in (flow.photometric, flow.photometric_map, flow.photometric_stats):
        for name, both in (("Img", lambda bad: (bad, good)), ("Other", lambda bad: (good, bad))):
            for bad in ("img", [1.0], 3, None):
                with pytest.raises(TypeError, match=pre + name + " needs to be a torch tensor or a numpy array"):
                    call(*both(bad))
            for bad in (good.double(), good.half(), good.to(torch.int32), np.zeros((2, 3, 6, 7)), np.zeros((2, 3, 6, 7), np.int8)):
                with pytest.raises(TypeError, match=pre + name + " needs to be of dtype float32 or uint8"):
                    call(*both(bad))
            for bad in (torch.zeros(6, 7), torch.zeros(1, 2, 3, 6, 7)):
                with pytest.raises(ValueError, match=pre + name + " needs to have 3 or 4 dimensions"):
                    call(*both(bad))
            for bad in (torch.zeros(2, 5, 6, 7), torch.zeros(0, 6, 7)):
                with pytest.raises(ValueError, match=pre + name + " needs to have 1 to 4 channels"):
                    call(*both(bad))
            for bad in (torch.zeros(2, 3, 7, 6), torch.zeros(3, 6, 8)):
                with pytest.raises(ValueError, match=pre + name + " needs to have the H-W shape of the flow"):
                    call(*both(bad))
            for bad in (torch.zeros(1, 3, 6, 7), torch.zeros(3, 3, 6, 7)):
                with pytest.raises(ValueError, match=pre + name + " needs to have the batch size of the flow"):
                    call(*both(bad))
        with pytest.raises(TypeError, match=pre + "Img and other need to be of the same dtype"):
            call(good, good.to(torch.uint8))
        with pytest.raises(ValueError, match=pre + "Img and other need to have the same number of channels"):
            call(good, torch.zeros(2, 1, 6, 7))
        for bad in (True, "1", [0.1], torch.tensor(0.1), np.ones(1)):
            with pytest.raises(TypeError, match=pre + "Eps needs to be an integer or a float"):
                call(good, good, eps=bad)
        for bad in (-1, -1e-9, float('nan'), float('inf'), -float('inf')):
            with pytest.raises(ValueError, match=pre + "Eps needs to be finite and not negative"):
                call(good, good, eps=bad)
        for bad in (1, 0, "True", 1.0):
            with pytest.raises(TypeError, match=pre + "Consider_mask needs to be boolean"):
                call(good, good, consider_mask=bad)
    # the order: types and dtypes, shapes, the frame's size, eps, consider_mask
    with pytest.raises(TypeError, match="same dtype"):
        flow.photometric(good, torch.zeros(2, 9, 6, 7, dtype=torch.uint8), eps="x")
    with pytest.raises(ValueError, match="channels"):
        flow.photometric(good, torch.zeros(2, 9, 6, 7), eps="x")
    with pytest.raises(TypeError, match="Eps"):
        flow.photometric(good, good, eps="x", consider_mask=1)
    with pytest.raises(ValueError, match="Eps"):
        flow.photometric(good, good, eps=-1, consider_mask=1)
    thin = ofl.Flow(torch.zeros(2, 2, 1, 7), 't')
    with pytest.raises(ValueError, match=pre + "Flow field needs to be at least 2 pixels high and wide"):
        thin.photometric(torch.zeros(2, 3, 1, 7), torch.zeros(2, 3, 1, 7), eps="x")
    with pytest.raises(ValueError, match=pre):
        ofl.flow_photometric(flow.vecs, good, good, 't', eps=-5)
    with pytest.raises(TypeError, match=pre):
        ofl.flow_photometric_stats(flow.vecs, good, good.double(), 's')


def test_the_methods_and_adapters_are_exported():
    import oflibpytorch_amd as ofl
    for name in ("photometric", "photometric_map", "photometric_stats"):
        assert callable(getattr(ofl.Flow, name))
    assert callable(ofl.flow_photometric) and callable(ofl.flow_photometric_stats)
    assert "carry no gradient" in ofl.Flow.photometric.__doc__


# ---- the C ABI: declared, exported, and every rejected argument is rejected before any launch --------------------------------------
def test_c_abi_argument_checks_need_no_gpu():
    from oflibpytorch_amd import _native, _photometric
    names = {"ofl_flow_photometric_workspace_bytes", "ofl_flow_photometric_f64", "ofl_flow_photometric_grad_f32"}
    assert names <= set(_native.exported_symbols())
    header = open(_native._build.HEADERS[0]).read()
    for name in names:
        assert (" %s(" % name) in header
    lib = _photometric._library()
    assert lib.ofl_version() == _native.ABI_VERSION == 36               # names were added, no signature changed
    ws = lib.ofl_flow_photometric_workspace_bytes
    # one block per 256 pixels, 256 at most; 64 bytes per block record
    assert ws(1, 2, 2) == 64 and ws(3, 16, 16) == 3 * 64 and ws(3, 1, 257) == -3 and ws(2, 37, 53) == 2 * 8 * 64
    assert ws(1, 1080, 1920) == 256 * 64 and ws(65535, 2, 2) == 65535 * 64 and ws(1, 32768, 65535) == 256 * 64
    for bad in ((0, 4, 4), (-1, 4, 4), (65536, 4, 4), (1, 1, 4), (1, 4, 1), (1, 0, 4), (1, 65536, 32768), (1, 46341, 46341)):
        assert ws(*bad) == -3, bad
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(4096)      # never dereferenced: every call below is rejected first

    def fwd(flow=one, flow_bs=0, half=0, mask=null, mask_bs=0, img=one, img_bs=0, other=one, other_bs=0, chan=3, u8=0, sign=-1.0,
            eps=0.001, wsp=one, pmap=one, rec=one, n=1, h=4, w=4):
        return lib.ofl_flow_photometric_f64(flow, flow_bs, half, mask, mask_bs, img, img_bs, other, other_bs, chan, u8, sign, eps, wsp,
                                            pmap, rec, n, h, w, null)

    def bwd(flow=one, flow_bs=0, half=0, mask=null, mask_bs=0, img=one, img_bs=0, other=one, other_bs=0, chan=3, u8=0, sign=-1.0,
            eps=0.001, scale=one, grad=one, n=1, h=4, w=4):
        return lib.ofl_flow_photometric_grad_f32(flow, flow_bs, half, mask, mask_bs, img, img_bs, other, other_bs, chan, u8, sign, eps,
                                                 scale, grad, n, h, w, null)
    odd = ctypes.c_void_p(4098)
    shared = (dict(n=0), dict(n=65536), dict(n=-3), dict(h=1), dict(w=1), dict(h=0), dict(h=65536, w=32768), dict(h=46341, w=46341),
              dict(sign=0.0), dict(sign=2.0), dict(sign=-0.5), dict(sign=float('nan')),
              dict(chan=0), dict(chan=5), dict(chan=-1), dict(u8=2), dict(u8=-1),
              dict(eps=-1e-9), dict(eps=float('nan')), dict(eps=float('inf')), dict(eps=-float('inf')),
              dict(flow=null), dict(img=null), dict(other=null),
              dict(flow_bs=-1), dict(mask_bs=-32), dict(img_bs=-1), dict(other_bs=-8), dict(half=2), dict(half=-1),
              dict(flow=odd), dict(flow=ctypes.c_void_p(4097), half=1), dict(img=odd), dict(other=odd))
    for kw in shared + (dict(pmap=null, rec=null), dict(wsp=null), dict(wsp=ctypes.c_void_p(4100)), dict(rec=ctypes.c_void_p(4100)),
                        dict(pmap=odd)):
        assert fwd(**kw) == -3, kw
    for kw in shared + (dict(scale=null), dict(grad=null), dict(scale=odd), dict(grad=odd)):
        assert bwd(**kw) == -3, kw
