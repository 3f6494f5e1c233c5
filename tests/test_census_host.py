"""CPU tier of Flow.census / census_map / census_stats: the oracle (tests/census_oracle.py) against torch's float64
autograd and on its planted case, the coverage conditions of the GPU tier's inputs, the host logic of the API with the native call
served by the oracle, every argument check that needs no device, and the C ABI's declarations and argument checks.  No device."""
import ctypes
import math

import numpy as np
import pytest
import torch

import census_oracle as cen
import grad_oracle64 as go
import photometric_oracle as po

FRAMES = cen.FRAMES                                  # the frames of the GPU tier (tests/test_gpu_census.py)


@pytest.fixture
def census_native(oracle_native, monkeypatch):
    from oflibpytorch_amd import _census
    monkeypatch.setattr(_census, "flow_census", cen.fake_flow_census)
    return _census


# ---- the oracle's gradient is the derivative ------------------------------------------------------------------------------------------
def _torch_loss(u, usable, img, other, sign, ims, patch, thresh, eps, q):
    """The definition as one differentiable float64 torch expression: explicit bilinear sample, grey, shifted slices, masked mean per
    image.  `usable` is piecewise constant and comes from the oracle."""
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
    assert c == 1
    gw, gi = ims * iw[:, 0], ims * img[:, 0]
    r = patch // 2
    soft = float(cen.SOFT)

    def at(x, dy, dx):
        return torch.nn.functional.pad(x, (r, r, r, r))[:, r + dy:r + dy + h, r + dx:r + dx + w]
    us = usable.double()
    total, cnt = 0.0, 0.0
    for dy, dx in cen.offsets(patch):
        term = at(us, dy, dx)
        dw, di = at(gw, dy, dx) - gw, at(gi, dy, dx) - gi
        e = di / torch.sqrt(soft + di * di) - dw / torch.sqrt(soft + dw * dw)
        s = e * e
        total = total + term * (s / (thresh + s))
        cnt = cnt + term
    known = us * (cnt > 0)
    rho = (total / cnt.clamp(min=1) + eps) ** q
    return (rho * known).sum((1, 2)) / known.sum((1, 2)), known.bool()


@pytest.mark.parametrize("q", [0.4, 1.0])
@pytest.mark.parametrize("patch", [3, 7])
@pytest.mark.parametrize("u8", [False, True], ids=["f32c1", "u8c1"])
@pytest.mark.parametrize("ref", cen.REFS)
def test_oracle_gradient_is_the_float64_derivative(ref, u8, patch, q):
    """A 9 x 17 frame (h - 1 and w - 1 powers of two) with vectors on a grid of 2^-6, |a| < 4: every float32 sample position is exact.
    One-channel images on a grid of 2^-8 -- float32 ones on its multiples of 2^-4, so that 255 Iw has no more than 24 bits, uint8 ones
    on the integers -- so that the float32 Gw and Gi of the definition are exact too (a three-channel grey rounds) and only the float32
    hd, b and scale differ from the float64 expression: the oracle's gradient is within 1e-6 of the gradient's scale."""
    n, h, w = 3, 9, 17
    rng = np.random.RandomState(23)
    a = (rng.randint(-255, 256, (n, 2, h, w)) / 64.0).astype(np.float32)
    mask = rng.uniform(size=(n, h, w)) >= 0.2
    if u8:
        img, other = (rng.randint(0, 256, (n, 1, h, w)).astype(np.uint8) for _ in range(2))
    else:
        img, other = ((rng.randint(0, 16, (n, 1, h, w)) / 16.0).astype(np.float32) for _ in range(2))
    sign = cen.sign_of(ref)
    sx, sy = go.warp_positions(a, n, sign)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    assert np.array_equal(sx.astype(np.float64), xs - sign * a[:, 0].astype(np.float64))          # the float32 positions are exact
    assert np.array_equal(sy.astype(np.float64), ys - sign * a[:, 1].astype(np.float64))
    res = cen.compute(a, mask, img, other, ref, patch, cen.THRESH, cen.EPS, q)
    assert 0.2 < res['known'].mean() < 0.8 and res['known'].any((1, 2)).all()
    got, big_a = cen.grad(a, mask, img, other, ref, patch, cen.THRESH, cen.EPS, q, cen.UPSTREAM)
    u = torch.from_numpy(a).double().requires_grad_(True)
    loss, known = _torch_loss(u, torch.from_numpy(res['usable']), torch.from_numpy(img).double(), torch.from_numpy(other).double(), sign,
                              1.0 if u8 else 255.0, patch, float(np.float32(cen.THRESH)), float(np.float32(cen.EPS)), float(np.float32(q)))
    assert np.array_equal(known.numpy(), res['known'])
    assert np.array_equal(res['gw'].astype(np.float64)[res['usable']],                              # the float32 greys are exact
                          _torch_grey(u.detach(), torch.from_numpy(other).double(), sign, 1.0 if u8 else 255.0)[res['usable']])
    assert np.allclose(loss.detach().numpy(), res['records'][:, 1] / res['records'][:, 0], rtol=1e-6)
    (loss * torch.tensor(cen.UPSTREAM, dtype=torch.float64)).sum().backward()
    want = u.grad.numpy()
    scale = np.abs(want).max()
    err = np.abs(got - want).max()
    print("ref %s u8 %s patch %d q %g: max |oracle - autograd| = %.3e of a gradient scale %.3e" % (ref, u8, patch, q, err, scale))
    assert got.dtype == np.float64 and big_a.dtype == np.float64
    assert scale > 1e-4 and err <= 1e-6 * scale
    unknown = ~np.broadcast_to(res['known'][:, None], got.shape)
    assert not got[unknown].any() and not want[unknown].any() and not big_a[unknown].any()
    assert np.all(np.abs(got) <= big_a * (1 + 1e-12) + 1e-300)


def _torch_grey(u, other, sign, ims):
    """Gw of `_torch_loss` alone, as a NumPy array"""
    n, c, h, w = other.shape
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing='ij')
    sx, sy = xs - sign * u[:, 0], ys - sign * u[:, 1]
    x0, y0 = torch.floor(sx), torch.floor(sy)
    ww, nn = sx - x0, sy - y0
    iw = 0.0
    for dy, wy in ((0, 1 - nn), (1, nn)):
        for dx, wx in ((0, 1 - ww), (1, ww)):
            xi, yi = x0 + dx, y0 + dy
            ok = (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)
            idx = (yi.clamp(0, h - 1) * w + xi.clamp(0, w - 1)).long()
            iw = iw + (wy * wx * ok) * torch.gather(other.reshape(n, h * w), 1, idx.reshape(n, -1)).reshape(n, h, w)
    return (ims * iw).numpy()


# ---- the coverage conditions of the GPU tier's inputs ---------------------------------------------------------------------------------
def test_every_larger_frame_of_the_gpu_table_shows_every_category():
    """No GPU test can pass on an empty set.  Per image and for both refs: with patch 7 in frames of 37 x 53 and larger, at least 50 %
    of the pixels are known, 5 % are known with a full patch, 20 % with a partial one and 5 % sample outside the frame; with patch 3
    in frames of 20 x 28 and larger, 10 % are known with a full patch and 5 % with a partial one; with patch 7 in every frame of
    20 x 28 and larger, at least 80 % of the known pixels have 0.05 < hd < 0.95: the penalty is not saturated.  Every frame of 5 x 7
    and larger has a known pixel in one of its images (the 2 x 2 frame has one usable pixel, which has no neighbour)."""
    for n, h, w in FRAMES:
        for ref in cen.REFS:
            for patch in (7, 3):
                known, full, partial, outside, mid = cen.categories(n, h, w, ref, patch)
                print("%d x %d x %d '%s' patch %d: known %s full %s partial %s outside %s, 0.05 < hd < 0.95 %s" % (
                    n, h, w, ref, patch, *(np.round(100 * x, 1).tolist() for x in (known, full, partial, outside, mid))))
                assert h * w < 35 or known.max() * h * w >= 1
                if patch == 7 and h * w >= 37 * 53:
                    assert known.min() >= 0.5 and full.min() >= 0.05 and partial.min() >= 0.2 and outside.min() >= 0.05, (n, h, w, ref)
                if patch == 3 and h * w >= 20 * 28:
                    assert full.min() >= 0.10 and partial.min() >= 0.05, (n, h, w, ref)
                if patch == 7 and h * w >= 20 * 28:
                    assert mid.min() >= 0.8, (n, h, w, ref)


def test_the_planted_case_shows_its_three_pixels():
    a, mask, img = cen.planted()
    for ref in cen.REFS:
        res = cen.compute(a, mask, img, img, ref)
        n, known, usable = res['n'][0], res['known'][0], res['usable'][0]
        assert np.array_equal(usable, mask[0])                                             # zero flow: every sample is inside
        assert usable[cen.PLANTED_LONE] and n[cen.PLANTED_LONE] == 0 and not known[cen.PLANTED_LONE]
        for p in cen.PLANTED_PAIR:
            assert n[p] == 1 and known[p]
        assert n[cen.PLANTED_CENTRE] == 48 and known[cen.PLANTED_CENTRE]
        assert known.sum() == cen.PLANTED_COUNT == res['records'][0, 0] and res['records'][0, 3] == n[known].sum()
        rho = np.float32(np.power(np.float64(np.float32(cen.EPS)), np.float64(np.float32(cen.Q))))
        assert np.array_equal(res['map'][0][known], np.full(cen.PLANTED_COUNT, rho, np.float32))
        assert not res['map'][0][~known].view(np.uint32).any() and res['records'][0, 2] == rho
        want, big_a = cen.grad(a, mask, img, img, ref, upstream=(1.0,))
        assert not want.any() and not np.isnan(want).any()                                  # every e is 0: so is every k


def test_hand_computed_pixel():
    """Two usable pixels side by side, zero flow on a 2 x 2 frame (positions exact), one channel: one term each."""
    a = np.zeros((1, 2, 2, 2), np.float32)
    mask = np.array([[[True, True], [False, False]]])
    img = np.array([[[[0.0, 0.0], [0.0, 0.0]]]], np.float32)
    other = np.array([[[[0.0, 1.0 / 255.0], [0.0, 0.0]]]], np.float32)
    res = cen.compute(a, mask, img, other, 's', 3, 0.1, 0.01, 1.0)
    f32 = np.float32
    gw1 = f32(255.0) * f32(1.0 / 255.0)
    tw = gw1 / np.sqrt(f32(0.81) + gw1 * gw1)
    s = (f32(0) - tw) * (f32(0) - tw)
    b = s / (f32(0.1) + s) / f32(1) + f32(0.01)
    assert res['n'][0].tolist() == [[1, 1], [0, 0]] and res['known'][0].tolist() == [[True, True], [False, False]]
    assert res['map'][0, 0].tolist() == [b, b] and res['map'].dtype == np.float32 and 0.8 < b < 0.9
    assert res['records'][0].tolist() == [2, float(b) + float(b), b, 2, 0, 0, 0, 0] and res['census'][0] == b
    none = cen.compute(a, np.zeros((1, 2, 2), bool), img, other, 's', 3)
    assert not none['records'].any() and math.isnan(none['census'][0]) and not none['map'].view(np.uint32).any()
    # uint8 images are read on the scale 0 .. 255 without a division: the same greys
    ru = cen.compute(a, mask, (img * 255).astype(np.uint8), (other * 255 + 0.5).astype(np.uint8), 's', 3, 0.1, 0.01, 1.0)
    assert np.array_equal(ru['map'], res['map'])


# ---- host logic: the API with the native call served by the oracle -------------------------------------------------------------------
def _flow(ref='s', n=2, h=20, w=28, mask=True):
    import oflibpytorch_amd as ofl
    a, m = po.case(n, h, w, ref)[:2]
    return ofl.Flow(torch.from_numpy(a.copy()), ref, torch.from_numpy(m.copy()) if mask else None)


@pytest.mark.parametrize("ref", cen.REFS)
def test_stats_keys_dtypes_shapes_and_values(census_native, ref):
    n, h, w = 2, 20, 28
    flow = _flow(ref)
    a, m, img, other, img_u8, other_u8 = po.case(n, h, w, ref)
    res = flow.census_stats(torch.from_numpy(img.copy()), torch.from_numpy(other.copy()))
    assert sorted(res) == ['census', 'count', 'fill', 'max', 'sum']
    assert res['count'].dtype == torch.int64 and res['count'].shape == (n,)
    for k in ('sum', 'max', 'census', 'fill'):
        assert res[k].dtype == torch.float64 and res[k].shape == (n,)
    want = cen.compute(a, m, img, other, ref)                 # the defaults: patch 7, thresh 0.1, eps 0.01, q 0.4
    rec = want['records']
    assert res['count'].tolist() == rec[:, 0].tolist() and res['sum'].tolist() == rec[:, 1].tolist()
    assert res['max'].tolist() == rec[:, 2].tolist() and res['census'].tolist() == (rec[:, 1] / rec[:, 0]).tolist()
    assert res['fill'].tolist() == (rec[:, 3] / (rec[:, 0] * 48)).tolist() and 0 < res['fill'].min() and res['fill'].max() < 1
    loss = flow.census(img.copy(), other.copy())
    assert loss.tolist() == want['census'].tolist() and loss.dtype == torch.float32 and loss.shape == (n,)
    kw = dict(patch=3, thresh=0.2, eps=0.5, q=1)
    cmap = flow.census_map(img.copy(), other.copy(), **kw)
    assert cmap.dtype == torch.float32 and np.array_equal(cmap.numpy(), cen.compute(a, m, img, other, ref, 3, 0.2, 0.5, 1.0)['map'])
    assert flow.census_stats(img.copy(), other.copy(), patch=3)['fill'].tolist() == \
        (lambda r: (r[:, 3] / (r[:, 0] * 8)).tolist())(cen.compute(a, m, img, other, ref, 3)['records'])
    # consider_mask=False drops the mask; C-H-W images, uint8 images, one-channel and non-contiguous ones are taken
    assert flow.census_stats(img.copy(), other.copy(), consider_mask=False)['count'].tolist() == \
        cen.compute(a, None, img, other, ref)['records'][:, 0].tolist()
    assert flow.census(img[0].copy(), other[0].copy()).tolist() == cen.compute(a, m, img[0], other[0], ref)['census'].tolist()
    assert flow.census(img_u8.copy(), other_u8.copy()).tolist() == cen.compute(a, m, img_u8, other_u8, ref)['census'].tolist()
    assert flow.census(img[:, :1].copy(), other[:, :1].copy()).tolist() == cen.compute(a, m, img[:, :1], other[:, :1], ref)['census'].tolist()
    nhwc = [torch.from_numpy(x.copy()).contiguous(memory_format=torch.channels_last) for x in (img, other)]
    assert flow.census(*nhwc).tolist() == want['census'].tolist()


def test_adapters_on_tensors_and_arrays(census_native):
    import oflibpytorch_amd as ofl
    n, h, w = 2, 20, 28
    a, m, img, other, _, _ = po.case(n, h, w, 't')
    want = cen.compute(a, m, img, other, 't')
    got = ofl.flow_census(a.copy(), img.copy(), other.copy(), 't', m.copy())
    assert got.shape == (n,) and got.tolist() == want['census'].tolist()
    one = ofl.flow_census(torch.from_numpy(a[1].copy()), torch.from_numpy(img[1].copy()), torch.from_numpy(other[1].copy()), 't',
                          torch.from_numpy(m[1].copy()))
    assert one.shape == () and float(one) == float(want['census'][1])
    stats = ofl.flow_census_stats(a[1].copy(), img[1].copy(), other[1].copy(), 't', m[1].copy())
    assert stats['count'].shape == () and int(stats['count']) == want['records'][1, 0]
    stats = ofl.flow_census_stats(a.copy(), img.copy(), other.copy(), 's', patch=5, q=1)
    assert stats['sum'].tolist() == cen.compute(a, None, img, other, 's', 5, q=1.0)['records'][:, 1].tolist()


def test_a_flow_that_requires_a_gradient_goes_through_census_fn(oracle_native, monkeypatch):
    import oflibpytorch_amd as ofl
    from oflibpytorch_amd import _autograd, _census
    calls = []

    def fake_grad(vecs, mask, img, other, flow_sign, patch, thresh, eps, q, scale):
        calls.append((flow_sign, patch, thresh, eps, q, scale.clone()))
        return torch.ones_like(vecs, dtype=torch.float32)
    monkeypatch.setattr(_census, "flow_census", cen.fake_flow_census)
    monkeypatch.setattr(_census, "flow_census_grad", fake_grad)
    n, h, w = 2, 20, 28
    a, m, img, other, _, _ = po.case(n, h, w, 's')
    v = torch.from_numpy(a.copy()).requires_grad_(True)
    im = torch.from_numpy(img.copy()).requires_grad_(True)
    loss = ofl.Flow(v, 's', torch.from_numpy(m.copy())).census(im, torch.from_numpy(other.copy()), patch=5, q=0.5)
    assert loss.requires_grad and type(loss.grad_fn).__name__ == "CensusFnBackward" and issubclass(_autograd.CensusFn, torch.autograd.Function)
    loss.backward(torch.tensor([0.75, -2.0]))
    want = cen.compute(a, m, img, other, 's', 5, q=0.5)
    assert loss.tolist() == want['census'].tolist()
    (sign, patch, thresh, eps, q, scale), = calls
    assert (sign, patch, thresh, eps, q) == (-1.0, 5, 0.1, 0.01, 0.5)
    assert scale.dtype == torch.float32 and scale.tolist() == (np.array([0.75, -2.0]) / want['records'][:, 0]).astype(np.float32).tolist()
    assert im.grad is None and torch.equal(v.grad, torch.ones_like(v))
    with torch.no_grad():
        assert not ofl.Flow(v, 's').census(im, im).requires_grad and len(calls) == 1


# ---- the checks of the API, none of which needs a device ------------------------------------------------------------------------------
def test_api_checks_and_their_messages(oracle_native, monkeypatch):
    import oflibpytorch_amd as ofl
    from oflibpytorch_amd import _census

    def never(*args, **kw):
        raise AssertionError("the checks come before the kernel")
    monkeypatch.setattr(_census, "flow_census", never)
    monkeypatch.setattr(_census, "census", never)
    flow = _flow(n=2, h=6, w=7)
    pre = r"Error computing census loss: "
    good = torch.zeros(2, 3, 6, 7)
    for call in (flow.census, flow.census_map, flow.census_stats):
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
            for bad in (torch.zeros(2, 2, 6, 7), torch.zeros(2, 4, 6, 7), torch.zeros(0, 6, 7)):
                with pytest.raises(ValueError, match=pre + name + " needs to have 1 or 3 channels"):
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
        for bad in (True, "3", 3.0, [3], torch.tensor(3)):
            with pytest.raises(TypeError, match=pre + "Patch needs to be an integer"):
                call(good, good, patch=bad)
        for bad in (1, 0, -3, 4, 9, 49):
            with pytest.raises(ValueError, match=pre + "Patch needs to be 3, 5 or 7"):
                call(good, good, patch=bad)
        for key, name in (("thresh", "Thresh"), ("eps", "Eps"), ("q", "Q")):
            for bad in (True, "1", [0.1], torch.tensor(0.1), np.ones(1)):
                with pytest.raises(TypeError, match=pre + name + " needs to be an integer or a float"):
                    call(good, good, **{key: bad})
            for bad in (0, 0.0, -1, -1e-9, 1e-60, float('nan'), float('inf'), -float('inf')):
                with pytest.raises(ValueError, match=pre + name + " needs to be finite and larger than 0"):
                    call(good, good, **{key: bad})
        for bad in (1.0000001, 2, 1e30):
            with pytest.raises(ValueError, match=pre + "Q needs to be at most 1"):
                call(good, good, q=bad)
        for bad in (1, 0, "True", 1.0):
            with pytest.raises(TypeError, match=pre + "Consider_mask needs to be boolean"):
                call(good, good, consider_mask=bad)
    # the order: types and dtypes, shapes, the frame's size, patch, thresh, eps, q, consider_mask
    with pytest.raises(TypeError, match="same dtype"):
        flow.census(good, torch.zeros(2, 9, 6, 7, dtype=torch.uint8), patch="x")
    with pytest.raises(ValueError, match="channels"):
        flow.census(good, torch.zeros(2, 9, 6, 7), patch="x")
    with pytest.raises(TypeError, match="Patch"):
        flow.census(good, good, patch="x", thresh=-1)
    with pytest.raises(ValueError, match="Thresh"):
        flow.census(good, good, thresh=-1, eps="x")
    with pytest.raises(TypeError, match="Eps"):
        flow.census(good, good, eps="x", q=5)
    with pytest.raises(ValueError, match="Q"):
        flow.census(good, good, q=5, consider_mask=1)
    thin = ofl.Flow(torch.zeros(2, 2, 1, 7), 't')
    with pytest.raises(ValueError, match=pre + "Flow field needs to be at least 2 pixels high and wide"):
        thin.census(torch.zeros(2, 3, 1, 7), torch.zeros(2, 3, 1, 7), patch="x")
    with pytest.raises(ValueError, match=pre):
        ofl.flow_census(flow.vecs, good, good, 't', eps=-5)
    with pytest.raises(TypeError, match=pre):
        ofl.flow_census_stats(flow.vecs, good, good.double(), 's')


def test_the_methods_and_adapters_are_exported():
    import oflibpytorch_amd as ofl
    for name in ("census", "census_map", "census_stats"):
        assert callable(getattr(ofl.Flow, name))
    assert callable(ofl.flow_census) and callable(ofl.flow_census_stats)
    assert "carry no gradient" in ofl.Flow.census.__doc__


# ---- the C ABI: declared, exported, and every rejected argument is rejected before any launch --------------------------------------
def test_c_abi_declarations_and_argument_checks_need_no_gpu():
    from oflibpytorch_amd import _census, _native
    names = {"ofl_flow_census_workspace_bytes", "ofl_flow_census_f64", "ofl_flow_census_grad_f32"}
    assert names <= set(_native.exported_symbols())
    header = open(_native._build.HEADERS[0]).read()
    for name in names:
        assert (" %s(" % name) in header
    assert "#define OFL_CENSUS_RECORD 8\n" in header and _census.RECORD == 8
    lib = _census._library()
    assert lib.ofl_version() == _native.ABI_VERSION                      # names were added, no signature changed
    ws = lib.ofl_flow_census_workspace_bytes
    # one block per tile of 64 x 16 pixels, whatever the patch; 64 bytes per block record
    for patch in (3, 5, 7):
        assert ws(1, 2, 2, patch) == 64 and ws(3, 16, 64, patch) == 3 * 64 and ws(2, 17, 65, patch) == 2 * 4 * 64
        assert ws(1, 1080, 1920, patch) == 68 * 30 * 64 and ws(65535, 2, 2, patch) == 65535 * 64
    for bad in ((0, 4, 4, 7), (-1, 4, 4, 7), (65536, 4, 4, 7), (1, 1, 4, 7), (1, 4, 1, 7), (1, 0, 4, 7), (1, 65536, 32768, 7),
                (1, 46341, 46341, 7), (1, 4, 4, 0), (1, 4, 4, 1), (1, 4, 4, 4), (1, 4, 4, 9), (1, 4, 4, -7)):
        assert ws(*bad) == -3, bad
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(4096)      # never dereferenced: every call below is rejected first

    def fwd(flow=one, flow_bs=0, half=0, mask=null, mask_bs=0, img=one, img_bs=0, other=one, other_bs=0, chan=3, u8=0, sign=-1.0,
            patch=7, thresh=0.1, eps=0.01, q=0.4, wsp=one, cmap=one, rec=one, n=1, h=4, w=4):
        return lib.ofl_flow_census_f64(flow, flow_bs, half, mask, mask_bs, img, img_bs, other, other_bs, chan, u8, sign, patch, thresh,
                                       eps, q, wsp, cmap, rec, n, h, w, null)

    def bwd(flow=one, flow_bs=0, half=0, mask=null, mask_bs=0, img=one, img_bs=0, other=one, other_bs=0, chan=3, u8=0, sign=-1.0,
            patch=7, thresh=0.1, eps=0.01, q=0.4, scale=one, grad=one, n=1, h=4, w=4):
        return lib.ofl_flow_census_grad_f32(flow, flow_bs, half, mask, mask_bs, img, img_bs, other, other_bs, chan, u8, sign, patch,
                                            thresh, eps, q, scale, grad, n, h, w, null)
    odd = ctypes.c_void_p(4098)
    nan, inf = float('nan'), float('inf')
    shared = (dict(n=0), dict(n=65536), dict(n=-3), dict(h=1), dict(w=1), dict(h=0), dict(h=65536, w=32768), dict(h=46341, w=46341),
              dict(sign=0.0), dict(sign=2.0), dict(sign=-0.5), dict(sign=nan),
              dict(chan=0), dict(chan=2), dict(chan=4), dict(chan=-1), dict(u8=2), dict(u8=-1),
              dict(patch=0), dict(patch=1), dict(patch=4), dict(patch=6), dict(patch=9), dict(patch=-3),
              dict(thresh=0.0), dict(thresh=-0.1), dict(thresh=nan), dict(thresh=inf), dict(thresh=-inf),
              dict(eps=0.0), dict(eps=-1e-9), dict(eps=nan), dict(eps=inf), dict(eps=-inf),
              dict(q=0.0), dict(q=-0.4), dict(q=1.0000001), dict(q=2.0), dict(q=nan), dict(q=inf), dict(q=-inf),
              dict(flow=null), dict(img=null), dict(other=null),
              dict(flow_bs=-1), dict(mask_bs=-32), dict(img_bs=-1), dict(other_bs=-8), dict(half=2), dict(half=-1),
              dict(flow=odd), dict(flow=ctypes.c_void_p(4097), half=1), dict(img=odd), dict(other=odd))
    for kw in shared + (dict(cmap=null, rec=null), dict(wsp=null), dict(wsp=ctypes.c_void_p(4100)), dict(rec=ctypes.c_void_p(4100)),
                        dict(cmap=odd)):
        assert fwd(**kw) == -3, kw
    for kw in shared + (dict(scale=null), dict(grad=null), dict(scale=odd), dict(grad=odd)):
        assert bwd(**kw) == -3, kw
