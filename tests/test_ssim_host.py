"""CPU tier of Flow.ssim / ssim_map / ssim_stats: the oracle (tests/ssim_oracle.py) against the expression people mean
and against torch's float64 autograd, on its planted cases, the coverage conditions of the GPU tier's inputs, the host logic of the API
with the native call served by the oracle, every argument check that needs no device, and the C ABI's declarations and argument checks.
No device."""
import ctypes
import math

import numpy as np
import pytest
import torch

import census_oracle as cen
import grad_oracle64 as go
import photometric_oracle as po
import ssim_oracle as so

FRAMES = so.FRAMES                                   # the frames of the GPU tier (tests/test_gpu_ssim.py)


@pytest.fixture
def ssim_native(oracle_native, monkeypatch):
    from oflibpytorch_amd import _ssim
    monkeypatch.setattr(_ssim, "flow_ssim", so.fake_flow_ssim)
    return _ssim


# ---- the oracle computes the expression people mean ----------------------------------------------------------------------------------
def test_float64_evaluation_is_the_pooled_expression():
    """avg_pool2d 3 x 3 means, E[xy] - mx my, clamp((1 - SSIM) / 2, 0, 1) in torch float64 on the oracle's own X and Y, against the
    oracle's float64 evaluation, on the interior of an unmasked zero-flow frame (every window full): both sides float64 and
    algebraically equal (the one-pass and the two-pass variance differ by rounding alone): within 1e-12."""
    n, h, w = 2, 20, 28
    _, _, img, other, _, _ = po.case(n, h, w, 's')
    a = np.zeros((n, 2, h, w), np.float32)
    worst = 0.0
    for ref in so.REFS:
        res = so.compute(a, None, img, other, ref, 3, float64=True)
        assert res['map'].dtype == np.float64 and res['usable'].all() and (res['n'][:, 1:-1, 1:-1] == 9).all()
        x, y = torch.from_numpy(res['x'].copy()).double(), torch.from_numpy(res['y'].copy()).double()
        pool = lambda t: torch.nn.functional.avg_pool2d(t, 3, 1)
        c1, c2 = float(np.float32(so.C1)), float(np.float32(so.C2))
        mx, my = pool(x), pool(y)
        sxx, syy, sxy = pool(x * x) - mx * mx, pool(y * y) - my * my, pool(x * y) - mx * my
        ssim = (2 * mx * my + c1) * (2 * sxy + c2) / ((mx * mx + my * my + c1) * (sxx + syy + c2))
        want = torch.clamp((1 - ssim) / 2, 0, 1).mean(1).numpy()
        err = np.abs(res['map'][:, 1:-1, 1:-1] - want).max()
        worst = max(worst, float(err))
        assert 0.2 < want.mean() < 0.8
    print("largest |oracle float64 - pooled expression| on the interior: %.3e" % worst)
    assert worst <= 1e-12


def test_float32_definition_against_its_float64_evaluation():
    """The observed largest difference is printed (DESIGN.md 3.22 quotes it); the assertion is a sanity cap on a quantity in [0, 1],
    not a precision bar."""
    worst = 0.0
    for n, h, w in FRAMES:
        for ref in so.REFS:
            a, m, img, other, _, _ = po.case(n, h, w, ref)
            for window in so.WINDOWS:
                r32, r64 = so.compute(a, m, img, other, ref, window), so.compute(a, m, img, other, ref, window, float64=True)
                assert np.array_equal(r32['known'], r64['known']) and r32['map'].dtype == np.float32
                worst = max(worst, float(np.abs(r32['map'].astype(np.float64) - r64['map']).max()))
    print("largest |float32 map - float64 evaluation| over the frames of the GPU tier: %.3e" % worst)
    assert worst <= 1e-3


# ---- the oracle's gradient is the derivative ------------------------------------------------------------------------------------------
def _torch_loss(u, usable, img, other, sign, window, c1, c2):
    """The definition as one differentiable float64 torch expression: explicit bilinear sample, shifted slices, masked mean per image
    (no clamp: it is not active).  `usable` is piecewise constant and comes from the oracle."""
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
    r = window // 2

    def at(x, dy, dx):
        return torch.nn.functional.pad(x, (r, r, r, r))[..., r + dy:r + dy + h, r + dx:r + dx + w]
    us = usable.double()[:, None]
    cnt = sum(at(us, dy, dx) for dy, dx in so.offsets(window)).clamp(min=1)
    mean = lambda t: sum(at(us * t, dy, dx) for dy, dx in so.offsets(window)) / cnt
    mx, my = mean(iw), mean(img)
    sxx, syy, sxy = mean(iw * iw) - mx * mx, mean(img * img) - my * my, mean(iw * img) - mx * my
    ssim = (2 * mx * my + c1) * (2 * sxy + c2) / ((mx * mx + my * my + c1) * (sxx + syy + c2))
    rho = ((1 - ssim) / 2).mean(1)
    known = us[:, 0]
    return (rho * known).sum((1, 2)) / known.sum((1, 2)), iw


@pytest.mark.parametrize("chan", [1, 3])
@pytest.mark.parametrize("window", [3, 7])
@pytest.mark.parametrize("ref", so.REFS)
def test_oracle_gradient_is_the_float64_derivative(ref, window, chan):
    """A 9 x 17 frame (h - 1 and w - 1 powers of two) with vectors on a grid of 2^-6, |a| < 4: every float32 sample position is exact.
    Images on a grid of 2^-8, so that every float32 X of the definition is exact too and only the float32 scale differs from the
    float64 expression: the oracle's gradient is within 1e-6 of the gradient's scale."""
    n, h, w = 3, 9, 17
    rng = np.random.RandomState(29)
    a = (rng.randint(-255, 256, (n, 2, h, w)) / 64.0).astype(np.float32)
    mask = rng.uniform(size=(n, h, w)) >= 0.2
    img, other = ((rng.randint(0, 256, (n, chan, h, w)) / 256.0).astype(np.float32) for _ in range(2))
    sign = so.sign_of(ref)
    sx, sy = go.warp_positions(a, n, sign)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    assert np.array_equal(sx.astype(np.float64), xs - sign * a[:, 0].astype(np.float64))          # the float32 positions are exact
    assert np.array_equal(sy.astype(np.float64), ys - sign * a[:, 1].astype(np.float64))
    res = so.compute(a, mask, img, other, ref, window)
    assert 0.2 < res['known'].mean() < 0.8 and res['known'].any((1, 2)).all()
    raw = res['raw'][np.broadcast_to(res['known'][:, None], res['raw'].shape)]
    assert raw.min() > 0 and raw.max() < 1                                                         # the clamp is not active
    got, big_a = so.grad(a, mask, img, other, ref, window, so.C1, so.C2, so.UPSTREAM)
    u = torch.from_numpy(a).double().requires_grad_(True)
    loss, iw = _torch_loss(u, torch.from_numpy(res['usable']), torch.from_numpy(img).double(), torch.from_numpy(other).double(), sign,
                           window, float(np.float32(so.C1)), float(np.float32(so.C2)))
    us = np.broadcast_to(res['usable'][:, None], res['x'].shape)
    assert np.array_equal(res['x'].astype(np.float64)[us], iw.detach().numpy()[us])                # the float32 X are exact
    assert np.allclose(loss.detach().numpy(), res['records'][:, 1] / res['records'][:, 0], rtol=1e-5)
    (loss * torch.tensor(so.UPSTREAM, dtype=torch.float64)).sum().backward()
    want = u.grad.numpy()
    scale = np.abs(want).max()
    err = np.abs(got - want).max()
    print("ref %s window %d C %d: max |oracle - autograd| = %.3e of a gradient scale %.3e" % (ref, window, chan, err, scale))
    assert got.dtype == np.float64 and big_a.dtype == np.float64
    assert scale > 1e-4 and err <= 1e-6 * scale
    unknown = ~np.broadcast_to(res['known'][:, None], got.shape)
    assert not got[unknown].any() and not want[unknown].any() and not big_a[unknown].any()
    assert np.all(np.abs(got) <= big_a * (1 + 1e-12) + 1e-300)


# ---- the coverage conditions of the GPU tier's inputs ---------------------------------------------------------------------------------
def test_every_larger_frame_of_the_gpu_table_shows_every_category():
    """No GPU test can pass on an empty set.  Per image and for both refs: with window 3 in frames of 20 x 28 and larger, at least 50 %
    of the pixels are known, 15 % are known with a full window, 5 % with a partial one and 5 % sample outside the frame; with window 7
    in frames of 37 x 53 and larger, 5 % are known with a full window and 20 % with a partial one; with windows 3 and 7 in every frame
    of the table, at least 95 % of the known pixels have 0.05 < rho < 0.95: no clamp is active on these inputs (the planted case is)."""
    for n, h, w in FRAMES:
        for ref in so.REFS:
            for window in (3, 7):
                known, full, partial, outside, mid = so.categories(n, h, w, ref, window)
                print("%d x %d x %d '%s' window %d: known %s full %s partial %s outside %s, 0.05 < rho < 0.95 %s" % (
                    n, h, w, ref, window, *(np.round(100 * x, 1).tolist() for x in (known, full, partial, outside, mid))))
                if window == 3 and h * w >= 20 * 28:
                    assert known.min() >= 0.5 and full.min() >= 0.15 and partial.min() >= 0.05 and outside.min() >= 0.05, (n, h, w, ref)
                if window == 7 and h * w >= 37 * 53:
                    assert full.min() >= 0.05 and partial.min() >= 0.2, (n, h, w, ref)
                if (n, h, w) in po.TABLE + so.TILE_FRAMES:
                    assert mid[known > 0].min() >= 0.95, (n, h, w, ref)
                a, m, img, other, _, _ = po.case(n, h, w, ref)
                res = so.compute(a, m, img, other, ref, window)
                raw = res['raw'][np.broadcast_to(res['known'][:, None], res['raw'].shape)]
                assert raw.size == 0 or (raw.min() >= 0 and raw.max() <= 1), (n, h, w, ref)


# ---- the planted cases ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", so.WINDOWS)
def test_identical_images_give_exactly_zero(window):
    a, mask, img = so.planted_identical()
    for ref in so.REFS:
        res = so.compute(a, mask, img, img, ref, window)
        n, known = res['n'][0], res['known'][0]
        assert np.array_equal(known, mask[0])                                              # zero flow: every sample is inside
        assert known[cen.PLANTED_LONE] and n[cen.PLANTED_LONE] == 1                        # its own window
        for p in cen.PLANTED_PAIR:
            assert n[p] == 2 and known[p]
        assert n[cen.PLANTED_CENTRE] == window * window
        assert known.sum() == so.PLANTED_IDENTICAL_COUNT == res['records'][0, 0] and res['records'][0, 3] == n[known].sum()
        assert np.array_equal(res['x'][0][:, known], res['y'][0][:, known])                # X = Y bit for bit
        assert not res['map'].view(np.uint32).any() and not res['raw'][0][:, known].view(np.uint32).any()    # rho = +0 exactly
        assert res['records'][0, 1:3].tolist() == [0.0, 0.0] and res['ssim'][0] == 0
        want, big_a = so.grad(a, mask, img, img, ref, window, upstream=(1.0,))
        assert np.all(np.abs(want) <= so.grad_bound(np.zeros_like(want), big_a)) and not np.isnan(want).any()
        assert big_a[0][:, known].min() > 0 and not want[0][:, ~known].any()


def test_the_clamp_case_is_clamped():
    a, img, other = so.planted_clamp()
    assert a.shape == (1, 2, 12, 16) and img.shape == other.shape == (1, 3, 12, 16) and not a.any()
    assert np.all(np.abs(other.view(np.int32) - img.view(np.int32)) == 1)                  # one float32 step up or down
    for window, count in zip(so.WINDOWS, (129, 146, 131)):
        res = so.compute(a, None, img, other, 's', window)
        low, high = int((res['raw'] < 0).sum()), int((res['raw'] > 1).sum())
        print("window %d: raw d_c < 0 on %d channel-pixels, > 1 on %d" % (window, low, high))
        assert res['known'].all() and low >= 50 and high == 0
        assert low == count                                                                # (the CPU oracle's figure)
        assert res['map'].min() >= 0 and not np.signbit(res['map']).any()
        # without the clamp the map would differ: the GPU tier's bit-for-bit comparison sees the clamp
        assert (res['raw'].sum(1) / np.float32(3) < 0).any()


def test_hand_computed_pixel():
    """One usable pixel, zero flow on a 2 x 2 frame (positions exact), one channel: n = 1, the means are the samples and the
    moments 0."""
    f32 = np.float32
    a = np.zeros((1, 2, 2, 2), f32)
    mask = np.array([[[True, False], [False, False]]])
    img = np.array([[[[0.25, 0.0], [0.0, 0.0]]]], f32)
    other = np.array([[[[0.75, 1.0], [0.0, 0.0]]]], f32)
    res = so.compute(a, mask, img, other, 's', 3)
    c1, c2 = f32(so.C1), f32(so.C2)
    l1, l2 = (f32(2) * f32(0.75)) * f32(0.25) + c1, (f32(0.75) * f32(0.75) + f32(0.25) * f32(0.25)) + c1
    d = (f32(1) - (l1 * c2) / (l2 * c2)) * f32(0.5)
    assert res['n'][0].tolist() == [[1, 0], [0, 0]] and res['known'][0].tolist() == [[True, False], [False, False]]
    assert res['map'][0].tolist() == [[d, 0], [0, 0]] and res['map'].dtype == np.float32 and 0.19 < d < 0.21
    assert res['records'][0].tolist() == [1, d, d, 1, 0, 0, 0, 0] and res['ssim'][0] == d
    none = so.compute(a, np.zeros((1, 2, 2), bool), img, other, 's', 3)
    assert not none['records'].any() and math.isnan(none['ssim'][0]) and not none['map'].view(np.uint32).any()
    # uint8 images are read as s / 255
    ru = so.compute(a, mask, np.full((1, 1, 2, 2), 51, np.uint8), np.full((1, 1, 2, 2), 204, np.uint8), 's', 3)
    assert np.array_equal(ru['x'][0, 0, 0, 0], f32(204) / f32(255)) and np.array_equal(ru['y'][0, 0, 0, 0], f32(51) / f32(255))


# ---- host logic: the API with the native call served by the oracle -------------------------------------------------------------------
def _flow(ref='s', n=2, h=20, w=28, mask=True):
    import oflibpytorch_amd as ofl
    a, m = po.case(n, h, w, ref)[:2]
    return ofl.Flow(torch.from_numpy(a.copy()), ref, torch.from_numpy(m.copy()) if mask else None)


@pytest.mark.parametrize("ref", so.REFS)
def test_stats_keys_dtypes_shapes_and_values(ssim_native, ref):
    n, h, w = 2, 20, 28
    flow = _flow(ref)
    a, m, img, other, img_u8, other_u8 = po.case(n, h, w, ref)
    res = flow.ssim_stats(torch.from_numpy(img.copy()), torch.from_numpy(other.copy()))
    assert sorted(res) == ['count', 'fill', 'max', 'ssim', 'sum']
    assert res['count'].dtype == torch.int64 and res['count'].shape == (n,)
    for k in ('sum', 'max', 'ssim', 'fill'):
        assert res[k].dtype == torch.float64 and res[k].shape == (n,)
    want = so.compute(a, m, img, other, ref)                  # the defaults: window 3, c1 1e-4, c2 9e-4
    rec = want['records']
    assert res['count'].tolist() == rec[:, 0].tolist() and res['sum'].tolist() == rec[:, 1].tolist()
    assert res['max'].tolist() == rec[:, 2].tolist() and res['ssim'].tolist() == (rec[:, 1] / rec[:, 0]).tolist()
    assert res['fill'].tolist() == (rec[:, 3] / (rec[:, 0] * 9)).tolist() and 0 < res['fill'].min() and res['fill'].max() < 1
    loss = flow.ssim(img.copy(), other.copy())
    assert loss.tolist() == want['ssim'].tolist() and loss.dtype == torch.float32 and loss.shape == (n,)
    assert np.array_equal(so.compute(a, m, img, other, ref, 3, 1e-4, 9e-4)['map'], want['map'])
    kw = dict(window=7, c1=0.01, c2=1)
    smap = flow.ssim_map(img.copy(), other.copy(), **kw)
    assert smap.dtype == torch.float32 and np.array_equal(smap.numpy(), so.compute(a, m, img, other, ref, 7, 0.01, 1.0)['map'])
    assert flow.ssim_stats(img.copy(), other.copy(), window=5)['fill'].tolist() == \
        (lambda r: (r[:, 3] / (r[:, 0] * 25)).tolist())(so.compute(a, m, img, other, ref, 5)['records'])
    # consider_mask=False drops the mask; C-H-W images, uint8 images, one-channel and non-contiguous ones are taken
    assert flow.ssim_stats(img.copy(), other.copy(), consider_mask=False)['count'].tolist() == \
        so.compute(a, None, img, other, ref)['records'][:, 0].tolist()
    assert flow.ssim(img[0].copy(), other[0].copy()).tolist() == so.compute(a, m, img[0], other[0], ref)['ssim'].tolist()
    assert flow.ssim(img_u8.copy(), other_u8.copy()).tolist() == so.compute(a, m, img_u8, other_u8, ref)['ssim'].tolist()
    assert flow.ssim(img[:, :1].copy(), other[:, :1].copy()).tolist() == so.compute(a, m, img[:, :1], other[:, :1], ref)['ssim'].tolist()
    nhwc = [torch.from_numpy(x.copy()).contiguous(memory_format=torch.channels_last) for x in (img, other)]
    assert flow.ssim(*nhwc).tolist() == want['ssim'].tolist()


def test_adapters_on_tensors_and_arrays(ssim_native):
    import oflibpytorch_amd as ofl
    n, h, w = 2, 20, 28
    a, m, img, other, _, _ = po.case(n, h, w, 't')
    want = so.compute(a, m, img, other, 't')
    got = ofl.flow_ssim(a.copy(), img.copy(), other.copy(), 't', m.copy())
    assert got.shape == (n,) and got.tolist() == want['ssim'].tolist()
    one = ofl.flow_ssim(torch.from_numpy(a[1].copy()), torch.from_numpy(img[1].copy()), torch.from_numpy(other[1].copy()), 't',
                        torch.from_numpy(m[1].copy()))
    assert one.shape == () and float(one) == float(want['ssim'][1])
    stats = ofl.flow_ssim_stats(a[1].copy(), img[1].copy(), other[1].copy(), 't', m[1].copy())
    assert stats['count'].shape == () and int(stats['count']) == want['records'][1, 0]
    stats = ofl.flow_ssim_stats(a.copy(), img.copy(), other.copy(), 's', window=5, c2=0.5)
    assert stats['sum'].tolist() == so.compute(a, None, img, other, 's', 5, c2=0.5)['records'][:, 1].tolist()


def test_a_flow_that_requires_a_gradient_goes_through_ssim_fn(oracle_native, monkeypatch):
    import oflibpytorch_amd as ofl
    from oflibpytorch_amd import _autograd, _ssim
    calls = []

    def fake_grad(vecs, mask, img, other, flow_sign, window, c1, c2, scale):
        calls.append((flow_sign, window, c1, c2, scale.clone()))
        return torch.ones_like(vecs, dtype=torch.float32)
    monkeypatch.setattr(_ssim, "flow_ssim", so.fake_flow_ssim)
    monkeypatch.setattr(_ssim, "flow_ssim_grad", fake_grad)
    n, h, w = 2, 20, 28
    a, m, img, other, _, _ = po.case(n, h, w, 's')
    v = torch.from_numpy(a.copy()).requires_grad_(True)
    im = torch.from_numpy(img.copy()).requires_grad_(True)
    loss = ofl.Flow(v, 's', torch.from_numpy(m.copy())).ssim(im, torch.from_numpy(other.copy()), window=5, c2=0.5)
    assert loss.requires_grad and type(loss.grad_fn).__name__ == "SsimFnBackward" and issubclass(_autograd.SsimFn, torch.autograd.Function)
    loss.backward(torch.tensor([0.75, -2.0]))
    want = so.compute(a, m, img, other, 's', 5, c2=0.5)
    assert loss.tolist() == want['ssim'].tolist()
    (sign, window, c1, c2, scale), = calls
    assert (sign, window, c1, c2) == (-1.0, 5, 1e-4, 0.5)
    assert scale.dtype == torch.float32 and scale.tolist() == (np.array([0.75, -2.0]) / want['records'][:, 0]).astype(np.float32).tolist()
    assert im.grad is None and torch.equal(v.grad, torch.ones_like(v))
    with torch.no_grad():
        assert not ofl.Flow(v, 's').ssim(im, im).requires_grad and len(calls) == 1


# ---- the checks of the API, none of which needs a device ------------------------------------------------------------------------------
def test_api_checks_and_their_messages(oracle_native, monkeypatch):
    import oflibpytorch_amd as ofl
    from oflibpytorch_amd import _ssim

    def never(*args, **kw):
        raise AssertionError("the checks come before the kernel")
    monkeypatch.setattr(_ssim, "flow_ssim", never)
    monkeypatch.setattr(_ssim, "ssim", never)
    flow = _flow(n=2, h=6, w=7)
    pre = r"Error computing SSIM loss: "
    good = torch.zeros(2, 3, 6, 7)
    for call in (flow.ssim, flow.ssim_map, flow.ssim_stats):
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
            with pytest.raises(TypeError, match=pre + "Window needs to be an integer"):
                call(good, good, window=bad)
        for bad in (1, 0, -3, 4, 9, 49):
            with pytest.raises(ValueError, match=pre + "Window needs to be 3, 5 or 7"):
                call(good, good, window=bad)
        for key, name in (("c1", "C1"), ("c2", "C2")):
            for bad in (True, "1", [0.1], torch.tensor(0.1), np.ones(1)):
                with pytest.raises(TypeError, match=pre + name + " needs to be an integer or a float"):
                    call(good, good, **{key: bad})
            for bad in (0, 0.0, -1, -1e-9, 1e-60, float('nan'), float('inf'), -float('inf')):
                with pytest.raises(ValueError, match=pre + name + " needs to be finite and larger than 0"):
                    call(good, good, **{key: bad})
        for bad in (1, 0, "True", 1.0):
            with pytest.raises(TypeError, match=pre + "Consider_mask needs to be boolean"):
                call(good, good, consider_mask=bad)
    # the order: types and dtypes, shapes, the frame's size, window, c1, c2, consider_mask
    with pytest.raises(TypeError, match="same dtype"):
        flow.ssim(good, torch.zeros(2, 9, 6, 7, dtype=torch.uint8), window="x")
    with pytest.raises(ValueError, match="channels"):
        flow.ssim(good, torch.zeros(2, 9, 6, 7), window="x")
    with pytest.raises(TypeError, match="Window"):
        flow.ssim(good, good, window="x", c1=-1)
    with pytest.raises(ValueError, match="C1"):
        flow.ssim(good, good, c1=-1, c2="x")
    with pytest.raises(TypeError, match="C2"):
        flow.ssim(good, good, c2="x", consider_mask=1)
    thin = ofl.Flow(torch.zeros(2, 2, 1, 7), 't')
    with pytest.raises(ValueError, match=pre + "Flow field needs to be at least 2 pixels high and wide"):
        thin.ssim(torch.zeros(2, 3, 1, 7), torch.zeros(2, 3, 1, 7), window="x")
    with pytest.raises(ValueError, match=pre):
        ofl.flow_ssim(flow.vecs, good, good, 't', c2=-5)
    with pytest.raises(TypeError, match=pre):
        ofl.flow_ssim_stats(flow.vecs, good, good.double(), 's')


def test_the_methods_and_adapters_are_exported():
    import oflibpytorch_amd as ofl
    for name in ("ssim", "ssim_map", "ssim_stats"):
        assert callable(getattr(ofl.Flow, name))
    assert callable(ofl.flow_ssim) and callable(ofl.flow_ssim_stats)
    assert "carry no gradient" in ofl.Flow.ssim.__doc__


# ---- the C ABI: declared, exported, and every rejected argument is rejected before any launch --------------------------------------
def test_c_abi_declarations_and_argument_checks_need_no_gpu():
    from oflibpytorch_amd import _native, _ssim
    names = {"ofl_flow_ssim_workspace_bytes", "ofl_flow_ssim_f64", "ofl_flow_ssim_grad_f32"}
    assert names <= set(_native.exported_symbols())
    header = open(_native._build.HEADERS[0]).read()
    for name in names:
        assert (" %s(" % name) in header
    assert "#define OFL_SSIM_RECORD 8\n" in header and _ssim.RECORD == 8
    assert (_ssim.WINDOW, _ssim.C1, _ssim.C2) == (so.WINDOW, so.C1, so.C2) == (3, 1e-4, 9e-4)
    lib = _ssim._library()
    assert lib.ofl_version() == _native.ABI_VERSION == 36                # names were added, no signature changed
    ws = lib.ofl_flow_ssim_workspace_bytes
    # one block per tile of 64 x 16 pixels, whatever the window; 64 bytes per block record
    for window in (3, 5, 7):
        assert ws(1, 2, 2, window) == 64 and ws(3, 16, 64, window) == 3 * 64 and ws(2, 17, 65, window) == 2 * 4 * 64
        assert ws(1, 1080, 1920, window) == 68 * 30 * 64 and ws(65535, 2, 2, window) == 65535 * 64
    for bad in ((0, 4, 4, 7), (-1, 4, 4, 7), (65536, 4, 4, 7), (1, 1, 4, 7), (1, 4, 1, 7), (1, 0, 4, 7), (1, 65536, 32768, 7),
                (1, 46341, 46341, 7), (1, 4, 4, 0), (1, 4, 4, 1), (1, 4, 4, 4), (1, 4, 4, 9), (1, 4, 4, -7)):
        assert ws(*bad) == -3, bad
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(4096)      # never dereferenced: every call below is rejected first

    def fwd(flow=one, flow_bs=0, half=0, mask=null, mask_bs=0, img=one, img_bs=0, other=one, other_bs=0, chan=3, u8=0, sign=-1.0,
            window=3, c1=1e-4, c2=9e-4, wsp=one, smap=one, rec=one, n=1, h=4, w=4):
        return lib.ofl_flow_ssim_f64(flow, flow_bs, half, mask, mask_bs, img, img_bs, other, other_bs, chan, u8, sign, window, c1, c2,
                                     wsp, smap, rec, n, h, w, null)

    def bwd(flow=one, flow_bs=0, half=0, mask=null, mask_bs=0, img=one, img_bs=0, other=one, other_bs=0, chan=3, u8=0, sign=-1.0,
            window=3, c1=1e-4, c2=9e-4, scale=one, grad=one, n=1, h=4, w=4):
        return lib.ofl_flow_ssim_grad_f32(flow, flow_bs, half, mask, mask_bs, img, img_bs, other, other_bs, chan, u8, sign, window, c1,
                                          c2, scale, grad, n, h, w, null)
    odd = ctypes.c_void_p(4098)
    nan, inf = float('nan'), float('inf')
    shared = (dict(n=0), dict(n=65536), dict(n=-3), dict(h=1), dict(w=1), dict(h=0), dict(h=65536, w=32768), dict(h=46341, w=46341),
              dict(sign=0.0), dict(sign=2.0), dict(sign=-0.5), dict(sign=nan),
              dict(chan=0), dict(chan=2), dict(chan=4), dict(chan=-1), dict(u8=2), dict(u8=-1),
              dict(window=0), dict(window=1), dict(window=4), dict(window=6), dict(window=9), dict(window=-3),
              dict(c1=0.0), dict(c1=-0.1), dict(c1=nan), dict(c1=inf), dict(c1=-inf),
              dict(c2=0.0), dict(c2=-1e-9), dict(c2=nan), dict(c2=inf), dict(c2=-inf),
              dict(flow=null), dict(img=null), dict(other=null),
              dict(flow_bs=-1), dict(mask_bs=-32), dict(img_bs=-1), dict(other_bs=-8), dict(half=2), dict(half=-1),
              dict(flow=odd), dict(flow=ctypes.c_void_p(4097), half=1), dict(img=odd), dict(other=odd))
    for kw in shared + (dict(smap=null, rec=null), dict(wsp=null), dict(wsp=ctypes.c_void_p(4100)), dict(rec=ctypes.c_void_p(4100)),
                        dict(smap=odd)):
        assert fwd(**kw) == -3, kw
    for kw in shared + (dict(scale=null), dict(grad=null), dict(scale=odd), dict(grad=odd)):
        assert bwd(**kw) == -3, kw
