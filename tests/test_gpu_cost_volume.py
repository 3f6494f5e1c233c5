"""GPU tier of Flow.cost_volume (ofl_cost_volume.hip) against tests/cost_volume_oracle.py.  The bars: the warp is
bit-exact against the C oracle and every later step is a single IEEE operation in a fixed order, so the volume, d feat and d W are the
oracle's BIT FOR BIT (the bits of a NaN's payload exempt).  d other and d flow are made from d W by the warp's own backward kernels: they
are held to the float64 autograd of the definition within the bar of DESIGN.md 4 for those kernels, 2e-4 of the gradient's scale, which
proves the wiring and the `usable` gating.

Frames (cost_volume_oracle.frames()): 20 x 28; 15 x 31, 16 x 32, 17 x 33 and 33 x 65 (the kernel's 32 x 16 tile minus one, itself, plus
one, two tiles plus one: a window crosses every tile edge and the frame edge); 3 x 3 (smaller than the window of radius 4); a batch of
3 of 16 x 64.  Channel counts (channel_counts()): 1, a chunk of the kernel's channel loop minus one, the chunk, plus one, two chunks and
three."""
import functools

import numpy as np
import pytest
import torch

import cost_volume_oracle as cv
import grad_oracle64 as go

gpu = pytest.mark.gpu
FRAMES = cv.frames()
TABLE = FRAMES[0]                                    # (2, 20, 28)


def _dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


def _ids(frames):
    return ["%dx%dx%d" % f for f in frames]


def _to(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x).copy()).to(_dev())


@functools.lru_cache(maxsize=None)
def _vecs(n, h, w, ref, half):
    a = cv.case(n, h, w, ref)[0]
    a = a.astype(np.float16) if half else a
    a.setflags(write=False)
    return a


def _operands(n, c, h, w, ref, masked=True, half=False, chw=False):
    """(a, mask or None, feat, other) as arrays"""
    feat, other = cv.features(n, c, h, w, ref)
    if chw:
        feat, other = feat[0], other[n - 1]
    return _vecs(n, h, w, ref, half), (cv.case(n, h, w, ref)[1] if masked else None), feat, other


def same_bits(got, want, what):
    """Equal bit for bit; where both are NaN the payload is exempt"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    bad = (got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))
    if bad.any():
        at = tuple(int(i[0]) for i in np.nonzero(bad))
        raise AssertionError("%s: %d of %d elements differ, first at %s: got %r, expected %r" % (what, int(bad.sum()), bad.size, at,
                                                                                                 got[at], want[at]))


def _volume(ops, ref, radius):
    from oflibpytorch_amd import _cost_volume
    a, m, feat, other = ops
    return _cost_volume.flow_cost_volume(_to(a), _to(m), _to(feat), _to(other), cv.sign_of(ref), radius)


def _configs(n, h, w):
    """(masked, half, radius, channels, chw) of a frame"""
    if (n, h, w) == TABLE:
        return [(True, False, r, 3, False) for r in cv.RADII] + [(True, False, 4, c, False) for c in cv.channel_counts()] + \
               [(True, True, 4, 5, False), (True, True, 1, 2, False), (False, False, 2, 4, False), (False, True, 3, 4, False),
                (True, False, 3, 6, True), (False, False, 1, 17, True)]
    return [(True, False, 4, 3, False), (True, False, 1, 18, False), (False, True, 2, 2, False)]


# ---- bar 1: the volume ----------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n,h,w", FRAMES, ids=_ids(FRAMES))
def test_volume_against_the_oracle(n, h, w):
    import oflibpytorch_amd as ofl
    from oflibpytorch_amd import _native
    for ref in cv.REFS:
        for masked, half, radius, c, chw in _configs(n, h, w):
            ops = _operands(n, c, h, w, ref, masked, half, chw)
            what = "%d x %d '%s' masked %s half %s radius %d C %d chw %s" % (h, w, ref, masked, half, radius, c, chw)
            want = cv.compute(*ops, ref, radius)['volume']
            vol = _volume(ops, ref, radius)
            assert 'flow_cost_volume_kernel' in _native.last_kernel_name()
            assert vol.dtype == torch.float32 and vol.shape == (n, (2 * radius + 1) ** 2, h, w) and vol.is_contiguous(), what
            same_bits(vol.cpu().numpy(), want, what)
            # the API: the same bits
            a, m, feat, other = ops
            flow = ofl.Flow(_to(a), ref, _to(cv.case(n, h, w, ref)[1]))
            got = flow.cost_volume(_to(feat), _to(other), radius=radius, consider_mask=masked)
            assert not got.requires_grad
            same_bits(got.cpu().numpy(), want, what + " (Flow.cost_volume)")
        assert np.abs(want).max() > 1e-3


@gpu
def test_a_batch_gives_the_bits_of_its_images_run_singly():
    n, h, w = FRAMES[-1]
    assert n == 3
    for ref, radius, c in (('s', 4, cv.channel_counts()[3]), ('t', 2, 3)):
        a, m, feat, other = _operands(n, c, h, w, ref)
        batch = _volume((a, m, feat, other), ref, radius).cpu().numpy()
        same_bits(batch, cv.compute(a, m, feat, other, ref, radius)['volume'], "the batch")
        for i in range(n):
            one = _volume((a[i:i + 1], m[i:i + 1], feat[i:i + 1], other[i:i + 1]), ref, radius).cpu().numpy()
            same_bits(one[0], batch[i], "image %d alone against the batch" % i)


# ---- bar 2: d feat and d W ------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n,h,w", FRAMES, ids=_ids(FRAMES))
def test_feature_gradients_against_the_oracle(n, h, w):
    from oflibpytorch_amd import _cost_volume, _native
    k = cv.geometry()["kChanChunk"]
    for ref in cv.REFS:
        for masked, half, radius, c, chw in ((True, False, 4, k + 1, False), (True, False, 1, 3, False), (False, True, 1, 2, True),
                                             (True, True, 4, 2, True)):
            ops = _operands(n, c, h, w, ref, masked, half, chw)
            what = "%d x %d '%s' masked %s half %s radius %d C %d chw %s" % (h, w, ref, masked, half, radius, c, chw)
            g = cv.upstream(n, (2 * radius + 1) ** 2, h, w)
            want_f, want_w = cv.grads(*ops, ref, radius, g)
            args = tuple(_to(x) for x in ops) + (cv.sign_of(ref), radius, _to(g))
            d_feat, d_w = _cost_volume.flow_cost_volume_grad(*args)
            assert 'flow_cost_volume_grad_kernel' in _native.last_kernel_name()
            for t in (d_feat, d_w):
                assert t.dtype == torch.float32 and t.shape == (n, c, h, w) and t.is_contiguous(), what
            same_bits(d_feat.cpu().numpy(), want_f, what + ": d feat")
            same_bits(d_w.cpu().numpy(), want_w, what + ": d W")
            # one output alone: the same bits, the other not made
            only_f, none = _cost_volume.flow_cost_volume_grad(*args, want_warped=False)
            assert none is None and torch.equal(only_f, d_feat)
            none, only_w = _cost_volume.flow_cost_volume_grad(*args, want_feat=False)
            assert none is None and torch.equal(only_w, d_w)
        assert h < 9 or (np.abs(want_f).max() > 1e-3 and np.abs(want_w).max() > 1e-3)      # (the masked 3 x 3 't' case has no usable pixel)


# ---- bar 3: the whole backward through autograd -------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("chw", [False, True], ids=["nchw", "chw"])
@pytest.mark.parametrize("ref", cv.REFS)
def test_backward_against_the_float64_reference(ref, chw):
    """d feat, d other and d flow of `backward()` against torch's float64 autograd of the definition (cost_volume_oracle.torch_reference,
    the reference of the host tier) within 2e-4 of each gradient's scale; d flow is exactly 0 where the pixel is not usable."""
    import oflibpytorch_amd as ofl
    n, h, w = TABLE
    for radius, c, masked in ((4, 5, True), (1, 3, False)):
        a, m, feat, other = _operands(n, c, h, w, ref, masked, False, chw)
        g = cv.upstream(n, (2 * radius + 1) ** 2, h, w)
        v, ft, ot = (_to(x).requires_grad_(True) for x in (a, feat, other))
        vol = ofl.Flow(v, ref, _to(cv.case(n, h, w, ref)[1])).cost_volume(ft, ot, radius=radius, consider_mask=masked)
        assert vol.requires_grad and type(vol.grad_fn).__name__ == "CostVolumeFnBackward"
        res = cv.compute(a, m, feat, other, ref, radius)
        same_bits(vol.detach().cpu().numpy(), res['volume'], "the forward of the autograd route")
        vol.backward(_to(g))
        want = cv.torch_reference(a, res['usable'], feat, other, ref, radius, g)
        for name, got, ref64 in (("feat", ft.grad, want['d_feat']), ("other", ot.grad, want['d_other']), ("flow", v.grad, want['d_flow'])):
            got = got.cpu().numpy()
            scale = np.abs(ref64).max()
            err = np.abs(got - ref64).max()
            print("'%s' radius %d chw %s d %s: max error %.3e of a scale %.3e" % (ref, radius, chw, name, err, scale))
            assert got.dtype == np.float32 and got.shape == ref64.shape and scale > 1e-2, name
            assert err <= 2e-4 * scale, name
        unusable = ~np.broadcast_to(res['usable'][:, None], (n, 2, h, w))
        assert not v.grad.cpu().numpy()[unusable].any() and unusable.mean() > 0.1
    # a gradient of `feat` alone: bit for bit the oracle's, summed over the batch by torch for a C-H-W tensor
    ft2 = _to(feat).requires_grad_(True)
    ofl.Flow(_to(a), ref).cost_volume(ft2, _to(other), radius=1).backward(_to(g))
    want_f = cv.grads(a, None, feat, other, ref, 1, g)[0]
    if chw:
        assert n == 2
        same_bits(ft2.grad.cpu().numpy(), want_f[0] + want_f[1], "d feat alone, summed over the batch")
    else:
        same_bits(ft2.grad.cpu().numpy(), want_f, "d feat alone")


# ---- the planted case ---------------------------------------------------------------------------------------------------------------
@gpu
def test_planted_shift_peaks_at_the_centre():
    """`other` is `feat` shifted by (2, -1) and the flow is that shift everywhere, on a 17 x 33 frame (h - 1 and w - 1 powers of two:
    the positions are exact), no mask: where the sample is inside the frame W' = feat bit for bit, the centre entry is sum_c feat^2 / C
    bit for bit and the arg-max over o."""
    n, c, h, w, radius = 1, 32, 17, 33, 4
    feat, other = (x.copy() for x in cv.features(n, c, h, w, 's'))
    other[:, :, :h - 1, 2:] = feat[:, :, 1:, :w - 2]                                          # other(p) = feat(p - (2, -1))
    a = np.zeros((n, 2, h, w), np.float32)
    a[:, 0], a[:, 1] = 2.0, -1.0
    res = cv.compute(a, None, feat, other, 's', radius)
    usable = res['usable']
    assert usable[0, 1:, :w - 2].all() and not usable[0, 0].any() and not usable[0, :, w - 2:].any()
    assert np.array_equal(res['warped'][:, :, 1:, :w - 2], feat[:, :, 1:, :w - 2])
    vol = _volume((a, None, feat, other), 's', radius).cpu().numpy()
    same_bits(vol, res['volume'], "the planted shift")
    acc = np.zeros((n, h, w), np.float32)
    for k in range(c):
        acc = acc + feat[:, k] * feat[:, k]
    centre = (2 * radius + 1) ** 2 // 2
    same_bits(vol[:, centre][usable], (acc / np.float32(c))[usable], "the centre entry")
    assert (vol.argmax(1)[usable] == centre).all() and vol[:, centre][usable].min() > 0.1


# ---- non-finite values ----------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("ref", cv.REFS)
def test_non_finite_values_stay_where_the_definition_puts_them(ref):
    n, h, w = TABLE
    c, radius = 3, 4
    a, m, feat, other = _operands(n, c, h, w, ref)
    # the pixels of `other` that are no tap of any usable sample (a tap inside the frame is read whatever its weight) and are masked
    # themselves: a NaN and an inf there are under a masked pixel and out of every usable sample
    taps = go.warp_taps(a, n, cv.sign_of(ref))
    usable = cv.warped(a, m, other, ref)[1]
    touched = np.zeros((n, h * w), bool)
    for j in range(4):
        ok = taps.ok[j] & usable
        bi, yy, xx = np.nonzero(ok)
        touched[bi, taps.idx[j][ok]] = True
    free = ~touched.reshape(n, h, w) & ~m
    assert free.sum((1, 2)).min() >= 2
    other = other.copy()
    for i in range(n):
        (y0, x0), (y1, x1) = np.argwhere(free[i])[:2]
        other[i, 0, y0, x0], other[i, 1, y1, x1] = np.nan, np.inf
    want = cv.compute(a, m, feat, other, ref, radius)['volume']
    assert np.isfinite(want).all()
    vol = _volume((a, m, feat, other), ref, radius).cpu().numpy()
    assert np.isfinite(vol).all()
    same_bits(vol, want, "NaN and inf in `other` out of every usable sample")
    # a NaN in feat: exactly the D entries of its pixel
    feat = feat.copy()
    feat[1, 2, 7, 11] = np.nan
    vol = _volume((a, m, feat, other), ref, radius).cpu().numpy()
    expect = np.zeros((n, 81, h, w), bool)
    expect[1, :, 7, 11] = True
    assert np.array_equal(np.isnan(vol), expect)
    same_bits(vol, cv.compute(a, m, feat, other, ref, radius)['volume'], "a NaN in feat")
