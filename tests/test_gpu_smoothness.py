"""GPU tier of Flow.smoothness / smoothness_map / smoothness_stats (ofl_smoothness.hip) against tests/smoothness_oracle.py (DESIGN.md
3.19).  Without an image the map is the oracle's bit for bit and counts and max are exact; with an image every term-bearing map element
is within 4 float32 ulp (the float64 exp of device and NumPy each within 1 ulp of float64 and rounded once: the weight differs by at most
1 ulp, the product by 2, the sum of two such non-negative terms by 3, plus a margin of 1); every float64 sum is within count * 2^-52
relative of the exact sum of the oracle's terms (the terms are not negative, so this bounds ANY summation order), plus 2^-22 with an
image; the gradient is within 2^-22 A + ulp32(want) per element, A being the sum of the absolute contributions.

Frames (smoothness_oracle.FRAMES): 1 x 1 (no term), 1 x 5 and 5 x 1 (one direction), 2 x 2 (order 2 has no term), 3 x 3 (order 2's single
centre term), 5 x 7 (scalar form), 37 x 53 (odd, 5 blocks), 96 x 136 (16-byte form, 24 blocks), the kernel's tile 8 x 128 and 9 x 129,
2 x 1080 x 1920 (2025 tiles for the 256 forward and 1024 backward blocks an image gets at most: every block loops)."""
import functools

import numpy as np
import pytest
import torch

import smoothness_oracle as so

gpu = pytest.mark.gpu
LARGE = so.FRAMES[-1]
ORDERS = (1, 2)
IMAGES = {"f32c3": dict(c=3), "u8c3": dict(c=3, u8=True), "f32c1": dict(c=1), "chw": dict(c=3, batch=False)}
ALPHA = 10.0
MAP_ULPS, MAX_ULPS = 4, 2     # with an image: the bars of a map element and of the record's maximum, float32 ulp


def _dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


def _ids(frames):
    return ["%dx%dx%d" % f for f in frames]


@functools.lru_cache(maxsize=None)
def _vecs(n, h, w, half):
    f, _ = so.case(n, h, w)
    f = f.astype(np.float16) if half else f
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def _oracle(n, h, w, order, eps, half=False, masked=True, kind=None):
    img = None if kind is None else so.image(n, h, w, **IMAGES[kind])
    return so.compute(_vecs(n, h, w, half), so.case(n, h, w)[1] if masked else None, img, order, ALPHA, eps)


@functools.lru_cache(maxsize=None)
def _grad_oracle(n, h, w, order, eps, kind):
    img = None if kind is None else so.image(n, h, w, **IMAGES[kind])
    return so.grad(_vecs(n, h, w, False), so.case(n, h, w)[1], img, order, ALPHA, eps, so.UPSTREAM)


def _flow(n, h, w, half=False, requires_grad=False):
    import oflibpytorch_amd as ofl
    v = torch.from_numpy(_vecs(n, h, w, half).copy()).to(_dev())
    if requires_grad:
        v.requires_grad_(True)
    return ofl.Flow(v, 't', torch.from_numpy(so.case(n, h, w)[1].copy()).to(_dev())), v


def _image(n, h, w, kind):
    return None if kind is None else torch.from_numpy(so.image(n, h, w, **IMAGES[kind]).copy()).to(_dev())


def _record(flow, img, order, eps, consider_mask=True):
    s = flow.smoothness_stats(img, order=order, alpha=ALPHA, eps=eps, consider_mask=consider_mask)
    return s, np.stack([s[k].cpu().numpy().astype(np.float64) for k in ('count_x', 'count_y', 'sum_x', 'sum_y', 'max')], 1)


def _ulps(got, want):
    """The distance in float32 steps of non-negative finite values"""
    assert got.dtype == np.float32 and want.dtype == np.float32 and (got >= 0).all() and (want >= 0).all()
    return np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))


# ---- the inputs -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("n,h,w", [f for f in so.FRAMES if f[1] >= 5 and f[2] >= 7], ids=lambda v: str(v))
def test_the_inputs_show_valid_invalid_and_zero_terms(n, h, w, order):
    """On the oracle alone: in every image of every frame of at least 5 x 7 some terms are valid and some are not, in both directions,
    and with eps = 0 at least one valid term is exactly 0 (the constant patch)."""
    f, mask = so.case(n, h, w)
    for axis in ('x', 'y'):
        t = so.direction_terms(f, mask, None, order, ALPHA, 0.0, axis)
        for i in range(n):
            count = int(t['ok'][i].sum())
            zeros = int((t['t'][i][t['ok'][i]] == 0).sum())
            print("%d x %d order %d image %d: count_%s %d of %d, %d valid terms exactly 0" % (h, w, order, i, axis, count, h * w, zeros))
            assert 0 < count < h * w and zeros >= 1
    if order == 1 and h * w >= 37 * 53:
        # both ends of exp are seen: across the step g is about 0.8 (weight e^-8 and less), between equal samples it is near 0
        wgt = so.direction_terms(f, mask, so.image(n, h, w), order, ALPHA, 0.0, 'x')
        print("weights from %.3g to %.3g" % (wgt['w'][wgt['ok']].min(), wgt['w'][wgt['ok']].max()))
        assert wgt['w'][wgt['ok']].min() < 1e-3 and wgt['w'][wgt['ok']].max() > 0.3


# ---- bar 1: without an image ----------------------------------------------------------------------------------------------------------
def _plain_configs(frame):
    if frame == LARGE:
        return [(1, 1e-3, False, True), (2, 0.0, True, False)]
    return [(o, e, hf, m) for o in ORDERS for e in (1e-3, 0.0) for hf in (False, True) for m in (True, False)]


@gpu
@pytest.mark.parametrize("n,h,w", so.FRAMES, ids=_ids(so.FRAMES))
def test_without_an_image_the_map_is_bit_exact(n, h, w):
    from oflibpytorch_amd import _native
    worst = 0.0
    for order, eps, half, masked in _plain_configs((n, h, w)):
        ref = _oracle(n, h, w, order, eps, half, masked)
        flow, _ = _flow(n, h, w, half)
        smap = flow.smoothness_map(order=order, eps=eps, consider_mask=masked)
        assert 'smoothness' in _native.last_kernel_name()
        assert smap.dtype == torch.float32 and smap.shape == (n, h, w)
        what = "order %d eps %g half %s masked %s" % (order, eps, half, masked)
        assert np.array_equal(smap.cpu().numpy().view(np.uint32), ref['map'].view(np.uint32)), what      # +0 where no term is valid
        stats, rec = _record(flow, None, order, eps, masked)
        assert 'smoothness' in _native.last_kernel_name()
        want = ref['records']
        assert stats['count_x'].dtype == torch.int64 and stats['sum_x'].dtype == torch.float64
        assert np.array_equal(rec[:, :2], want[:, :2]) and np.array_equal(rec[:, 4], want[:, 4]), what
        for k in (2, 3):
            rel = np.abs(rec[:, k] - want[:, k]) / np.maximum(want[:, k], 1e-300)
            worst = max(worst, float((rel / np.maximum(want[:, k - 2], 1) / 2.0 ** -52).max()))
            assert np.all(np.abs(rec[:, k] - want[:, k]) <= want[:, k - 2] * 2.0 ** -52 * want[:, k]), (what, rec[:, k], want[:, k])
    print("%d x %d: map bit for bit; largest sum error %.3f of the bound count * 2^-52" % (h, w, worst))


# ---- bar 2: with an image -------------------------------------------------------------------------------------------------------------
def _image_configs(frame):
    if frame == LARGE:
        return [(1, "f32c3"), (2, "u8c3")]
    return [(o, k) for o in ORDERS for k in sorted(IMAGES)]


@gpu
@pytest.mark.parametrize("n,h,w", so.FRAMES, ids=_ids(so.FRAMES))
def test_with_an_image_the_map_is_within_4_ulp(n, h, w):
    from oflibpytorch_amd import _native
    worst_map, worst_sum, worst_max = 0, 0.0, 0
    for order, kind in _image_configs((n, h, w)):
        ref = _oracle(n, h, w, order, 1e-3, False, True, kind)
        flow, _ = _flow(n, h, w)
        img = _image(n, h, w, kind)
        what = "order %d image %s" % (order, kind)
        got = flow.smoothness_map(img, order=order, alpha=ALPHA).cpu().numpy()
        assert 'smoothness' in _native.last_kernel_name()
        bearing = ref['x']['ok'] | ref['y']['ok']
        assert not got[~bearing].view(np.uint32).any(), what                              # exactly +0
        if bearing.any():
            d = _ulps(got[bearing], ref['map'][bearing])
            worst_map = max(worst_map, int(d.max()))
            assert d.max() <= MAP_ULPS, (what, int(d.max()))
        _, rec = _record(flow, img, order, 1e-3)
        want = ref['records']
        assert np.array_equal(rec[:, :2], want[:, :2]), what
        for k in (2, 3):
            bound = (2.0 ** -22 + want[:, k - 2] * 2.0 ** -52) * want[:, k]
            err = np.abs(rec[:, k] - want[:, k])
            worst_sum = max(worst_sum, float((err / np.maximum(bound, 1e-300)).max()))
            assert np.all(err <= bound), (what, rec[:, k], want[:, k])
        dm = _ulps(rec[:, 4].astype(np.float32), want[:, 4].astype(np.float32))
        assert np.array_equal(rec[:, 4].astype(np.float32).astype(np.float64), rec[:, 4])    # a float32 value
        worst_max = max(worst_max, int(dm.max()))
        assert dm.max() <= MAX_ULPS, what
    print("%d x %d: largest map error %d ulp (bar 4), sum error %.3g of its bound, max error %d ulp (bar 2)" % (h, w, worst_map, worst_sum,
                                                                                                              worst_max))


# ---- bar 3: the loss is the quotient of the call's own record ----------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n,h,w", so.SMALL, ids=_ids(so.SMALL))
def test_the_loss_is_the_quotient_of_its_own_record(n, h, w):
    from oflibpytorch_amd import _native
    for order in ORDERS:
        for kind in (None, "f32c3"):
            flow, _ = _flow(n, h, w)
            img = _image(n, h, w, kind)
            stats, rec = _record(flow, img, order, 1e-3)
            loss = flow.smoothness(img, order=order, alpha=ALPHA)
            assert 'smoothness' in _native.last_kernel_name()
            assert loss.dtype == torch.float32 and loss.shape == (n,) and not loss.requires_grad
            with np.errstate(invalid='ignore', divide='ignore'):
                want = ((rec[:, 2] + rec[:, 3]) / (rec[:, 0] + rec[:, 1])).astype(np.float32)
            assert np.array_equal(loss.cpu().numpy().view(np.uint32), want.view(np.uint32)), (order, kind)
            assert np.array_equal(stats['smoothness'].cpu().numpy().astype(np.float32).view(np.uint32), want.view(np.uint32))
            if h * w == 1 or (order == 2 and h < 3 and w < 3):
                assert np.isnan(want).all() and not rec.any()


# ---- bar 4: an image's bits do not depend on the batch, its position in it, or the run ----------------------------------------------
@gpu
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("n,h,w", [(3, 5, 7), (3, 37, 53), (3, 96, 136)], ids=_ids([(3, 5, 7), (3, 37, 53), (3, 96, 136)]))
def test_batch_independence_and_reproducibility(n, h, w, order):
    import oflibpytorch_amd as ofl
    from oflibpytorch_amd import _smoothness
    f, m = (torch.from_numpy(a.copy()).to(_dev()) for a in so.case(n, h, w))
    img = _image(n, h, w, "f32c3")
    up = torch.tensor(so.UPSTREAM, device=_dev())

    def run(idx):
        idx = torch.tensor(idx, device=_dev())
        v = f[idx].clone().requires_grad_(True)
        rec, smap = _smoothness.flow_smoothness(v.detach(), m[idx].clone(), img[idx].clone(), order, ALPHA, 1e-3, want_map=True)
        loss = ofl.Flow(v, 't', m[idx].clone()).smoothness(img[idx].clone(), order=order, alpha=ALPHA)
        (loss * up[idx]).sum().backward()
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in (rec, smap, loss.detach(), v.grad)]
    whole = run([0, 1, 2])
    again = run([0, 1, 2])
    for a, b in zip(whole, again):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))                          # two runs, gradient included
    moved = run([2, 0, 1])
    for i in range(n):
        alone = run([i])
        for a, b, c in zip(whole, alone, moved):
            j = (i + 1) % 3                                                                 # where image i sits in `moved`
            assert np.array_equal(a[i:i + 1].view(np.uint8), b[0:1].view(np.uint8)), i
            assert np.array_equal(a[i:i + 1].view(np.uint8), c[j:j + 1].view(np.uint8)), i


# ---- bar 5: the gradient ----------------------------------------------------------------------------------------------------------------
def _grad_configs(frame):
    if frame == LARGE:
        return [(2, "f32c3")]
    return [(o, k) for o in ORDERS for k in (None, "f32c3", "u8c3")]


@gpu
@pytest.mark.parametrize("n,h,w", so.FRAMES, ids=_ids(so.FRAMES))
def test_gradient_against_the_float64_oracle(n, h, w):
    from oflibpytorch_amd import _native
    worst = 0.0
    for order, kind in _grad_configs((n, h, w)):
        for eps in ((1e-3,) if (n, h, w) == LARGE else (1e-3, 0.0)):
            want, a, read = _grad_oracle(n, h, w, order, eps, kind)
            flow, v = _flow(n, h, w, requires_grad=True)
            img = _image(n, h, w, kind)
            if img is not None and img.dtype == torch.float32:
                img.requires_grad_(True)
            loss = flow.smoothness(img, order=order, alpha=ALPHA, eps=eps)
            assert loss.requires_grad
            (loss * torch.tensor(so.UPSTREAM[:n], device=_dev())).sum().backward()
            assert 'smoothness' in _native.last_kernel_name()
            assert img is None or img.grad is None                                          # guidance: no gradient
            got = v.grad.cpu().numpy()
            assert got.dtype == np.float32 and got.shape == (n, 2, h, w)
            what = "order %d image %s eps %g" % (order, kind, eps)
            assert not got[~np.broadcast_to(read[:, None], got.shape)].view(np.uint32).any(), what       # exactly 0 where nothing reads
            if h * w == 1:
                assert not got.view(np.uint32).any() and bool(torch.isnan(loss).all())
            assert h * w < 35 or (want != 0).any(), what                                      # the oracle's gradient is not vacuous
            bound = so.grad_bound(want, a)
            err = np.abs(got.astype(np.float64) - want.astype(np.float64))
            worst = max(worst, float((err / bound).max()))
            assert np.all(err <= bound), (what, float((err / bound).max()))
    print("%d x %d: largest gradient error %.3f of the bound 2^-22 A + ulp32" % (h, w, worst))
