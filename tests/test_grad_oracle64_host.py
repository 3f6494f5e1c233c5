"""CPU tier of the per-element gradient bar (tests/grad_oracle64.py).  No GPU.

  1. The oracle against double precision: torch float64 autograd through a ten-line bilinear gather / scatter written with torch
     ops, on the oracle's own float32 positions -- agreement to 1e-12 of the gradient's scale.
  2. The reference alone meets the bar: ATen's float32 CPU autograd through the restated op sequences (tests/grad_ref.py:
     RFlow.apply 't' and 's', track, and the splat with a density gradient and explicit end points) stays within
     (k + r) * 2^-24 * M + (k + r) * 2^-126 of the oracle on EVERY element, on every input family and shape of
     tests/grad_cases64.py, with the r of grad_oracle64.R (<= 8).  This licenses the bar and r.  (Largest err / bound met: 0.43.)
  3. Sharpness: small corruptions of ATen's result that the per-tensor GRAD_RTOL bar accepts and the per-element bar rejects.
     Kept: one element scaled by 1 + 3e-5 (all six outputs); the smallest-weight tap of one border pixel dropped (five outputs:
     the per-element bar is exceeded 5 to 10^6 times over).  Not kept, because one of the two assertions does not hold:
       * the dropped tap on warp grad_flow: a tap's term there is value * (the OTHER axis' fraction) * g, not small when the tap's
         weight is, and at the pixel chosen the old bar rejects it too;
       * a division replaced by x * float32(1 / d) (the / size_m1 of warp grad_flow and sampler grad_pts, applied to ATen's
         result; 13 % / 18 % of the elements change): at most 1.5 ulp of the element, inside a bar that grants k + r >= 5
         roundings of M -- the per-element bar accepts it (err / bound 0.21 / 0.26 measured, 0.14 / 0.19 without it), as it must
         accept ATen's own differently rounded chain.  What the bar does see of a cheaper division is an error that grows past
         (k + r) * 2^-24 of M, e.g. a reciprocal of reduced precision or a 16-bit intermediate (2^-11: 10^3 times the bound).
"""
import numpy as np
import pytest
import torch

import case_runner
import grad_cases64 as gc
import grad_oracle64 as go
import grad_ref
from grad_ref import RFlow

POS_RTOL = 5e-4                       # the old bar of position gradients (tests/test_gpu_gradients.py)
CHANNELS = (1, 2, 3, 5)
DEN_MIN = float(np.float32(1e-3))


# ------------------------------------------------------------------------------------------------
# 1. the oracle against float64 autograd
# ------------------------------------------------------------------------------------------------
def _corners64(px, py, h, w):
    """The four corners of float64 positions: (weight, flat offset) with weight 0 outside the frame."""
    x0, y0 = torch.floor(px.detach()), torch.floor(py.detach())
    for dy in (0, 1):
        for dx in (0, 1):
            xi, yi = x0 + dx, y0 + dy
            inside = (xi >= 0) & (xi <= w - 1) & (yi >= 0) & (yi <= h - 1)
            wgt = (1 - (px - xi).abs()) * (1 - (py - yi).abs()) * inside
            yield wgt, (yi.clamp(0, h - 1) * w + xi.clamp(0, w - 1)).long()


def _gather64(src, px, py):
    n, c, h, w = src.shape
    flat = src.flatten(2)
    return sum(wgt.unsqueeze(1) * torch.gather(flat, 2, idx.flatten(1).unsqueeze(1).expand(-1, c, -1)).view((n, c) + px.shape[1:])
               for wgt, idx in _corners64(px, py, h, w))


def _splat64(px, py, data, mask):
    n, c, h, w = data.shape
    acc, den = torch.zeros(n, c, h * w, dtype=torch.float64), torch.zeros(n, h * w, dtype=torch.float64)
    for wgt, idx in _corners64(px, py, h, w):
        wgt = (wgt * mask).flatten(1)
        den = den.scatter_add(1, idx.flatten(1), wgt)
        acc = acc.scatter_add(2, idx.flatten(1).unsqueeze(1).expand(-1, c, -1), wgt.unsqueeze(1) * data.flatten(2))
    return (acc / den.clamp_min(DEN_MIN).unsqueeze(1)).view(n, c, h, w), den.view(n, h, w)


def _same64(got, ref, what):
    val = ref[0]
    err, scale = float(np.abs(got.numpy() - val).max()), float(np.abs(val).max())
    assert scale > 0 and err <= 1e-12 * scale, "%s: max |diff| %.3g against a scale of %.3g" % (what, err, scale)


def _leaves_every_border(px, py, h, w):
    return bool((px < 0).any() and (px > w - 1).any() and (py < 0).any() and (py > h - 1).any()
                and (px != np.floor(px)).all() and (py != np.floor(py)).all())


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_warp_oracle_equals_float64_autograd(sign):
    n, c, h, w = 2, 3, 11, 13
    g = torch.Generator().manual_seed(1)
    f = ((torch.rand(n, 2, h, w, generator=g) - 0.5) * 9).contiguous()
    src, gout = gc.image(1, c, h, w), gc.upstream(n, c, h, w)              # a batch-1 source: its gradient sums over the batch
    sx, sy = go.warp_positions(f.numpy(), n, sign)
    assert _leaves_every_border(sx, sy, h, w)
    px, py = torch.tensor(sx, dtype=torch.float64, requires_grad=True), torch.tensor(sy, dtype=torch.float64, requires_grad=True)
    s64 = src.double().requires_grad_()
    (_gather64(s64.expand(n, -1, -1, -1), px, py) * (gout.double() * gc.G_SCALE)).sum().backward()
    ref = go.warp_grad(f.numpy(), src.numpy(), gout.numpy(), sign, gc.G_SCALE)
    _same64(s64.grad, ref['grad_src'], "grad_src")
    _same64(-sign * torch.stack([px.grad, py.grad], 1), ref['grad_flow'], "grad_flow")   # d position / d flow = -flow_sign
    k = ref['grad_src'][2]
    assert k.min() == 0 and k.max() > 4                                     # pixels no tap reaches, and pixels many reach


def test_splat_oracle_equals_float64_autograd():
    n, c, h, w = 2, 5, 11, 13
    g = torch.Generator().manual_seed(2)
    xs = (torch.rand(n, h, w, generator=g) * (w + 3) - 2).contiguous()
    ys = (torch.rand(n, h, w, generator=g) * (h + 3) - 2).contiguous()
    assert _leaves_every_border(xs.numpy(), ys.numpy(), h, w)
    data, gout, gden, m = gc.image(n, c, h, w), gc.upstream(n, c, h, w), gc.upstream(n, 1, h, w, 1)[:, 0], gc.holes(n, h, w)
    px, py, d64 = xs.double().requires_grad_(), ys.double().requires_grad_(), data.double().requires_grad_()
    out, den = _splat64(px, py, d64, m)
    assert bool((den.detach() < DEN_MIN).any()) and bool((den.detach() > 1).any())   # both sides of the clamp
    ((out * gout.double()).sum() + (den * gden.double()).sum()).backward()
    ref = go.splat_grad(None, data.numpy(), out.detach().numpy(), den.detach().numpy(), gout.numpy(), gden.numpy(), m.numpy(),
                        False, xs=xs.numpy(), ys=ys.numpy())
    _same64(d64.grad, ref['grad_data'], "grad_data")
    _same64(torch.stack([px.grad, py.grad], 1), ref['grad_xy'], "grad_xy")


def test_sampler_oracle_equals_float64_autograd():
    n, h, w = 2, 11, 13
    f = gc.flow('smooth', n, h, w)
    pts = gc.points(n, h, w)
    pts = pts[:, ~torch.isnan(pts[0]).any(-1)].contiguous()                 # (NaN rows: section 2, against ATen)
    pts = pts + (pts == torch.floor(pts)) * 0.37                            # no integers here
    gout = torch.randn(n, pts.shape[1], 2, generator=torch.Generator().manual_seed(3))
    _, T = go.pts_taps((h, w), pts.numpy(), n)
    sx32, sy32 = go.unnormalise(pts[..., 1].numpy(), w), go.unnormalise(pts[..., 0].numpy(), h)
    assert _leaves_every_border(sx32, sy32, h, w)
    p64, f64 = pts.double().requires_grad_(), f.double().requires_grad_()
    # the float32 positions, with the derivative 1 of normalise / un-normalise with respect to the point
    px = torch.tensor(sx32, dtype=torch.float64) + (p64[..., 1] - p64[..., 1].detach())
    py = torch.tensor(sy32, dtype=torch.float64) + (p64[..., 0] - p64[..., 0].detach())
    val = _gather64(f64, px, py)                                            # [n, 2, m]: (u, v)
    ((torch.stack([p64[..., 0] + val[:, 1], p64[..., 1] + val[:, 0]], -1)) * gout.double()).sum().backward()
    ref = go.sample_pts_grad(f.numpy(), pts.numpy(), gout.numpy())
    _same64(f64.grad, ref['grad_flow'], "grad_flow")
    _same64(p64.grad, ref['grad_pts'], "grad_pts")


def test_positions_are_the_forward_oracles():
    """The NumPy restatement of the float32 position chain against oracle/ (the forward's own): bit for bit."""
    from oracle import oracle
    n, h, w = 2, 37, 70
    f = gc.flow('shift_pos', n, h, w).numpy()
    gy, gx = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing='ij')
    coords = np.stack([gx[None] - f[:, 0], gy[None] - f[:, 1]], -1)
    nc = oracle.normalise_coords(coords, (h, w))
    sx, sy = go.warp_positions(f, n, 1.0)
    assert np.array_equal(sx, (nc[..., 0] + np.float32(1)) * (np.float32(w - 1) / np.float32(2)))
    assert np.array_equal(sy, (nc[..., 1] + np.float32(1)) * (np.float32(h - 1) / np.float32(2)))
    x, y = oracle.flow_endpoints(f, 's')
    assert np.array_equal(x, np.float32(1) * f[:, 0] + gx[None]) and np.array_equal(y, np.float32(1) * f[:, 1] + gy[None])


# ------------------------------------------------------------------------------------------------
# 2. ATen float32 autograd inside the bar, every element
# ------------------------------------------------------------------------------------------------
def _inside(got, ref, key, what):
    assert go.R[key] <= 8
    ex = go.excess(got, ref, go.R[key])
    assert ex <= 1.0, "%s: |got - ref64| reaches %.3g of the per-element bound (r = %d)" % (what, ex, go.R[key])
    return ex


def aten_warp(f0, img, wts, sign):
    """ATen's gradients of RFlow.apply 't' (flow_sign -1: through the negated flow) as the kernel reports them."""
    fa, ia = (f0 * sign).clone().requires_grad_(), img.clone().requires_grad_()
    (RFlow(fa, 't').apply(ia) * wts * gc.G_SCALE).sum().backward()
    return ia.grad.numpy(), fa.grad.numpy() * sign


def aten_splat(f0, img, wts, m):
    """ATen's gradients of RFlow.apply 's' and the forward outputs the backward kernel is handed."""
    fb, ib = f0.clone().requires_grad_(), img.clone().requires_grad_()
    out = RFlow(fb, 's', m).apply(ib)
    (out * wts * gc.G_SCALE).sum().backward()
    x, y = grad_ref.get_flow_endpoints(f0, 's')
    zero = torch.sum(grad_ref.threshold_vectors(f0) == 0, dim=1) == 2
    _, den = grad_ref.grid_from_unstructured_data(x, y, img, ~zero if m is None else m & ~zero)
    return ib.grad.numpy(), fb.grad.numpy(), out.detach().numpy(), den.numpy()


def point_weights(n, m, seed=0):
    g = torch.Generator().manual_seed(6000 + seed)
    return (torch.randn(n, m, 2, generator=g) * torch.logspace(-4, 0, m).view(1, m, 1)).contiguous()


def aten_track(f0, p0, wts):
    fa, pa = f0.clone().requires_grad_(), p0.clone().requires_grad_()
    (RFlow(fa, 's').track(pa) * wts).sum().backward()
    return fa.grad.numpy(), pa.grad.numpy()


def reduce_rows(ref, rows):
    """The oracle's per-image rows summed over the batch, for points broadcast over it."""
    return ref if rows == ref[0].shape[0] else tuple(a.sum(0, keepdims=True) for a in ref)


@pytest.mark.parametrize("shape", gc.SHAPES)
@pytest.mark.parametrize("family", gc.FAMILIES)
def test_aten_warp_is_inside_the_bar(family, shape):
    n, h, w = shape
    f0 = gc.flow(family, n, h, w)
    for c in CHANNELS:
        for sign in (1.0, -1.0):
            for bcast in (False, True):                                     # a batch-1 image under N flows
                img, wts = gc.image(1 if bcast else n, c, h, w), gc.upstream(n, c, h, w)
                gs, gf = aten_warp(f0, img, wts, sign)
                ref = go.warp_grad(f0.numpy(), img.numpy(), wts.numpy(), sign, gc.G_SCALE)
                what = "%s %s C=%d sign %+d bcast %s" % (family, shape, c, sign, bcast)
                _inside(gs, ref['grad_src'], 'warp.grad_src', what + ": grad_src")
                _inside(gf, ref['grad_flow'], 'warp.grad_flow', what + ": grad_flow")


@pytest.mark.parametrize("shape", gc.SHAPES)
@pytest.mark.parametrize("family", gc.FAMILIES)
def test_aten_splat_is_inside_the_bar(family, shape):
    n, h, w = shape
    f0 = gc.flow(family, n, h, w)
    for c in CHANNELS:
        for m in (None, gc.holes(n, h, w)):
            img, wts = gc.image(n, c, h, w), gc.upstream(n, c, h, w)
            gd, gxy, out, den = aten_splat(f0, img, wts, m)
            ref = go.splat_grad(f0.numpy(), img.numpy(), out, den, (wts * gc.G_SCALE).numpy(), None,
                                None if m is None else m.numpy(), True, 1.0)
            what = "%s %s C=%d holes %s" % (family, shape, c, m is not None)
            _inside(gd, ref['grad_data'], 'splat.grad_data', what + ": grad_data")
            _inside(gxy, ref['grad_xy'], 'splat.grad_xy', what + ": grad_xy")


@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("family", gc.FAMILIES)
def test_aten_splat_with_density_gradient_is_inside_the_bar(family, sign):
    """The splat itself (utils.py:1098-1144): a gradient arriving through the density output too, no occlusion rule, once along
    flow_sign * flow and once at explicit end points."""
    n, c, h, w = 2, 5, 37, 70
    f0, m = gc.flow(family, n, h, w), gc.holes(n, h, w)
    img, wts, wden = gc.image(n, c, h, w), gc.upstream(n, c, h, w), gc.upstream(n, 1, h, w, 1)[:, 0]
    x0 = sign * f0[:, 0] + torch.arange(w, dtype=torch.float32)[None, None, :]
    y0 = sign * f0[:, 1] + torch.arange(h, dtype=torch.float32)[None, :, None]
    xa, ya, ia = x0.clone().requires_grad_(), y0.clone().requires_grad_(), img.clone().requires_grad_()
    out, den = grad_ref._ref_splat(xa, ya, ia, m)
    ((out * wts * gc.G_SCALE).sum() + (den * wden).sum()).backward()
    args = (img.numpy(), out.detach().numpy(), den.detach().numpy(), (wts * gc.G_SCALE).numpy(), wden.numpy(), m.numpy(), False)
    for ref in (go.splat_grad(f0.numpy(), *args, flow_sign=sign), go.splat_grad(None, *args, xs=x0.numpy(), ys=y0.numpy())):
        _inside(ia.grad.numpy(), ref['grad_data'], 'splat.grad_data', family + ": grad_data")
        _inside(torch.stack([xa.grad, ya.grad], 1).numpy(), ref['grad_xy'], 'splat.grad_xy', family + ": grad_xy")


@pytest.mark.parametrize("shape", gc.SHAPES)
@pytest.mark.parametrize("family", gc.FAMILIES)
def test_aten_track_is_inside_the_bar(family, shape):
    n, h, w = shape
    f0 = gc.flow(family, n, h, w)
    for rows in sorted({1, n}):                                             # batch-1 points against a batch-N flow, and N-M-2
        p0, wts = gc.points(rows, h, w), point_weights(n, 257)
        gf, gp = aten_track(f0, p0, wts)
        ref = go.sample_pts_grad(f0.numpy(), p0.numpy(), wts.numpy())
        assert int(np.isnan(ref['grad_pts'][0]).sum()) == n                 # the NaN row: 0 * NaN in one of its two components
        what = "%s %s rows %d" % (family, shape, rows)
        _inside(gf, ref['grad_flow'], 'pts.grad_flow', what + ": grad_flow")
        _inside(gp, reduce_rows(ref['grad_pts'], rows), 'pts.grad_pts', what + ": grad_pts")


# ------------------------------------------------------------------------------------------------
# 3. sharpness: what the per-tensor bar lets through and the per-element bar does not
# ------------------------------------------------------------------------------------------------
def _old_bar_accepts(got, exp, rtol):
    return float(np.abs(got.astype(np.float64) - exp.astype(np.float64)).max()) <= rtol * max(float(np.abs(exp).max()), 1e-6)


def _pick_tap(wgt, ok):
    """Among the border samples (some taps inside, some not) the one whose smallest inside weight is nearest 1e-4, and that tap:
    -> (tap index, sample index tuple)."""
    border = ok.any(0) & ~ok.all(0)
    wmin = np.where(ok & (wgt > 0), wgt, np.inf).min(0)
    score = np.where(border & np.isfinite(wmin), np.abs(np.log(np.where(np.isfinite(wmin), wmin, 1.0) / 1e-4)), np.inf)
    at = np.unravel_index(int(np.argmin(score)), score.shape)
    assert np.isfinite(score[at])
    return int(np.argmin(np.where(ok[(slice(None),) + at] & (wgt[(slice(None),) + at] > 0), wgt[(slice(None),) + at], np.inf))), at


@pytest.fixture(scope="module")
def sharp():
    """ATen's six gradients on one frame, the oracle's triples, and per output the oracle's value with one tap dropped."""
    n, c, h, w, sign = 2, 3, 37, 70, 1.0
    f0, img, wts, m = gc.flow('smooth', n, h, w), gc.image(n, c, h, w), gc.upstream(n, c, h, w), gc.holes(n, h, w)
    fn, gn = f0.numpy(), wts.numpy()
    out = {}
    gs, gf = aten_warp(f0, img, wts, sign)
    T = go.warp_taps(fn, n, sign)
    j, at = _pick_tap(T.wgt, T.ok)
    keep = np.ones((4, n, h, w), bool)
    keep[(j,) + at] = False
    full, cut = (go.warp_grad(fn, img.numpy(), gn, sign, gc.G_SCALE, keep=k) for k in (None, keep))
    out['warp.grad_src'] = (gs, full['grad_src'], cut['grad_src'][0], case_runner.GRAD_RTOL)
    out['warp.grad_flow'] = (gf, full['grad_flow'], cut['grad_flow'][0], POS_RTOL)

    gd, gxy, o, den = aten_splat(f0, img, wts, m)
    args = (fn, img.numpy(), o, den, (wts * gc.G_SCALE).numpy(), None, m.numpy(), True, 1.0)
    full = go.splat_grad(*args)
    cw = full['corners'].reshape(4, n, h, w)
    j, at = _pick_tap(cw, cw > 0)
    keep = np.ones((4, n, h, w), bool)
    keep[(j,) + at] = False
    cut = go.splat_grad(*args, keep=keep.reshape(2, 2, n, h, w))
    out['splat.grad_data'] = (gd, full['grad_data'], cut['grad_data'][0], case_runner.GRAD_RTOL)
    out['splat.grad_xy'] = (gxy, full['grad_xy'], cut['grad_xy'][0], POS_RTOL)

    p0, pw = gc.points(n, h, w), point_weights(n, 257)
    gfl, gp = aten_track(f0, p0, pw)
    _, T = go.pts_taps((h, w), p0.numpy(), n)
    j, at = _pick_tap(T.wgt, T.ok)
    keep = np.ones((4, n, 257), bool)
    keep[(j,) + at] = False
    full, cut = (go.sample_pts_grad(fn, p0.numpy(), pw.numpy(), keep=k) for k in (None, keep))
    out['pts.grad_flow'] = (gfl, full['grad_flow'], cut['grad_flow'][0], case_runner.GRAD_RTOL)
    out['pts.grad_pts'] = (gp, full['grad_pts'], cut['grad_pts'][0], POS_RTOL)
    return out


def _scaled(aten, ref):
    """One element times 1 + 3e-5: the one with the most room between its value and its bound."""
    val, M, k = ref
    with np.errstate(invalid='ignore'):
        at = np.unravel_index(int(np.nanargmax(np.abs(val) / go.bound(M, k, 8))), val.shape)
    got = aten.copy()
    got[at] = np.float32(np.float64(aten[at]) * (1 + 3e-5))
    return got


def _dropped(aten, ref, cut):
    with np.errstate(invalid='ignore'):
        return (aten.astype(np.float64) - np.nan_to_num(ref[0] - cut)).astype(np.float32)


@pytest.mark.parametrize("key", sorted(go.R))
def test_one_scaled_element_is_caught_by_the_new_bar_only(key, sharp):
    aten, ref, _, rtol = sharp[key]
    got = _scaled(aten, ref)
    assert _old_bar_accepts(np.nan_to_num(got), np.nan_to_num(aten), rtol), key
    assert go.excess(got, ref, go.R[key]) > 1.0, key


@pytest.mark.parametrize("key", ['warp.grad_src', 'splat.grad_data', 'splat.grad_xy', 'pts.grad_flow', 'pts.grad_pts'])
def test_one_dropped_tap_is_caught_by_the_new_bar_only(key, sharp):
    aten, ref, cut, rtol = sharp[key]
    got = _dropped(aten, ref, cut)
    assert not np.array_equal(got, aten, equal_nan=True)
    assert _old_bar_accepts(np.nan_to_num(got), np.nan_to_num(aten), rtol), key
    assert go.excess(got, ref, go.R[key]) > 1.0, key
