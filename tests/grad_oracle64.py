"""A float64 reference of the three backward passes (ofl_warp_bwd_grad_f32, ofl_splat_grad_f32, ofl_sample_pts_grad_f32) with a
per-element error bound.  Not a conftest: test modules import it.

Sample positions are formed in float32, in the kernels' operation order (`unnormalise`: p * 2, / size_m1, - 1, (+ 1) * half for
the warp and the point sampler; sign * u + x for the splat), so every floor() and every tap-inside decision is the kernel's
own.  Everything after the positions -- fractional parts, weights, products, sums -- is float64 on the kernel's inputs widened
exactly.

Every output comes as a triple (value, M, k): the float64 value, the sum M of the absolute values of the terms added into the
element, and their number k.  A float32 implementation whose every term passes through at most r roundings, summed in any order,
stays within

    |got - value| <= (k + r) * 2^-24 * M + (k + r) * 2^-126                                              (`bound`)

(each rounding costs a relative 2^-24 of its term, a sum of k terms at most k - 1 more of M, the second term covers underflow).
r per output, counted from the kernels' chains, is in `R`; a tap outside the frame, a clamped corner and a masked source pixel
add an exact zero and are no terms.
"""
import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
TINY = 2.0 ** -126
DEN_MIN = F32(1e-3)          # kDenMin
ZERO_THR = F32(1e-3)         # kZeroThr

# Roundings a term passes through before it is summed, plus those after the sum.  A fractional part p - floor(p) is exact for
# p >= 0; for -1 < p < 0 it rounds once, but its complement 1 - frac then only ever weighs taps outside the frame -- so each of the
# two 1-D weights of a tap inside the frame carries one rounding.
R = {
    # wx, wy, wx * wy, g_scale * g, w * g
    'warp.grad_src': 5,
    # s (or nn, e, ww), v * s, g_scale * g, (v * s) * g; after the sum: * half_size_m1, / size_m1 (* 2 and the sign are exact)
    'warp.grad_flow': 6,
    # wx, wy, wy * wx, g / max(D, 1e-3), wgt * gA
    'splat.grad_data': 5,
    # wy, gA = g / dcl, dat * gA, wy * gw   (density leaves: g * out, / dcl, wy, wy * gw; the eq factors are exact)
    'splat.grad_xy': 4,
    # wx, wy, wx * wy, w * g
    'pts.grad_flow': 4,
    # e (or ww, s, nn), tv * e, (tv * e) * g; after the inner sum: * half_size_m1, / size_m1
    'pts.grad_pts': 5,
}


def bound(M, k, r):
    return (k + r) * (U * M + TINY)


def excess(got, ref, r):
    """max over ALL elements of |got - value| / bound (inf where one side is NaN and the other is not)."""
    val, M, k = ref
    got = np.asarray(got, F64)
    assert got.shape == val.shape, (got.shape, val.shape)
    nan_g, nan_v = np.isnan(got), np.isnan(val)
    if not np.array_equal(nan_g, nan_v):
        return np.inf
    with np.errstate(invalid='ignore'):
        ratio = np.abs(got - val) / bound(M, k, r)
    ratio = np.where(nan_v, 0.0, ratio)
    return float(ratio.max()) if ratio.size else 0.0


def unnormalise(p, size):
    """normalise_coords followed by the grid sampler's align_corners un-normalise, float32 op by op."""
    p = np.asarray(p, F32)
    sm1 = F32(size - 1)
    half = sm1 / F32(2)
    g = p * F32(2)
    g = g / sm1
    g = g - F32(1)
    return (g + F32(1)) * half


class Taps(object):
    """The four taps (nw, ne, sw, se) of bilinear samples at float32 positions: float64 fractions and weights, the kernel's inside
    tests on the float32 floors, flat offsets (0 where outside)."""

    def __init__(self, sx, sy, h, w, keep=None):
        with np.errstate(invalid='ignore'):
            xw, yn = np.floor(sx), np.floor(sy)
            xe, ys = xw + F32(1), yn + F32(1)
            x0, x1 = (xw > -1) & (xw < w), (xe > -1) & (xe < w)
            y0, y1 = (yn > -1) & (yn < h), (ys > -1) & (ys < h)
            self.ww = sx.astype(F64) - xw.astype(F64)
            self.nn = sy.astype(F64) - yn.astype(F64)
        self.e, self.s = 1.0 - self.ww, 1.0 - self.nn
        ix0, ix1 = np.where(x0, xw, 0).astype(np.int64), np.where(x1, xe, 0).astype(np.int64)
        iy0, iy1 = np.where(y0, yn, 0).astype(np.int64), np.where(y1, ys, 0).astype(np.int64)
        self.wgt = np.stack([self.s * self.e, self.s * self.ww, self.nn * self.e, self.nn * self.ww])
        self.ok = np.stack([x0 & y0, x1 & y0, x0 & y1, x1 & y1])
        if keep is not None:
            self.ok = self.ok & keep
        self.idx = np.where(self.ok, np.stack([iy0 * w + ix0, iy0 * w + ix1, iy1 * w + ix0, iy1 * w + ix1]), 0)
        # d(sample)/dx and /dy: sign and the other axis' fraction per tap (ATen's gix / giy sums)
        self.dx = [(-1.0, self.s), (1.0, self.s), (-1.0, self.nn), (1.0, self.nn)]
        self.dy = [(-1.0, self.e), (-1.0, self.ww), (1.0, self.e), (1.0, self.ww)]


def warp_positions(flow, n, flow_sign):
    """The float32 sample positions (sx, sy) [N,H,W] of the backward warp: unnormalise(grid - flow_sign * flow)."""
    flow = np.asarray(flow, F32)
    h, w = flow.shape[2:]
    fl = np.broadcast_to(flow, (n, 2, h, w))
    sgn = F32(flow_sign)
    xs, ys = np.arange(w, dtype=F32)[None, None, :], np.arange(h, dtype=F32)[None, :, None]
    return unnormalise(xs - sgn * fl[:, 0], w), unnormalise(ys - sgn * fl[:, 1], h)


def warp_taps(flow, n, flow_sign, keep=None):
    sx, sy = warp_positions(flow, n, flow_sign)
    return Taps(sx, sy, sx.shape[1], sx.shape[2], keep)


def _gather(planes, idx):
    """planes [n, c, hw], idx [n, ...] -> [n, c, ...]"""
    n, c = planes.shape[:2]
    flat = idx.reshape(n, 1, -1)
    return np.take_along_axis(planes, np.broadcast_to(flat, (n, c, flat.shape[2])), 2).reshape((n, c) + idx.shape[1:])


def warp_grad(flow, src, gout, flow_sign, g_scale, keep=None):
    """ofl_warp_bwd_grad_f32.  flow [N|1,2,H,W] f32, src [N|1,C,H,W], gout [N,C,H,W] (f32, or 16-bit widened exactly).
    -> {'grad_src': (value, M, k) [Ns,C,H,W], 'grad_flow': (value, M, k) [N,2,H,W]}.  `keep` [4,N,H,W] bool switches taps off."""
    gout = np.asarray(gout)
    n, c, h, w = gout.shape
    T = warp_taps(flow, n, flow_sign, keep)
    g = F64(F32(g_scale)) * gout.astype(F64)
    ns = src.shape[0]
    S = np.broadcast_to(np.asarray(src).astype(F64), (n, c, h, w)).reshape(n, c, h * w)
    gs, Ms, ks = np.zeros((ns, c, h * w)), np.zeros((ns, c, h * w)), np.zeros((ns, c, h * w), np.int64)
    gf, Mf, kf = np.zeros((2, n, h, w)), np.zeros((2, n, h, w)), np.zeros((n, h, w), np.int64)
    for j in range(4):
        ok = T.ok[j]
        bi, yy, xx = np.nonzero(ok)
        at = (bi if ns == n else np.zeros_like(bi), T.idx[j][ok])
        for ch in range(c):
            t = T.wgt[j][ok] * g[bi, ch, yy, xx]
            np.add.at(gs[:, ch], at, t)
            np.add.at(Ms[:, ch], at, np.abs(t))
            np.add.at(ks[:, ch], at, 1)
        v = np.where(ok[:, None], _gather(S, T.idx[j]), 0.0)
        for axis, (sg, fr) in enumerate((T.dx[j], T.dy[j])):
            t = np.where(ok[:, None], v * fr[:, None] * g, 0.0)
            gf[axis] += sg * t.sum(1)
            Mf[axis] += np.abs(t).sum(1)
        kf += ok * c
    shp = (ns, c, h, w)
    return {'grad_src': (gs.reshape(shp), Ms.reshape(shp), ks.reshape(shp)),
            'grad_flow': (-float(flow_sign) * gf.transpose(1, 0, 2, 3), Mf.transpose(1, 0, 2, 3),
                          np.broadcast_to(kf[:, None], (n, 2, h, w)))}


def _is_zero_vec(fl):
    u, v = fl[:, 0], fl[:, 1]
    return (u < ZERO_THR) & (u > -ZERO_THR) & (v < ZERO_THR) & (v > -ZERO_THR)


def splat_grad(flow, data, out, density, gout, gden=None, weight_mask=None, occlude=True, flow_sign=1.0, xs=None, ys=None,
               keep=None):
    """ofl_splat_grad_f32 (all channels at once: the density term is shared by the host's groups of 3, its leaves summed over every
    channel).  flow [N|1,2,H,W] or xs / ys [N|1,H,W]; data [N|1,C,H,W]; out [N,C,H,W] and density [N,H,W] are the float32 forward
    outputs (the D >= 1e-3, D > 0, zero-vector and filled decisions are made on their bits); gout [N,C,H,W]; gden [N,H,W] | None.
    -> {'grad_data': (value, M, k) [N,C,H,W], 'grad_xy': (value, M, k) [N,2,H,W]}.  `keep` [2,2,N,H,W] (ky, kx) switches corners
    off."""
    gout = np.asarray(gout, F32)
    n, c, h, w = gout.shape
    hw = h * w
    gx_, gy_ = np.arange(w, dtype=F32)[None, None, :], np.arange(h, dtype=F32)[None, :, None]
    if flow is not None:
        fl = np.broadcast_to(np.asarray(flow, F32), (n, 2, h, w))
        sgn = F32(flow_sign)
        xv, yv = sgn * fl[:, 0] + gx_, sgn * fl[:, 1] + gy_
        zvec = _is_zero_vec(fl)
        occ = bool(occlude)
    else:
        xv, yv = np.broadcast_to(np.asarray(xs, F32), (n, h, w)), np.broadcast_to(np.asarray(ys, F32), (n, h, w))
        zvec = np.zeros((n, h, w), bool)
        occ = False
    zero = zvec & occ
    wm = np.ones((n, h, w), bool) if weight_mask is None else np.broadcast_to(np.asarray(weight_mask, bool), (n, h, w))
    D = np.asarray(density)                                               # (float32 from the kernels; kept as given)
    filled = ~(D > 0) & occ & wm & zvec                                   # destination pixels the forward filled from the data
    dcl = np.where(D < DEN_MIN, DEN_MIN, D).astype(F64)[:, None]
    g = np.where(filled[:, None], 0.0, gout.astype(F64))
    gA = (g / dcl).reshape(n, c, hw)
    passes = D >= DEN_MIN
    gDt = np.where(passes[:, None], -(g * np.asarray(out).astype(F64)) / dcl, 0.0).reshape(n, c, hw)
    kD = (passes * c).reshape(n, 1, hw)
    gdn = None if gden is None else np.asarray(gden, F32).astype(F64).reshape(n, 1, hw)
    dat = np.broadcast_to(np.asarray(data, F32).astype(F64), (n, c, h, w))

    x0, y0 = np.floor(xv), np.floor(yv)
    x1, y1 = x0 + F32(1), y0 + F32(1)
    wmax, hmax = F32(w - 1), F32(h - 1)
    xc, yc = [np.clip(x0, 0, wmax), np.clip(x1, 0, wmax)], [np.clip(y0, 0, hmax), np.clip(y1, 0, hmax)]
    eqx, eqy = [x0 == xc[0], x1 == xc[1]], [y0 == yc[0], y1 == yc[1]]
    xv64, yv64 = xv.astype(F64), yv.astype(F64)
    wx, wy = [x1.astype(F64) - xv64, xv64 - x0.astype(F64)], [y1.astype(F64) - yv64, yv64 - y0.astype(F64)]
    active = wm & ~zero
    gd, Md, kd = np.zeros((n, c, h, w)), np.zeros((n, c, h, w)), np.zeros((n, h, w), np.int64)
    gxy, Mxy, kxy = np.zeros((2, n, h, w)), np.zeros((2, n, h, w)), np.zeros((n, h, w), np.int64)
    corners = np.zeros((2, 2, n, h, w))                                   # weights of the live corners (0 elsewhere), for the tests
    for ky in range(2):
        for kx in range(2):
            live = active & eqy[ky] & eqx[kx]
            if keep is not None:
                live = live & keep[ky][kx]
            idx = np.where(live, yc[ky].astype(np.int64) * w + xc[kx].astype(np.int64), 0)
            corners[ky, kx] = np.where(live, wy[ky] * wx[kx], 0.0)
            gAp = _gather(gA, idx)
            t = np.where(live[:, None], (wy[ky] * wx[kx])[:, None] * gAp, 0.0)
            gd += t
            Md += np.abs(t)
            kd += live
            leaves = [dat * gAp, _gather(gDt, idx)] + ([] if gdn is None else [_gather(gdn, idx)])
            gw = sum(l.sum(1) for l in leaves)
            Mgw = sum(np.abs(l).sum(1) for l in leaves)
            kgw = c + _gather(kD, idx)[:, 0] + (0 if gdn is None else 1)
            for axis, (sg, wt) in enumerate(((2 * kx - 1, wy[ky]), (2 * ky - 1, wx[kx]))):
                gxy[axis] += np.where(live, sg * wt * gw, 0.0)
                Mxy[axis] += np.where(live, np.abs(wt) * Mgw, 0.0)
            kxy += np.where(live, kgw, 0)
    src_filled = occ & wm & zvec & ~(D > 0)                               # the un-occlude fill passes the gradient straight to the data
    gd = np.where(src_filled[:, None], gout.astype(F64), gd)
    Md = np.where(src_filled[:, None], np.abs(gout.astype(F64)), Md)
    kd = np.where(src_filled, 1, kd)
    return {'corners': corners, 'grad_data': (gd, Md, np.broadcast_to(kd[:, None], (n, c, h, w))),
            'grad_xy': (gxy.transpose(1, 0, 2, 3), Mxy.transpose(1, 0, 2, 3), np.broadcast_to(kxy[:, None], (n, 2, h, w)))}


def pts_taps(flow_hw, pts, n, keep=None):
    h, w = flow_hw
    P = np.broadcast_to(np.asarray(pts, F32), (n,) + tuple(np.shape(pts)[-2:]))
    return P, Taps(unnormalise(P[..., 1], w), unnormalise(P[..., 0], h), h, w, keep)


def sample_pts_grad(flow, pts, gout, keep=None):
    """ofl_sample_pts_grad_f32.  flow [N|1,2,H,W], pts [N|1,M,2] (y, x), gout [N,M,2].
    -> {'grad_flow': (value, M, k) [N,2,H,W], 'grad_pts': (value, M, k) [N,M,2]}.  A row whose forward result is NaN was overwritten
    with zeros: its upstream gradient is dropped (its own position gradient is whatever 0 * NaN gives, as in the sampler)."""
    gout = np.asarray(gout, F32)
    n, m = gout.shape[:2]
    h, w = flow.shape[2:]
    hw = h * w
    fl = np.broadcast_to(np.asarray(flow, F32).astype(F64), (n, 2, h, w)).reshape(n, 2, hw)
    P, T = pts_taps((h, w), pts, n, keep)
    with np.errstate(invalid='ignore'):
        tv = [np.where(T.ok[j][:, None], _gather(fl, T.idx[j]), 0.0) for j in range(4)]       # [n, 2, m] each
        val = sum(tv[j] * T.wgt[j][:, None] for j in range(4))
        bad = np.isnan(P[..., 0].astype(F64) + val[:, 1]) | np.isnan(P[..., 1].astype(F64) + val[:, 0])
        gc = np.where(bad[:, None], 0.0, np.stack([gout[..., 1], gout[..., 0]], 1).astype(F64))   # (gxo, gyo): u feeds x, v feeds y
        gf, Mf, kf = np.zeros((n, 2, hw)), np.zeros((n, 2, hw)), np.zeros((n, 2, hw), np.int64)
        gp, Mp, kp = np.zeros((2, n, m)), np.zeros((2, n, m)), np.ones((n, m), np.int64)
        for j in range(4):
            ok = T.ok[j]
            bi, mi = np.nonzero(ok)
            for ch in range(2):
                t = T.wgt[j][ok] * gc[bi, ch, mi]
                at = (bi, T.idx[j][ok])
                np.add.at(gf[:, ch], at, t)
                np.add.at(Mf[:, ch], at, np.abs(t))
                np.add.at(kf[:, ch], at, 1)
            for axis, (sg, fr) in enumerate((T.dx[j], T.dy[j])):
                t = tv[j] * fr[:, None] * gc                                # 0 * NaN stays NaN, as in the kernel
                gp[axis] += sg * t.sum(1)
                Mp[axis] += np.abs(t).sum(1)
            kp += ok * 2
        gpts = np.stack([gc[:, 1] + gp[1], gc[:, 0] + gp[0]], -1)           # (y, x)
        Mpts = np.stack([np.abs(gc[:, 1]) + Mp[1], np.abs(gc[:, 0]) + Mp[0]], -1)
    return {'grad_flow': (gf.reshape(n, 2, h, w), Mf.reshape(n, 2, h, w), kf.reshape(n, 2, h, w)),
            'grad_pts': (gpts, Mpts, np.broadcast_to(kp[..., None], (n, m, 2)))}
