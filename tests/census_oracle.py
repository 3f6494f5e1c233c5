"""The definition of Flow.census / census_map / census_stats in NumPy (a helper module, not a test; test modules import
it).  The inputs are those of the photometric tier (`photometric_oracle.case` / `images`), plus one planted case.

The sampled image Iw and the weight test mr > 0.99999 come from `oracle_backend.warp_bwd(..., want_valid=True)` (the C oracle of the
backward warp, which the reference pins), on the image as the kernel reads it: a uint8 sample s is float(s).  Everything after it is
elementwise np.float32 arithmetic, one rounding per operation, the terms of a pixel added in the order dy ascending, dx ascending; rho is
the float64 pow rounded once; the sums of a record are math.fsum (exact, rounded once).  The gradient is float64 on the float32 Gw, Gi and
b of the forward, written as the definition's two sums (terms in which x is the neighbour, terms in which x is the centre), with the
fractions and the inside tests of `grad_oracle64.warp_taps`; next to it `grad` returns, per element, A = the sum of the absolute
contributions (they can cancel, so a bound on the gradient's error is relative to A, not to the gradient).
"""
import functools

import numpy as np
import torch

import grad_oracle64 as go
import oracle_backend as ob
import photometric_oracle as po
import special_values as sv

F32, F64 = np.float32, np.float64
PATCHES = (3, 5, 7)
PATCH, THRESH, EPS, Q = 7, 0.1, 0.01, 0.4
SOFT = F32(0.81)
GREY = (F32(0.299), F32(0.587), F32(0.114))
# the frames of both tiers: the photometric tier's without 1080p (2 x 2, 2 x 5 and 5 x 2 are narrower than the halo), and the kernel's
# tile of 64 x 16 output pixels: exactly one tile, and one tile plus 1 in both axes
TILE_FRAMES = [(2, 16, 64), (2, 17, 65)]
FRAMES = po.SMALL + po.TABLE + [f for f in TILE_FRAMES if f not in po.SMALL + po.TABLE]
UPSTREAM = po.UPSTREAM
REFS = po.REFS
sign_of = po.sign_of
ulp32 = po.ulp32
grad_bound = po.grad_bound


# ---- the definition -------------------------------------------------------------------------------------------------------------------
def _as_image(img, n):
    """(float32 [n, C, H, W] as the kernel reads it, is_uint8); a uint8 sample s is float(s); C-H-W broadcasts over the batch"""
    img = np.asarray(img)
    assert img.dtype in (np.float32, np.uint8) and img.ndim in (3, 4) and img.shape[-3] in (1, 3)
    u8 = img.dtype == np.uint8
    if img.ndim == 3:
        img = img[None]
    assert img.shape[0] in (1, n)
    return np.ascontiguousarray(np.broadcast_to(img.astype(F32), (n,) + img.shape[1:])), u8


def _grey(v, u8):
    """G of float32 [n, C, H, W]: the grey on the scale 0 .. 255"""
    g = v[:, 0] if v.shape[1] == 1 else (GREY[0] * v[:, 0] + GREY[1] * v[:, 1]) + GREY[2] * v[:, 2]
    g = g if u8 else F32(255.0) * g
    assert g.dtype == F32
    return g


def _shifted(x, r, dy, dx):
    """x(p + o) for o = (dy, dx), the fill value 0 / False outside the frame: x [n, h, w]"""
    h, w = x.shape[1:]
    return np.pad(x, ((0, 0), (r, r), (r, r)))[:, r + dy:r + dy + h, r + dx:r + dx + w]


def offsets(patch):
    r = patch // 2
    return [(dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if (dy, dx) != (0, 0)]


def compute(a, mask, img, other, ref, patch=PATCH, thresh=THRESH, eps=EPS, q=Q):
    """dict: 'map' float32 [N,H,W] (+0 where not known); 'known', 'usable', 'inside' bool [N,H,W]; 'n' int64 [N,H,W] (0 where not
    usable); 'hd', 'b', 'gw', 'gi' float32 [N,H,W]; 'records' float64 [N,8]; 'census' float32 [N]"""
    assert patch in PATCHES and np.asarray(img).dtype == np.asarray(other).dtype
    f = po._as_f32(a)
    n, _, h, w = f.shape
    (im, u8), (ot, _) = _as_image(img, n), _as_image(other, n)
    assert im.shape == ot.shape and im.shape[2:] == (h, w)
    out, valid, _, _ = ob.warp_bwd(torch.from_numpy(f.copy()), torch.from_numpy(ot.copy()), flow_sign=sign_of(ref), want_valid=True)
    inside = valid.numpy().astype(bool)
    usable = inside if mask is None else inside & np.asarray(mask, bool)
    r = patch // 2
    th = F32(thresh)
    with np.errstate(all='ignore'):
        gw, gi = _grey(out.numpy(), u8), _grey(im, u8)
        total, cnt = np.zeros((n, h, w), F32), np.zeros((n, h, w), np.int64)
        for dy, dx in offsets(patch):
            term = _shifted(usable, r, dy, dx)
            dw, di = _shifted(gw, r, dy, dx) - gw, _shifted(gi, r, dy, dx) - gi
            tw, ti = dw / np.sqrt(SOFT + dw * dw), di / np.sqrt(SOFT + di * di)
            e = ti - tw
            s = e * e
            fterm = s / (th + s)
            assert fterm.dtype == F32
            total = np.where(term, total + fterm, total)
            cnt += term
        cnt = np.where(usable, cnt, 0)
        known = usable & (cnt >= 1)
        hd = total / cnt.astype(F32)
        b = hd + F32(eps)
        rho = np.power(b.astype(F64), F64(F32(q))).astype(F32)
    assert hd.dtype == F32 and b.dtype == F32
    cmap = np.where(known, rho, F32(0.0)).astype(F32)
    rec = np.zeros((n, 8), F64)
    for i in range(n):
        vals = rho[i][known[i]].astype(F64)
        rec[i, :4] = [vals.size, sv.record_sum(vals), sv.record_max(vals), cnt[i][known[i]].sum()]
    with np.errstate(invalid='ignore', divide='ignore'):
        loss = (rec[:, 1] / rec[:, 0]).astype(F32)
    return {'map': cmap, 'known': known, 'usable': usable, 'inside': inside, 'n': cnt, 'hd': hd, 'b': b, 'gw': gw, 'gi': gi,
            'records': rec, 'census': loss}


def grad(a, mask, img, other, ref, patch=PATCH, thresh=THRESH, eps=EPS, q=Q, upstream=UPSTREAM):
    """(want float64 [N,2,H,W], A float64 [N,2,H,W]) of sum_n upstream[n] * census[n] with respect to the vectors"""
    res = compute(a, mask, img, other, ref, patch, thresh, eps, q)
    f = po._as_f32(a)
    n, _, h, w = f.shape
    ot, u8 = _as_image(other, n)
    ot = ot.astype(F64).reshape(n, -1, h * w)
    chan = ot.shape[1]
    sign = sign_of(ref)
    r = patch // 2
    up = np.asarray(upstream[:n], F32).astype(F64)
    with np.errstate(invalid='ignore', divide='ignore'):
        scale = (up / res['records'][:, 0]).astype(F32).astype(F64)                        # the fp32 device tensor
    known, usable = res['known'], res['usable']
    gw, gi = res['gw'].astype(F64), res['gi'].astype(F64)
    th, soft, qq = F64(F32(thresh)), F64(SOFT), F64(F32(q))
    with np.errstate(all='ignore'):
        kappa = np.where(known, scale[:, None, None] * qq * np.power(res['b'].astype(F64), qq - 1.0) / res['n'], 0.0)
    # dL/dGw(x) = sum_{p known, x - p in U(p)} kappa(p) k_{x-p}(p)  -  [x known] kappa(x) sum_{o in U(x)} k_o(x)
    dg, dg_abs = np.zeros((n, h + 2 * r, w + 2 * r)), np.zeros((n, h + 2 * r, w + 2 * r))
    for dy, dx in offsets(patch):
        term = known & _shifted(usable, r, dy, dx)                                          # o in U(p), p known
        with np.errstate(all='ignore'):
            dw, di = _shifted(gw, r, dy, dx) - gw, _shifted(gi, r, dy, dx) - gi
            e = di / np.sqrt(soft + di * di) - dw / np.sqrt(soft + dw * dw)
            s = e * e
            k = th / (th + s) ** 2 * (-2.0 * e) * soft / (soft + dw * dw) ** 1.5
            t = np.where(term, kappa * k, 0.0)
        dg[:, r + dy:r + dy + h, r + dx:r + dx + w] += t                                    # to the neighbour x = p + o
        dg[:, r:r + h, r:r + w] -= t                                                        # to the centre x = p
        dg_abs[:, r + dy:r + dy + h, r + dx:r + dx + w] += np.abs(t)
        dg_abs[:, r:r + h, r:r + w] += np.abs(t)
    dg, dg_abs = dg[:, r:r + h, r:r + w], dg_abs[:, r:r + h, r:r + w]
    # dGw / d flow: the grey weights (and 255 for float32 images) times the derivative of every channel's sample
    taps = go.warp_taps(f, n, sign)
    weights = (1.0,) if chan == 1 else tuple(F64(g) for g in GREY)
    acc, absacc = np.zeros((2, n, h, w)), np.zeros((2, n, h, w))
    for c in range(chan):
        for j in range(4):                                                                  # nw, ne, sw, se
            v = np.where(taps.ok[j], np.take_along_axis(ot[:, c], taps.idx[j].reshape(n, -1), 1).reshape(n, h, w), 0.0)
            for axis, (sg, fr) in enumerate((taps.dx[j], taps.dy[j])):
                with np.errstate(invalid='ignore'):
                    t = np.where(taps.ok[j], fr * v, 0.0)
                acc[axis] += weights[c] * sg * t
                absacc[axis] += weights[c] * np.abs(t)
    ims = 1.0 if u8 else 255.0
    with np.errstate(invalid='ignore', over='ignore'):
        want = np.where(known[:, None], (-sign) * ims * dg[:, None] * acc.transpose(1, 0, 2, 3), 0.0)
        big_a = np.where(known[:, None], ims * dg_abs[:, None] * absacc.transpose(1, 0, 2, 3), 0.0)
    return want, big_a


def categories(n, h, w, ref, patch=PATCH):
    """Per image of a case (`photometric_oracle.case`, float32 images), the share of its pixels that are known, known with a full
    patch, known with a partial patch, sampled from outside the frame; and the share of the known pixels with 0.05 < hd < 0.95: five
    float arrays [n]"""
    a, a_mask, img, other, _, _ = po.case(n, h, w, ref)
    res = compute(a, a_mask, img, other, ref, patch)
    total, full = float(h * w), patch * patch - 1
    known = res['known']
    kn = known.sum((1, 2))
    mid = (known & (res['hd'] > 0.05) & (res['hd'] < 0.95)).sum((1, 2)) / np.maximum(kn, 1)
    return (kn / total, (known & (res['n'] == full)).sum((1, 2)) / total, (known & (res['n'] < full)).sum((1, 2)) / total,
            (~res['inside']).sum((1, 2)) / total, mid)


# ---- the planted case -----------------------------------------------------------------------------------------------------------------
PLANTED_LONE, PLANTED_PAIR, PLANTED_CENTRE = (3, 5), ((10, 4), (10, 5)), (8, 12)
PLANTED_COUNT = 49 + 2


@functools.lru_cache(maxsize=None)
def planted():
    """(a, mask, img) of a 1 x 12 x 16 frame with zero flow, to be run with other = img and patch 7.  The mask leaves: the pixel
    PLANTED_LONE, usable with all 48 neighbours masked (n = 0: not known); the two pixels PLANTED_PAIR, each other's only usable
    neighbour (n = 1); the block of rows 5 .. 11 and columns 9 .. 15, whose centre PLANTED_CENTRE has n = 48.  Every pixel left lies
    in a column whose float32 sample position is exact (w - 1 = 15 is no power of two: columns 1 .. 3 are off by an ulp or two), so
    Gw = Gi there bit for bit, every term is 0 and rho = pow(eps, q) on the PLANTED_COUNT known pixels."""
    a = np.zeros((1, 2, 12, 16), F32)
    mask = np.zeros((1, 12, 16), bool)
    mask[0][PLANTED_LONE] = True
    for p in PLANTED_PAIR:
        mask[0][p] = True
    mask[0, 5:12, 9:16] = True
    img = np.random.RandomState(2121).uniform(size=(1, 3, 12, 16)).astype(F32)
    for arr in (a, mask, img):
        arr.setflags(write=False)
    return a, mask, img


# ---- the native call served by this module (host-logic tests) -----------------------------------------------------------------------
def fake_flow_census(vecs, mask, img, other, flow_sign=-1.0, patch=PATCH, thresh=THRESH, eps=EPS, q=Q, want_map=False,
                     want_record=True):
    res = compute(vecs.detach().numpy(), None if mask is None else mask.numpy(), img.numpy(), other.numpy(),
                  's' if flow_sign < 0 else 't', patch, thresh, eps, q)
    return (torch.from_numpy(res['records']) if want_record else None), (torch.from_numpy(res['map']) if want_map else None)
