"""The definition of Flow.ssim / ssim_map / ssim_stats in NumPy (a helper module, not a test; test modules import it).
The inputs are those of the photometric tier (`photometric_oracle.case` / `images`), plus two planted cases.

The sampled image X = Iw and the weight test mr > 0.99999 come from `oracle_backend.warp_bwd(..., want_valid=True)` (the C oracle of the
backward warp, which the reference pins), on the image as the kernel reads it: a uint8 sample s is float(s) / 255.0f.  Everything after
it is elementwise np.float32 arithmetic, one rounding per operation, the pixels of a window added in the order dy ascending, dx
ascending, in two walks (the means, then the moments about them); the sums of a record are math.fsum (exact, rounded once).  With
`float64=True` the same steps run in float64 on the same float32 X and Y.  The gradient is float64 on the float32 X, Y of the forward:
three coefficient maps a0, a1, a2 per channel, box-summed, times the derivative of the pixel's own sample with the fractions and the
inside tests of `grad_oracle64.warp_taps`; next to it `grad` returns, per element, A = the sum of the absolute contributions (they can
cancel, so a bound on the gradient's error is relative to A, not to the gradient).
"""
import functools

import numpy as np
import torch

import census_oracle as cen
import grad_oracle64 as go
import oracle_backend as ob
import photometric_oracle as po
import special_values as sv

F32, F64 = np.float32, np.float64
WINDOWS = (3, 5, 7)
WINDOW, C1, C2 = 3, 1e-4, 9e-4
# the frames of both tiers: the photometric tier's without 1080p (every frame from 2 x 2 upward is legal: the centre is always in its
# window), and the kernel's tile of 64 x 16 output pixels: exactly one tile, and one tile plus 1 in both axes
TILE_FRAMES = [(2, 16, 64), (2, 17, 65)]
FRAMES = po.SMALL + po.TABLE + [f for f in TILE_FRAMES if f not in po.SMALL + po.TABLE]
UPSTREAM = po.UPSTREAM
REFS = po.REFS
sign_of = po.sign_of
ulp32 = po.ulp32
grad_bound = po.grad_bound


# ---- the definition -------------------------------------------------------------------------------------------------------------------
def _views(x, r):
    """[x(p + o) for o in offsets(2 r + 1)], the fill value 0 / False outside the frame: x [n, h, w]"""
    h, w = x.shape[1:]
    pad = np.pad(x, ((0, 0), (r, r), (r, r)))
    return [pad[:, r + dy:r + dy + h, r + dx:r + dx + w] for dy in range(-r, r + 1) for dx in range(-r, r + 1)]


def offsets(window):
    r = window // 2
    return [(dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1)]


def _moments(x, y, usable, cnt, window, T):
    """(mux, muy, sxx, syy, sxy) of one channel in the type T: two walks of the window, one rounding per operation"""
    r = window // 2
    terms = list(zip(_views(usable, r), _views(x, r), _views(y, r)))
    fn = cnt.astype(T)
    sx, sy = np.zeros(x.shape, T), np.zeros(x.shape, T)
    for term, xs, ys in terms:
        sx, sy = np.where(term, sx + xs, sx), np.where(term, sy + ys, sy)
    mux, muy = sx / fn, sy / fn
    vxx, vyy, vxy = np.zeros(x.shape, T), np.zeros(x.shape, T), np.zeros(x.shape, T)
    for term, xs, ys in terms:
        ax, ay = xs - mux, ys - muy
        vxx, vyy, vxy = np.where(term, vxx + ax * ax, vxx), np.where(term, vyy + ay * ay, vyy), np.where(term, vxy + ax * ay, vxy)
    out = (mux, muy, vxx / fn, vyy / fn, vxy / fn)
    assert all(o.dtype == T for o in out)
    return out


def compute(a, mask, img, other, ref, window=WINDOW, c1=C1, c2=C2, float64=False):
    """dict: 'map' [N,H,W] (+0 where not known; float32, or float64 with `float64`); 'known' (= 'usable'), 'inside' bool [N,H,W]; 'n'
    int64 [N,H,W] (0 where not usable); 'x', 'y' float32 [N,C,H,W]; 'raw' [N,C,H,W], d_c before the clamp; 'records' float64 [N,8];
    'ssim' float32 [N]"""
    assert window in WINDOWS and np.asarray(img).dtype == np.asarray(other).dtype
    T = F64 if float64 else F32
    f = po._as_f32(a)
    n, _, h, w = f.shape
    im, ot = po._as_image(img, n), po._as_image(other, n)
    assert im.shape == ot.shape and im.shape[2:] == (h, w) and im.shape[1] in (1, 3)
    chan = im.shape[1]
    out, valid, _, _ = ob.warp_bwd(torch.from_numpy(f.copy()), torch.from_numpy(ot.copy()), flow_sign=sign_of(ref), want_valid=True)
    x, inside = out.numpy(), valid.numpy().astype(bool)
    usable = inside if mask is None else inside & np.asarray(mask, bool)
    r = window // 2
    cnt = np.zeros((n, h, w), np.int64)
    for term in _views(usable, r):
        cnt += term
    cnt = np.where(usable, cnt, 0)
    k1, k2, one, two, half = T(F32(c1)), T(F32(c2)), T(1.0), T(2.0), T(0.5)
    raw = np.zeros((n, chan, h, w), T)
    with np.errstate(all='ignore'):
        total = None
        for c in range(chan):
            mux, muy, sxx, syy, sxy = _moments(x[:, c].astype(T), im[:, c].astype(T), usable, cnt, window, T)
            l1 = (two * mux) * muy + k1
            l2 = (mux * mux + muy * muy) + k1
            s1 = two * sxy + k2
            s2 = (sxx + syy) + k2
            d = (one - (l1 * s1) / (l2 * s2)) * half
            raw[:, c] = d
            d = np.where(d < 0, T(0.0), np.where(d > 1, T(1.0), d))                           # (comparisons: a NaN passes through)
            total = d if total is None else total + d
        rho = total / T(chan)
    assert rho.dtype == T
    smap = np.where(usable, rho, T(0.0)).astype(T)
    rec = np.zeros((n, 8), F64)
    for i in range(n):
        vals = rho[i][usable[i]].astype(F64)
        rec[i, :4] = [vals.size, sv.record_sum(vals), sv.record_max(vals), cnt[i][usable[i]].sum()]
    with np.errstate(invalid='ignore', divide='ignore'):
        loss = (rec[:, 1] / rec[:, 0]).astype(F32)
    return {'map': smap, 'known': usable, 'usable': usable, 'inside': inside, 'n': cnt, 'x': x, 'y': im, 'raw': raw, 'records': rec,
            'ssim': loss}


def coefficients(x, y, usable, cnt, window, c1=C1, c2=C2):
    """((a0, a1, a2), |a0| as the sum of its four terms' absolute values) of one channel, float64 [n, h, w], 0 where not known:
    d ssim(p) / d X(q) = a0(p) + a1(p) Y(q) + a2(p) X(q) for q in W(p)"""
    k1, k2 = F64(F32(c1)), F64(F32(c2))
    with np.errstate(all='ignore'):
        mux, muy, sxx, syy, sxy = _moments(x.astype(F64), y.astype(F64), usable, cnt, window, F64)
        A, D = (2.0 * mux) * muy + k1, (mux * mux + muy * muy) + k1
        B, E = 2.0 * sxy + k2, (sxx + syy) + k2
        tn = 2.0 / cnt
        t = [B * muy / (D * E), -A * B * mux / (D * D * E), -A * muy / (D * E), A * B * mux / (D * E * E)]
        a0 = tn * (((t[0] + t[1]) + t[2]) + t[3])
        a0_abs = tn * (((np.abs(t[0]) + np.abs(t[1])) + np.abs(t[2])) + np.abs(t[3]))
        a1 = tn * A / (D * E)
        a2 = -tn * A * B / (D * E * E)
    return tuple(np.where(usable, v, 0.0) for v in (a0, a1, a2)), np.where(usable, a0_abs, 0.0)


def grad(a, mask, img, other, ref, window=WINDOW, c1=C1, c2=C2, upstream=UPSTREAM, res=None):
    """(want float64 [N,2,H,W], A float64 [N,2,H,W]) of sum_n upstream[n] * ssim[n] with respect to the vectors; `res`: what `compute`
    gave for the same arguments, if the caller has it"""
    res = compute(a, mask, img, other, ref, window, c1, c2) if res is None else res
    f = po._as_f32(a)
    n, _, h, w = f.shape
    ot = po._as_image(other, n).astype(F64).reshape(n, -1, h * w)
    chan = ot.shape[1]
    sign = sign_of(ref)
    r = window // 2
    up = np.asarray(upstream[:n], F32).astype(F64)
    with np.errstate(invalid='ignore', divide='ignore'):
        scale = (up / res['records'][:, 0]).astype(F32).astype(F64)                        # the fp32 device tensor
    usable, cnt = res['usable'], res['n']
    taps = go.warp_taps(f, n, sign)
    acc, absacc = np.zeros((2, n, h, w)), np.zeros((2, n, h, w))
    for c in range(chan):
        x, y = res['x'][:, c].astype(F64), res['y'][:, c].astype(F64)
        (a0, a1, a2), a0_abs = coefficients(res['x'][:, c], res['y'][:, c], usable, cnt, window, c1, c2)
        s = [np.zeros((n, h, w)) for _ in range(3)]
        s_abs = [np.zeros((n, h, w)) for _ in range(3)]
        for k, (v, va) in enumerate(((a0, a0_abs), (a1, np.abs(a1)), (a2, np.abs(a2)))):
            for sv_, sa_ in zip(_views(v, r), _views(va, r)):                                   # S_k(x): a_k(p) over the known p = x + o,
                s[k] += sv_                                                                     # dy ascending, dx ascending
                s_abs[k] += sa_
        with np.errstate(invalid='ignore', over='ignore'):
            dx_c = (s[0] + s[1] * y) + s[2] * x                                             # sum over p of d ssim_c(p) / d X_c(x)
            dx_abs = (s_abs[0] + s_abs[1] * np.abs(y)) + s_abs[2] * np.abs(x)
        for j in range(4):                                                                  # nw, ne, sw, se
            v = np.where(taps.ok[j], np.take_along_axis(ot[:, c], taps.idx[j].reshape(n, -1), 1).reshape(n, h, w), 0.0)
            for axis, (sg, fr) in enumerate((taps.dx[j], taps.dy[j])):
                with np.errstate(invalid='ignore'):
                    t = np.where(taps.ok[j], fr * v, 0.0)
                    acc[axis] += np.where(usable, dx_c * sg * t, 0.0)
                    absacc[axis] += np.where(usable, dx_abs * np.abs(t), 0.0)
    known = usable[:, None]
    with np.errstate(invalid='ignore', over='ignore'):
        # dL/dX_c = -scale / (2 C) * dx_c;  dX_c / d flow = -sign * (gx_c, gy_c)
        want = np.where(known, (scale[:, None, None, None] * sign / (2.0 * chan)) * acc.transpose(1, 0, 2, 3), 0.0)
        big_a = np.where(known, (np.abs(scale)[:, None, None, None] / (2.0 * chan)) * absacc.transpose(1, 0, 2, 3), 0.0)
    return want, big_a


def categories(n, h, w, ref, window=WINDOW):
    """Per image of a case (`photometric_oracle.case`, float32 images), the share of its pixels that are known, known with a full
    window, known with a partial window, sampled from outside the frame; and the share of the known pixels with 0.05 < rho < 0.95: five
    float arrays [n]"""
    a, a_mask, img, other, _, _ = po.case(n, h, w, ref)
    res = compute(a, a_mask, img, other, ref, window)
    total, full = float(h * w), window * window
    known = res['known']
    kn = known.sum((1, 2))
    mid = (known & (res['map'] > 0.05) & (res['map'] < 0.95)).sum((1, 2)) / np.maximum(kn, 1)
    return (kn / total, (known & (res['n'] == full)).sum((1, 2)) / total, (known & (res['n'] < full)).sum((1, 2)) / total,
            (~res['inside']).sum((1, 2)) / total, mid)


# ---- the planted cases ----------------------------------------------------------------------------------------------------------------
def planted_identical():
    """(a, mask, img) of `census_oracle.planted()`, to be run with other = img: every pixel the mask leaves lies in a column whose
    float32 sample position is exact, so X = Y bit for bit, (2 mu) mu = mu mu + mu mu and 2 s = s + s hold in IEEE, ssim_c is exactly 1
    and rho exactly +0 on every known pixel -- the lone pixel `census_oracle.PLANTED_LONE` (n = 1: known here, its own window) and the
    pair whose two pixels are each other's only neighbour (n = 2) included."""
    return cen.planted()


PLANTED_IDENTICAL_COUNT = cen.PLANTED_COUNT + 1           # the block, the pair and the lone pixel


@functools.lru_cache(maxsize=None)
def planted_clamp():
    """(a, img, other) of a 1 x 12 x 16 frame with zero flow, to be run without a mask: `other` is `img` with every sample moved one
    float32 step up or down, so ssim_c is 1 within a few float32 steps on either side and the raw d_c is negative on more than a
    hundred channel-pixels per window (129 / 146 / 131 at window 3 / 5 / 7): the lower clamp is active.  (The upper clamp cannot be:
    d_c > 1 needs ssim_c < -1, and |2 sxy| <= sxx + syy with c2 > 0 keeps |ssim_c| below 1 up to rounding.)"""
    rng = np.random.RandomState(77)
    img = rng.uniform(size=(1, 3, 12, 16)).astype(F32)
    up = rng.randint(0, 2, size=img.shape).astype(bool)
    other = np.where(up, np.nextafter(img, F32(np.inf)), np.nextafter(img, F32(-np.inf))).astype(F32)
    a = np.zeros((1, 2, 12, 16), F32)
    for arr in (a, img, other):
        arr.setflags(write=False)
    return a, img, other


# ---- the native call served by this module (host-logic tests) -----------------------------------------------------------------------
def fake_flow_ssim(vecs, mask, img, other, flow_sign=-1.0, window=WINDOW, c1=C1, c2=C2, want_map=False, want_record=True):
    res = compute(vecs.detach().numpy(), None if mask is None else mask.numpy(), img.numpy(), other.numpy(),
                  's' if flow_sign < 0 else 't', window, c1, c2)
    return (torch.from_numpy(res['records']) if want_record else None), (torch.from_numpy(res['map']) if want_map else None)


def fake_flow_ssim_grad_for(upstream):
    """A stand-in for `_ssim.flow_ssim_grad` that answers with the oracle's float64 gradient for the upstream gradient `upstream`, rounded
    to float32; it checks that the scale it is handed is that upstream over the count"""
    def fake(vecs, mask, img, other, flow_sign, window, c1, c2, scale):
        ref = 's' if flow_sign < 0 else 't'
        args = (vecs.detach().numpy(), None if mask is None else mask.numpy(), img.numpy(), other.numpy(), ref, window, c1, c2)
        res = compute(*args)
        with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
            assert np.array_equal(scale.numpy(), (np.asarray(upstream, F32).astype(F64) / res['records'][:, 0]).astype(F32), equal_nan=True)
            return torch.from_numpy(grad(*args, upstream=upstream, res=res)[0].astype(F32))
    return fake
