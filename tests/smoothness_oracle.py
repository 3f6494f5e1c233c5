"""The definition of Flow.smoothness / smoothness_map / smoothness_stats in NumPy, function for function (a helper
module, not a test; test modules import it), and the inputs the GPU tier runs on.

Every per-pixel step is float32 with one rounding per operation; the weight is np.exp on float64 rounded once; the sums of a record are
math.fsum (exact, rounded once); the gradient is float64 throughout and rounded once.  Next to the gradient `grad` returns, per element,
A = |scale| * sum_k |coef_k q_Tk|, the sum of the absolute contributions (the contributions can cancel, so a bound on the gradient's error
is relative to A, not to the gradient), and the pixels that a valid term reads.
"""
import functools

import numpy as np

import special_values as sv

F32 = np.float32
TH, TW = 8, 128               # the kernel's tile (ofl_smoothness.hip)
# (n, h, w): no term; one direction only; order 2 has no term; order 2's single centre term; the scalar form; odd, more than one block;
# the 16-byte form, several blocks; the tile and the tile plus one; every block loops
FRAMES = [(3, 1, 1), (3, 1, 5), (3, 5, 1), (3, 2, 2), (3, 3, 3), (3, 5, 7), (3, 37, 53), (3, 96, 136), (3, TH, TW), (3, TH + 1, TW + 1),
          (2, 1080, 1920)]
SMALL = [f for f in FRAMES if f[1] * f[2] < 100000]
UPSTREAM = (0.75, -2.0, 1.0)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def patch_of(h, w):
    """The constant patch: rows and columns [h // 4, h // 4 + max(3, h // 4)), clipped to the frame."""
    return slice(h // 4, min(h, h // 4 + max(3, h // 4))), slice(w // 4, min(w, w // 4 + max(3, w // 4)))


@functools.lru_cache(maxsize=None)
def case(n, h, w):
    """(flow float32 [n,2,h,w], mask bool [n,h,w]), read-only and computed once: a smooth field plus noise of sigma 0.3, constant on
    the patch (so that d = 0 occurs); a mask with about 20 % holes, none of them on the patch."""
    rng = np.random.RandomState(1000 * n + 10 * h + w)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    f = np.empty((n, 2, h, w), np.float64)
    for i in range(n):
        f[i, 0] = 2.0 * np.sin(x / 9.0 + i) + 0.05 * y
        f[i, 1] = 1.5 * np.cos(y / 7.0 - i) - 0.03 * x
    f += rng.normal(0.0, 0.3, f.shape)
    ys, xs = patch_of(h, w)
    f[:, 0, ys, xs], f[:, 1, ys, xs] = 1.25, -0.5
    mask = rng.uniform(size=(n, h, w)) >= 0.2
    mask[:, ys, xs] = True
    f = f.astype(F32)
    f.flags.writeable = False
    mask.flags.writeable = False
    return f, mask


@functools.lru_cache(maxsize=None)
def image(n, h, w, c=3, u8=False, batch=True):
    """Uniform noise in [0, 1) with a step of 0.8 from column w // 2 on: float32 [n,c,h,w] ([c,h,w] without `batch`), or uint8 with
    the range [0, 1.8) scaled to [0, 255]."""
    rng = np.random.RandomState(77 + 1000 * n + 10 * h + w + c)
    img = rng.uniform(size=(n if batch else 1, c, h, w))
    img[..., w // 2:] += 0.8
    img = np.floor(img * (255.0 / 1.8)).astype(np.uint8) if u8 else img.astype(F32)
    img = img if batch else img[0]
    img.flags.writeable = False
    return img


# ---- the definition -------------------------------------------------------------------------------------------------------------------
def _as_f32(flow):
    flow = np.asarray(flow)
    assert flow.dtype in (np.float32, np.float16) and flow.ndim == 4 and flow.shape[1] == 2
    return flow.astype(F32)                                   # fp16 storage is up-converted exactly


def _as_image(img, n):
    """float32 [n or 1, C, H, W]; a uint8 sample s is float(s) / 255.0f"""
    if img is None:
        return None
    img = np.asarray(img)
    assert img.dtype in (np.float32, np.uint8) and img.ndim in (3, 4) and 1 <= img.shape[-3] <= 4
    if img.ndim == 3:
        img = img[None]
    assert img.shape[0] in (1, n)
    return img.astype(F32) / F32(255.0) if img.dtype == np.uint8 else img


def direction_terms(f, valid, img, order, alpha, eps, axis):
    """The terms of one direction (axis 'x' or 'y'), each at the pixel it is attributed to: dict of [N,H,W] arrays `ok` (valid), `t`
    (float32, +0 where not valid), `du`, `dv`, `w` (float32)."""
    assert order in (1, 2) and axis in ('x', 'y')
    alpha, eps = F32(alpha), F32(eps)
    sw = (lambda a: a) if axis == 'x' else (lambda a: np.swapaxes(a, -1, -2))
    f, valid = sw(f), sw(valid)
    n, hh, ww = valid.shape
    out = {'ok': np.zeros((n, hh, ww), bool), 't': np.zeros((n, hh, ww), F32), 'du': np.zeros((n, hh, ww), F32),
           'dv': np.zeros((n, hh, ww), F32), 'w': np.ones((n, hh, ww), F32)}
    if ww >= order + 1:
        if order == 1:
            at, lo, hi = slice(0, ww - 1), slice(0, ww - 1), slice(1, ww)
            d = f[..., hi] - f[..., at]
            ok = valid[..., at] & valid[..., hi]
        else:
            at, lo, hi = slice(1, ww - 1), slice(0, ww - 2), slice(2, ww)
            d = (f[..., lo] - (f[..., at] + f[..., at])) + f[..., hi]
            ok = valid[..., lo] & valid[..., at] & valid[..., hi]
        assert d.dtype == F32
        wgt = np.ones(ok.shape, F32)
        if img is not None:
            im = sw(img)
            s = np.zeros((im.shape[0],) + ok.shape[1:], F32)
            for c in range(im.shape[1]):                      # channels in ascending order, then one division
                s = s + np.abs(im[:, c][..., hi] - im[:, c][..., lo])
            g = s / F32(im.shape[1])
            if order == 2:
                g = g * F32(0.5)
            arg = -(alpha * g)
            assert arg.dtype == F32
            wgt = np.broadcast_to(np.exp(arg.astype(np.float64)).astype(F32), ok.shape)
        du, dv = d[:, 0], d[:, 1]
        with np.errstate(over='ignore'):
            ee = eps * eps
            r = np.sqrt(du * du + ee) + np.sqrt(dv * dv + ee)
            t = wgt * r
        assert t.dtype == F32 and type(ee) is F32
        out['ok'][..., at], out['du'][..., at], out['dv'][..., at], out['w'][..., at] = ok, du, dv, wgt
        out['t'][..., at] = np.where(ok, t, F32(0.0))
    return {k: np.ascontiguousarray(sw(v)) for k, v in out.items()}


def compute(flow, mask=None, img=None, order=1, alpha=10.0, eps=0.001):
    """dict: 'map' float32 [N,H,W]; 'x', 'y' the direction_terms; 'records' float64 [N,8]; 'smoothness' float32 [N]"""
    f = _as_f32(flow)
    n, _, h, w = f.shape
    valid = np.ones((n, h, w), bool) if mask is None else np.asarray(mask).astype(bool)
    im = _as_image(img, n)
    tx = direction_terms(f, valid, im, order, alpha, eps, 'x')
    ty = direction_terms(f, valid, im, order, alpha, eps, 'y')
    rec = np.zeros((n, 8), np.float64)
    for i in range(n):
        vx, vy = tx['t'][i][tx['ok'][i]], ty['t'][i][ty['ok'][i]]
        rec[i, 0], rec[i, 1] = vx.size, vy.size
        rec[i, 2], rec[i, 3] = sv.record_sum(vx), sv.record_sum(vy)                     # (total on NaN / inf terms: special_values.py)
        rec[i, 4] = sv.record_max(np.concatenate([vx, vy]))
    with np.errstate(invalid='ignore', divide='ignore'):
        loss = ((rec[:, 2] + rec[:, 3]) / (rec[:, 0] + rec[:, 1])).astype(F32)
    smap = tx['t'] + ty['t']
    assert smap.dtype == F32
    return {'map': smap, 'x': tx, 'y': ty, 'records': rec, 'smoothness': loss}


def _shift(a, k, axis):
    """out[s] = a[s + k] along `axis`, 0 where s + k is outside"""
    out = np.zeros_like(a)
    n = a.shape[axis]
    if abs(k) >= n:
        return out
    src = [slice(None)] * a.ndim
    dst = [slice(None)] * a.ndim
    src[axis] = slice(max(k, 0), n + min(k, 0))
    dst[axis] = slice(max(-k, 0), n - max(k, 0))
    out[tuple(dst)] = a[tuple(src)]
    return out


def grad(flow, mask=None, img=None, order=1, alpha=10.0, eps=0.001, upstream=UPSTREAM):
    """(gradient float32 [N,2,H,W], A float64 [N,2,H,W], read bool [N,H,W]) of sum_n upstream[n] * smoothness[n]"""
    res = compute(flow, mask, img, order, alpha, eps)
    n = res['map'].shape[0]
    up = np.asarray(upstream[:n], F32).astype(np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        scale = (up / (res['records'][:, 0] + res['records'][:, 1])).astype(F32).astype(np.float64)      # the fp32 device tensor
    ee = np.float64(F32(eps)) * np.float64(F32(eps))
    acc = np.zeros((n, 2) + res['map'].shape[1:], np.float64)
    absacc = np.zeros_like(acc)
    read = np.zeros(res['map'].shape, bool)
    coefs = {1: ((-1, 1.0), (0, -1.0)), 2: ((-1, 1.0), (0, -2.0), (1, 1.0))}[order]      # (term at s + k, coefficient), lower index first
    for name, axis in (('x', -1), ('y', -2)):                                            # x before y
        t = res[name]
        q = np.zeros_like(acc)
        for c, key in enumerate(('du', 'dv')):
            d = t[key].astype(np.float64)
            den = np.sqrt(d * d + ee)
            with np.errstate(invalid='ignore', divide='ignore'):
                qq = (t['w'].astype(np.float64) * d) / den
            q[:, c] = np.where(t['ok'] & (den != 0.0), qq, 0.0)
        for k, coef in coefs:
            acc = acc + coef * _shift(q, k, axis)
            absacc = absacc + np.abs(coef * _shift(q, k, axis))
            read |= _shift(t['ok'], k, axis)
    with np.errstate(invalid='ignore', over='ignore'):
        g = np.where(read[:, None], (scale[:, None, None, None] * acc).astype(F32), F32(0.0)).astype(F32)
        a = np.where(read[:, None], np.abs(scale)[:, None, None, None] * absacc, 0.0)
    return g, a, read


def ulp32(x):
    """The spacing of float32 at |x| (of the smallest normal below it)"""
    x = np.maximum(np.abs(np.asarray(x, np.float64)), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(x)) - 23)


def grad_bound(want, big_a):
    """The gradient's bar per element: 2^-22 of the sum of the absolute contributions plus one float32 step of the value"""
    return 2.0 ** -22 * big_a + ulp32(want)


# ---- the native call served by this module (host-logic tests) -----------------------------------------------------------------------
def fake_flow_smoothness(vecs, mask=None, img=None, order=1, alpha=10.0, eps=0.001, want_map=False):
    import torch
    res = compute(vecs.detach().numpy(), None if mask is None else mask.numpy(), None if img is None else img.numpy(), order, alpha, eps)
    return torch.from_numpy(res['records']), (torch.from_numpy(res['map']) if want_map else None)
