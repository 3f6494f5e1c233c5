"""The definition of Flow.photometric / photometric_map / photometric_stats in NumPy (a helper module, not a test; test
modules import it), and the inputs the CPU and the GPU tier share.

The sampled image Iw and the weight test mr > 0.99999 come from `oracle_backend.warp_bwd(..., want_valid=True)` (the C oracle of the
backward warp, which the reference pins); everything after it is elementwise np.float32 arithmetic, one rounding per operation; the sums
of a record are math.fsum (exact, rounded once).  The gradient is float64 on the float32 d of the forward, with the fractions and the
inside tests of `grad_oracle64.warp_taps`; next to it `grad` returns, per element, A = |scale| sum_c sum_j |q_c fr_j v_jc| / C, the sum
of the absolute contributions (they can cancel, so a bound on the gradient's error is relative to A, not to the gradient).
"""
import functools

import numpy as np
import torch

import consistency_oracle as co
import grad_oracle64 as go
import oracle_backend as ob
import special_values as sv

F32 = np.float32
# (n, h, w): the smallest frame; one row / column pair; odd and smaller than a wave; 8 x 12 and up show every category
# (test_photometric_host.py); 20 x 28 = 3 blocks; odd sizes, several blocks; a row of 4 waves, 64 rows of it, and one past both; 1080p:
# every block walks 31 or 32 rounds
SMALL = [(1, 2, 2), (2, 2, 5), (2, 5, 2), (2, 5, 7)]
TABLE = [(3, 8, 12), (2, 20, 28), (3, 37, 53), (2, 67, 131), (2, 64, 256), (2, 65, 257)]
LARGE = (1, 1080, 1920)
FRAMES = SMALL + TABLE + [LARGE]
UPSTREAM = (0.75, -2.0, 1.0)
REFS = ('s', 't')


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def flow_scale(h, w):
    """The factor on the vectors of `consistency_oracle.case`: at 0.1 the samples of the smallest frames stay inside them"""
    return 0.1 if h * w < 64 else 1.0


@functools.lru_cache(maxsize=None)
def case(n, h, w, ref):
    """(a float32 [n,2,h,w], a_mask bool [n,h,w], img, other float32 [n,3,h,w] uniform in [0, 1), img_u8, other_u8 = floor(256 img)),
    read-only and computed once."""
    got = co.case(n, h, w, ref, flow_scale(h, w))
    a, a_mask = got[0], got[2]
    rng = np.random.RandomState(4421 + 1000 * n + 10 * h + w + (0 if ref == 's' else 7))
    img = rng.uniform(size=(n, 3, h, w)).astype(F32)
    other = rng.uniform(size=(n, 3, h, w)).astype(F32)
    img, other = np.minimum(img, np.nextafter(F32(1), F32(0))), np.minimum(other, np.nextafter(F32(1), F32(0)))
    img_u8, other_u8 = np.floor(256.0 * img).astype(np.uint8), np.floor(256.0 * other).astype(np.uint8)
    for arr in (img, other, img_u8, other_u8):
        arr.setflags(write=False)
    return a, a_mask, img, other, img_u8, other_u8


def images(n, h, w, ref, kind):
    """(img, other) of `case` as the kind names it: 'f32c3', 'u8c3', 'f32c1' (channel 0 alone), 'chw' (image 0, broadcast)"""
    _, _, img, other, img_u8, other_u8 = case(n, h, w, ref)
    if kind == 'u8c3':
        return img_u8, other_u8
    if kind == 'f32c1':
        return np.ascontiguousarray(img[:, :1]), np.ascontiguousarray(other[:, :1])
    if kind == 'chw':
        return img[0], other[0]
    assert kind == 'f32c3'
    return img, other


# ---- the definition -------------------------------------------------------------------------------------------------------------------
def _as_f32(flow):
    flow = np.asarray(flow)
    assert flow.dtype in (np.float32, np.float16) and flow.ndim == 4 and flow.shape[1] == 2
    return np.ascontiguousarray(flow.astype(F32))             # fp16 storage is up-converted exactly


def _as_image(img, n):
    """float32 [n, C, H, W]; a uint8 sample s is float(s) / 255.0f; C-H-W broadcasts over the batch"""
    img = np.asarray(img)
    assert img.dtype in (np.float32, np.uint8) and img.ndim in (3, 4) and 1 <= img.shape[-3] <= 4
    if img.ndim == 3:
        img = img[None]
    assert img.shape[0] in (1, n)
    img = img.astype(F32) / F32(255.0) if img.dtype == np.uint8 else img
    return np.ascontiguousarray(np.broadcast_to(img, (n,) + img.shape[1:]))


def sign_of(ref):
    assert ref in REFS
    return -1.0 if ref == 's' else 1.0


def compute(a, mask, img, other, ref, eps=0.001):
    """dict: 'map' float32 [N,H,W] (+0 where not known); 'known' bool [N,H,W]; 'inside' bool (the weight test alone); 'd' float32
    [N,C,H,W]; 'records' float64 [N,8]; 'photometric' float32 [N]"""
    assert np.asarray(img).dtype == np.asarray(other).dtype
    f = _as_f32(a)
    n, _, h, w = f.shape
    im, ot = _as_image(img, n), _as_image(other, n)
    assert im.shape == ot.shape and im.shape[2:] == (h, w)
    chan = im.shape[1]
    out, valid, _, _ = ob.warp_bwd(torch.from_numpy(f.copy()), torch.from_numpy(ot.copy()), flow_sign=sign_of(ref), want_valid=True)
    iw, inside = out.numpy(), valid.numpy().astype(bool)
    known = inside if mask is None else inside & np.asarray(mask, bool)
    e = F32(eps)
    with np.errstate(all='ignore'):
        ee = e * e
        d = iw - im
        s = np.zeros((n, h, w), F32)
        for c in range(chan):                                 # channels in ascending order, then one division
            s = s + np.sqrt(d[:, c] * d[:, c] + ee)
        rho = s / F32(chan)
    assert d.dtype == F32 and rho.dtype == F32 and type(ee) is F32
    pmap = np.where(known, rho, F32(0.0)).astype(F32)
    rec = np.zeros((n, 8), np.float64)
    for i in range(n):
        vals = rho[i][known[i]].astype(np.float64)
        rec[i, :3] = [vals.size, sv.record_sum(vals), sv.record_max(vals)]          # (total on NaN / inf terms: special_values.py)
    with np.errstate(invalid='ignore', divide='ignore'):
        loss = (rec[:, 1] / rec[:, 0]).astype(F32)
    return {'map': pmap, 'known': known, 'inside': inside, 'd': d, 'records': rec, 'photometric': loss}


def grad(a, mask, img, other, ref, eps=0.001, upstream=UPSTREAM):
    """(want float64 [N,2,H,W], A float64 [N,2,H,W]) of sum_n upstream[n] * photometric[n] with respect to the vectors"""
    res = compute(a, mask, img, other, ref, eps)
    f = _as_f32(a)
    n, _, h, w = f.shape
    ot = _as_image(other, n).astype(np.float64).reshape(n, -1, h * w)
    chan = ot.shape[1]
    sign = sign_of(ref)
    taps = go.warp_taps(f, n, sign)
    up = np.asarray(upstream[:n], F32).astype(np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        scale = (up / res['records'][:, 0]).astype(F32).astype(np.float64)                 # the fp32 device tensor
    ee = np.float64(F32(eps)) * np.float64(F32(eps))
    d = res['d'].astype(np.float64)
    den = np.sqrt(d * d + ee)
    with np.errstate(invalid='ignore', divide='ignore'):
        q = np.where(den != 0.0, d / den, 0.0)                                             # [n, C, h, w]
    acc, absacc = np.zeros((2, n, h, w)), np.zeros((2, n, h, w))
    for c in range(chan):
        g, ga = np.zeros((2, n, h, w)), np.zeros((2, n, h, w))
        for j in range(4):                                                                  # nw, ne, sw, se
            v = np.where(taps.ok[j], np.take_along_axis(ot[:, c], taps.idx[j].reshape(n, -1), 1).reshape(n, h, w), 0.0)
            for axis, (sg, fr) in enumerate((taps.dx[j], taps.dy[j])):
                with np.errstate(invalid='ignore'):
                    t = np.where(taps.ok[j], fr * v, 0.0)
                g[axis] += sg * t
                ga[axis] += np.abs(t)
        acc += q[:, c] * g
        absacc += np.abs(q[:, c]) * ga
    known = res['known'][:, None]
    with np.errstate(invalid='ignore', over='ignore'):
        want = np.where(known, (scale[:, None, None, None] * (-sign)) * (acc.transpose(1, 0, 2, 3) / float(chan)), 0.0)
        big_a = np.where(known, np.abs(scale)[:, None, None, None] * (absacc.transpose(1, 0, 2, 3) / float(chan)), 0.0)
    return want, big_a


def ulp32(x):
    """The spacing of float32 at |x| (of the smallest normal below it)"""
    x = np.maximum(np.abs(np.asarray(x, np.float64)), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(x)) - 23)


def grad_bound(want, big_a):
    """The gradient's bar per element: 2^-22 of the sum of the absolute contributions plus one float32 step of the value"""
    return 2.0 ** -22 * big_a + ulp32(want)


def categories(n, h, w, ref):
    """Per image of a case, the share of its pixels that are known, unknown because the sample leaves the frame, unknown by the mask
    alone: three float arrays [n]"""
    a, a_mask, img, other, _, _ = case(n, h, w, ref)
    res = compute(a, a_mask, img, other, ref)
    total = float(h * w)
    return (res['known'].sum((1, 2)) / total, (~res['inside']).sum((1, 2)) / total, (res['inside'] & ~res['known']).sum((1, 2)) / total)


# ---- the native call served by this module (host-logic tests) -----------------------------------------------------------------------
def fake_flow_photometric(vecs, mask, img, other, flow_sign=-1.0, eps=0.001, want_map=False, want_record=True):
    res = compute(vecs.detach().numpy(), None if mask is None else mask.numpy(), img.numpy(), other.numpy(),
                  's' if flow_sign < 0 else 't', eps)
    return (torch.from_numpy(res['records']) if want_record else None), (torch.from_numpy(res['map']) if want_map else None)
