"""The sequence loss of DESIGN.md 3.30 in NumPy (a helper module, not a test; the tests of Flow.sequence_loss import it).

The definition, per pixel in float32 with one rounding per operation:
    mag = sqrt(ug ug + vg vg);  valid = m and mag < (float32)max_flow          (a float compare: NaN and inf fail it)
    du = u_i - ug, dv = v_i - vg;  e_i = sqrt(du du + dv dv);  t_i = |du| + |dv| ('l1') or e_i ('l2')
and per image a record of 2 T + 4 float64 values over its valid pixels: [0] count, [1 + i] sum t_i, [1 + T + i] sum e_i,
[1 + 2 T + k] #(e_{T-1} < 1, 3, 5).  The sums here are `math.fsum` of the float32 terms: the correctly rounded sum, which any order of
float64 additions reproduces bit for bit on the exact inputs (`require_exact`) and approaches within count * 2^-52 relative on general
ones (the terms are >= 0).  loss_n = (sum_i gamma^(T-1-i) S_{n,i}) / D_n with D the number of terms of the mean.

`wide=True` evaluates the same expressions in float64 throughout: what RAFT's loop in torch float64 computes.  `mutant` names a deliberate
error (MUTANTS) that the host tests must tell apart.
"""
import math

import numpy as np
import torch

MAX_T = 32
CHUNK = 2048                                   # OFL_SEQUENCE_LOSS_CHUNK: the pixels a block of the kernels owns
WITHIN = (1.0, 3.0, 5.0)
MUTANTS = ("weights-reversed", "magnitude-of-prediction", "inclusive-max-flow", "divisor-without-2")
FLT_MAX = float(np.finfo(np.float32).max)


def ulp32(x):
    """The spacing of float32 at |x| (float64 array), at least that of the smallest normal"""
    x = np.maximum(np.abs(np.asarray(x, np.float64)), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(x)) - 23)


def weights(t, gamma):
    return [gamma ** (t - 1 - i) for i in range(t)]


def _f32(a):
    return np.asarray(a).astype(np.float32)                # (float16 -> float32 is exact)


def valid_of(gt, mask, max_flow, wide=False, inclusive=False):
    ft = np.float64 if wide else np.float32
    g = _f32(gt).astype(ft)
    with np.errstate(all='ignore'):
        mag = np.sqrt(g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1])
        below = (mag <= ft(np.float32(max_flow))) if inclusive else (mag < ft(np.float32(max_flow)))
    m = np.ones(mag.shape, bool) if mask is None else np.asarray(mask, bool)
    return m & below


def terms_of(pred, gt, penalty, wide=False):
    """(t, e, du, dv) of one prediction, [N,H,W] each"""
    ft = np.float64 if wide else np.float32
    p, g = _f32(pred).astype(ft), _f32(gt).astype(ft)
    with np.errstate(all='ignore'):
        du, dv = p[:, 0] - g[:, 0], p[:, 1] - g[:, 1]
        e = np.sqrt(du * du + dv * dv)
        t = e if penalty == 'l2' else np.abs(du) + np.abs(dv)
    return t, e, du, dv


def _fsum(values):
    values = [float(v) for v in values]
    if any(math.isnan(v) for v in values):
        return float('nan')
    if any(math.isinf(v) for v in values):
        return float('inf')                                  # (the terms are >= 0)
    return math.fsum(values)


def compute(preds, gt, mask=None, max_flow=400.0, penalty='l1', wide=False, mutant=None):
    """dict: 'valid' bool [N,H,W] (a list of T of them under the mutant that tests the predictions), 't' and 'e' [T,N,H,W], 'record'
    float64 [N, 2 T + 4]"""
    t_count = len(preds)
    n = np.asarray(gt).shape[0]
    valid = valid_of(gt, mask, max_flow, wide, inclusive=mutant == "inclusive-max-flow")
    valids = [valid_of(p, mask, max_flow, wide) if mutant == "magnitude-of-prediction" else valid for p in preds]
    ts, es = [], []
    rec = np.zeros((n, 2 * t_count + 4), np.float64)
    for i, pred in enumerate(preds):
        t, e, _, _ = terms_of(pred, gt, penalty, wide)
        ts.append(t)
        es.append(e)
        for k in range(n):
            v = valids[i][k]
            rec[k, 1 + i] = _fsum(t[k][v])
            rec[k, 1 + t_count + i] = _fsum(e[k][v])
            if i == t_count - 1:
                for j, thr in enumerate(WITHIN):
                    with np.errstate(invalid='ignore'):
                        rec[k, 1 + 2 * t_count + j] = float((v & (e[k] < e.dtype.type(thr))).sum())
    rec[:, 0] = valid.reshape(n, -1).sum(1)
    return {'valid': valid, 't': np.stack(ts), 'e': np.stack(es), 'record': rec}


def divisor(record, hw, penalty, normalise, mutant=None):
    per_pixel = 2.0 if (penalty == 'l1' and mutant != "divisor-without-2") else 1.0
    return np.full(record.shape[0], per_pixel * hw) if normalise == 'all' else record[:, 0] * per_pixel


def loss64(record, hw, gamma=0.8, penalty='l1', normalise='all', mutant=None):
    """loss_n in float64 [N]"""
    t = (record.shape[1] - 4) // 2
    w = np.array(weights(t, gamma)[::-1] if mutant == "weights-reversed" else weights(t, gamma), np.float64)
    with np.errstate(all='ignore'):
        return (record[:, 1:1 + t] * w).sum(1) / divisor(record, hw, penalty, normalise, mutant)


def scale_of(g, record, hw, gamma, penalty, normalise):
    """(float32 [N,T], float64 [N,T] before the rounding): g_n w_i / D_n"""
    t = (record.shape[1] - 4) // 2
    w = np.array(weights(t, gamma), np.float64)
    with np.errstate(all='ignore'):
        s = (np.asarray(g, np.float64)[:, None] * w[None, :]) / divisor(record, hw, penalty, normalise)[:, None]
        return s.astype(np.float32), s


def grad_of(du, dv, valid, sc, penalty):
    """The gradient of one prediction from its differences [N,H,W], the valid pixels and scale[:, i] [N] (float32 by the definition):
    float64 [N,2,H,W], to be rounded once.  'l1': +-scale by the sign of the difference, +0 at 0 and NaN; 'l2': the float64 quotient
    (scale d) / sqrt(du du + dv dv), +0 where the sum of squares in the differences' own precision is not > 0; +0 where not valid"""
    d, v = np.stack([du, dv], 1), valid[:, None]
    s = np.asarray(sc)[:, None, None, None]
    with np.errstate(all='ignore'):
        if penalty == 'l1':
            return np.where(v & (d > 0), s, np.where(v & (d < 0), -s, s.dtype.type(0.0))).astype(np.float64)
        d64 = d.astype(np.float64)
        e64 = np.sqrt(d64[:, 0] * d64[:, 0] + d64[:, 1] * d64[:, 1])[:, None]
        return np.where(v & ((du * du + dv * dv) > 0)[:, None], (s.astype(np.float64) * d64) / e64, 0.0)


def grads(preds, gt, mask, max_flow, penalty, normalise, gamma, g, wide=False):
    """The gradient with respect to every prediction, [T][N,2,H,W]: float32 by the definition, float64 with `wide`"""
    r = compute(preds, gt, mask, max_flow, penalty, wide)
    hw = r['valid'].shape[1] * r['valid'].shape[2]
    s32, s64 = scale_of(g, r['record'], hw, gamma, penalty, normalise)
    out = []
    for i, pred in enumerate(preds):
        _, _, du, dv = terms_of(pred, gt, penalty, wide)
        out.append(grad_of(du, dv, r['valid'], (s64 if wide else s32)[:, i], penalty).astype(np.float64 if wide else np.float32))
    return out


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def masks(n, h, w, seed=3):
    """bool [N,H,W] with about 20 % holes (none for a frame of one pixel)"""
    m = np.random.RandomState(seed).uniform(size=(n, h, w)) > 0.2
    m.reshape(n, -1)[:, 0] = True
    return m


def vectors_general(t, n, h, w, sigma=3.0, seed=11):
    """(T predictions, the ground truth): N(0, sigma) float32, the predictions approaching the ground truth with i"""
    rs = np.random.RandomState(seed)
    gt = rs.normal(0.0, sigma, (n, 2, h, w)).astype(np.float32)
    preds = [(gt + rs.normal(0.0, sigma * (t - i) / t, gt.shape)).astype(np.float32) for i in range(t)]
    return preds, gt


def vectors_exact(t, n, h, w, seed=17, spread=16.0, cells=64.0):
    """The same on a grid of 1 / `cells` (2^-6, or a coarser power of two: with gamma = 0.5 the weight of the first of 32 predictions is
    2^-31, and the weighted sum of the loss stays exact only if the sums have few low bits) with every magnitude below 2^10: every 'l1'
    term is a multiple of 2^-6 below 2^12"""
    rs = np.random.RandomState(seed)
    grid = lambda a: (np.round(np.clip(a, -500.0, 500.0) * cells) / cells).astype(np.float32)     # noqa: E731
    gt = grid(rs.normal(0.0, spread, (n, 2, h, w)))
    preds = [grid(gt + rs.normal(0.0, spread * (t - i) / t, gt.shape)) for i in range(t)]
    return preds, gt


def vectors_pythagorean(t, n, h, w, seed=19, cells=64.0):
    """Exact inputs for 'l2': every difference is a multiple k (3, 4) / cells or (5, 12) / cells ... of a Pythagorean pair, k an integer
    in 1 .. cells and 0 < e < 2^5: every e is an exact multiple of 1 / cells (2^-6 or a coarser power of two), and so is every sum"""
    rs = np.random.RandomState(seed)
    pairs = np.array([(3, 4), (4, 3), (5, 12), (12, 5), (8, 15), (-3, 4), (4, -3), (-5, -12), (0, 1), (1, 0)], np.float64)
    gt = (np.round(rs.normal(0.0, 16.0, (n, 2, h, w)) * cells) / cells).astype(np.float32)
    preds = []
    for i in range(t):
        pick = pairs[rs.randint(0, len(pairs), (n, h, w))]                      # [N,H,W,2]
        k = rs.randint(1, int(cells) + 1, (n, h, w))[..., None]
        d = np.moveaxis(pick * k / cells, -1, 1)
        preds.append((gt.astype(np.float64) + d).astype(np.float32))
    return preds, gt


def plant(preds, gt, mask, max_flow=400.0):
    """Named pixels (in place; frames of at least 8 pixels): pixel 1 has a magnitude of exactly max_flow = 400 (not valid); at pixels
    2, 3, 4 the LAST prediction is off by exactly 1, 3 and 5 px (not within); pixel 5 is off by exactly 0 in every prediction"""
    assert max_flow == 400.0
    n, _, h, w = gt.shape
    flat = lambda a: a.reshape(n, 2, h * w)                                      # noqa: E731
    g = flat(gt)
    old = g[:, :, 1:5].copy()
    g[:, 0, 1], g[:, 1, 1] = 240.0, 320.0
    g[:, :, 2:5] = np.float32(8.0)
    for p in preds:                                                              # the predictions move along: their differences stay
        flat(p)[:, :, 1:5] += g[:, :, 1:5] - old                                 # (exact on the grid of 2^-6)
    for k, (dx, dy) in zip((2, 3, 4), ((1.0, 0.0), (0.0, 3.0), (3.0, 4.0))):
        flat(preds[-1])[:, 0, k] = g[:, 0, k] + np.float32(dx)
        flat(preds[-1])[:, 1, k] = g[:, 1, k] + np.float32(dy)
    for p in preds:
        flat(p)[:, :, 5] = g[:, :, 5]
    if mask is not None:
        mask.reshape(n, h * w)[:, 1:6] = True


def require_exact(preds, gt, mask, max_flow, penalty, gamma=None, normalise='all'):
    """Fail unless every float64 sum of the record -- and, with `gamma`, the weighted sum of the loss -- is exact in ANY order of
    additions.  'l1': all vectors on the grid of 2^-6 with magnitude below 2^10, so every term is a multiple of 2^-6 below 2^12 and any
    sum of fewer than 2^20 of them is exact.  Both penalties: ceil(log2 count) + 24 + (the exponent span of the summed float32 terms)
    <= 53.  The loss: the span from the lowest set bit of any w_i S_i to the exponent of their sum is at most 53 bits."""
    r = compute(preds, gt, mask, max_flow, penalty)
    assert r['valid'].reshape(len(gt), -1).sum(1).max() < 2 ** 20
    if penalty == 'l1':
        for a in list(preds) + [gt]:
            a = _f32(a).astype(np.float64)
            assert np.array_equal(a * 64.0, np.round(a * 64.0)) and np.abs(a).max() < 2.0 ** 10
    for k in range(len(gt)):
        v = r['valid'][k]
        count = int(v.sum())
        for name in ('t', 'e') if penalty == 'l1' else ('e',):
            x = r[name][:, k][:, v].astype(np.float64)
            x = x[x > 0]
            if x.size == 0:
                continue
            assert np.isfinite(x).all()
            span = int(np.floor(np.log2(x.max()))) - int(np.floor(np.log2(x.min())))
            assert math.ceil(math.log2(max(count, 1))) + 24 + span <= 53, "the %s sums of image %d are not exact in any order" % (name, k)
    if gamma is not None:
        t = len(preds)
        for k in range(len(gt)):
            prods = [wi * s for wi, s in zip(weights(t, gamma), r['record'][k, 1:1 + t]) if s > 0]
            if not prods:
                continue
            assert all(math.frexp(wi)[0] == 0.5 for wi in weights(t, gamma)), "the weights need to be powers of two"
            lowest = min(math.frexp(p)[1] - 53 + _trailing_zeros(p) for p in prods)
            top = math.frexp(math.fsum(prods))[1]
            assert top - lowest <= 53, "the weighted sum of image %d is not exact in any order" % k


def _trailing_zeros(x):
    m = int(math.frexp(x)[0] * 2 ** 53)
    return (m & -m).bit_length() - 1


# ---- the oracle in the bindings' place (host tests) -------------------------------------------------------------------------------------
def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def fake_flow_sequence_loss(preds, gt, gt_mask=None, max_flow=400.0, penalty='l1', normalise='all'):
    return torch.from_numpy(compute([_np(p) for p in preds], _np(gt), _np(gt_mask), max_flow, penalty)['record'])


def fake_flow_sequence_loss_grad(preds, gt, gt_mask, max_flow, penalty, normalise, scale, wants):
    ps, g, m = [_np(p) for p in preds], _np(gt), _np(gt_mask)
    valid = valid_of(g, m, max_flow)
    sc = _np(scale).astype(np.float32)
    out = []
    for i, want in enumerate(wants):
        if not want:
            out.append(None)
            continue
        _, _, du, dv = terms_of(ps[i], g, penalty)
        out.append(torch.from_numpy(np.ascontiguousarray(grad_of(du, dv, valid, sc[:, i], penalty).astype(np.float32))))
    return out
