"""NumPy oracle of Flow.error_stats / epe_map / epe, written from DESIGN.md 3.16 alone.

Per pixel, every step float32 with one rounding per operation: du = u - ug, dv = v - vg, e = sqrt(du du + dv dv), g = sqrt(ug ug + vg vg)
(np.sqrt on float32 is correctly rounded); a pixel counts where both masks are True (None: all True).  Counts are exact integers, sums are
`math.fsum` of the float32 e: the correctly rounded float64 sum, whatever the order.  The gradient is computed per element in float64.
"""
import numpy as np

import special_values as sv

RECORD = 16
FL_ABS, FL_REL = np.float32(3.0), np.float32(0.05)
SPEED_EDGES = (np.float32(10.0), np.float32(40.0))
DEFAULT_THRESHOLDS = (1, 3, 5)


def _f32(a):
    a = np.asarray(a)
    return a.astype(np.float32)          # (float16 -> float32 is exact)


def valid_of(shape, est_mask, gt_mask):
    valid = np.ones(shape, dtype=bool)
    for m in (est_mask, gt_mask):
        if m is not None:
            valid &= np.broadcast_to(np.asarray(m).astype(bool), shape)
    return valid


def pixel_terms(est, gt):
    """(du, dv, e, g) float32 [N,H,W] of vectors [N,2,H,W]"""
    est, gt = _f32(est), _f32(gt)
    with np.errstate(over='ignore', invalid='ignore'):
        du, dv = est[:, 0] - gt[:, 0], est[:, 1] - gt[:, 1]
        e = np.sqrt(du * du + dv * dv)
        g = np.sqrt(gt[:, 0] * gt[:, 0] + gt[:, 1] * gt[:, 1])
    assert e.dtype == np.float32 and g.dtype == np.float32
    return du, dv, e, g


def score(est, gt, est_mask=None, gt_mask=None, thresholds=DEFAULT_THRESHOLDS):
    """dict: 'map' float32 [N,H,W] (0 where not valid), 'count' / 'n_over' [N,K] / 'n_fl' / 'speed_count' [N,3] int64, 'sum' / 'max' /
    'speed_sum' [N,3] float64 -- and 'records' float64 [N,16] in the layout of include/oflib_hip.h"""
    du, dv, e, g = pixel_terms(est, gt)
    n = e.shape[0]
    valid = valid_of(e.shape, est_mask, gt_mask)
    thr = [np.float32(t) for t in thresholds]
    assert len(thr) <= 4
    out = dict(map=np.where(valid, e, np.float32(0)).astype(np.float32), count=np.zeros(n, np.int64), sum=np.zeros(n), max=np.zeros(n),
               n_over=np.zeros((n, len(thr)), np.int64), n_fl=np.zeros(n, np.int64), speed_count=np.zeros((n, 3), np.int64),
               speed_sum=np.zeros((n, 3)), records=np.zeros((n, RECORD)))
    for i in range(n):
        ev, gv = e[i][valid[i]], g[i][valid[i]]
        out['count'][i] = ev.size
        out['sum'][i] = sv.record_sum(ev)                                                # (total on NaN / inf terms: special_values.py)
        out['max'][i] = sv.record_max(ev)
        for k, t in enumerate(thr):
            out['n_over'][i, k] = int(np.count_nonzero(ev > t))
        out['n_fl'][i] = int(np.count_nonzero((ev > FL_ABS) & (ev > FL_REL * gv)))       # the product in float32: no division at g = 0
        bins = [gv < SPEED_EDGES[0], (gv >= SPEED_EDGES[0]) & (gv < SPEED_EDGES[1]), ~(gv < SPEED_EDGES[1])]
        for b, sel in enumerate(bins):
            out['speed_count'][i, b] = int(np.count_nonzero(sel))
            out['speed_sum'][i, b] = sv.record_sum(ev[sel])
        r = out['records'][i]
        r[0], r[1], r[2], r[7] = out['count'][i], out['sum'][i], out['max'][i], out['n_fl'][i]
        r[3:3 + len(thr)] = out['n_over'][i]
        r[8:11], r[11:14] = out['speed_count'][i], out['speed_sum'][i]
    return out


def epe_grad(est, gt, est_mask, gt_mask, scale):
    """float64 [N,2,H,W]: scale[n] * (du, dv) / sqrt(du du + dv dv) from the float32 differences, every further step float64; exactly 0
    where a pixel is not valid or its float32 e is 0"""
    du, dv, e, _ = pixel_terms(est, gt)
    valid = valid_of(e.shape, est_mask, gt_mask) & (e > 0)
    dx, dy = du.astype(np.float64), dv.astype(np.float64)
    sc = np.asarray(scale, dtype=np.float32).astype(np.float64).reshape(-1, 1, 1)
    with np.errstate(divide='ignore', invalid='ignore'):
        e64 = np.sqrt(dx * dx + dy * dy)
        gu, gv = (sc * dx) / e64, (sc * dy) / e64
    return np.stack([np.where(valid, gu, 0.0), np.where(valid, gv, 0.0)], axis=1)


# ---- the two native primitives, served by the oracle (CPU tier: monkeypatched over oflibpytorch_amd._native) -------------------------
def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def fake_flow_error(est, gt, est_mask=None, gt_mask=None, thresholds=(), want_map=False):
    import torch
    res = score(_np(est), _np(gt), _np(est_mask), _np(gt_mask), tuple(thresholds))
    return torch.from_numpy(res['records']), (torch.from_numpy(res['map']) if want_map else None)


def fake_flow_epe_grad(est, gt, est_mask, gt_mask, scale, want_est=True, want_gt=False):
    import torch
    g = epe_grad(_np(est), _np(gt), _np(est_mask), _np(gt_mask), _np(scale)).astype(np.float32)
    return (torch.from_numpy(g) if want_est else None), (torch.from_numpy(-g) if want_gt else None)
