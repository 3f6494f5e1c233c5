"""NumPy restatement of DESIGN.md section 3.10 (Flow.matrix) -- the checker of ofl_matrix.hip.

Everything discrete is reproduced exactly: the draws (splitmix64 of a counter), the minimal solves (scalar float64 operations in
the documented order), the fp32 residuals (NumPy's fp32 arithmetic rounds every operation, as the kernels do without contraction),
the inlier tests, the medians, the winner.  The least-squares sums are taken with math.fsum (exactly rounded), so the matrices
differ from the kernels' only through the order of the kernels' float64 sums.  Restated, not checked against OpenCV."""
import math

import numpy as np

K_RANSAC, K_LMEDS = 256, 128
SEED = 0x0F1E2D3C4B5A6978
RANSAC_THR = np.float32(9.0)
METHODS = {'lms': 0, 'ransac': 1, 'lmeds': 2}
ST_OK, ST_FEW_POINTS, ST_NO_HYPOTHESIS, ST_REFIT_SINGULAR = 0, 1, 2, 3
_M64 = (1 << 64) - 1
_FLT_MAX = float(np.finfo(np.float32).max)


def draw_hash(k, j):
    z = (SEED + (k * 8 + j + 1) * 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def point_pairs(flow, ref):
    """flow [2,H,W] (fp32 or fp16) -> src, dst float64 [H*W, 2] (flow_class.py:1600-1610)"""
    _, h, w = flow.shape
    v = flow.astype(np.float64)
    gy, gx = np.mgrid[:h, :w].astype(np.float64)
    if ref == 's':
        src = np.stack([gx, gy], -1)
        dst = np.stack([gx + v[0], gy + v[1]], -1)
    else:
        dst = np.stack([gx, gy], -1)
        src = np.stack([gx - v[0], gy - v[1]], -1)
    return src.reshape(-1, 2), dst.reshape(-1, 2)


def residuals(hm, src32, dst32, proj):
    """fp32 squared reprojection residuals of the fp32 model hm[9]; not finite -> +inf"""
    sx, sy, dx, dy = src32[:, 0], src32[:, 1], dst32[:, 0], dst32[:, 1]
    with np.errstate(all='ignore'):
        px = (hm[0] * sx + hm[1] * sy) + hm[2]
        py = (hm[3] * sx + hm[4] * sy) + hm[5]
        if proj:
            wz = (hm[6] * sx + hm[7] * sy) + hm[8]
            px = px / wz
            py = py / wz
        ex, ey = px - dx, py - dy
        r = ex * ex + ey * ey
        return np.where(r <= np.float32(_FLT_MAX), r, np.float32(np.inf)).astype(np.float32)


def gauss_solve(a, b):
    """Gaussian elimination with partial pivoting in the documented order; a: n x n, b: n x nr lists of Python floats.
    -> x (n x nr) or None."""
    n, nr = len(a), len(b[0])
    a = [list(r) for r in a]
    b = [list(r) for r in b]
    for col in range(n):
        piv, best = col, abs(a[col][col])
        for i in range(col + 1, n):
            if abs(a[i][col]) > best:
                best, piv = abs(a[i][col]), i
        if not (best > 0.0) or not (best <= 1.7976931348623157e308):
            return None
        if piv != col:
            a[col], a[piv] = a[piv], a[col]
            b[col], b[piv] = b[piv], b[col]
        for i in range(col + 1, n):
            f = a[i][col] / a[col][col]
            for j in range(col + 1, n):
                a[i][j] -= f * a[col][j]
            for r in range(nr):
                b[i][r] -= f * b[col][r]
    x = [[0.0] * nr for _ in range(n)]
    for r in range(nr):
        for i in range(n - 1, -1, -1):
            s = b[i][r]
            for j in range(i + 1, n):
                s -= a[i][j] * x[j][r]
            x[i][r] = _div(s, a[i][i])
    return x


def _div(a, b):
    try:
        return a / b
    except ZeroDivisionError:
        return math.nan if a == 0 or a != a else math.copysign(math.inf, a) * math.copysign(1.0, b)
    except OverflowError:
        return math.inf


def _collinear(a, b, c):
    t1 = (b[0] - a[0]) * (c[1] - a[1])
    t2 = (b[1] - a[1]) * (c[0] - a[0])
    return abs(t1 - t2) <= 1e-6 * (abs(t1) + abs(t2))


def hypothesis(k, m, valid_idx, src, dst):
    """-> fp32 model [9] or None (invalid)"""
    nv = len(valid_idx)
    q = [int(valid_idx[draw_hash(k, j) % nv]) for j in range(m)]
    if len(set(q)) < m:
        return None
    s = [(float(src[i, 0]), float(src[i, 1])) for i in q]
    d = [(float(dst[i, 0]), float(dst[i, 1])) for i in q]
    for c in range(2, m):
        for b in range(1, c):
            for a in range(b):
                if _collinear(s[a], s[b], s[c]) or _collinear(d[a], d[b], d[c]):
                    return None
    hm = [0.0] * 8 + [1.0]
    if m == 2:
        ex, ey, fu, fv = s[1][0] - s[0][0], s[1][1] - s[0][1], d[1][0] - d[0][0], d[1][1] - d[0][1]
        den = ex * ex + ey * ey
        if not den > 0.0:
            return None
        a, b = (ex * fu + ey * fv) / den, (ex * fv - ey * fu) / den
        hm[0], hm[1], hm[2] = a, -b, d[0][0] - (a * s[0][0] - b * s[0][1])
        hm[3], hm[4], hm[5] = b, a, d[0][1] - (b * s[0][0] + a * s[0][1])
    elif m == 3:
        x = gauss_solve([[s[j][0], s[j][1], 1.0] for j in range(3)], [[d[j][0], d[j][1]] for j in range(3)])
        if x is None:
            return None
        hm[0], hm[1], hm[2] = x[0][0], x[1][0], x[2][0]
        hm[3], hm[4], hm[5] = x[0][1], x[1][1], x[2][1]
    else:
        a, b = [], []
        for j in range(4):
            a.append([s[j][0], s[j][1], 1.0, 0.0, 0.0, 0.0, -(d[j][0] * s[j][0]), -(d[j][0] * s[j][1])])
            a.append([0.0, 0.0, 0.0, s[j][0], s[j][1], 1.0, -(d[j][1] * s[j][0]), -(d[j][1] * s[j][1])])
            b.append([d[j][0]])
            b.append([d[j][1]])
        x = gauss_solve(a, b)
        if x is None:
            return None
        for i in range(8):
            hm[i] = x[i][0]
    if not all(abs(v) <= _FLT_MAX for v in hm):
        return None
    return np.array(hm, np.float64).astype(np.float32)


def _fsum(a):
    return math.fsum(a.tolist())


def least_squares(src, dst, dof, h, w):
    """float64 fit over the given pairs, in the coordinates shifted by the image centre.  -> (3 x 3, status)"""
    n = len(src)
    if n < dof // 2:
        return None, ST_FEW_POINTS
    cx, cy = 0.5 * (w - 1), 0.5 * (h - 1)
    x, y, u, v = src[:, 0] - cx, src[:, 1] - cy, dst[:, 0] - cx, dst[:, 1] - cy
    cnt = float(n)
    sx, sy, su, sv = _fsum(x), _fsum(y), _fsum(u), _fsum(v)
    sxx, sxy, syy = _fsum(x * x), _fsum(x * y), _fsum(y * y)
    m = np.eye(3)
    tc = np.array([[1, 0, cx], [0, 1, cy], [0, 0, 1.0]])
    tci = np.array([[1, 0, -cx], [0, 1, -cy], [0, 0, 1.0]])
    if dof in (4, 6):
        sxu, sxv, syu, syv = _fsum(x * u), _fsum(x * v), _fsum(y * u), _fsum(y * v)
        if dof == 4:
            mx, my, mu, mv = sx / cnt, sy / cnt, su / cnt, sv / cnt
            den = (sxx - sx * mx) + (syy - sy * my)
            if not den > 0.0:
                return None, ST_REFIT_SINGULAR
            a = ((sxu - sx * mu) + (syv - sy * mv)) / den
            b = ((sxv - sx * mv) - (syu - sy * mu)) / den
            m[0] = [a, -b, mu - (a * mx - b * my)]
            m[1] = [b, a, mv - (b * mx + a * my)]
        else:
            nm = np.array([[sxx, sxy, sx], [sxy, syy, sy], [sx, sy, cnt]])
            try:
                sol = np.linalg.solve(nm, np.array([[sxu, sxv], [syu, syv], [su, sv]]))
            except np.linalg.LinAlgError:
                return None, ST_REFIT_SINGULAR
            m[0], m[1] = sol[:, 0], sol[:, 1]
        return tc @ m @ tci, ST_OK
    suu, svv = _fsum(u * u), _fsum(v * v)
    mx, my, mu, mv = sx / cnt, sy / cnt, su / cnt, sv / cnt
    vs = ((sxx - sx * mx) + (syy - sy * my)) / cnt
    vd = ((suu - su * mu) + (svv - sv * mv)) / cnt
    if not vs > 0.0 or not vd > 0.0:
        return None, ST_REFIT_SINGULAR
    ss, sd = math.sqrt(2.0 / vs), math.sqrt(2.0 / vd)
    x, y, u, v = (x - mx) * ss, (y - my) * ss, (u - mu) * sd, (v - mv) * sd
    pp = [x * x, x * y, x, y * y, y, np.ones_like(x)]
    ww = [np.ones_like(x), u, v, u * u + v * v]
    s = [[_fsum(wq * pq) for pq in pp] for wq in ww]
    pidx = [[0, 1, 2], [1, 3, 4], [2, 4, 5]]
    ata = np.zeros((9, 9))
    for i in range(3):
        for j in range(3):
            e = pidx[i][j]
            ata[i, j] = ata[3 + i, 3 + j] = s[0][e]
            ata[i, 6 + j] = ata[6 + j, i] = -s[1][e]
            ata[3 + i, 6 + j] = ata[6 + j, 3 + i] = -s[2][e]
            ata[6 + i, 6 + j] = s[3][e]
    _, vecs = np.linalg.eigh(ata)
    hn = vecs[:, 0].reshape(3, 3)
    ts = np.array([[ss, 0, -ss * mx], [0, ss, -ss * my], [0, 0, 1.0]])
    tdi = np.array([[1 / sd, 0, mu], [0, 1 / sd, mv], [0, 0, 1.0]])
    hm = tc @ tdi @ hn @ ts @ tci
    if hm[2, 2] == 0.0 or not np.all(np.isfinite(hm / hm[2, 2])):
        return None, ST_REFIT_SINGULAR
    return hm / hm[2, 2], ST_OK


def median_f32(r):
    """sorted[n / 2] for odd n, the fp32 mean of the two middle values for even n"""
    n = r.size
    if n & 1:
        return np.partition(r, n // 2)[n // 2]
    part = np.partition(r, [n // 2 - 1, n // 2])
    with np.errstate(all='ignore'):
        return np.float32((part[n // 2 - 1] + part[n // 2]) / np.float32(2.0))


def fit_image(flow, ref, mask, dof, method):
    """One image: flow [2,H,W], mask [H,W] bool or None.  -> (3 x 3 float64 (zeros unless status 0), [n_valid, winner, inliers,
    status])"""
    _, h, w = flow.shape
    m = dof // 2
    src, dst = point_pairs(flow, ref)
    valid_idx = np.arange(h * w) if mask is None else np.flatnonzero(np.asarray(mask).reshape(-1))
    nv = len(valid_idx)
    zero = np.zeros((3, 3))
    if method == 'lms':
        mat, st = least_squares(src[valid_idx], dst[valid_idx], dof, h, w)
        return (zero if st else mat), [nv, -1, nv, st]
    if nv < m:
        return zero, [nv, -1, 0, ST_FEW_POINTS]
    kk = K_RANSAC if method == 'ransac' else K_LMEDS
    s32, d32 = src[valid_idx].astype(np.float32), dst[valid_idx].astype(np.float32)
    best, best_score, best_h = -1, None, None
    for k in range(kk):
        hm = hypothesis(k, m, valid_idx, src, dst)
        if hm is None:
            continue
        r = residuals(hm, s32, d32, dof == 8)
        if method == 'ransac':
            score = int(np.count_nonzero(r <= RANSAC_THR))
            better = best < 0 or score > best_score
        else:
            score = median_f32(r)
            better = best < 0 or score < best_score
        if better:
            best, best_score, best_h = k, score, hm
    if best < 0:
        return zero, [nv, -1, 0, ST_NO_HYPOTHESIS]
    thr = RANSAC_THR
    if method == 'lmeds':
        with np.errstate(all='ignore'):
            sigma = 2.5 * 1.4826 * (1.0 + np.float64(5.0) / np.float64(nv - m)) * math.sqrt(float(best_score))
            sigma = sigma if sigma > 0.001 else 0.001          # (fmax: a NaN gives 0.001)
            thr = np.float32(sigma * sigma)
    inl = residuals(best_h, s32, d32, dof == 8) <= thr
    cnt = int(np.count_nonzero(inl))
    mat, st = least_squares(src[valid_idx][inl], dst[valid_idx][inl], dof, h, w)
    if st:
        return zero, [nv, best, cnt, ST_REFIT_SINGULAR]
    return mat, [nv, best, cnt, ST_OK]


def fit(flow, ref, mask, dof, method):
    """flow [N,2,H,W] fp32 / fp16, mask [N,H,W] bool or None -> (float64 [N,3,3], int32 [N,4])"""
    mats, infos = [], []
    for i in range(flow.shape[0]):
        mat, info = fit_image(flow[i], ref, None if mask is None else mask[i], dof, method)
        mats.append(mat)
        infos.append(info)
    return np.stack(mats), np.array(infos, np.int32)
