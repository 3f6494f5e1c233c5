"""NumPy restatement of Flow.visualise_arrows -- the checker of ofl_arrows.hip.

Everything the reference computes in NumPy / Python (flow_class.py:1448-1496) is restated with the same expressions and dtypes
(NumPy 2.2.6): the thresholded vectors, the grid, cartToPolar (vis_oracle's FMA form), the batch-wide np.percentile, the in-place
fp32 scaling, np.round of the end points (int32 + fp32 promotes to float64), the fp32 division behind tip_length, the hue, the
painter's order, the red grid pixels, the mask halving and the borders.  The arrow itself is the definition of DESIGN.md 3.11,
not OpenCV's: three capsules in float64 with + - * / sqrt only, one blend per arrow and pixel.
"""
import math

import numpy as np

import vis_oracle as vo

FAR = np.float32(2 ** 20)            # longer (or non-finite) arrows are skipped
INV_SQRT2 = 0.7071067811865476


def grid_points(h: int, w: int, grid_dist: int) -> np.ndarray:
    """flow_class.py:1452-1454: the points (row, column) in np.mgrid order, int32 [P, 2]"""
    x, y = np.mgrid[grid_dist // 2:h - 1:grid_dist, grid_dist // 2:w - 1:grid_dist]
    return np.reshape(np.dstack((x, y)), (-1, 2)).astype('i')


def effective_grid_dist(h: int, w: int, grid_dist: int = None) -> int:
    grid_dist = 20 if grid_dist is None else grid_dist
    return min(grid_dist, min(h, w) // 2)


def hue_table() -> np.ndarray:
    """uint8 [181, 3] BGR: vis_oracle.hsv_to_rgb on (h, 255, 255), reversed"""
    hsv = np.full((181, 3), 255, np.float32)
    hsv[:, 0] = np.arange(181, dtype=np.float32)
    return vo.hsv_to_rgb(hsv)[:, ::-1].copy()


HUES = hue_table()


def sample(vecs: np.ndarray, grid_dist: int):
    """-> f (thresholded fp32 [N,H,W,2]), points [P,2], magnitudes and angles at the points (fp32 [N,P])"""
    v = np.asarray(vecs, np.float32)
    f = np.stack([vo.threshold(v[:, 0]), vo.threshold(v[:, 1])], axis=-1)
    pts = grid_points(f.shape[1], f.shape[2], grid_dist)
    at = f[:, pts[:, 0], pts[:, 1]]
    mags, ang = vo.cart_to_polar(at[..., 0], at[..., 1])
    return f, pts, mags, ang


def default_scaling(mags: np.ndarray, grid_dist: int) -> np.float32:
    """flow_class.py:1458"""
    with np.errstate(divide='ignore'):
        return grid_dist / np.percentile(mags, 99)


def barbs(p1, p2, tip_length: float):
    """The two barb ends of an arrow p1 -> p2 (points as (x, y) integers), float64 without contraction"""
    dx, dy = float(p1[0] - p2[0]), float(p1[1] - p2[1])
    k = np.float64(tip_length) * np.float64(INV_SQRT2)
    bp = (int(np.rint(p2[0] + k * (dx - dy))), int(np.rint(p2[1] + k * (dx + dy))))
    bm = (int(np.rint(p2[0] + k * (dx + dy))), int(np.rint(p2[1] + k * (dy - dx))))
    return bp, bm


def _seg_d2(qx, qy, a, b):
    """squared distance of the pixel centres (int64 arrays) to the segment a -> b (integer points): float64"""
    ex, ey = int(b[0] - a[0]), int(b[1] - a[1])
    l2 = ex * ex + ey * ey
    dx, dy = qx - int(a[0]), qy - int(a[1])
    da = (dx * dx + dy * dy).astype(np.float64)
    if l2 == 0:
        return da
    u = dx * ex + dy * ey
    fx, fy = qx - int(b[0]), qy - int(b[1])
    db = (fx * fx + fy * fy).astype(np.float64)
    cross = (dx * ey - dy * ex).astype(np.float64)
    mid = cross * cross / np.float64(l2)
    return np.where(u <= 0, da, np.where(u >= l2, db, mid))


def draw_arrow(img: np.ndarray, p1, p2, colour, thickness: int, tip_length: float):
    """Blend one arrow p1 -> p2 (tip at p2; (x, y) integers) into img [H,W,3] uint8, inside its bounding box"""
    h, w = img.shape[:2]
    bp, bm = barbs(p1, p2, tip_length)
    pad = thickness // 2 + 1
    xs = [p1[0], p2[0], bp[0], bm[0]]
    ys = [p1[1], p2[1], bp[1], bm[1]]
    x0, x1 = max(min(xs) - pad, 0), min(max(xs) + pad, w - 1)
    y0, y1 = max(min(ys) - pad, 0), min(max(ys) + pad, h - 1)
    if x0 > x1 or y0 > y1:
        return
    qy, qx = np.mgrid[y0:y1 + 1, x0:x1 + 1].astype(np.int64)
    d2 = np.minimum(np.minimum(_seg_d2(qx, qy, p1, p2), _seg_d2(qx, qy, bp, p2)), _seg_d2(qx, qy, bm, p2))
    alpha = np.clip(thickness / 2 + 0.5 - np.sqrt(d2), 0.0, 1.0)
    old = img[y0:y1 + 1, x0:x1 + 1].astype(np.float64)
    col = np.array([float(c) for c in colour], np.float64)
    img[y0:y1 + 1, x0:x1 + 1] = np.rint(old + alpha[..., None] * (col - old)).astype(np.uint8)


def prepare_img(img, n: int, h: int, w: int) -> np.ndarray:
    """flow_class.py:1406-1422 on an already validated uint8 array: a fresh N-H-W-3 array"""
    if img is None:
        return np.full((n, h, w, 3), 255, 'uint8')
    img = np.asarray(img)
    if img.ndim == 3:
        img = img[None]
    return np.broadcast_to(img, (n, h, w, 3)).copy()


def visualise_arrows(vecs, ref: str, mask=None, grid_dist: int = None, img=None, scaling=None, show_mask: bool = False,
                     show_mask_borders: bool = False, colour=None, thickness: int = 1, return_scaling: bool = False):
    """uint8 N-H-W-3 (BGR).  vecs [N,2,H,W]; mask [N,H,W] bool or None (all True); img None or uint8 N-H-W-3 / H-W-3 / 1-H-W-3."""
    vecs = np.asarray(vecs, np.float32)
    n, _, h, w = vecs.shape
    grid_dist = effective_grid_dist(h, w, grid_dist)
    img = prepare_img(img, n, h, w)
    f, pts, flow_mags, ang = sample(vecs, grid_dist)
    if scaling is None:
        scaling = default_scaling(flow_mags, grid_dist)
    used = scaling
    with np.errstate(invalid='ignore', over='ignore'):
        flow_mags *= scaling
        f *= scaling
    tip_size = math.sqrt(thickness) * 3.5
    if colour is None:
        hue = np.zeros(ang.shape, 'uint8')
        hue[...] = np.round(np.mod(ang, 360) / 2)
    for b in range(n):
        for i_num, i_pt in enumerate(pts):
            m = flow_mags[b][i_num]
            if m > 0.5 and m <= FAR:
                c = tuple(int(v) for v in HUES[hue[b][i_num]]) if colour is None else colour
                tip_length = float(tip_size / m)
                if ref == 's':
                    e_pt = np.round(i_pt + f[b][i_pt[0], i_pt[1]][::-1]).astype('i')
                    draw_arrow(img[b], (int(i_pt[1]), int(i_pt[0])), (int(e_pt[1]), int(e_pt[0])), c, 1, tip_length)
                else:
                    e_pt = np.round(i_pt - f[b][i_pt[0], i_pt[1]][::-1]).astype('i')
                    draw_arrow(img[b], (int(e_pt[1]), int(e_pt[0])), (int(i_pt[1]), int(i_pt[0])), c, thickness, tip_length)
            img[b, i_pt[0], i_pt[1]] = [0, 0, 255]
    mask = np.ones((n, h, w), bool) if mask is None else np.asarray(mask, bool)
    if show_mask:
        img[~mask] = np.round(0.5 * img[~mask]).astype('uint8')
    if show_mask_borders:
        img[vo.mask_borders(mask)] = 0
    return (img, used) if return_scaling else img
