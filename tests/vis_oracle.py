"""NumPy restatement of the reference's Flow.visualise (flow_class.py:1246-1356) -- the checker of ofl_visualise.hip.

Every step in the dtype NumPy uses for it in the reference: fp32 planes, float64 where NumPy promotes (the saturation's
division, the HSV -> RGB), the percentile by np.percentile itself.  cv2 is not needed: cartToPolar and the border rule of
findContours / drawContours are restated (OpenCV 4.x, mathfuncs_core.simd.hpp / the 0-framed border of contour tracing), with
`fmaf` emulated exactly in float64.
"""
import numpy as np

THRESHOLD = np.float32(1e-3)          # utils.py:23 DEFAULT_THRESHOLD, compared in fp32
# cartToPolar's form: True = OpenCV's AVX2 path (explicit FMA) for every value, as OFL_CART_FMA in ofl_visualise.hip
CART_FMA = True
_RAD2DEG = np.float32(180.0 / np.pi)
P1 = np.float32(0.9997878412794807) * _RAD2DEG
P3 = np.float32(-0.3258083974640975) * _RAD2DEG
P5 = np.float32(0.1555786518463281) * _RAD2DEG
P7 = np.float32(-0.04432655554792128) * _RAD2DEG
DBL_EPS_F32 = np.float32(np.finfo(np.float64).eps)
MODES = ('hsv', 'rgb', 'bgr')
# flow_class.py:1342: rows of (r, g, b) picked from (0: v, 1: p, 2: q, 3: t) by i = int(h * 6) % 6
ORDER = np.array([[0, 3, 1], [2, 0, 1], [1, 0, 3], [1, 2, 0], [3, 1, 0], [0, 1, 2]])


def fmaf(a, b, c) -> np.ndarray:
    """fp32 fused multiply-add, exact: the product of two fp32 values is exact in float64; the sum is TwoSum'd, rounded to odd
    in float64, then rounded to nearest fp32 (53 >= 24 + 2 bits: no double rounding)."""
    a, b, c = (np.asarray(v, dtype=np.float32) for v in (a, b, c))
    p = a.astype(np.float64) * b.astype(np.float64)
    cd = c.astype(np.float64)
    with np.errstate(over='ignore', invalid='ignore'):
        s = p + cd
        bb = s - p
        err = (p - (s - bb)) + (cd - bb)
        odd = (s.view(np.int64) & 1) == 1
        fix = (err != 0) & ~odd & np.isfinite(s)
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def threshold(v: np.ndarray) -> np.ndarray:
    v = np.asarray(v, dtype=np.float32)
    return np.where((v < THRESHOLD) & (v > -THRESHOLD), np.float32(0), v).astype(np.float32)


def cart_to_polar(x: np.ndarray, y: np.ndarray, fma: bool = None):
    """cv2.cartToPolar(x, y, angleInDegrees=True) on fp32 arrays -> (magnitude, angle in [0, 360]) fp32"""
    fma = CART_FMA if fma is None else fma
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    with np.errstate(over='ignore', invalid='ignore', under='ignore'):
        if fma:
            mag = np.sqrt(fmaf(x, x, y * y))
        else:
            mag = np.sqrt(x * x + y * y)
        ax, ay = np.abs(x), np.abs(y)
        c = np.minimum(ax, ay) / (np.maximum(ax, ay) + DBL_EPS_F32)
        cc = c * c
        if fma:
            a = fmaf(fmaf(fmaf(cc, P7, P5), cc, P3), cc, P1) * c
        else:
            a = (((P7 * cc + P5) * cc + P3) * cc + P1) * c
    a = np.where(~(ax >= ay), np.float32(90) - a, a).astype(np.float32)
    a = np.where(x < 0, np.float32(180) - a, a).astype(np.float32)
    a = np.where(y < 0, np.float32(360) - a, a).astype(np.float32)
    return mag.astype(np.float32), a


def mask_borders(mask: np.ndarray) -> np.ndarray:
    """findContours(RETR_TREE, CHAIN_APPROX_SIMPLE) + drawContours(thickness 1) on the 0-framed mask: the True pixels with a
    False (or outside) 4-neighbour.  mask [..., H, W] bool."""
    m = np.asarray(mask, dtype=bool)
    pad = [(0, 0)] * (m.ndim - 2) + [(1, 1), (1, 1)]
    f = np.pad(m, pad, constant_values=False)
    out_nb = ~f[..., :-2, 1:-1] | ~f[..., 2:, 1:-1] | ~f[..., 1:-1, :-2] | ~f[..., 1:-1, 2:]
    return m & out_nb


def percentile_lerp(values: np.ndarray) -> np.float32:
    """np.percentile(values, 99) of fp32 values as ofl_visualise_range_f32 forms it from two order statistics (numpy 2.2.6,
    'linear'): q = float32(99 / 100), the virtual index (n - 1) * q in fp32, previous / next index (both the last one at or
    past n - 1), gamma = fp32(float64(vi) - previous), and _lerp in fp32 with its t >= 0.5 branch."""
    v = np.sort(np.asarray(values, np.float32).ravel())
    n = v.size
    if n == 0:
        raise IndexError("index -1 is out of bounds for axis 0 with size 0")
    q = np.float32(99) / np.float32(100)
    vi = np.float32(np.float32(n - 1) * q)
    if vi >= np.float32(n - 1):
        k0 = k1 = n - 1
        gamma = np.float32(np.float64(vi) - (-1.0))
    else:
        k0 = int(np.floor(vi))
        k1 = k0 + 1
        gamma = np.float32(np.float64(vi) - k0)
    a, b = v[k0], v[k1]
    with np.errstate(invalid='ignore', over='ignore'):
        d = np.float32(b - a)
        if gamma >= np.float32(0.5):
            return np.float32(b - d * (np.float32(1) - gamma))
        return np.float32(a + d * gamma)


def default_range(mag: np.ndarray, mask: np.ndarray = None) -> np.ndarray:
    """flow_class.py:1300-1309 -> float64[N]; mask given = show_mask (an empty selection raises numpy's IndexError)"""
    out = []
    for i in range(mag.shape[0]):
        m = mag[i][mask[i]] if mask is not None else mag[i].ravel()
        pct = np.percentile(m, 99)
        if pct > 0:
            out.append(float(pct))
        elif np.max(m) > 0:
            out.append(float(np.max(m)))
        else:
            out.append(1)
    return np.array(out, dtype=np.float64)


def hsv_planes(vecs: np.ndarray, mask: np.ndarray = None, show_mask: bool = False, show_mask_borders: bool = False,
               range_max=None) -> np.ndarray:
    """The fp32 N-H-W-3 HSV array of flow_class.py:1287-1327.  vecs [N,2,H,W], mask [N,H,W] bool (None: all True), range_max
    None (the default) or float64 values per image."""
    vecs = np.asarray(vecs, dtype=np.float32)
    n, _, h, w = vecs.shape
    mask = np.ones((n, h, w), bool) if mask is None else np.asarray(mask, bool)
    x, y = threshold(vecs[:, 0]), threshold(vecs[:, 1])
    mag, ang = cart_to_polar(x, y)
    hsv = np.zeros((n, h, w, 3), np.float32)
    hsv[..., 0] = np.mod(ang, np.float32(360)) / np.float32(2)
    hsv[..., 2] = np.where(show_mask & ~mask, np.float32(180), np.float32(255))
    rng = default_range(mag, mask if show_mask else None) if range_max is None else np.asarray(range_max, np.float64)
    sat = (mag * np.float32(255)).astype(np.float64) / rng[:, None, None]
    hsv[..., 1] = np.clip(sat, 0, 255).astype(np.float32)
    if show_mask_borders:
        hsv[mask_borders(mask)] = 0
    return hsv


def hsv_to_rgb(hsv: np.ndarray) -> np.ndarray:
    """flow_class.py:1333-1346: fp32 h, s, v; i = int(h * 6) (fp32 product); f in float64; v, p, q, t = (1 - s * {0, 1, f, 1 - f})
    * v in float64; rounded half to even -> uint8 N-H-W-3 (r, g, b)"""
    h = hsv[..., 0] / np.float32(180)
    s = (hsv[..., 1] / np.float32(255)).astype(np.float64)
    v = (hsv[..., 2] / np.float32(255)).astype(np.float64)
    h6 = (h * np.float32(6)).astype(np.float32)
    i = h6.astype(np.int64)
    f = h6.astype(np.float64) - i
    t = 1.0 - f
    i = i % 6
    c = np.stack([(1.0 - s * 0.0) * v, (1.0 - s * 1.0) * v, (1.0 - s * f) * v, (1.0 - s * t) * v], axis=-1)
    rgb = np.take_along_axis(c, ORDER[i], axis=-1)
    return np.round(rgb * 255.0).astype(np.uint8)


def visualise(vecs, mode: str, mask=None, show_mask: bool = False, show_mask_borders: bool = False, range_max=None) -> np.ndarray:
    """uint8 N-H-W-3 image of `mode` ('hsv' / 'rgb' / 'bgr')"""
    hsv = hsv_planes(vecs, mask, show_mask, show_mask_borders, range_max)
    if mode == 'hsv':
        return np.round(hsv).astype(np.uint8)
    rgb = hsv_to_rgb(hsv)
    return rgb[..., ::-1].copy() if mode == 'bgr' else rgb
