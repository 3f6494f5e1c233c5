"""Host side of tests/test_special_values_host.py and tests/test_gpu_special_values.py: images that carry NaN, +-inf, denormals, -0.0
and values near FLT_MAX at NAMED positions, and a NumPy restatement of the forward splat with a per-corner inclusion predicate.

Builders.  `splat_case` plants one special per named position on a finite background: the name says where the source pixel's end
point falls (integer displacement, on the frame's border lines, outside, under the occlusion rule, behind the weight mask ...), i.e.
which corners receive weight 0, which leave the frame and which pixels the splat excludes.  `warp_case` does the same for the
backward warp: sample positions on integers (east / south taps of weight 0), on the last row and column, at -1 and w, specials read
only through a tap of weight 0, and flow components of +-3.4e38, +-1e-42, 2^24, 2^31.  Backgrounds, flows and finite data are
multiples of 1/64 of modest size, so the same inputs are exact in fp16 (`half=True` swaps the fp32-only specials and end points for
their fp16 counterparts).

Restatement.  `splat_restated` is grid_from_unstructured_data plus the occlusion step of apply_s_flow (reference utils.py:1098-1144,
1187-1203): four per-corner planes, each filled in raster order of the source pixels (scatter_add_), summed as ((c0 + c1) + c2) + c3,
divided by the clamped density, then the un-occlude fill.  A PREDICATE decides which (source pixel, corner) pairs are added at all:

    ALL              every pair, as the reference: an excluded pixel adds (wgt * 0) * data, a corner outside the frame adds
                     0 * data at its clamped position -- 0 * NaN and 0 * inf are NaN
    NO_ZERO_WEIGHT   ALL without the corners INSIDE the frame whose weight is 0 (integer end points)
    NO_EXCLUDED      ALL without the pixels the weight mask or the occlusion rule excludes
    NO_OUT_OF_FRAME  ALL without the corners outside the frame of a pixel that has a corner inside it
    NO_LEFT_FRAME    ALL without the pixels none of whose corners lies inside the frame
    G                the library's rule: the pixel is included AND the corner lies inside the frame
                     (= NO_EXCLUDED, NO_OUT_OF_FRAME and NO_LEFT_FRAME together; zero weights stay)
    NONZERO          G and NO_ZERO_WEIGHT together: `wgt != 0`, what the atomics paths did before they took rule G

On finite data every predicate gives the reference's bits: all a predicate removes is the addition of a zero.
"""
import math

import numpy as np

F32 = np.float32
NAN, PINF, NINF = F32(np.nan), F32(np.inf), F32(-np.inf)
FLT_MAX = np.finfo(np.float32).max
DEN_MIN = F32(2.0 ** -149)                                   # the smallest denormal
DEN_MAX = np.nextafter(np.finfo(np.float32).tiny, F32(0))     # the largest
NEG_ZERO = F32(-0.0)
H_MAX, H_DEN_MIN, H_DEN_MAX = F32(65504.0), F32(2.0 ** -24), F32(1023 * 2.0 ** -24)   # the same three of fp16
NONFINITE = (NAN, PINF, NINF)
ZERO_THR = F32(1e-3)                                          # utils.py:23 (threshold_vectors)
SUB_THR = F32(np.float16(2e-4))                               # below the zero threshold, not zero, exact in fp16
FAR, H_FAR = F32(1e6), F32(60000.0)
HUGE = F32(3.4e38)


def finite_specials(half=False):
    return {"flt_max": H_MAX if half else FLT_MAX, "den_min": H_DEN_MIN if half else DEN_MIN,
            "den_max": H_DEN_MAX if half else DEN_MAX, "neg_zero": NEG_ZERO}


def classes(a):
    """0 finite, 1 NaN, 2 +inf, 3 -inf, element by element."""
    a = np.asarray(a)
    if a.dtype == bool:
        return a.astype(np.uint8)
    return (np.isnan(a) * 1 + np.isposinf(a) * 2 + np.isneginf(a) * 3).astype(np.uint8)


def same_bits(got, exp):
    """Element by element: equal bits where `exp` is finite (the sign of a zero included), NaN where it is NaN (payload and sign
    of a NaN are not compared), the same infinity where it is infinite."""
    got, exp = np.ascontiguousarray(got), np.ascontiguousarray(exp)
    assert got.shape == exp.shape and got.dtype == exp.dtype, (got.shape, exp.shape, got.dtype, exp.dtype)
    if got.dtype == bool:
        return got == exp
    u = {4: np.uint32, 2: np.uint16}[got.dtype.itemsize]
    return np.where(np.isnan(exp), np.isnan(got), got.view(u) == exp.view(u))


def record_sum(terms):
    """The sum of a record over terms that are not negative: NaN if a term is NaN, else +inf if a term is +inf, else math.fsum (the
    exact sum rounded once)."""
    terms = np.asarray(terms, np.float64).reshape(-1)
    if np.isnan(terms).any():
        return float("nan")
    if np.isposinf(terms).any():
        return float("inf")
    return math.fsum(terms.tolist())


def record_max(terms):
    """The maximum of a record: the largest term that is not NaN (+inf included), 0 if there is none -- the selection `t > mx` from
    mx = 0, which a NaN never passes."""
    terms = np.asarray(terms, np.float64).reshape(-1)
    terms = terms[~np.isnan(terms)]
    return float(terms.max()) if terms.size else 0.0


def describe(got, exp, limit=6):
    """The first elements where `got` misses `exp` on the terms of same_bits, for an assertion message."""
    bad = np.argwhere(~same_bits(got, exp))
    out = ["%d of %d elements differ" % (len(bad), exp.size)]
    for idx in bad[:limit]:
        idx = tuple(int(i) for i in idx)
        out.append("%s: got %r, expected %r" % (idx, got[idx], exp[idx]))
    return "; ".join(out)


# ------------------------------------------------------------------------------------------------------------------------------------
# the splat: inputs
# ------------------------------------------------------------------------------------------------------------------------------------
def _background(n, c, h, w, rng):
    """Flow components in [0.25, 0.375) (multiples of 1/64: generic fractional end points, nothing near the zero threshold) and data
    in [-8, 8) (multiples of 1/64)."""
    yy, xx = np.mgrid[0:h, 0:w]
    flow = np.empty((n, 2, h, w), np.float32)
    for b in range(n):
        flow[b, 0] = 0.25 + ((3 * xx + 5 * yy + b) % 8) / 64.0
        flow[b, 1] = 0.25 + ((5 * xx + 3 * yy + 2 * b) % 8) / 64.0
    data = (rng.integers(-512, 512, size=(n, c, h, w)) / 64.0).astype(np.float32)
    return flow, data


def _slots(h, w, rng):
    """Source pixels for the named positions: interior, two rows and three columns apart (small frames: as many as fit), shuffled.
    The pixel to the right of a slot is reserved with it."""
    slots = [(y, x) for y in range(1, h - 1, 2) for x in range(1, w - 2, 3)]
    return [slots[i] for i in rng.permutation(len(slots))]


def splat_positions(h, w, half=False):
    """name -> f(sy, sx) = (u, v): the flow that takes source pixel (sx, sy) to the named end point."""
    far = H_FAR if half else FAR
    q = 0.375
    pos = {
        "int_both": lambda y, x: (1.0, -1.0),
        "int_x_half_y": lambda y, x: (-1.0, 0.5),
        "half_x_int_y": lambda y, x: (0.5, 1.0),
        "generic": lambda y, x: (0.375, 0.625),
        "zero_occluded": lambda y, x: (0.0, 0.0),
        "sub_threshold": lambda y, x: (float(SUB_THR), -float(SUB_THR)),
        "masked": lambda y, x: (0.375, 0.625),
        "far_x": lambda y, x: (float(far), q),
        "far_y": lambda y, x: (q, -float(far)),
        "shared_cell": lambda y, x: (0.25, 0.25),              # (its right neighbour, finite, is sent to the same cell)
        "inf_pair": lambda y, x: None,                         # +inf here, -inf to the right, on the background flow
    }
    if not half:
        pos["huge_x"] = lambda y, x: (float(HUGE), q)
        pos["huge_y"] = lambda y, x: (q, -float(HUGE))
    for tag, t in (("m1", -1.0), ("mhalf", -0.5), ("0", 0.0)):
        pos["x_" + tag] = lambda y, x, t=t: (t - x, q)
        pos["y_" + tag] = lambda y, x, t=t: (q, t - y)
    for tag, t in (("last", -1.0), ("last_half", -0.5), ("size", 0.0)):
        pos["x_" + tag] = lambda y, x, t=t: (w + t - x, q)
        pos["y_" + tag] = lambda y, x, t=t: (q, h + t - y)
    return pos


# the order in which a frame too small for all of them takes the names: every kind of corner first
_PRIORITY = ("int_both", "x_mhalf", "masked", "x_size", "zero_occluded", "y_last_half", "x_m1", "far_y", "inf_pair",
             "y_size", "int_x_half_y", "y_m1", "x_last", "sub_threshold", "shared_cell", "generic", "x_0", "half_x_int_y")


def splat_case(h, w, c=2, n=2, seed=0, half=False, finite_only=False):
    """A splat input with specials at named positions.  -> dict(flow [n,2,h,w], data [n,c,h,w], mask [n,h,w] bool (the weight mask),
    ca, cb [n,h,w] bool (the two masks of the mask channel), names {name: [(b, y, x)]} the source pixels that hold a NON-FINITE
    special, finite {name: [(b, y, x)]} those that hold FLT_MAX, a denormal or -0.0).  finite_only: the same flow and masks over the finite background alone."""
    rng = np.random.default_rng(1000 * seed + 7 * h + w)
    flow, data = _background(n, c, h, w, rng)
    mask = rng.random((n, h, w)) > 0.06
    ca = rng.random((n, h, w)) > 0.1
    cb = rng.random((n, h, w)) > 0.1
    kinds = splat_positions(h, w, half)
    order = [k for k in _PRIORITY if k in kinds] + sorted(k for k in kinds if k not in _PRIORITY)
    fin = finite_specials(half)
    names, finite = {}, {}
    for b in range(n):
        slots = _slots(h, w, rng)
        # a small frame holds a part of the list: each image takes up where the one before stopped
        start = b * len(slots) if len(slots) < len(order) else 0
        todo = [order[(i + start) % len(order)] for i in range(len(order))]
        todo += ["fin_int_" + k for k in sorted(fin)] + ["fin_generic_" + k for k in sorted(fin)]
        for i, name in enumerate(todo):
            if not slots:
                break
            y, x = slots.pop()
            mask[b, y, x:x + 2] = True
            if name.startswith("fin_"):
                u, v = (1.0, 1.0) if name.startswith("fin_int_") else (0.375, 0.625)
                flow[b, :, y, x] = (u, v)
                if not finite_only:
                    data[b, :, y, x] = fin[name.split("_", 2)[2]]
                finite.setdefault(name, []).append((b, y, x))
                continue
            uv = kinds[name](y, x)
            if uv is not None:
                flow[b, :, y, x] = uv
            if name == "masked":
                mask[b, y, x] = False
            if name == "shared_cell":
                flow[b, :, y, x + 1] = (-0.5, 0.5)
            if not finite_only:
                # (a corner outside the frame is clamped on to the corner inside it: only an infinity tells 0 * data there from nothing)
                pool = NONFINITE[1:] if name.endswith("half") and name[1] == "_" else NONFINITE
                for ch in range(c):
                    data[b, ch, y, x] = pool[(i + ch + b + seed) % len(pool)]
                if name == "inf_pair":
                    data[b, :, y, x], data[b, :, y, x + 1] = PINF, NINF
            names.setdefault(name, []).append((b, y, x))
    return dict(flow=flow, data=data, mask=mask, ca=ca, cb=cb, names=names, finite=finite, h=h, w=w, c=c, n=n, half=half)


# ------------------------------------------------------------------------------------------------------------------------------------
# the splat: restatement
# ------------------------------------------------------------------------------------------------------------------------------------
def ALL(inc, inside, zero_w, left):
    return np.ones_like(inside)


def NO_ZERO_WEIGHT(inc, inside, zero_w, left):
    return ~(inc & inside & zero_w)


def NO_EXCLUDED(inc, inside, zero_w, left):
    return inc & np.ones_like(inside)


def NO_OUT_OF_FRAME(inc, inside, zero_w, left):
    return ~(inc & ~inside & ~left)


def NO_LEFT_FRAME(inc, inside, zero_w, left):
    return ~(inc & left) & np.ones_like(inside)


def G(inc, inside, zero_w, left):
    return inc & inside


def NONZERO(inc, inside, zero_w, left):
    return inc & inside & ~zero_w


SINGLE_RULES = {"zero-weight corner": NO_ZERO_WEIGHT, "excluded pixel": NO_EXCLUDED, "out-of-frame corner": NO_OUT_OF_FRAME,
                "pixel that left the frame": NO_LEFT_FRAME}
PREDICATES = dict(SINGLE_RULES, ALL=ALL, G=G, NONZERO=NONZERO)


def zero_flow(flow):
    """apply_s_flow's zero mask: both components strictly inside (-1e-3, 1e-3) (threshold_vectors, utils.py:642, 1191)."""
    f = np.asarray(flow, np.float32)
    z = (f < ZERO_THR) & (f > -ZERO_THR)
    return z[:, 0] & z[:, 1]


def corner_terms(flow, mask=None, occlude=True, xy=None):
    """What the reference forms per (source pixel, corner) before it scatters (utils.py:1098-1123), corner = ky * 2 + kx.
    -> dict(wgt [n,4,h,w] fp32 (already multiplied by the flow mask), pos [n,4,h,w] int64 (clamped), inc [n,1,h,w] the pixel passes the
    mask and the occlusion rule, inside [n,4,h,w] the corner lies inside the frame, zero_w [n,4,h,w] its weight BEFORE the mask is 0,
    left [n,1,h,w] no corner of the pixel lies inside the frame, zero [n,h,w], mask [n,h,w])."""
    flow = np.asarray(flow, np.float32)
    n, _, h, w = flow.shape
    with np.errstate(all="ignore"):
        x = flow[:, 0] + np.arange(w, dtype=np.float32)[None, None, :]
        y = flow[:, 1] + np.arange(h, dtype=np.float32)[None, :, None]
        if xy is not None:                                         # (end points given instead: xy(x, y) -> (x, y))
            x, y = xy(x, y)
        x0, y0 = np.floor(x), np.floor(y)
        xx, yy = np.stack([x0, x0 + F32(1)], -1), np.stack([y0, y0 + F32(1)], -1)
        xs, ys = np.clip(xx, F32(0), F32(w - 1)), np.clip(yy, F32(0), F32(h - 1))
        inx, iny = xx == xs, yy == ys
        wtx = np.stack([xx[..., 1] - x, x - xx[..., 0]], -1) * inx.astype(np.float32)
        wty = np.stack([yy[..., 1] - y, y - yy[..., 0]], -1) * iny.astype(np.float32)
        wgt = (wty[..., :, None] * wtx[..., None, :]).astype(np.float32)            # n h w 2 2
        pos = (F32(w) * ys)[..., :, None] + xs[..., None, :]
    inside = iny[..., :, None] & inx[..., None, :]
    to4 = lambda a: np.ascontiguousarray(np.moveaxis(a.reshape(n, h, w, 4), -1, 1))
    wgt, pos, inside = to4(wgt), to4(pos).astype(np.int64), to4(inside)
    m = np.ones((n, h, w), bool) if mask is None else np.asarray(mask, bool)
    zero = zero_flow(flow) if occlude else np.zeros((n, h, w), bool)
    inc = m & ~zero
    zero_w = wgt == 0
    with np.errstate(all="ignore"):
        wgt = wgt * inc[:, None].astype(np.uint8).astype(np.float32)
    return dict(wgt=wgt, pos=pos, inc=inc[:, None], inside=inside, zero_w=zero_w, left=~inside.any(1, keepdims=True), zero=zero, mask=m)


def splat_restated(flow, data, mask=None, occlude=True, predicate=ALL, reverse=False, xy=None, raw=False):
    """apply_s_flow(flow, data, mask, occlude) restated -> (warped data [n,c,h,w], warped mask [n,h,w] bool, density [n,h,w]).
    predicate: which (pixel, corner) pairs are added (module docstring); reverse: the sources are added in reversed raster order;
    xy: a function of the end points (corner_terms); raw: the sums themselves, not divided by the density."""
    flow, data = np.asarray(flow, np.float32), np.asarray(data, np.float32)
    n, c, h, w = data.shape
    t = corner_terms(flow, mask, occlude, xy)
    keep = predicate(t["inc"], t["inside"], t["zero_w"], t["left"])
    out = np.empty((n, c, h, w), np.float32)
    den = np.empty((n, h, w), np.float32)
    with np.errstate(all="ignore"):
        for b in range(n):
            dplane = np.zeros((4, h * w), np.float32)
            gplane = np.zeros((4, c, h * w), np.float32)
            for k in range(4):
                sel = np.flatnonzero(keep[b, k].reshape(-1))                       # raster order of the sources
                if reverse:
                    sel = sel[::-1]
                p = t["pos"][b, k].reshape(-1)[sel]
                wk = t["wgt"][b, k].reshape(-1)[sel]
                np.add.at(dplane[k], p, wk)
                for ch in range(c):
                    np.add.at(gplane[k, ch], p, wk * data[b, ch].reshape(-1)[sel])
            d = ((dplane[0] + dplane[1]) + dplane[2]) + dplane[3]
            g = ((gplane[0] + gplane[1]) + gplane[2]) + gplane[3]
            den[b] = d.reshape(h, w)
            out[b] = (g if raw else g / np.maximum(d, ZERO_THR)).reshape(c, h, w)  # clamp_min(density, 1e-3)
    warped = den > 0
    if occlude and not raw:
        fill = t["mask"] & t["zero"] & ~warped                                     # utils.py:1202-1203
        out = np.where(fill[:, None], data, out)
    return out, warped, den


def splat_sum_restated(flow, data, predicate=G):
    """The transpose of the backward warp: every pixel's data added, undivided, at the corners of the position the warp samples for
    it (sample_coord of x - u, y - v), in the splat's order."""
    h, w = data.shape[2:]
    xy = lambda x, y: (sample_coord(x, w) if w > 1 else x, sample_coord(y, h) if h > 1 else y)
    return splat_restated(-np.asarray(flow, np.float32), data, None, False, predicate, xy=xy, raw=True)[0]


def with_mask_channel(case, use_a=True, use_b=True):
    """The case's data with the mask channel appended (the float of ca & cb, as Flow.apply appends it)."""
    m = np.ones(case["mask"].shape, bool)
    if use_a:
        m &= case["ca"]
    if use_b:
        m &= case["cb"]
    return np.concatenate([case["data"], m[:, None].astype(np.float32)], 1)


# ------------------------------------------------------------------------------------------------------------------------------------
# the warp: inputs
# ------------------------------------------------------------------------------------------------------------------------------------
WARP_FLOW_EXTREMES = (HUGE, -HUGE, F32(1e-42), F32(-1e-42), F32(2.0 ** 24), F32(2.0 ** 31))


def sample_coord(p, size):
    """Where the backward warp samples for the position p = x - u: normalise_coords then grid_sample's un-normalisation, each step
    rounded to fp32 (utils.py:462-465; align_corners=True).  An integer p does not always come back as that integer."""
    p = np.asarray(p, np.float32)
    with np.errstate(all="ignore"):
        g = p * F32(2)
        g = g / F32(size - 1)
        g = g - F32(1)
        return (g + F32(1)) * (F32(size - 1) / F32(2))


def exact_coords(size):
    """The integers of [1, size - 2] that sample_coord returns unchanged: sample positions with east / south weight exactly 0."""
    k = np.arange(1, size - 1, dtype=np.float32)
    return [int(v) for v in k[sample_coord(k, size) == k]]


def _nearest(cands, v):
    return min(cands, key=lambda k: (abs(k - v), k))


def _plant_cycle(i, half):
    fin = finite_specials(half)
    pool = list(NONFINITE) + [fin[k] for k in sorted(fin)]
    return pool[i % len(pool)]


def warp_case(n, h, w, c, seed=0, half=False, sprinkle=0.02, finite=False, plant_names=None):
    """A backward-warp input with specials in the source.  The output pixel (x, y) samples the source at (x - u, y - v).
    -> dict(flow [n,2,h,w], src [n,c,h,w], names {name: [(y, x)]} the OUTPUT pixels (the same in every image) whose sample position is
    the named one, weight0 [(y, x)] the SOURCE pixels that hold a special and are read by a named output pixel only through a tap of
    weight 0, aimed {name: (sy, sx)} the integer position each name aims at, planted [(y, x)] every SOURCE pixel a name planted a
    special on).  The source also carries specials on a random `sprinkle` of its pixels, another draw for each image.  finite: the
    same flow and the same finite source values, no special anywhere (the lists say where they would be); plant_names: the names
    whose source pixel receives a special (default: all of them)."""
    rng = np.random.default_rng(77 * seed + 13 * h + w + 1000 * c)
    flow = (rng.integers(-320, 320, size=(n, 2, h, w)) / 64.0).astype(np.float32)
    src = (rng.integers(0, 2048, size=(n, c, h, w)) / (128.0 if half else 8.0)).astype(np.float32)      # (11 bits: exact in fp16)
    hit = rng.random((n, c, h, w)) < sprinkle
    pool = np.array([_plant_cycle(i, half) for i in range(7)], np.float32)
    if not finite:
        src[hit] = pool[np.arange(int(hit.sum())) % len(pool)]
    names, weight0, aimed, planted = {}, [], {}, []
    outs = [(y, x) for y in range(0, h) for x in range(0, w)]
    outs = [outs[i] for i in rng.permutation(len(outs))]

    def aim(name, sy, sx, plant=None, special_i=0):
        """The next free output pixel samples (sx, sy); `plant`: the source pixel that receives a special (default: the sampled one)."""
        y, x = outs.pop()
        flow[:, 0, y, x], flow[:, 1, y, x] = x - sx, y - sy
        py, px = (sy, sx) if plant is None else plant
        if 0 <= py < h and 0 <= px < w and (plant_names is None or name in plant_names):
            if not finite:
                for ch in range(c):
                    src[:, ch, py, px] = NONFINITE[(special_i + ch) % 3]
            planted.append((py, px))
            if plant is not None:
                weight0.append((py, px))
        names.setdefault(name, []).append((y, x))
        aimed[name] = (sy, sx)

    ey, ex = exact_coords(h), exact_coords(w)
    my, mx = _nearest(ey, h // 2), _nearest(ex, w // 2)
    aim_y = lambda v: _nearest(ey, v)
    aim_x = lambda v: _nearest(ex, v)
    aim("on_integer", my, mx, special_i=0)
    sy, sx = aim_y(my - 3), aim_x(mx - 4)
    aim("weight0_east", sy, sx, plant=(sy, sx + 1), special_i=1)
    sy, sx = aim_y(my + 3), aim_x(mx + 4)
    aim("weight0_south", sy, sx, plant=(sy + 1, sx), special_i=2)
    aim("last_row", h - 1, aim_x(mx + 2), special_i=0)
    aim("last_col", aim_y(my + 2), w - 1, special_i=1)
    aim("last_corner", h - 1, w - 1, special_i=2)
    sy, sx = aim_y(my - 2), aim_x(mx - 2)
    aim("x_m1", sy, -1, plant=(sy, 0), special_i=0)
    aim("y_m1", -1, sx, plant=(0, sx), special_i=1)
    aim("x_0", aim_y(2), 0, special_i=2)
    aim("x_last", aim_y(3), w - 1, special_i=0)
    aim("x_size", my, w)
    aim("y_size", h, mx)
    for i, e in enumerate(WARP_FLOW_EXTREMES):
        y, x = outs.pop()
        flow[:, i % 2, y, x] = e
        names.setdefault("flow_extreme", []).append((y, x))
    return dict(flow=flow, src=src, names=names, weight0=weight0, aimed=aimed, planted=planted, n=n, h=h, w=w, c=c, half=half)


# ------------------------------------------------------------------------------------------------------------------------------------
# the cases both tiers use
# ------------------------------------------------------------------------------------------------------------------------------------
SPLAT_FRAMES = ((20, 5, 1), (37, 52, 3), (64, 96, 2), (40, 52, 5))      # (h, w, data channels)
_MADE = {}


def make_splat(h, w, c, half=False, finite_only=False):
    """splat_case of a frame of SPLAT_FRAMES (cached; treat as read-only)."""
    key = (h, w, c, half, finite_only)
    if key not in _MADE:
        _MADE[key] = splat_case(h, w, c, n=2, seed=0, half=half, finite_only=finite_only)
    return _MADE[key]


_EXPECTED = {}


def expected_splat(h, w, c, half, occlude, masked, mask_chan, predicate=G, finite_only=False):
    """The restatement's (values [n,c,h,w], mask channel [n,h,w] | None, density, warped mask) for a cached case; mask_chan: None or
    (use ca, use cb); finite_only: of the same flow and masks over the finite background alone."""
    key = (h, w, c, half, occlude, masked, mask_chan, predicate.__name__, finite_only)
    if key not in _EXPECTED:
        case = make_splat(h, w, c, half, finite_only)
        dd = case["data"] if mask_chan is None else with_mask_channel(case, *mask_chan)
        out, warped, den = splat_restated(case["flow"], dd, case["mask"] if masked else None, occlude, predicate)
        _EXPECTED[key] = dict(v=out[:, :c], m=None if mask_chan is None else out[:, c], den=den, warped=warped)
    return _EXPECTED[key]


def background_scale(exp):
    """{key: max |.|} of an expected result over FINITE data: what the absolute part of a tolerance is taken from.  The planted FLT_MAX
    (1e38 in a tensor of values below 8) must not set it: 2e-5 of that would let any finite value pass."""
    return {k: float(np.abs(v).max()) for k, v in exp.items() if v is not None and v.dtype != bool}
