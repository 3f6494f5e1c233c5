"""Inputs of tests/test_loss_specials_host.py and tests/test_gpu_loss_specials.py (a helper module, not a test): the fused loss and
metric kernels at NAMED sample positions and on NaN, +-inf and +-FLT_MAX.

Samplers (photometric, census, consistency).  `sampler_case` puts `special_values.warp_case` under the three kernels that restate the
sampler of warp_bwd_kernel: the named OUTPUT pixels sample an integer position (east / south weight exactly 0), the last row, column
and corner (the east / south taps leave the frame at fraction 0), -1, 0, w - 1, w, and carry vectors of +-3.4e38, +-1e-42, 2^24, 2^31.
Variants: 'finite' (positions only), 'other' (specials in the sampled frame: at the sampled and the weight-0 source pixels, plus a
sprinkle), 'img' (specials in the frame on the flow's own grid), 'vectors' (NaN, +inf, -inf in the vectors themselves).

Stencils (smoothness, error_stats).  `smoothness_case` and `error_case` plant the same values in the vectors, in the ground truth and in
the guidance image: inside the frame, on its first and last row and column and on both sides of a tile edge.

Every case has N = 4 images, so that every class of record is seen next to a clean neighbour:
    image 0   the mixed pool (NaN, +inf, -inf, FLT_MAX, denormals, -0)
    image 1   +FLT_MAX wherever image 0 holds a special: products overflow to +inf and nothing is NaN
    image 2   NaN wherever image 0 holds a special: sums are NaN, the maximum stays finite
    image 3   no special at all: it must carry the bits of the finite variant
"""
import functools

import numpy as np

import grad_oracle64 as go
import smoothness_oracle as so
import special_values as sv

F32 = np.float32
NAN, PINF, NINF = sv.NAN, sv.PINF, sv.NINF
FLT_MAX = F32(sv.FLT_MAX)
N = 4
MIXED, MAX_ONLY, NAN_ONLY, CLEAN = 0, 1, 2, 3
UPSTREAM = (0.75, -2.0, 1.0, 0.5)
REFS = ('s', 't')

INSIDE = ('on_integer', 'weight0_east', 'weight0_south', 'last_row', 'last_col', 'last_corner', 'x_0', 'x_last')
OUTSIDE = ('x_m1', 'y_m1', 'x_size', 'y_size')
BORDER = ('last_row', 'last_col', 'last_corner')
NAMES = INSIDE + OUTSIDE + ('flow_extreme',)
VARIANTS = ('finite', 'other', 'img', 'vectors')
SAMPLER_FRAMES = [(20, 28), (37, 53)]
CENSUS_TILE_FRAME = (17, 65)                                   # one past the census tile of 16 x 64
CENSUS_TILE_PIXELS = [(15, 63), (15, 64), (16, 63), (16, 64)]
# the share of source elements that carry a special besides the named ones: photometric and consistency contaminate the reader alone;
# a census centre reads 9 (patch 3) readers and its gradient 25, so its cases keep to the named pixels
SPRINKLE = 0.004
CENSUS_PLANTS = ('on_integer', 'weight0_east', 'last_corner')


def sign_of(ref):
    return -1.0 if ref == 's' else 1.0


def differs(a, b):
    """[N,H,W]: the pixels at which two [N,C,H,W] arrays do not hold the same bits in every channel"""
    u = {4: np.uint32, 2: np.uint16, 1: np.uint8}[a.dtype.itemsize]
    return (np.ascontiguousarray(a).view(u) != np.ascontiguousarray(b).view(u)).any(1)


def pools(special, finite):
    """The four images of a case (module docstring) from an array with the mixed pool planted and the same array without"""
    out = special.copy()
    hit = np.ascontiguousarray(special).view(np.uint32) != np.ascontiguousarray(finite).view(np.uint32)
    out[MAX_ONLY][hit[MAX_ONLY]] = FLT_MAX
    out[NAN_ONLY][hit[NAN_ONLY]] = NAN
    out[CLEAN] = finite[CLEAN]
    return out


def dilate(m, r):
    """[N,H,W] bool: True within r pixels (Chebyshev) of a True"""
    n, h, w = m.shape
    p = np.pad(m, ((0, 0), (r, r), (r, r)))
    out = np.zeros_like(m)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out |= p[:, dy:dy + h, dx:dx + w]
    return out


def readers(a, ref, src_hit):
    """[N,H,W] bool: the output pixels one of whose taps INSIDE the frame is a source pixel of `src_hit` [N,H,W] -- from the taps
    of `grad_oracle64.warp_taps`, whatever the tap's weight"""
    a = np.asarray(a).astype(F32)
    n, _, h, w = a.shape
    t = go.warp_taps(a, n, sign_of(ref))
    flat = src_hit.reshape(n, -1)
    out = np.zeros((n, h, w), bool)
    for j in range(4):
        out |= t.ok[j] & np.take_along_axis(flat, t.idx[j].reshape(n, -1), 1).reshape(n, h, w)
    return out


# ---- samplers -------------------------------------------------------------------------------------------------------------------------
VECTOR_PLANTS = ((0, NAN), (1, PINF), (0, NINF), (1, NAN), (0, PINF), (1, NINF))      # (component, value) per planted pixel


@functools.lru_cache(maxsize=None)
def sampler_case(h, w, ref, variant, c=3, half=False, census=False):
    """dict: a float32 [N,2,h,w] (float16 with `half`), mask, back_mask bool [N,h,w], img, other float32 [N,c,h,w], names {name:
    [(y, x)]}, aimed {name: (sy, sx)}, planted, weight0 [(y, x)] (special_values.warp_case), bad_vec [(b, y, x)] the pixels whose own
    vector is not finite, src_hit / img_hit bool [N,h,w] the pixels of `other` / `img` that differ from the finite variant.
    Read-only.  census: only CENSUS_PLANTS receive a special and nothing is sprinkled."""
    assert variant in VARIANTS and ref in REFS
    kw = dict(seed=5, half=half, sprinkle=0.0 if census else SPRINKLE, plant_names=CENSUS_PLANTS if census else None)
    fin = sv.warp_case(N, h, w, c, finite=True, **kw)
    spec = sv.warp_case(N, h, w, c, finite=False, **kw)
    assert np.array_equal(fin['flow'], spec['flow']) and fin['names'] == spec['names']
    rng = np.random.default_rng(9000 + 31 * h + w + c + (0 if ref == 's' else 500))
    a = fin['flow'].copy() if ref == 't' else -fin['flow']
    named = sorted(set(p for v in fin['names'].values() for p in v))
    src = spec['src'].copy()
    if not census:
        # warp_case cycles NaN, +inf, -inf over the channels of a planted pixel, which makes every reader NaN: two pixels hold one
        # infinity in every channel, so that a known pixel of each sign of infinity exists whatever the sprinkle hits
        for name, val in (('x_0', NINF), ('x_last', PINF)):
            sy, sx = fin['aimed'][name]
            src[:, :, sy, sx] = val
    other = pools(src, fin['src']) if variant == 'other' else fin['src'].copy()
    img_f = (rng.integers(0, 2048, size=(N, c, h, w)) / (128.0 if half else 8.0)).astype(F32)
    for name in OUTSIDE:                                       # a pixel that is not known and holds a larger rho than every known one
        y, x = fin['names'][name][0]
        img_f[:, :, y, x] = 1024.0
    img = img_f.copy()
    mask = rng.random((N, h, w)) > 0.15                        # (drawn before anything a variant draws: the same in every variant)
    back_mask = rng.random((N, h, w)) > 0.15
    if variant == 'img':
        pool = np.array([sv._plant_cycle(i, half) for i in range(7)], F32)
        if not census:
            hit = rng.random((N, c, h, w)) < SPRINKLE
            img[hit] = pool[np.arange(int(hit.sum())) % len(pool)]
        for i, name in enumerate(CENSUS_PLANTS if census else ('on_integer', 'last_row', 'last_corner', 'x_m1', 'weight0_east')):
            y, x = fin['names'][name][0]
            for ch in range(c):
                img[:, ch, y, x] = sv.NONFINITE[(i + ch) % 3]
        if not census:
            for name, val in (('x_0', NINF), ('x_last', PINF)):                            # (one infinity in every channel, as above)
                y, x = fin['names'][name][0]
                img[:, :, y, x] = val
        if census and (h, w) == CENSUS_TILE_FRAME:
            for i, (y, x) in enumerate(CENSUS_TILE_PIXELS):
                img[:, :, y, x] = sv.NONFINITE[i % 3]
        img = pools(img, img_f)
    if variant == 'other' and census and (h, w) == CENSUS_TILE_FRAME:
        for i, (y, x) in enumerate(CENSUS_TILE_PIXELS):
            other[MIXED, :, y, x], other[MAX_ONLY, :, y, x], other[NAN_ONLY, :, y, x] = sv.NONFINITE[i % 3], FLT_MAX, NAN
    for y, x in named:
        mask[:, y, x] = True
    for sy, sx in fin['aimed'].values():
        back_mask[:, max(sy, 0):sy + 2, max(sx, 0):sx + 2] = True
    bad_vec = []
    if variant == 'vectors':
        free = [(y, x) for y in range(h) for x in range(w) if (y, x) not in set(named)]
        for b in (MIXED, MAX_ONLY, NAN_ONLY):
            for k, i in enumerate(rng.permutation(len(free))[:len(VECTOR_PLANTS)]):
                y, x = free[i]
                comp, val = VECTOR_PLANTS[k]
                a[b, comp, y, x] = NAN if b == NAN_ONLY else val
                mask[b, y, x] = True
                bad_vec.append((b, y, x))
    if half:
        with np.errstate(over='ignore'):
            a = a.astype(np.float16)
    out = dict(a=a, mask=mask, back_mask=back_mask, img=img, other=other, names=fin['names'], aimed=fin['aimed'],
               planted=spec['planted'], weight0=spec['weight0'], bad_vec=bad_vec, src_hit=differs(other, fin['src']),
               img_hit=differs(img, img_f), h=h, w=w, c=c, ref=ref, variant=variant, half=half)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def as_uint8(x):
    """The finite images (multiples of 1/8 in [0, 256), 1024 on the pixels that are not known) as uint8 samples"""
    return np.floor(np.minimum(x, F32(255.0))).astype(np.uint8)


def sampler_touched(case, radius=0):
    """[N,h,w] bool: the output pixels that may differ from the finite variant -- a tap on a differing pixel of `other`, a differing
    pixel of `img`, a vector of their own that is not the finite variant's; for the census the set is widened by `radius` (the patch
    radius for the map, twice that for the gradient)"""
    hit = readers(case['a'], case['ref'], case['src_hit']) | case['img_hit']
    for b, y, x in case['bad_vec']:
        hit[b, y, x] = True
    return dilate(hit, radius) if radius else hit


# ---- smoothness -----------------------------------------------------------------------------------------------------------------------
SMOOTH_FRAMES = [(9, 129), (12, 132)]                          # the element path (w mod 4 = 1) and the 16-byte path; 2 x 2 tiles of 8 x 128
SMOOTH_VARIANTS = ('finite', 'vectors', 'image', 'both')
SMOOTH_CYCLE = (NAN, PINF, NINF, FLT_MAX, -FLT_MAX)


def smooth_runs(variant):
    """[(order, alpha, with image)] of a smoothness variant: alpha = 0 too wherever the image holds an infinity"""
    if variant in ('finite', 'vectors'):
        return [(o, 10.0, im) for o in (1, 2) for im in (False, True)]
    return [(o, al, True) for o in (1, 2) for al in (10.0, 0.0)]


def smooth_plants(h, w):
    """[(y, x)]: interior, first and last row and column, both sides of the tile edges (7 | 8, 127 | 128), and the left pixel of an
    adjacent pair"""
    return [(4, 60), (0, 5), (h - 1, 9), (3, 0), (5, w - 1), (7, 127), (7, 128), (8, 127), (8, 128), (2, 20), (2, 40)]


@functools.lru_cache(maxsize=None)
def smoothness_case(h, w, variant):
    """dict: flow float32 [N,2,h,w], mask bool [N,h,w], img float32 [N,3,h,w], hit bool [N,h,w] (the pixels that differ from the
    finite variant).  (2, 20) | (2, 21) is the adjacent +inf / -inf pair, (2, 40) a +inf next to finite pixels."""
    assert variant in SMOOTH_VARIANTS
    f0, m0 = so.case(N, h, w)
    i0 = so.image(N, h, w)
    f0, mask, img = f0.copy(), m0.copy(), i0.copy()
    plants = smooth_plants(h, w)
    for y, x in plants + [(2, 21)]:
        mask[:, max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = True
    mask[:, 6, 30], f0[:, :, 6, 30] = False, 1000.0            # a term that is not valid and larger than every valid one
    flow = f0.copy()
    if variant in ('vectors', 'both'):
        for i, (y, x) in enumerate(plants[:-2]):
            flow[:, i % 2, y, x] = SMOOTH_CYCLE[i % len(SMOOTH_CYCLE)]
        flow[:, 0, 2, 20], flow[:, 0, 2, 21] = PINF, NINF
        flow[:, 1, 2, 40] = PINF
        flow = pools(flow, f0)
    if variant in ('image', 'both'):
        for i, (y, x) in enumerate(plants[:-2]):
            img[:, i % 3, y, x] = SMOOTH_CYCLE[(i + 1) % len(SMOOTH_CYCLE)]
        img[:, :, 2, 20], img[:, :, 2, 21] = PINF, NINF
        img[:, :, 2, 40] = PINF
        img = pools(img, i0)
    out = dict(flow=flow, mask=mask, img=img, hit=differs(flow, f0) | differs(img, i0), h=h, w=w, variant=variant)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


# ---- error_stats ----------------------------------------------------------------------------------------------------------------------
ERROR_FRAMES = [(20, 28), (67, 131)]                           # one block, 16-byte path; 9 blocks, element path (ofl_metrics.hip, blocks_of)
ERROR_VARIANTS = ('finite', 'est', 'gt')


@functools.lru_cache(maxsize=None)
def error_case(h, w, variant):
    """dict: est, gt float32 [N,2,h,w], est_mask, gt_mask bool [N,h,w], hit bool [N,h,w].  Speeds reach every bin; a component of
    +-FLT_MAX against a modest one overflows du du (and ug ug)."""
    assert variant in ERROR_VARIANTS
    rng = np.random.default_rng(4100 + 31 * h + w)
    gt0 = (rng.integers(-4096, 4096, size=(N, 2, h, w)) / 64.0).astype(F32)
    est0 = gt0 + (rng.integers(-512, 512, size=(N, 2, h, w)) / 64.0).astype(F32)
    est_mask, gt_mask = rng.random((N, h, w)) > 0.1, rng.random((N, h, w)) > 0.1
    est_mask[:, 1, 1], est0[:, 0, 1, 1] = False, 1000.0        # an error that does not count and is larger than every one that does
    plants = [(h // 2, w // 2), (0, 3), (h - 1, 6), (4, 0), (7, w - 1), (h - 1, w - 1), (0, 0), (5, 8), (5, 9), (9, 11), (9, 12)]
    values = (NAN, PINF, NINF, FLT_MAX, -FLT_MAX, NAN, PINF, PINF, NINF, FLT_MAX, -FLT_MAX)
    est, gt = est0.copy(), gt0.copy()
    target = {'finite': None, 'est': est, 'gt': gt}[variant]
    for i, ((y, x), val) in enumerate(zip(plants, values)):
        est_mask[:, y, x] = gt_mask[:, y, x] = True
        if target is not None:
            target[:, i % 2, y, x] = val
    if variant == 'est':
        est = pools(est, est0)
    elif variant == 'gt':
        gt = pools(gt, gt0)
    hit = differs(est, est0) | differs(gt, gt0)
    out = dict(est=est, gt=gt, est_mask=est_mask, gt_mask=gt_mask, hit=hit, h=h, w=w, variant=variant)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


# ---- the comparisons both tiers use ---------------------------------------------------------------------------------------------------
def check_record_sum(got, want, count, bound_rel=2.0 ** -52):
    """The rule of the record sums: NaN, +inf, or within count * bound_rel relative of the exact sum (scalars or arrays of one shape)"""
    shape = np.shape(want)
    for g, e, c, b in zip(np.ravel(got), np.ravel(want), np.broadcast_to(count, shape).ravel(), np.broadcast_to(bound_rel, shape).ravel()):
        if np.isnan(e) or np.isinf(e):
            assert sv.classes(np.float64(g)) == sv.classes(np.float64(e)), (g, e)
        else:
            assert np.isfinite(g) and abs(g - e) <= c * b * e, (g, e, c)


def check_gradient(got, want, big_a, zero, ulp32, what=""):
    """got float32 against (want, A) float64: exactly +0 on `zero`; the oracle's class where its value (as float32) or A is not
    finite; within 2^-22 A + ulp32(want) everywhere else.  Returns (worst ratio, share of the non-zero elements checked by class)."""
    got = np.ascontiguousarray(got)
    assert got.dtype == np.float32 and got.shape == want.shape
    assert not got[zero].view(np.uint32).any(), what
    with np.errstate(over='ignore', invalid='ignore'):
        want32 = want.astype(F32)
    by_class = (~np.isfinite(want32) | ~np.isfinite(big_a)) & ~zero
    assert np.array_equal(sv.classes(got)[by_class], sv.classes(want32)[by_class]), (what, "class")
    rest = ~by_class & ~zero
    assert np.isfinite(got[rest]).all(), what
    with np.errstate(invalid='ignore'):
        bound = 2.0 ** -22 * big_a + ulp32(np.where(rest, want, 0.0))
        ratio = np.where(rest, np.abs(got.astype(np.float64) - np.where(rest, want, 0.0)) / bound, 0.0)
    assert np.all(ratio <= 1.0), (what, float(ratio.max()))
    return float(ratio.max()), float(by_class.sum()) / max(int((~zero).sum()), 1)
