"""Inputs of tests/test_loss_specials_host.py and tests/test_gpu_loss_specials*.py (a helper module, not a test): the fused loss and
metric kernels and the cost volume (3.24) at NAMED sample positions and on NaN, +-inf and +-FLT_MAX.

Samplers (photometric, census, consistency).  `sampler_case` puts `special_values.warp_case` under the three kernels that restate the
sampler of warp_bwd_kernel: the named OUTPUT pixels sample an integer position (east / south weight exactly 0), the last row, column
and corner (the east / south taps leave the frame at fraction 0), -1, 0, w - 1, w, and carry vectors of +-3.4e38, +-1e-42, 2^24, 2^31.
Variants: 'finite' (positions only), 'other' (specials in the sampled frame: at the sampled and the weight-0 source pixels, plus a
sprinkle), 'img' (specials in the frame on the flow's own grid), 'vectors' (NaN, +inf, -inf in the vectors themselves).

Stencils (smoothness, error_stats).  `smoothness_case` and `error_case` plant the same values in the vectors, in the ground truth and in
the guidance image: inside the frame, on its first and last row and column and on both sides of a tile edge.

SSIM and the cost volume.  `ssim_case` and `cost_volume_case` take the positions, flow and masks of `sampler_case` with the images on the
scale 0 .. 1 and specials at the named pixels only; the cost volume adds 'unsampled' (specials in `other` that only pixels that are not
usable tap) and 'upstream' (specials in the upstream gradient of the volume).  `check_ssim`, `check_cost_volume_kernels` and
`check_cost_volume_backward` are the comparisons of the GPU tier, which the host tier runs on the oracles.

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


# ---- SSIM and the cost volume -----------------------------------------------------------------------------------
# Both take the named positions, the flow and the masks of `sampler_case` with specials at CENSUS_PLANTS only (a plant reaches every
# centre within R of a reader and every gradient element within 2 R: no sprinkle).  The images are on the scale 0 .. 1: the finite images
# of `sampler_case` divided by 256.0f (exact), the specials planted AFTER the scaling -- FLT_MAX stays FLT_MAX, a denormal a denormal.
SSIM_VARIANTS = ('finite', 'other', 'img', 'vectors')
SSIM_FRAMES = [(37, 53, 3), (67, 131, 5), (67, 131, 7), CENSUS_TILE_FRAME + (3,)]          # (h, w, window); the 64 x 16 tile of ofl_ssim.hip
CV_VARIANTS = ('finite', 'other', 'feat', 'vectors', 'unsampled', 'upstream')
CV_TILE_FRAME = (17, 33)                                       # one past the cost volume's tile of 32 x 16
CV_TILE_PIXELS = [(15, 31), (15, 32), (16, 31), (16, 32)]
SCALE = F32(256.0)


def _bits_differ(a, b):
    """Element by element: not the same bits"""
    return np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)


def _scaled(special, finite):
    """`finite` / 256 with the elements of `special` that are not `finite`'s put in afterwards, as they are"""
    return np.where(_bits_differ(special, finite), special, finite / SCALE).astype(F32)


def _plant_vectors(a, mask, was_usable, named, rng):
    """NaN, +inf, -inf (VECTOR_PLANTS) in the vectors of pixels that are usable in the finite variant, have a usable neighbour and are no
    named pixel: [(b, y, x)]; `a` and `mask` are written"""
    bad = []
    near = dilate(was_usable, 1)
    for b in (MIXED, MAX_ONLY, NAN_ONLY):
        free = [(y, x) for y, x in np.argwhere(was_usable[b]) if (y, x) not in named and near[b, y, x]
                and was_usable[b, max(y - 1, 0):y + 2, max(x - 1, 0):x + 2].sum() >= 2]
        for k, i in enumerate(rng.permutation(len(free))[:len(VECTOR_PLANTS)]):
            y, x = (int(v) for v in free[i])
            comp, val = VECTOR_PLANTS[k]
            a[b, comp, y, x] = NAN if b == NAN_ONLY else val
            mask[b, y, x] = True
            bad.append((b, y, x))
    return bad


def _freeze(out):
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def ssim_case(h, w, ref, variant, c=3, half=False, u8=False):
    """The dict of `sampler_case(..., census=True)` with the images on the scale 0 .. 1 (uint8 samples with `u8`, finite variant only);
    'vectors' plants its own: every planted pixel is usable in the finite variant next to another usable pixel."""
    assert variant in SSIM_VARIANTS and not (u8 and variant != 'finite')
    import ssim_oracle as sso
    fin = sampler_case(h, w, ref, 'finite', c, half, True)
    base = fin if variant == 'vectors' else sampler_case(h, w, ref, variant, c, half, True)
    out = dict(base)
    if u8:
        out['img'], out['other'] = as_uint8(fin['img']), as_uint8(fin['other'])
    else:
        out['img'], out['other'] = _scaled(base['img'], fin['img']), _scaled(base['other'], fin['other'])
    if variant == 'vectors':
        a, mask = np.array(fin['a'], np.float32), fin['mask'].copy()
        res = sso.compute(fin['a'], fin['mask'], fin['img'] / SCALE, fin['other'] / SCALE, ref)
        named = set(p for v in fin['names'].values() for p in v)
        out['bad_vec'] = _plant_vectors(a, mask, res['usable'], named, np.random.default_rng(77 + 31 * h + w))
        with np.errstate(over='ignore'):
            out['a'], out['mask'] = (a.astype(np.float16) if half else a), mask
    out.update(variant=variant, u8=u8)
    return _freeze(out)


def cv_frames():
    """[(h, w, radius, C)] of the cost-volume cases: 20 x 28 at r = 1; 37 x 53 at r = 4 (a 32 x 16 tile + 21 by two tiles + 5) with one
    channel more than the kernel stages together; 17 x 33 at r = 1 with the plants on both sides of the tile edges"""
    import cost_volume_oracle as cvo
    return [(20, 28, 1, 3), (37, 53, 4, cvo.geometry()["kChanChunk"] + 1), CV_TILE_FRAME + (1, 3)]


def tapped(a, ref, out_hit):
    """[N,H,W] bool: the source pixels that a tap INSIDE the frame of an output pixel of `out_hit` [N,H,W] falls on, whatever its weight
    (the transpose of `readers`)"""
    a = np.asarray(a).astype(F32)
    n, _, h, w = a.shape
    t = go.warp_taps(a, n, sign_of(ref))
    out = np.zeros((n, h * w), bool)
    for j in range(4):
        ok = t.ok[j] & out_hit
        out[np.nonzero(ok)[0], t.idx[j][ok]] = True
    return out.reshape(n, h, w)


@functools.lru_cache(maxsize=None)
def cost_volume_case(h, w, ref, variant, c, half=False):
    """dict: a float32 [N,2,h,w] (float16 with `half`), mask bool [N,h,w], feat, other float32 [N,c,h,w], g float32 [N,D,h,w], radius,
    names, aimed, bad_vec [(b, y, x)], feat_hit / other_hit / g_hit bool [N,h,w] (the pixels at which feat, other, any plane of g differ
    from the finite variant), usable bool [N,h,w] of the oracle.  'other' and 'feat' plant at the named pixels only (the tile frame: at
    CV_TILE_PIXELS only); 'unsampled' plants NaN / +inf / -inf in pixels of `other` that no usable sample taps and an unusable one
    does; 'upstream' plants in g inside the frame, on its last row and column and on both sides of a tile edge."""
    import cost_volume_oracle as cvo
    assert variant in CV_VARIANTS and ref in REFS
    radius = {f[:2]: f[2] for f in cv_frames()}[(h, w)]
    fin = sampler_case(h, w, ref, 'finite', c, half, True)
    tile = (h, w) == CV_TILE_FRAME
    rng = np.random.default_rng(4242 + 31 * h + w + c + (0 if ref == 's' else 500))
    feat0, other0 = fin['img'] / SCALE, fin['other'] / SCALE
    g0 = cvo.upstream(N, (2 * radius + 1) ** 2, h, w)
    a, mask = np.array(fin['a'], np.float32), fin['mask'].copy()
    feat, other, g = feat0.copy(), other0.copy(), g0.copy()
    usable0 = cvo.usable_of(fin['a'], fin['mask'], ref)
    bad_vec = []
    if variant in ('other', 'feat'):
        key = 'other' if variant == 'other' else 'img'
        target = other if variant == 'other' else feat
        if tile:
            for i, (y, x) in enumerate(CV_TILE_PIXELS):
                for ch in range(c):
                    target[:, ch, y, x] = sv.NONFINITE[(i + ch) % 3]
        else:
            base = sampler_case(h, w, ref, key, c, half, True)
            target[...] = _scaled(base[key], fin[key])
        target[...] = pools(target, other0 if variant == 'other' else feat0)
    elif variant == 'vectors':
        named = set(p for v in fin['names'].values() for p in v)
        bad_vec = _plant_vectors(a, mask, usable0, named, rng)
    elif variant == 'unsampled':
        free = tapped(a, ref, ~usable0) & ~tapped(a, ref, usable0)
        assert free[:CLEAN].sum((1, 2)).min() >= 2, free.sum((1, 2))
        for b in range(N):
            for i, (y, x) in enumerate(np.argwhere(free[b])[:6]):
                other[b, i % c, y, x] = sv.NONFINITE[i % 3]
        other = pools(other, other0)
    elif variant == 'upstream':
        d = g.shape[1]
        spots = [(h // 2, w // 2), (h - 1, 5), (7, w - 1), (h - 1, w - 1), (15, 9), (16, 9)] + ([(3, 31), (3, 32)] if w > 32 else [])
        values = (NAN, PINF, NINF, FLT_MAX, -FLT_MAX)
        for i, (y, x) in enumerate(spots):
            g[:, (5 * i + 2) % d, y, x] = values[i % len(values)]
        g = pools(g, g0)
    usable = cvo.usable_of(a, mask, ref)
    if half:
        with np.errstate(over='ignore'):
            a = a.astype(np.float16)
    return _freeze(dict(a=a, mask=mask, feat=feat, other=other, g=g, radius=radius, names=fin['names'], aimed=fin['aimed'], bad_vec=bad_vec,
                        feat_hit=differs(feat, feat0), other_hit=differs(other, other0), g_hit=differs(g, g0), usable=usable, h=h, w=w,
                        c=c, ref=ref, variant=variant, half=half))


def cv_touched(case):
    """dict of [N,h,w] bool, the pixels whose element may differ from the finite variant: 'warped' (W': a tap on a differing pixel of
    `other`, a vector that is not finite), 'volume', 'd_feat' (a differing staged W' within r; feat, g at the pixel), 'd_w' (feat or g
    within r; usable itself), 'd_flow' (d W at the pixel, a tap, the vector), 'd_other' (d W at a reader of the pixel)"""
    r = case['radius']
    wp = readers(case['a'], case['ref'], case['other_hit'])
    bad = np.zeros_like(wp)
    for b, y, x in case['bad_vec']:
        bad[b, y, x] = True
    wp = wp | bad
    near = dilate(wp, r)
    d_w = dilate(case['feat_hit'] | case['g_hit'], r) | bad
    finite_a = np.where(np.isfinite(np.asarray(case['a'], F32)), np.asarray(case['a'], F32), F32(0.0))
    return {'warped': wp, 'volume': near | case['feat_hit'], 'd_feat': near | case['g_hit'], 'd_w': d_w, 'd_flow': d_w | wp,
            'd_other': tapped(finite_a, case['ref'], d_w) | tapped(np.asarray(case['a'], F32), case['ref'], bad)}


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


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _over(hit, like):
    """[N,h,w] -> the shape of `like` [N,*,h,w]"""
    return np.broadcast_to(hit[:, None], like.shape)


def _same(got, want, what):
    assert sv.same_bits(got, want).all(), (what, sv.describe(got, want))


# ---- SSIM: the comparison of one launch set with the oracle and with the finite variant ------------------------------------------------
def check_ssim(case, window, rec, smap, loss, grad, fin, what=""):
    """rec float64 [N,8], smap float32 [N,h,w], loss float32 [N], grad float32 [N,2,h,w] of one case at one window, and `fin` = (rec,
    smap, grad) of the finite variant with the same storage (None when this IS the finite variant): the bars of
    tests/test_gpu_loss_specials_ssim.py.  Returns (the worst gradient element as a share of its bound, the share of the non-zero
    elements held by class only)."""
    import ssim_oracle as sso
    ref, r = case['ref'], window // 2
    want = sso.compute(case['a'], case['mask'], case['img'], case['other'], ref, window)
    g_want, big_a = sso.grad(case['a'], case['mask'], case['img'], case['other'], ref, window, upstream=UPSTREAM, res=want)
    known = want['known']
    assert smap.dtype == np.float32 and rec.dtype == np.float64 and loss.dtype == np.float32
    _same(smap, want['map'], what + " map")                                                 # (+0 where not known)
    assert not _bits(smap)[~known].any(), what
    assert np.array_equal(rec[:, 0], want['records'][:, 0]) and np.array_equal(rec[:, 3], want['records'][:, 3]), what + " counts"
    for i in range(N):                                                                      # sum and max by the rule of 3.16
        vals = smap[i][known[i]].astype(np.float64)
        assert rec[i, 2] == sv.record_max(vals), (what, "max", i)
        check_record_sum(rec[i, 1], sv.record_sum(vals), vals.size)
    assert not rec[:, 4:].any(), what
    with np.errstate(invalid='ignore', divide='ignore'):
        _same(loss, (rec[:, 1] / rec[:, 0]).astype(np.float32), what + " loss")
    zero = ~_over(known, grad)
    ratio, share = check_gradient(grad, g_want, big_a, zero, sso.ulp32, what)
    for b, y, x in case['bad_vec']:
        assert not known[b, y, x] and not _bits(grad[b, :, y, x]).any() and not _bits(smap[b, y, x]), what
    if fin is None:
        assert np.isfinite(smap).all() and np.isfinite(grad).all() and np.isfinite(rec).all(), what
        for name in BORDER:
            y, x = case['names'][name][0]
            assert np.all(grad[:, :, y, x] != 0), (what, name)                              # the border pixels carry a gradient
        return ratio, share
    f_rec, f_map, f_grad = fin
    touched, touched2 = sampler_touched(case, r), sampler_touched(case, 2 * r)
    assert not touched2[CLEAN].any() and np.array_equal(rec[CLEAN].view(np.uint64), f_rec[CLEAN].view(np.uint64)), what + " clean record"
    assert np.array_equal(_bits(smap[CLEAN]), _bits(f_map[CLEAN])) and np.array_equal(_bits(grad[CLEAN]), _bits(f_grad[CLEAN])), what + " clean"
    assert np.array_equal(_bits(smap)[~touched], _bits(f_map)[~touched]), what + " isolation"
    # (a vector that is not finite takes its pixel out of the count, and with it changes the scale of its image's gradient)
    assert case['variant'] == 'vectors' or np.array_equal(rec[:, 0], f_rec[:, 0]), what
    t2 = _over(touched2 | (rec[:, 0] != f_rec[:, 0])[:, None, None], grad)
    assert np.array_equal(_bits(grad)[~t2], _bits(f_grad)[~t2]), what + " isolation of the gradient"
    return ratio, share


# ---- the cost volume ------------------------------------------------------------------------------------------------------------------
def check_cost_volume_kernels(case, got, fin, what=""):
    """got: {'volume', 'd_feat', 'd_w'} float32 arrays of the three launches on `case`; fin: the same of the finite variant (None when
    this IS it).  Bars (a) to (d) of tests/test_gpu_loss_specials_cost_volume.py."""
    import cost_volume_oracle as cvo
    ref, radius = case['ref'], case['radius']
    res = cvo.compute(case['a'], case['mask'], case['feat'], case['other'], ref, radius)
    want_f, want_w = cvo.grads(case['a'], case['mask'], case['feat'], case['other'], ref, radius, case['g'], res=res)
    assert np.array_equal(res['usable'], case['usable'])
    for name, want in (('volume', res['volume']), ('d_feat', want_f), ('d_w', want_w)):                         # (a)
        _same(got[name], want, what + " " + name)
    assert not _bits(got['d_w'])[~_over(case['usable'], got['d_w'])].any(), what + ": d W where not usable"
    if fin is None:
        assert all(np.isfinite(got[k]).all() for k in ('volume', 'd_feat', 'd_w')), what
        return
    touched = cv_touched(case)
    for name in ('volume', 'd_feat', 'd_w'):
        t = _over(touched[name], got[name])
        assert not touched[name][CLEAN].any(), what
        assert np.array_equal(_bits(got[name])[~t], _bits(fin[name])[~t]), what + ": isolation of " + name        # (b)
        assert np.array_equal(_bits(got[name][CLEAN]), _bits(fin[name][CLEAN])), what + ": clean " + name        # (c)
    for b, y, x in case['bad_vec']:                                                                              # (d)
        assert not case['usable'][b, y, x] and not _bits(res['warped'][b, :, y, x]).any(), what
        assert not _bits(got['d_w'][b, :, y, x]).any(), what


def check_cost_volume_backward(case, got, fin, what=""):
    """got: {'d_feat', 'd_other', 'd_flow'} float32 arrays of `backward()` on `case`; fin: the same of the finite variant.  Bar (e) on
    the variants 'finite', 'unsampled' and 'vectors', bar (f) on 'feat', 'other' and 'upstream'.  Returns {name: (max error, scale)}
    under (e)."""
    import cost_volume_oracle as cvo
    ref, radius, variant = case['ref'], case['radius'], case['variant']
    unusable = ~case['usable']
    assert all(got[k].dtype == np.float32 for k in ('d_feat', 'd_other', 'd_flow'))
    assert unusable.mean() > 0.1 and not _bits(got['d_flow'])[_over(unusable, got['d_flow'])].any(), what + ": d flow where not usable"
    if variant in ('finite', 'unsampled', 'vectors'):
        for name in ('d_feat', 'd_other', 'd_flow'):
            assert np.isfinite(got[name]).all(), (what, name, int((~np.isfinite(got[name])).sum()))
        planted = case['other_hit']
        assert variant != 'unsampled' or planted[:CLEAN].sum((1, 2)).min() >= 2
        assert not got['d_other'][_over(planted, got['d_other'])].any(), what + ": d other at the planted pixels"
        # the reference: the planted values are inputs of no usable sample, so it is evaluated with 0 in their place
        a32 = np.asarray(case['a'], F32)
        # (so are the vectors that are not finite and the extreme ones whose float32 position overflows: none of them is usable)
        with np.errstate(all='ignore'):
            sx, sy = go.warp_positions(a32, N, sign_of(ref))
        lost = ~(np.isfinite(sx) & np.isfinite(sy))
        assert not (lost & case['usable']).any()
        a0 = np.where(lost[:, None], F32(0.0), a32).astype(F32)
        other0 = np.where(_over(planted, case['other']), F32(0.0), case['other']).astype(F32)
        want = cvo.torch_reference(a0, case['usable'], case['feat'], other0, ref, radius, case['g'])
        out = {}
        for name in ('d_feat', 'd_other', 'd_flow'):
            scale, err = np.abs(want[name]).max(), np.abs(got[name] - want[name]).max()
            out[name] = (float(err), float(scale))
            assert scale > 1e-2 and err <= 2e-4 * scale, (what, name, err, scale)
        return out
    touched = cv_touched(case)
    for name in ('d_feat', 'd_other', 'd_flow'):
        assert np.array_equal(_bits(got[name][CLEAN]), _bits(fin[name][CLEAN])), what + ": clean " + name
        t = _over(touched[name], got[name])
        assert np.array_equal(_bits(got[name])[~t], _bits(fin[name])[~t]), what + ": isolation of " + name
    aimed = {'feat': 'd_flow', 'other': 'd_feat', 'upstream': 'd_feat'}[variant]
    assert all((~np.isfinite(got[aimed][b])).any() for b in (MIXED, NAN_ONLY)), what
    return {}
