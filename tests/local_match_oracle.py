"""The definition of Flow.match_local in NumPy, vectorised over the pixels with loops over the offsets and the channels (a
helper module, not a test; test modules import it), the inputs the CPU and the GPU tier share, and the textbook expression in torch.  The
warp (W', usable), the chain vectors and the float64 backward of the warp are those of cost_volume_oracle.py.

    offsets  o = (dy, dx), dy outermost, both ascending from -r.  A position p + o outside the frame takes NO part; one inside always
             does, with W' = +0 where it is not usable
    s(p, o)  = (sum_c feat_c(p) * W'_c(p + o)) / sqrt_rn(float32(C)): float32, from +0, c ascending, product then sum, one division
    softmax  m = the first participating logit, replaced by every later one with s > m; then e = exp(f64(s) - f64(m)), S = S + e,
             X = X + e f64(dx), Y = Y + e f64(dy) in offset order, float64 from +0
    result   ox = X / S, oy = Y / S; u' = float32(f64(u) + (-sign) ox), v' alike; prob = float32(1 / S)
    pair     G = -sign f64(g); w = exp(f64(s) - f64(m)) / S; ds = float32(w * ((G_x * (f64(dx) - ox)) + (G_y * (f64(dy) - oy))));
             dss = ds / root, exactly +0 outside the frame
    d feat_c(p) = sum_o dss(p, o) * W'_c(p + o);  d W_c(q) = usable(q) ? sum_o dss(q - o, o) * feat_c(q - o) : +0, q - o in the frame:
             o ascending, float32 product then sum from +0
    d flow   = g + gate(backward of the warp applied to d W): the upstream gradient itself where the pixel is not usable
"""
import functools
import os
import re

import numpy as np
import torch

import cost_volume_oracle as cvo
import grad_oracle64 as go
import matching_oracle as mo
import photometric_oracle as po
from cost_volume_oracle import chain, chain_vectors, usable_of, warped  # noqa: F401  (the definition's warp, by import)

F32, F64 = np.float32, np.float64
ROOT = mo.ROOT
RADII = (1, 2, 3, 4)
RADIUS = 4
REFS = cvo.REFS
sign_of = cvo.sign_of
offsets = cvo.offsets
ulp32 = mo.ulp32
MUTANTS = ("pad_zero", "unusable_excluded", "over_c", "swap_xy", "t_sign", "no_identity")


# ---- the kernels' geometry and the frames and channel counts it gives the GPU tier -----------------------------------------------------
def geometry():
    """The constants of ofl_local_match.hip: the forward's tile, the channel chunk, the gathers' tile"""
    with open(os.path.join(ROOT, 'oflibpytorch_amd', 'csrc', 'ofl_local_match.hip')) as fh:
        text = fh.read()
    out = {}
    for name in ("kTileW", "kTileH", "kChanChunk", "kGTileW", "kGTileH"):
        m = re.search(r"constexpr int [^;\n]*\b%s = (\d+)[,;]" % name, text)
        assert m, name
        out[name] = int(m.group(1))
    return out


def frames():
    """(n, h, w): four frames smaller than the window; the width and the height of the forward's and the gathers' tiles, each minus one,
    exact, plus one and twice plus one (the other extent small and odd); a batch of 3; a frame of one pixel more than the larger tile in
    both directions, which every tile border crosses"""
    g = geometry()
    out = [(1, 2, 2), (1, 2, 7), (1, 7, 2), (1, 2, 3)]
    for t in sorted(set((g["kTileW"], g["kGTileW"]))):
        out += [(1, 3, e) for e in (t - 1, t, t + 1, 2 * t + 1)]
    for t in sorted(set((g["kTileH"], g["kGTileH"]))):
        out += [(1, e, 5) for e in (t - 1, t, t + 1, 2 * t + 1)]
    out += [(3, 11, 13), (1, g["kGTileH"] + 1, g["kGTileW"] + 1)]
    seen = []
    for f in out:
        if f not in seen:
            seen.append(f)
    return seen


def channels():
    """1, then the channel chunk minus one, exact, plus one, and two chunks plus one"""
    k = geometry()["kChanChunk"]
    return sorted(set(c for c in (1, k - 1, k, k + 1, 2 * k + 1) if c >= 1))


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def features_general(n, c, h, w):
    """(feat, other) float32 [n,c,h,w]: N(0, 1) on a grid of 2^-6 (matching_oracle.features_general)"""
    return mo.features_general(n, c, h, w)


@functools.lru_cache(maxsize=None)
def upstream(n, h, w):
    """The upstream gradient float32 [n,2,h,w] on a grid of 2^-6 in [-1, 1]"""
    g = (np.random.RandomState(977 + 1000 * n + 10 * h + w).randint(-64, 65, size=(n, 2, h, w)) / 64.0).astype(F32)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def vectors_general(n, h, w):
    """The flow float32 [n,2,h,w] on a grid of 2^-6, a few pixels long; every seventh pixel points far out of the frame and the first
    column of a frame wider than 3 points left out of it: at least a tenth of the pixels are not usable"""
    rng = np.random.RandomState(5471 + 1000 * n + 10 * h + w)
    v = (rng.randint(-160, 161, size=(n, 2, h, w)) / 64.0).astype(F32)
    far = (np.arange(n * h * w).reshape(n, h, w) % 7) == 3
    v[:, 0][far] = F32(3.0 * (h + w))
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def vectors_integer(n, h, w, ref):
    """INTEGER-valued vectors that differ from pixel to pixel, in [-2, 2]; every eleventh pixel points wholly out of the frame, and so does
    every pixel whose sample position -- the float32 un-normalisation of an integer -- is not that integer bit for bit (a few columns and
    rows of a frame whose extent minus one is no power of two): W' is a value of `other` or +0 everywhere"""
    rng = np.random.RandomState(8111 + 1000 * n + 10 * h + w)
    v = rng.randint(-2, 3, size=(n, 2, h, w)).astype(F32)
    sx, sy = (np.asarray(s) for s in go.warp_positions(v, n, sign_of(ref)))
    far = ((np.arange(n * h * w).reshape(n, h, w) % 11) == 2) | (sx != np.round(sx)) | (sy != np.round(sy))
    v[:, 1][far] = F32(2 * (h + w) + 5)
    v.setflags(write=False)
    return v


def exact_kinds(c):
    return ('one-hot', 'two-hot', 'all-equal') + (('rising',) if c == 16 else ())


def planted_offsets(radius):
    """The offsets the one-hot family plants in turn away from the tile borders: the window's centre, its four corners and the middles of
    its edges"""
    r = radius
    return [(0, 0), (-r, -r), (-r, r), (r, -r), (r, r), (0, -r), (0, r), (-r, 0), (r, 0)]


def tile_borders(h, w):
    """(xs, ys): the columns and rows inside the frame at which a tile of the forward or of the gathers begins"""
    g = geometry()
    xs = sorted(set(b for t in (g["kTileW"], g["kGTileW"]) for b in range(t, w, t)))
    ys = sorted(set(b for t in (g["kTileH"], g["kGTileH"]) for b in range(t, h, t)))
    return xs, ys


def planted_field(h, w, radius):
    """(dy, dx) int [h, w]: the offset the one-hot family plants at every pixel -- planted_offsets() in turn, and ACROSS every tile border
    on both of its sides: the last column before a border plants (0, +d), the first one after it (0, -d), the last row before a border
    (+d, 0) and the first one after it (-d, 0), d running through 1 .. radius along the border (a corner takes the column's)"""
    yy, xx = np.mgrid[0:h, 0:w]
    plant = np.asarray(planted_offsets(radius))
    which = (yy * w + xx) % len(plant)
    dy, dx = plant[which, 0], plant[which, 1]
    xs, ys = tile_borders(h, w)
    for b in ys:                                                                             # (d stays inside the frame)
        d = 1 + np.arange(w) % radius
        dy[b - 1], dx[b - 1] = np.minimum(d, h - b), 0
        dy[b], dx[b] = -np.minimum(d, b), 0
    for b in xs:
        d = 1 + np.arange(h) % radius
        dy[:, b - 1], dx[:, b - 1] = 0, np.minimum(d, w - b)
        dy[:, b], dx[:, b] = 0, -np.minimum(d, b)
    return dy, dx


def crossings(fwd, radius, tile_w, tile_h):
    """{'+x', '-x', '+y', '-y': int}: the pairs (p, o) of compute()'s result `fwd` with a match -- the logit 0 against a usable position
    inside the frame -- whose position p + o lies in the next (+) or the previous (-) tile of tile_w x tile_h pixels along that axis"""
    n, _, h, w = fwd['s'].shape
    yy, xx = np.mgrid[0:h, 0:w]
    out = {'+x': 0, '-x': 0, '+y': 0, '-y': 0}
    for o, (dy, dx) in enumerate(offsets(radius)):
        hit = fwd['part'][:, o] & (fwd['s'][:, o] == 0) & cvo._shifted(fwd['usable'], radius, dy, dx)
        sx = np.clip(xx + dx, 0, w - 1) // tile_w - xx // tile_w
        sy = np.clip(yy + dy, 0, h - 1) // tile_h - yy // tile_h
        for key, m in (('+x', sx > 0), ('-x', sx < 0), ('+y', sy > 0), ('-y', sy < 0)):
            out[key] += int((hit & m[None]).sum())
    return out


def features_exact(kind, a, mask, ref, c, radius):
    """(feat, other) float32 [n,c,h,w] in {0, +-32} (matching_oracle._encode) for the INTEGER vectors `a`: the word of W'(q) is the word
    of `other` at the position q samples, and the logit of two words is 0 (the same) or at most -1024 (different) -- and +0 against the
    W' = +0 of a pixel that is not usable, which TIES with a match (not in 'two-hot').
    'one-hot'   `other` carries a matchable word at every third position of every third row, and at the position that the planted
                target p + o* of a pixel p beside a tile border samples, and the last word, which no pixel is given, elsewhere; pixel p
                carries the word of W'(p + o*), o* from planted_field() (word 0 where p + o* is outside the frame, not usable or carries
                the last word): a match straddles every tile border in both directions
    'two-hot'   `other` carries each matchable word at two neighbouring positions of every third row, and BOTH sides carry the `feat`
                encoding, in which equal bits add: a match has the largest logit, a different word and the +0 of a pixel that is not
                usable lie at least 1024 below it, and a pixel whose window holds its word twice has two weights of exactly 1/2
    'all-equal' every pixel and every position carry word 0
    'rising'    `other` carries the complement of word A, A's neighbour B and A in columns x mod 3 = 0, 1, 2: along a window row the
                maximum of a pixel with word A rises from -2048 to -1024 to 0"""
    a = np.asarray(a, F32)
    n, _, h, w = a.shape
    k = len(mo.codes(c))
    yy, xx = np.mgrid[0:h, 0:w]
    usable = usable_of(a, mask, ref)
    sign = sign_of(ref)
    sy = np.clip(yy[None] - (sign * a[:, 1]).astype(np.int64), 0, h - 1)                    # the position a usable pixel samples
    sx = np.clip(xx[None] - (sign * a[:, 0]).astype(np.int64), 0, w - 1)
    ocls = np.zeros((n, h, w), np.int64)
    if kind == 'one-hot':
        word = ((yy // 3) * 5 + xx // 3) % (k - 1)
        ocls[:] = np.where((yy % 3 == 0) & (xx % 3 == 0), word, k - 1)[None]
        pdy, pdx = planted_field(h, w, radius)
        ty, tx = yy + pdy, xx + pdx
        inside = (ty >= 0) & (ty < h) & (tx >= 0) & (tx < w)
        tyc, txc = np.clip(ty, 0, h - 1), np.clip(tx, 0, w - 1)
        xs, ys = tile_borders(h, w)
        beside = np.zeros((h, w), bool)
        for b in ys:
            beside[b - 1:b + 1] = True
        for b in xs:
            beside[:, b - 1:b + 1] = True
        for i in range(n):
            for y, x in zip(*np.nonzero(beside & inside & usable[i, tyc, txc])):
                t = (tyc[y, x], txc[y, x])
                ocls[i, sy[i][t], sx[i][t]] = word[t]
    elif kind == 'two-hot':
        word = ((yy // 3) * 5 + xx // 3) % (k - 1)
        ocls[:] = np.where((yy % 3 == 0) & (xx % 3 < 2), word, k - 1)[None]
    elif kind == 'rising':
        cw = mo.codes(c)
        comp = cw.index(tuple(1 - x for x in cw[0]))
        nb = next(i for i in range(k) if i not in (0, comp))
        ocls[:] = np.choose(xx % 3, [comp, nb, 0])[None]
    elif kind != 'all-equal':
        raise ValueError(kind)
    other = np.ascontiguousarray(np.moveaxis(mo._encode(ocls, c, 'other'), -1, 1))
    if kind == 'two-hot':
        other = np.ascontiguousarray(np.moveaxis(mo._encode(ocls, c, 'feat'), -1, 1))        # equal bits add: a match is the largest logit
    wcls = np.take_along_axis(ocls.reshape(n, -1), (sy * w + sx).reshape(n, -1), 1).reshape(n, h, w)     # the word of W' where usable
    fcls = wcls.copy()
    if kind == 'one-hot':
        ok = inside[None] & usable[:, tyc, txc] & (wcls[:, tyc, txc] != k - 1)
        fcls = np.where(ok, wcls[:, tyc, txc], 0)
    elif kind == 'two-hot':
        plant = np.asarray(planted_offsets(radius))[(yy * w + xx) % 9]
        ty, tx = yy + plant[..., 0], xx + plant[..., 1]
        inside = (ty >= 0) & (ty < h) & (tx >= 0) & (tx < w)
        tyc, txc = np.clip(ty, 0, h - 1), np.clip(tx, 0, w - 1)
        ok = inside[None] & usable[:, tyc, txc] & (wcls[:, tyc, txc] != k - 1)
        fcls = np.where(ok, wcls[:, tyc, txc], 0)
    elif kind == 'rising':
        fcls[:] = 0
    feat = np.ascontiguousarray(np.moveaxis(mo._encode(fcls, c, 'feat'), -1, 1))
    return feat, other


def masks(n, h, w):
    """{name: bool [n,h,w] or None}: none; single False pixels on either side of every tile border and at the corners; a checkerboard;
    one image fully False"""
    g = geometry()
    out = {'none': None}
    single = np.ones((n, h, w), bool)
    ys = sorted(set(y for t in (g["kTileH"], g["kGTileH"]) for y in (t - 1, t, 2 * t - 1, 2 * t)) | {0, h - 1})
    xs = sorted(set(x for t in (g["kTileW"], g["kGTileW"]) for x in (t - 1, t, 2 * t - 1, 2 * t)) | {0, w - 1})
    i = 0
    for y in ys:
        for x in xs:
            if 0 <= y < h and 0 <= x < w:
                single[i % n, y, x] = False
                i += 1
    out['single'] = single
    yy, xx = np.mgrid[0:h, 0:w]
    out['checker'] = np.broadcast_to(((yy + xx) % 2 == 0)[None], (n, h, w)).copy()
    full = np.ones((n, h, w), bool)
    full[n - 1] = False
    out['one-image-masked'] = full
    return out


# ---- the definition -------------------------------------------------------------------------------------------------------------------
def _inframe(h, w, radius):
    """bool [D, h, w]: is p + o inside the frame"""
    frame = np.ones((h, w), bool)
    return np.stack([cvo._shifted(frame, radius, dy, dx) for dy, dx in offsets(radius)], 0)


def compute(a, mask, feat, other, ref, radius=RADIUS, wide=False, mutant=None):
    """{'out': [n,2,h,w] float64, before the last rounding; 'out32': rounded once; 'prob' float32 [n,h,w]; 'm' (float32; float64 with
    `wide`), 'S', 'ox', 'oy' float64 [n,h,w]; 's' [n,D,h,w] the logits; 'part' bool [n,D,h,w]; 'w' float64 [n,D,h,w] the weights; 'mag'
    A = sum_o w |o - E[o]| per component [n,2,h,w]; 'terms' [n,h,w]; 'warped', 'usable'}.  `wide`: the same steps in float64."""
    assert radius in RADII
    T = F64 if wide else F32
    f = po._as_f32(a)
    wp, usable, _ = warped(f, mask, other, ref)
    n, chan, h, w = wp.shape
    ft = cvo._as_feat(feat, n)
    assert ft.shape == wp.shape
    offs = offsets(radius)
    root = np.sqrt(T(chan)) if mutant != 'over_c' else T(chan)
    inf = _inframe(h, w, radius)
    part = np.broadcast_to(inf[None], (n,) + inf.shape).copy()
    if mutant == 'pad_zero':
        part[:] = True
    if mutant == 'unusable_excluded':
        part &= np.stack([cvo._shifted(usable, radius, dy, dx) for dy, dx in offs], 1)
        part[:, len(offs) // 2] = True                                                       # (the centre stays: no pixel is empty)
    s = np.zeros((n, len(offs), h, w), T)
    with np.errstate(all='ignore'):
        for o, (dy, dx) in enumerate(offs):
            acc = np.zeros((n, h, w), T)
            sh = cvo._shifted(wp, radius, dy, dx)
            for c in range(chan):
                prod = ft[:, c].astype(T) * sh[:, c].astype(T)
                acc = acc + prod
            s[:, o] = acc / root
        started = np.zeros((n, h, w), bool)
        m = np.zeros((n, h, w), T)
        for o in range(len(offs)):
            on, st = part[:, o], s[:, o]
            m = np.where(on & ~started, st, np.where(on & started & (st > m), st, m))
            started = started | on
        S, X, Y = (np.zeros((n, h, w), F64) for _ in range(3))
        for o, (dy, dx) in enumerate(offs):
            if mutant == 'swap_xy':
                dy, dx = dx, dy
            on = part[:, o]
            e = np.exp(s[:, o].astype(F64) - m.astype(F64))
            S = np.where(on, S + e, S)
            X = np.where(on, X + e * F64(dx), X)
            Y = np.where(on, Y + e * F64(dy), Y)
        ox, oy = X / S, Y / S
        sg = -F64(sign_of(ref)) if mutant != 't_sign' else F64(1.0)
        out = np.stack([f[:, 0].astype(F64) + sg * ox, f[:, 1].astype(F64) + sg * oy], 1)
        wt = np.where(part, np.exp(s.astype(F64) - m.astype(F64)[:, None]) / S[:, None], 0.0)
        dxs = np.array([dx for _, dx in offs], F64)[None, :, None, None]
        dys = np.array([dy for dy, _ in offs], F64)[None, :, None, None]
        mag = np.stack([(wt * np.abs(dxs - ox[:, None])).sum(1), (wt * np.abs(dys - oy[:, None])).sum(1)], 1)
        prob = (1.0 / S).astype(F32)
    return {'out': out, 'out32': out.astype(F32), 'prob': prob, 'm': m, 'S': S, 'ox': ox, 'oy': oy, 's': s, 'part': part, 'w': wt,
            'mag': mag, 'terms': part.sum(1), 'warped': wp, 'usable': usable}


def grads(a, mask, feat, other, ref, radius, g, wide=False, mutant=None, res=None):
    """{'dss' [n,D,h,w]; 'd_feat', 'd_w' [n,C,h,w]: the definition's float32 sums (float64 throughout with `wide`); '<name>64': the
    float64 sums of the same terms; 'mag_<name>': the sums of the absolute terms; 'terms_<name>': the number of terms; 'd_other'
    [Ns,C,h,w], 'd_flow' [n,2,h,w] float64: the float64 backward of the warp applied to d W, gated, and the identity term added}"""
    T = F64 if wide else F32
    res = compute(a, mask, feat, other, ref, radius, wide) if res is None else res
    f = po._as_f32(a)
    wp, usable = res['warped'], res['usable']
    n, chan, h, w = wp.shape
    ft = cvo._as_feat(feat, n)
    g = np.asarray(g)
    assert g.dtype == F32 and g.shape == (n, 2, h, w)
    offs = offsets(radius)
    root = np.sqrt(T(chan))
    G = -F64(sign_of(ref)) * g.astype(F64)
    frame = np.ones((h, w), bool)
    dss = np.zeros((n, len(offs), h, w), T)
    with np.errstate(all='ignore'):
        for o, (dy, dx) in enumerate(offs):
            wt = np.exp(res['s'][:, o].astype(F64) - res['m'].astype(F64)) / res['S']
            t = (G[:, 0] * (F64(dx) - res['ox'])) + (G[:, 1] * (F64(dy) - res['oy']))
            dss[:, o] = np.where(res['part'][:, o], (wt * t).astype(T) / root, T(0))
        out = {'dss': dss}
        for name in ('d_feat', 'd_w'):
            out[name], out[name + '64'], out['mag_' + name] = (np.zeros((n, chan, h, w), t_) for t_ in (T, F64, F64))
            out['terms_' + name] = np.zeros((n, chan, h, w), np.int64)
        for c in range(chan):
            for o, (dy, dx) in enumerate(offs):
                inf = cvo._shifted(frame, radius, dy, dx)                                   # p + o inside
                term = dss[:, o] * cvo._shifted(wp[:, c], radius, dy, dx).astype(T)
                out['d_feat'][:, c] = np.where(inf, out['d_feat'][:, c] + term, out['d_feat'][:, c])
                out['d_feat64'][:, c] += np.where(inf, term.astype(F64), 0.0)
                out['mag_d_feat'][:, c] += np.where(inf, np.abs(term.astype(F64)), 0.0)
                out['terms_d_feat'][:, c] += inf
                back = cvo._shifted(frame, radius, -dy, -dx)                                # q - o inside
                term = cvo._shifted(dss[:, o] * ft[:, c].astype(T), radius, -dy, -dx)
                out['d_w'][:, c] = np.where(back, out['d_w'][:, c] + term, out['d_w'][:, c])
                out['d_w64'][:, c] += np.where(back, term.astype(F64), 0.0)
                out['mag_d_w'][:, c] += np.where(back, np.abs(term.astype(F64)), 0.0)
                out['terms_d_w'][:, c] += back
        for name in ('d_w', 'd_w64', 'mag_d_w'):
            out[name] = np.where(usable[:, None], out[name], out[name].dtype.type(0))
        d_other, d_warp = chain(chain_vectors(f, ref), other, out['d_w'].astype(F64), ref)
        d_warp = np.where(usable[:, None], d_warp, 0.0)
        out['d_other'] = d_other
        out['d_flow'] = d_warp if mutant == 'no_identity' else g.astype(F64) + d_warp
    return out


def forward_shift(t):
    """k of the forward's bar ulp32(want) + 2^-k A (propagate_oracle.forward_shift): k = 46 - ceil(log2 T)"""
    return 46 - np.ceil(np.log2(np.maximum(t, 1))).astype(int)


def grad_shift(t):
    """k of a gradient's bar ulp32(want) + 2^-k A (propagate_oracle.grad_shift): k = 20 - ceil(log2(T + 6))"""
    return 20 - np.ceil(np.log2(t + 6)).astype(int)


# ---- the textbook expression ----------------------------------------------------------------------------------------------------------
def textbook_expression(flow, feat, wp, sign, radius):
    """GMFlow's local matching on torch tensors of any floating dtype: the unfold-style window of the warped tensor `wp` [n,c,h,w], the
    positions outside the frame at -inf before the softmax, the expectation of the offsets added to the flow ('t': subtracted)"""
    n, c, h, w = wp.shape
    k = 2 * radius + 1
    win = torch.nn.functional.unfold(wp, k, padding=radius).reshape(n, c, k * k, h, w)
    corr = (feat[:, :, None] * win).sum(1) / (c ** 0.5)                                      # [n, D, h, w]
    ones = torch.ones((1, 1, h, w), dtype=wp.dtype)
    valid = torch.nn.functional.unfold(ones, k, padding=radius).reshape(1, k * k, h, w) > 0
    corr = corr.masked_fill(~valid, float('-inf'))
    p = torch.softmax(corr, dim=1)
    offs = torch.tensor([[dx, dy] for dy, dx in offsets(radius)], dtype=wp.dtype)            # [D, 2] = (x, y)
    exp = torch.einsum('ndhw,dk->nkhw', p, offs)
    return flow - sign * exp, p.max(1).values


def textbook(a, usable, feat, other, ref, radius, g=None):
    """float64: {'out', 'prob', and with g: 'd_feat', 'd_warped', 'd_other', 'd_flow'}: the warp as one differentiable expression (the
    explicit bilinear sample of cost_volume_oracle.torch_reference, `usable` piecewise constant and given), then textbook_expression"""
    f = po._as_f32(a)
    n, _, h, w = f.shape
    sign = sign_of(ref)
    u = torch.from_numpy(f.copy()).double().requires_grad_(True)
    ft = torch.from_numpy(np.asarray(feat).copy()).double().requires_grad_(True)
    ot = torch.from_numpy(np.asarray(other).copy()).double().requires_grad_(True)
    ft4 = (ft[None] if ft.dim() == 3 else ft).expand(n, -1, -1, -1)
    ot4 = (ot[None] if ot.dim() == 3 else ot).expand(n, -1, -1, -1)
    c = ot4.shape[1]
    px, py = (torch.from_numpy(np.ascontiguousarray(s)).double() for s in go.warp_positions(f, n, sign))
    sx, sy = px - sign * (u[:, 0] - u[:, 0].detach()), py - sign * (u[:, 1] - u[:, 1].detach())
    x0, y0 = torch.floor(sx.detach()), torch.floor(sy.detach())
    ww, nn = sx - x0, sy - y0
    iw = 0.0
    for dy, wy in ((0, 1 - nn), (1, nn)):
        for dx, wx in ((0, 1 - ww), (1, ww)):
            xi, yi = x0 + dx, y0 + dy
            ok = (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)
            idx = (yi.clamp(0, h - 1) * w + xi.clamp(0, w - 1)).long()
            v = torch.gather(ot4.reshape(n, c, h * w), 2, idx.reshape(n, 1, -1).expand(n, c, -1)).reshape(n, c, h, w)
            iw = iw + (wy * wx * ok)[:, None] * v
    us = torch.from_numpy(np.asarray(usable))[:, None]
    # the VALUES are the oracle's warped tensor (the float32 sample), the derivative is the expression's
    val = torch.from_numpy(warped(f, None, np.asarray(other), ref)[0]).double()
    wp = torch.where(us, val + (iw - iw.detach()), torch.zeros((), dtype=torch.float64))
    wp.retain_grad()
    out, prob = textbook_expression(u, ft4, wp, sign, radius)
    res = {'out': out.detach().numpy(), 'prob': prob.detach().numpy(), 'warped': wp.detach().numpy()}
    if g is not None:
        out.backward(torch.from_numpy(np.asarray(g, F32).astype(F64)))
        res.update({'d_feat': ft.grad.numpy(), 'd_warped': torch.where(us, wp.grad, torch.zeros((), dtype=torch.float64)).numpy(),
                    'd_other': ot.grad.numpy(), 'd_flow': u.grad.numpy()})
    return res


# ---- the bindings' stand-ins of the host tier -----------------------------------------------------------------------------------------
def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _ref_of(flow_sign):
    return 's' if flow_sign < 0 else 't'


def fake_flow_local_match(vecs, mask, feat, other, flow_sign=-1.0, radius=RADIUS, want_prob=False, want_stats=False):
    r = compute(_np(vecs), _np(mask), _np(feat), _np(other), _ref_of(flow_sign), radius)
    n, _, h, w = r['out'].shape
    return (torch.from_numpy(r['out32']), torch.from_numpy(r['prob']) if want_prob else None,
            torch.zeros(28 * n * h * w, dtype=torch.uint8) if want_stats else None)


def fake_flow_local_match_grad(vecs, mask, feat, other, flow_sign, radius, stats, grad_out, want_feat=True, want_warped=True):
    assert stats.dtype == torch.uint8 and stats.numel() == 28 * grad_out.numel() // 2
    r = grads(_np(vecs), _np(mask), _np(feat), _np(other), _ref_of(flow_sign), radius, _np(grad_out))
    return (torch.from_numpy(r['d_feat']) if want_feat else None, torch.from_numpy(r['d_w']) if want_warped else None)
