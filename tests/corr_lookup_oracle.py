"""The definition of Flow.corr_lookup in NumPy, vectorised over the pixels (a helper module, not a test; test modules
import it), the inputs the CPU and the GPU tier share, and the float64 reference people mean.

Per level l, with the float32 steps of the kernel (one rounding per operation; `vis_oracle.fmaf` is an exact fused multiply-add):

    px = float(x) - sign * u, sx = px * 2^-l, x_w = floor(sx), ww = sx - x_w, e = 1 - ww   (y alike: y_n, nn, s)
    nw = s e, ne = s ww, sw = nn e, se = nn ww
    node (j, i), j, i = 0 .. 2 r + 1: column x_w + float(i - r), row y_n + float(j - r); inside by float compares
    K[j,i]      = sum_c feat_c(p) * other_l[c, node]         from +0, c ascending, product then sum; +0 (selected) outside
    entry l D + (dx + r)(2 r + 1) + dy + r = fma(K[dy+r+1, dx+r+1], se, fma(K[dy+r+1, dx+r], sw, fma(K[dy+r, dx+r+1], ne, K[dy+r, dx+r] nw)))
                  / sqrt(float(C));  +0 (selected) where the pixel is not usable (masked, or a vector component not finite)
    gs = g / sqrt(float(C));  Gn[j,i] = from +0: gs[(i-r, j-r)] nw, gs[(i-1-r, j-r)] ne, gs[(i-r, j-1-r)] sw, gs[(i-1-r, j-1-r)] se
    d feat_c(p)     = sum_l sum_j sum_i Gn_l[j,i](p) * other_l[c, node]       one sum from +0, nodes outside skipped, +0 where not usable
    d other_l[c,q]  = sum_j sum_i sum_p Gn_l[j,i](p) * feat_c(p)              p ascending over the usable pixels whose node (j, i) is q

With `float64=True` the same steps run in float64 on the same float32 positions and weights, with sqrt(float64(C)).  `torch_reference`
is the expression people mean: the all-pairs volume einsum(feat, other) / sqrt(C), avg_pool2d(2, 2) over the frame-2 axes,
grid_sample(align_corners=True, zeros padding) at coords / 2^l + delta, in float64, and its autograd.
"""
import functools
import os
import re

import numpy as np
import torch

import photometric_oracle as po
import vis_oracle as vo

F32, F64 = np.float32, np.float64
RADII = (1, 2, 3, 4)
RADIUS, LEVELS, MAX_LEVELS = 4, 4, 6
REFS = po.REFS
sign_of = po.sign_of
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the kernel's geometry and the frames and channel counts it gives the GPU tier --------------------------------------------------
def geometry():
    """{kTileW, kTileH, kChanChunk} of ofl_corr_lookup.hip"""
    with open(os.path.join(ROOT, 'oflibpytorch_amd', 'csrc', 'ofl_corr_lookup.hip')) as fh:
        text = fh.read()
    out = {}
    for name in ("kTileW", "kTileH", "kChanChunk"):
        m = re.search(r"constexpr int [^;\n]*\b%s = (\d+)[,;]" % name, text)
        assert m, name
        out[name] = int(m.group(1))
    return out


def frames():
    """(n, h, w) of the GPU tier: 20 x 28; the kernel's tile minus one, itself, plus one and two tiles plus one in both axes; 3 x 3
    (smaller than every window); a batch of 3 on two tiles"""
    g = geometry()
    tw, th = g["kTileW"], g["kTileH"]
    return [(2, 20, 28), (1, th - 1, tw - 1), (1, th, tw), (1, th + 1, tw + 1), (1, 2 * th + 1, 2 * tw + 1), (1, 3, 3), (3, th, 2 * tw)]


def channel_counts():
    """One channel, one fewer than a chunk of the d other gather, a chunk, one more, two chunks and three"""
    k = geometry()["kChanChunk"]
    return [1, k - 1, k, k + 1, 2 * k + 3]


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(n, h, w, ref):
    """(a float32 [n,2,h,w], a_mask bool [n,h,w]), read-only and computed once.  The vectors are multiples of 2^-6 with |a| < 32: every
    position step is exact in float32 and the fp16-stored flow holds the same values.  They are uniform over +- min(24, 2 max(h, w)),
    so that windows lie inside the level, across each of its edges and outside it; per image pixel (1, 1) has the vector 0 (an integer
    position) and pixel (0, 0) points to the north-west out of the frame (a negative position); a fifth of the pixels are masked."""
    rng = np.random.RandomState(5077 + 1000 * n + 10 * h + w + (0 if ref == 's' else 7))
    reach = min(24, 2 * max(h, w))
    a = (rng.randint(-reach * 64, reach * 64 + 1, (n, 2, h, w)) / 64.0).astype(F32)
    mask = rng.uniform(size=(n, h, w)) >= 0.2
    if h > 1 and w > 1:
        a[:, :, 1, 1] = 0.0
        mask[:, 1, 1] = True
    a[:, :, 0, 0] = -sign_of(ref) * -1.5                    # p + a(p) for 's', p - a(p) for 't': (-1.5, -1.5)
    mask[:, 0, 0] = True
    if h * w >= 4:
        mask[:, h - 1, w - 1] = False
    assert np.abs(a).max() < 32 and np.array_equal(a.astype(np.float16).astype(F32), a)
    a.setflags(write=False)
    mask.setflags(write=False)
    return a, mask


@functools.lru_cache(maxsize=None)
def smooth_case(n, h, w, ref):
    """A smooth flow (a slow affine drift on a grid of 2^-6) with the mask of `case`: neighbouring windows overlap"""
    ys, xs = np.mgrid[0:h, 0:w]
    u = np.round((0.07 * xs - 0.03 * ys + 1.25) * 64) / 64
    v = np.round((0.05 * ys + 0.02 * xs - 2.5) * 64) / 64
    a = np.broadcast_to(np.stack([u, v])[None], (n, 2, h, w)).astype(F32) * F32(-sign_of(ref))
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a, case(n, h, w, ref)[1]


@functools.lru_cache(maxsize=None)
def one_cell_case(n, h, w, ref):
    """Every pixel looks at (w / 2 + 0.25, h / 2 + 0.5) + a fraction of its own: all windows start in one cell.  No mask."""
    ys, xs = np.mgrid[0:h, 0:w]
    tx = w // 2 + 0.25 + (xs % 4) / 8.0
    ty = h // 2 + 0.5 + (ys % 2) / 4.0
    a = np.broadcast_to(np.stack([tx - xs, ty - ys])[None], (n, 2, h, w)).astype(F32) * F32(-sign_of(ref))
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a, None


@functools.lru_cache(maxsize=None)
def features(n, c, h, w, ref, salt=0):
    """float32 [n,c,h,w], uniform in [-1, 1) from a seeded generator, read-only and computed once"""
    rng = np.random.RandomState(6203 + 1000 * n + 100 * c + 10 * h + w + (0 if ref == 's' else 7) + 13 * salt)
    x = (rng.uniform(size=(n, c, h, w)) * 2.0 - 1.0).astype(F32)
    x.setflags(write=False)
    return x


def level_sizes(h, w):
    """The sizes of the explicit level tensors of the GPU tier, l = 0 .. 3: the frame's, half of it, 1 x 1 and (h + 3) x (w - 5)"""
    return [(h, w), (max(h // 2, 1), max(w // 2, 1)), (1, 1), (h + 3, max(w - 5, 1))]


def explicit_levels(n, c, h, w, ref):
    """(feat, [level tensors]) for `level_sizes`"""
    return features(n, c, h, w, ref), [features(n, c, hl, wl, ref, salt=l + 1) for l, (hl, wl) in enumerate(level_sizes(h, w))]


@functools.lru_cache(maxsize=None)
def upstream(n, d, h, w):
    """The upstream gradient of the lookup, float32 [n,d,h,w], uniform in [-1, 1)"""
    g = (np.random.RandomState(811 + 1000 * n + 100 * d + 10 * h + w).uniform(size=(n, d, h, w)) * 2.0 - 1.0).astype(F32)
    g.setflags(write=False)
    return g


def pyramid(other, levels, float64=False):
    """other_0 = other, other_l = avg_pool2d(other_{l-1}, 2, 2), by torch on the CPU, in float32 (what the API does) or float64"""
    t = torch.from_numpy(np.asarray(other).copy())
    t = t.double() if float64 else t
    out = [t]
    for _ in range(levels - 1):
        out.append(torch.nn.functional.avg_pool2d(out[-1], 2, 2))
    return [x.numpy() for x in out]


# ---- the definition -------------------------------------------------------------------------------------------------------------------
def _as_feat(x, n):
    """[n, C, H, W]; C-H-W broadcasts over the batch"""
    x = np.asarray(x)
    assert x.ndim in (3, 4) and x.shape[-3] >= 1
    if x.ndim == 3:
        x = x[None]
    assert x.shape[0] in (1, n)
    return np.ascontiguousarray(np.broadcast_to(x, (n,) + x.shape[1:]))


def window(a, mask, ref, level):
    """The float32 position steps of level `level`: dict of float32 [N,H,W] x_w, y_n, nw, ne, sw, se and bool `usable`"""
    f = po._as_f32(a)
    n, _, h, w = f.shape
    sign = F32(sign_of(ref))
    xs, ys = np.arange(w, dtype=F32)[None, None, :], np.arange(h, dtype=F32)[None, :, None]
    with np.errstate(all='ignore'):
        px, py = xs - sign * f[:, 0], ys - sign * f[:, 1]
        scale = F32(2.0 ** -level)
        sx, sy = px * scale, py * scale
        x_w, y_n = np.floor(sx), np.floor(sy)
        ww, nn = sx - x_w, sy - y_n
        e, s = F32(1) - ww, F32(1) - nn
        res = {'x_w': x_w, 'y_n': y_n, 'nw': s * e, 'ne': s * ww, 'sw': nn * e, 'se': nn * ww, 'ww': ww, 'nn': nn, 'sx': sx, 'sy': sy}
    for v in res.values():
        assert v.dtype == F32
    usable = np.isfinite(f).all(1)
    res['usable'] = usable if mask is None else usable & np.asarray(mask, bool)
    return res


def nodes(win, radius, hl, wl):
    """(inside bool [2r+2, 2r+2, N, H, W], idx int64 of the same shape: the node's offset in a level plane, 0 where it is outside)"""
    k = 2 * radius + 2
    with np.errstate(all='ignore'):
        cx = np.stack([win['x_w'] + F32(i - radius) for i in range(k)])
        cy = np.stack([win['y_n'] + F32(j - radius) for j in range(k)])
        xok = (cx > F32(-1)) & (cx < F32(wl)) & win['usable'][None]
        yok = (cy > F32(-1)) & (cy < F32(hl)) & win['usable'][None]
    ix = np.where(xok, cx, 0).astype(np.int64)
    iy = np.where(yok, cy, 0).astype(np.int64)
    inside = yok[:, None] & xok[None, :]
    idx = np.where(inside, iy[:, None] * wl + ix[None, :], 0)
    return inside, idx


def _values(ot, idx):
    """other_l[c, node] for every channel: ot [N,C,hl,wl], idx [N,H,W] -> [N,C,H,W]"""
    n, c = ot.shape[:2]
    flat = ot.reshape(n, c, -1)
    return np.take_along_axis(flat, np.broadcast_to(idx.reshape(n, 1, -1), (n, c, idx[0].size)), 2).reshape((n, c) + idx.shape[1:])


def _sample(T, k_nw, k_ne, k_sw, k_se, win):
    if T is F32:
        r = k_nw * win['nw']
        r = vo.fmaf(k_ne, win['ne'], r)
        r = vo.fmaf(k_sw, win['sw'], r)
        return vo.fmaf(k_se, win['se'], r)
    return ((k_nw * win['nw'].astype(T) + k_ne * win['ne'].astype(T)) + k_sw * win['sw'].astype(T)) + k_se * win['se'].astype(T)


def offsets(radius):
    """(dx, dy) in the order of the entries: the x offset is the outer index"""
    return [(dx, dy) for dx in range(-radius, radius + 1) for dy in range(-radius, radius + 1)]


def compute(a, mask, feat, levels, ref, radius=RADIUS, float64=False):
    """dict: 'lookup' [N, L D, H, W] (float32, or float64 with `float64`); 'usable' bool [N,H,W]; 'any_inside' bool [L,N,H,W]: a node
    of the pixel's window of that level lies in the level"""
    assert radius in RADII and 1 <= len(levels) <= MAX_LEVELS
    T = F64 if float64 else F32
    f = po._as_f32(a)
    n, _, h, w = f.shape
    ft = _as_feat(feat, n)
    assert ft.shape[2:] == (h, w) and (float64 or ft.dtype == F32)
    chan = ft.shape[1]
    k, d = 2 * radius + 2, (2 * radius + 1) ** 2
    out = np.zeros((n, len(levels) * d, h, w), T)
    any_inside = np.zeros((len(levels), n, h, w), bool)
    root = np.sqrt(T(chan)) if float64 else np.sqrt(F32(chan))
    with np.errstate(all='ignore'):
        for l, lv in enumerate(levels):
            ot = _as_feat(lv, n)
            assert ot.shape[1] == chan and (float64 or ot.dtype == F32)
            hl, wl = ot.shape[2:]
            win = window(f, mask, ref, l)
            inside, idx = nodes(win, radius, hl, wl)
            any_inside[l] = inside.any((0, 1))
            K = np.zeros((k, k, n, h, w), T)
            for j in range(k):
                for i in range(k):
                    vals = _values(ot, idx[j, i])
                    acc = np.zeros((n, h, w), T)
                    for c in range(chan):                                                     # channels ascending: product, then sum
                        prod = ft[:, c].astype(T) * vals[:, c].astype(T)
                        acc = acc + prod
                    K[j, i] = np.where(inside[j, i], acc, T(0.0))                             # selected, not multiplied
            for o, (dx, dy) in enumerate(offsets(radius)):
                j, i = dy + radius, dx + radius
                val = _sample(T, K[j, i], K[j, i + 1], K[j + 1, i], K[j + 1, i + 1], win) / root
                out[:, l * d + o] = np.where(win['usable'], val, T(0.0))
    assert out.dtype == T
    return {'lookup': out, 'usable': window(f, mask, ref, 0)['usable'], 'any_inside': any_inside}


def node_grads(win, gs, radius, T):
    """Gn [2r+2, 2r+2, N, H, W] from gs [N, D, H, W] of one level, in the stated order"""
    k, wn = 2 * radius + 2, 2 * radius + 1
    n, _, h, w = gs.shape
    gn = np.zeros((k, k, n, h, w), T)
    at = lambda dx, dy: gs[:, (dx + radius) * wn + dy + radius]
    nw, ne, sw, se = (win[x].astype(T) for x in ('nw', 'ne', 'sw', 'se'))
    for j in range(k):
        for i in range(k):
            s = np.zeros((n, h, w), T)
            if j <= 2 * radius and i <= 2 * radius:
                s = s + at(i - radius, j - radius) * nw
            if j <= 2 * radius and i >= 1:
                s = s + at(i - 1 - radius, j - radius) * ne
            if j >= 1 and i <= 2 * radius:
                s = s + at(i - radius, j - 1 - radius) * sw
            if j >= 1 and i >= 1:
                s = s + at(i - 1 - radius, j - 1 - radius) * se
            gn[j, i] = s
    return gn


def grads(a, mask, feat, levels, ref, radius, g, float64=False):
    """(d feat [N,C,H,W], [d other_l [N,C,H_l,W_l]]) in the stated order, float32 (float64 with `float64`); a C-H-W operand still gets
    N images"""
    T = F64 if float64 else F32
    f = po._as_f32(a)
    n, _, h, w = f.shape
    ft = _as_feat(feat, n).astype(T)
    chan = ft.shape[1]
    k, d = 2 * radius + 2, (2 * radius + 1) ** 2
    g = np.asarray(g)
    assert g.shape == (n, len(levels) * d, h, w) and (float64 or g.dtype == F32)
    root = np.sqrt(T(chan)) if float64 else np.sqrt(F32(chan))
    d_feat = np.zeros((n, chan, h, w), T)
    d_levels = []
    with np.errstate(all='ignore'):
        for l, lv in enumerate(levels):
            ot = _as_feat(lv, n).astype(T)
            hl, wl = ot.shape[2:]
            win = window(f, mask, ref, l)
            inside, idx = nodes(win, radius, hl, wl)
            gs = g[:, l * d:(l + 1) * d].astype(T) / root
            gn = node_grads(win, gs, radius, T)
            d_ot = np.zeros((n, hl * wl, chan), T)
            for j in range(k):
                for i in range(k):
                    ok = inside[j, i]
                    vals = _values(ot, idx[j, i])
                    d_feat = np.where(ok[:, None], d_feat + gn[j, i][:, None] * vals, d_feat)
                    term = gn[j, i][:, None] * ft                                             # [N,C,H,W], rounded before it is added
                    for b in range(n):
                        sel = ok[b].reshape(-1)                                               # raster order: p ascending
                        np.add.at(d_ot[b], idx[j, i][b].reshape(-1)[sel], term[b].reshape(chan, -1)[:, sel].T)
            d_levels.append(np.ascontiguousarray(d_ot.transpose(0, 2, 1)).reshape(n, chan, hl, wl))
        usable = window(f, mask, ref, 0)['usable']
        d_feat = np.where(usable[:, None], d_feat, T(0.0))
    assert d_feat.dtype == T and all(x.dtype == T for x in d_levels)
    return d_feat, d_levels


# ---- the expression people mean -------------------------------------------------------------------------------------------------------
def torch_reference(a, mask, feat, other, ref, radius, levels=None, g=None):
    """RAFT's CorrBlock in float64: the all-pairs volume einsum(feat, other) / sqrt(C), avg_pool2d(2, 2) over the frame-2 axes (a single
    `other`; a sequence of level tensors gives one volume per level), grid_sample(align_corners=True, zeros padding) at
    coords / 2^l + delta with the x offset first, 0 where the pixel is not usable.  The coordinates are the float64 values of the
    float32 positions.  dict: 'lookup' float64 [N, L D, H, W]; with an upstream gradient `g` also 'd_feat' and 'd_other' (a list for a
    sequence), each of its operand's own shape"""
    f = po._as_f32(a)
    n, _, h, w = f.shape
    win0 = window(f, mask, ref, 0)
    ft = torch.from_numpy(np.asarray(feat).copy()).double().requires_grad_(True)
    ft4 = (ft[None] if ft.dim() == 3 else ft).expand(n, -1, -1, -1)
    c = ft4.shape[1]
    many = isinstance(other, (list, tuple))
    ots = [torch.from_numpy(np.asarray(x).copy()).double().requires_grad_(True) for x in (other if many else [other])]
    as4 = lambda t: (t[None] if t.dim() == 3 else t).expand(n, -1, -1, -1)
    if many:
        vols = [torch.einsum('nchw,ncyx->nhwyx', ft4, as4(t)) / np.sqrt(float(c)) for t in ots]
    else:
        vols = [torch.einsum('nchw,ncyx->nhwyx', ft4, as4(ots[0])) / np.sqrt(float(c))]
        for _ in range(levels - 1):
            v = vols[-1]
            vols.append(torch.nn.functional.avg_pool2d(v.reshape(n * h * w, 1, v.shape[3], v.shape[4]), 2, 2).reshape(
                n, h, w, v.shape[3] // 2, v.shape[4] // 2))
    cx = torch.from_numpy(win0['sx'].astype(F64)).reshape(-1, 1, 1)
    cy = torch.from_numpy(win0['sy'].astype(F64)).reshape(-1, 1, 1)
    cx, cy = torch.nan_to_num(cx, 0.0, 0.0, 0.0), torch.nan_to_num(cy, 0.0, 0.0, 0.0)         # (not usable there: selected out below)
    dd = torch.arange(-radius, radius + 1, dtype=torch.float64)
    d_first, d_second = torch.meshgrid(dd, dd, indexing='ij')                                 # delta[a, b] = (d[a], d[b]) on (x, y)
    us = torch.from_numpy(win0['usable'])[:, None]
    out = []
    for l, v in enumerate(vols):
        hl, wl = v.shape[3], v.shape[4]
        plane = v.reshape(n * h * w, 1, hl, wl)
        plane = torch.nn.functional.pad(plane, (0, 1 if wl == 1 else 0, 0, 1 if hl == 1 else 0))      # (a zero row / column: what zeros padding reads)
        hp, wp = plane.shape[2:]
        x = cx / 2 ** l + d_first[None]
        y = cy / 2 ** l + d_second[None]
        grid = torch.stack([2 * x / (wp - 1) - 1, 2 * y / (hp - 1) - 1], -1)
        s = torch.nn.functional.grid_sample(plane, grid, mode='bilinear', padding_mode='zeros', align_corners=True)
        s = s.reshape(n, h, w, -1).permute(0, 3, 1, 2)
        out.append(torch.where(us, s, torch.zeros((), dtype=torch.float64)))
    look = torch.cat(out, 1)
    res = {'lookup': look.detach().numpy()}
    if g is not None:
        (look * torch.from_numpy(np.asarray(g).copy()).double()).sum().backward()
        res['d_feat'] = ft.grad.numpy()
        grads_o = [t.grad.numpy() for t in ots]
        res['d_other'] = grads_o if many else grads_o[0]
    return res


def categories(a, mask, ref, radius, hl, wl, level=0):
    """dict of bool [N,H,W]: the categories of the pixels of a case on one level"""
    win = window(a, mask, ref, level)
    f = po._as_f32(a)
    k = 2 * radius + 2
    open_win = dict(win, usable=np.isfinite(f).all(1))                                        # (the window whatever the mask says)
    inside, _ = nodes(open_win, radius, hl, wl)
    rows, cols = inside.any(1), inside.any(0)                                                 # [k, N, H, W]: a row / column with a node inside
    hit = inside.any((0, 1))
    return {'inside': inside.all((0, 1)), 'outside': ~hit,
            'north': hit & ~rows[0], 'south': hit & ~rows[k - 1], 'west': hit & ~cols[0], 'east': hit & ~cols[k - 1],
            'masked': ~win['usable'], 'integer': win['usable'] & (win['ww'] == 0) & (win['nn'] == 0),
            'negative': win['usable'] & ((win['sx'] < 0) | (win['sy'] < 0))}


# ---- the native calls served by this module (host-logic tests) ----------------------------------------------------------------------
def fake_flow_corr_lookup(vecs, mask, feat, levels, flow_sign=-1.0, radius=RADIUS):
    res = compute(vecs.detach().numpy(), None if mask is None else mask.numpy(), feat.detach().numpy(), [lv.detach().numpy() for lv in levels],
                  's' if flow_sign < 0 else 't', radius)
    return torch.from_numpy(res['lookup'])


def fake_flow_corr_lookup_grad(vecs, mask, feat, levels, flow_sign, radius, grad_out, want_feat=True, want_levels=None):
    want_levels = [True] * len(levels) if want_levels is None else list(want_levels)
    d_feat, d_levels = grads(vecs.detach().numpy(), None if mask is None else mask.numpy(), feat.detach().numpy(),
                             [lv.detach().numpy() for lv in levels], 's' if flow_sign < 0 else 't', radius, grad_out.detach().numpy())
    return (torch.from_numpy(d_feat) if want_feat else None), [torch.from_numpy(x) if wl else None for x, wl in zip(d_levels, want_levels)]
