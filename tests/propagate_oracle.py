"""The definition of Flow.propagate in NumPy, vectorised over the pixels p with a loop over the steps of a pixel's softmax
(a helper module, not a test; test modules import it), the inputs the CPU and the GPU tier share, and the two textbook expressions in
torch.  Features, upstream gradients and the exact-softmax families are those of matching_oracle.py.

A pixel p has an ordered list of STEPS.  Global form (radius None): every position q in ascending raster order.  Local form: the offsets
(dy, dx), dy outermost, both ascending from -r; the position p + (dy, dx) may lie outside the frame (PADDED).

    s      = (sum_c query_c(p) * key_c(q)) / sqrt_rn(float32(C)): float32, from +0, c ascending, product then sum, one division; padded: +0
    takes part  a padded position always; a position inside the frame unless the mask is given and False at q (EXCLUDED)
    global m float32; S, X, Y float64.  First participating step: m = s, S = X = Y = +0.  Every participating step: if s > m: r = exp(f64(m)
           - f64(s)), S = S r, X = X r, Y = Y r, m = s; then e = exp(f64(s) - f64(m)), S = S + e, X = X + e f64(u(q)), Y = Y + e f64(v(q))
    local  m = the first participating logit, replaced by every later one with s > m; then S, X, Y as above on that FINAL m, no rescale;
           a padded position has u = v = 0 and its products are formed
    result ox = X / S, oy = Y / S, out = float32 of each.  EMPTY pixel (no position inside the frame takes part): out = +0, valid = False,
           m = S = ox = oy = +0
    pair   w = exp(f64(s) - f64(m)) / S; ds = float32(w * ((f64(g_x) * (f64(u(q)) - ox)) + (f64(g_y) * (f64(v(q)) - oy)))); dss = ds /
           root; tx = float32(w * f64(g_x)), ty alike; all three exactly +0 where q is excluded or p is empty; none for a padded position
    d query_c(p) = sum over the steps of p, in order, of dss * key_c(q);  d key_c(q) = sum over p ascending of dss(p, q) * query_c(p);
    d u(q) = sum over p ascending of tx(p, q), d v(q) alike: float32 products and one float32 sum per element from +0
"""
import functools
import os
import re

import numpy as np
import torch

import matching_oracle as mo

F32, F64 = np.float32, np.float64
ROOT = mo.ROOT
MUTANTS = ("over_p", "no_scale", "swap_uv", "pad_excluded", "mask_ignored", "dx_outer")
ulp32 = mo.ulp32
features_general = mo.features_general
upstream = mo.upstream


# ---- the kernels' geometry and the frames and channel counts it gives the GPU tier -----------------------------------------------------
def geometry():
    """The constants of ofl_propagate.hip: the global kernels' pixel tile, position chunk, channel chunk, gradient waves and channels per
    wave; the local kernel's tile width and height and the channels it stages at a time"""
    with open(os.path.join(ROOT, 'oflibpytorch_amd', 'csrc', 'ofl_propagate.hip')) as fh:
        text = fh.read()
    out = {}
    for name in ("kTileP", "kChunkQ", "kChanChunk", "kGradWaves", "kGradChan", "kLTileW", "kLTileH", "kLChan"):
        m = re.search(r"constexpr int [^;\n]*\b%s = (\d+)[,;]" % name, text)
        assert m, name
        out[name] = int(m.group(1))
    return out


def global_frames():
    """(n, h, w) of the global form by Q = h w: 1; 1 x 5, 5 x 1; the chunk, the tile and a gradient block's chunks, each minus one, exact,
    plus one and twice plus one; a batch of 3"""
    g = geometry()
    qs = []
    for t in (g["kChunkQ"], g["kTileP"], g["kGradWaves"] * g["kChunkQ"]):
        qs += [t - 1, t, t + 1, 2 * t + 1]
    out = [(1, 1, 1), (1, 1, 5), (1, 5, 1)] + [(1,) + mo._shape_of(q) for q in sorted(set(qs))] + [(3, 5, 7)]
    assert all(f[1] * f[2] <= 1100 for f in out)
    return out


def local_frames():
    """(n, h, w) of the local form: frames smaller than the window; the tile's width and height, each minus one, exact, plus one and
    twice plus one (the other extent small and odd); a batch of 3"""
    g = geometry()
    out = [(1, 1, 1), (1, 1, 7), (1, 7, 1), (1, 2, 3)]
    for t in (g["kLTileW"] - 1, g["kLTileW"], g["kLTileW"] + 1, 2 * g["kLTileW"] + 1):
        out.append((1, 3, t))
    for t in (g["kLTileH"] - 1, g["kLTileH"], g["kLTileH"] + 1, 2 * g["kLTileH"] + 1):
        out.append((1, t, 5))
    return out + [(3, 5, 7)]


def channels(radius=None):
    """C of the general tier: 1 and around the channel chunk of the form's forward kernel"""
    g = geometry()
    k = g["kChanChunk"] if radius is None else g["kLChan"]
    return sorted(set(c for c in (1, k - 1, k, k + 1, 2 * k + 3) if c >= 1))


def grad_channels():
    """C at which the global gradient kernels take another path (matching_oracle.grad_channels on this source's constants)"""
    g = geometry()
    a, b = g["kGradChan"], g["kGradWaves"] * g["kGradChan"]
    return [a - 1, a, a + 1, b - 1, b, b + 1, 2 * b + 3]


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def vectors(n, h, w):
    """The flow, float32 [n,2,h,w], read-only: multiples of 2^-6 in [-4, 4], so that every float64 sum of the exact families is exact"""
    v = (np.random.RandomState(4241 + 1000 * n + 10 * h + w).randint(-256, 257, size=(n, 2, h, w)) / 64.0).astype(F32)
    v.setflags(write=False)
    return v


def features_exact(kind, n, c, h, w):
    """(query, key) of matching_oracle.features_exact: entries in {0, +-32}, every logit 0 or at most -1024 -- and so is the difference of
    any two: exp gives exactly 1 or +0, and the padded logit +0 TIES with the maximum wherever a window holds a match"""
    return mo.features_exact(kind, n, c, h, w)


def exact_kinds(c):
    return ('one-hot', 'two-hot', 'all-equal') + (('rising',) if c == 16 else ())


def masks(n, h, w, radius=None):
    """{name: bool [n,h,w] or None}: none; single excluded positions at the first and last q and on either side of every chunk and tile
    border; a checkerboard; one image fully masked (all three only where n > 1 or alone); for the local form a masked block wider than
    the window"""
    g = geometry()
    q = h * w
    out = {'none': None}
    cand = [0, q - 1]
    for t in (g["kChunkQ"], g["kTileP"], g["kGradWaves"] * g["kChunkQ"]):
        cand += [t - 1, t, 2 * t - 1, 2 * t]
    if radius is not None:
        for y in (g["kLTileH"] - 1, g["kLTileH"]):
            for x in (g["kLTileW"] - 1, g["kLTileW"]):
                cand.append(y * w + x if y < h and x < w else -1)
    single = np.ones((n, q), bool)
    for i, pos in enumerate(sorted(set(p for p in cand if 0 <= p < q))):
        single[i % n, pos] = False
    out['single'] = single.reshape(n, h, w)
    yy, xx = np.mgrid[0:h, 0:w]
    out['checker'] = np.broadcast_to(((yy + xx) % 2 == 0)[None], (n, h, w)).copy()
    full = out['checker'].copy()
    full[n - 1] = False
    out['one-image-masked'] = full
    if radius is not None:
        blk = np.ones((n, h, w), bool)
        blk[:, :min(h, 2 * radius + 3), :min(w, 2 * radius + 3)] = False
        out['block'] = blk
    return out


# ---- the definition -------------------------------------------------------------------------------------------------------------------
def _flat(a):
    a = np.asarray(a)
    a = a[None] if a.ndim == 3 else a
    n, c, h, w = a.shape
    return a.reshape(n, c, h * w), (n, c, h, w)


def steps(h, w, radius):
    """idx int [P, T]: the position of step t of pixel p, -1 for a padded one.  Global: T = Q, idx[p, t] = t"""
    q = h * w
    if radius is None:
        return np.broadcast_to(np.arange(q)[None], (q, q))
    py, px = np.arange(q) // w, np.arange(q) % w
    cols = []
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            y, x = py + dy, px + dx
            cols.append(np.where((y >= 0) & (y < h) & (x >= 0) & (x < w), y * w + x, -1))
    return np.stack(cols, 1)


def _operands(flow, mask, query, key, n):
    qf, (nq, c, h, w) = _flat(query)
    kf, _ = _flat(key)
    qf = np.broadcast_to(qf, (n, c, h * w)) if nq != n else qf
    kf = np.broadcast_to(kf, (n, c, h * w)) if kf.shape[0] != n else kf
    return qf, kf, (n, c, h, w)


def compute(flow, mask, query, key, radius=None, wide=False, mutant=None):
    """{'out': [n,2,h,w] float64, before the last rounding; 'out32': rounded once; 'valid': bool [n,h,w]; 'm', 'S', 'ox', 'oy': the saved
    statistics [n, h w]; 'mag': A = sum w |value - out| per component [n,2,h,w]; 'terms': participating steps per pixel [n,h,w]; and
    the per-step arrays 's', 'w', 'part', 'inside', 'U', 'V', 'idx' that grads() uses}.  `wide`: float64 logits, the textbook's."""
    flow = np.asarray(flow, F32)
    n = flow.shape[0]
    qf, kf, (_, c, h, w) = _operands(flow, mask, query, key, n)
    q = h * w
    s_all = mo.logits(qf.reshape(n, c, h, w), kf.reshape(n, c, h, w), wide, no_scale=(mutant == 'no_scale'))        # [n, P, Q]
    if mutant == 'over_p':
        s_all = np.ascontiguousarray(s_all.transpose(0, 2, 1))
    T = F64 if wide else F32
    idx = steps(h, w, radius)
    inside = idx >= 0
    safe = np.where(inside, idx, 0)
    s = np.where(inside[None], np.take_along_axis(s_all, np.broadcast_to(safe[None], (n,) + safe.shape), 2), T(0))
    vidx = safe
    if mutant == 'dx_outer' and radius is not None:
        side = 2 * radius + 1
        perm = np.array([(t % side) * side + t // side for t in range(side * side)])
        vidx = safe[:, perm]                                                                 # (the values of the transposed offset)
        vin = inside[:, perm]
    else:
        vin = inside
    uv = flow.reshape(n, 2, q).astype(F64)
    if mutant == 'swap_uv':
        uv = uv[:, ::-1]
    U = np.where(vin[None], uv[:, 0][:, vidx], 0.0)
    V = np.where(vin[None], uv[:, 1][:, vidx], 0.0)
    if mask is None or mutant == 'mask_ignored':
        part = np.broadcast_to(np.ones_like(inside)[None], (n,) + inside.shape).copy()
    else:
        mk = np.broadcast_to(np.asarray(mask, bool).reshape(-1, q), (n, q))
        part = np.where(inside[None], mk[:, safe], True)
    if mutant == 'pad_excluded':
        part = part & inside[None]
    steps_n = idx.shape[1]
    started = np.zeros((n, q), bool)
    m = np.zeros((n, q), T)
    S, X, Y = (np.zeros((n, q), F64) for _ in range(3))
    with np.errstate(all='ignore'):
        if radius is None:
            for t in range(steps_n):
                on = part[:, :, t]
                if not on.any():
                    continue
                st = s[:, :, t]
                m = np.where(on & ~started, st, m)
                started = started | on
                rise = on & (st > m)
                if rise.any():
                    r = np.exp(m.astype(F64) - st.astype(F64))
                    S, X, Y = np.where(rise, S * r, S), np.where(rise, X * r, X), np.where(rise, Y * r, Y)
                    m = np.where(rise, st, m)
                e = np.exp(st.astype(F64) - m.astype(F64))
                S = np.where(on, S + e, S)
                X = np.where(on, X + e * U[:, :, t], X)
                Y = np.where(on, Y + e * V[:, :, t], Y)
        else:
            for t in range(steps_n):
                on, st = part[:, :, t], s[:, :, t]
                m = np.where(on & ~started, st, np.where(on & started & (st > m), st, m))
                started = started | on
            for t in range(steps_n):
                on = part[:, :, t]
                e = np.exp(s[:, :, t].astype(F64) - m.astype(F64))
                S = np.where(on, S + e, S)
                X = np.where(on, X + e * U[:, :, t], X)
                Y = np.where(on, Y + e * V[:, :, t], Y)
        valid = (part & inside[None]).any(2)
        ox, oy = np.where(valid, X / S, 0.0), np.where(valid, Y / S, 0.0)
        m, S = np.where(valid, m, T(0)), np.where(valid, S, 0.0)
        wt = np.where(part & valid[:, :, None], np.exp(s.astype(F64) - m.astype(F64)[:, :, None]) / S[:, :, None], 0.0)
        mag = np.stack([(wt * np.abs(U - ox[:, :, None])).sum(2), (wt * np.abs(V - oy[:, :, None])).sum(2)], 1).reshape(n, 2, h, w)
    out = np.stack([ox, oy], 1).reshape(n, 2, h, w)
    return {'out': out, 'out32': out.astype(F32), 'valid': valid.reshape(n, h, w), 'm': m, 'S': S, 'ox': ox, 'oy': oy, 'mag': mag,
            'terms': part.sum(2).reshape(n, h, w), 's': s, 'w': wt, 'part': part, 'inside': inside, 'U': U, 'V': V, 'idx': idx}


def grads(flow, mask, query, key, radius, g, wide=False):
    """{'d_query', 'd_key' [n,c,h,w], 'd_flow' [n,2,h,w]: the definition's float32 sums (float64 throughout with `wide`); '<name>64': the
    float64 sums of the same float32 terms; 'mag_<name>': the sums of the absolute terms; 'terms_<name>': the number of terms}"""
    flow = np.asarray(flow, F32)
    n = flow.shape[0]
    qf, kf, (_, c, h, w) = _operands(flow, mask, query, key, n)
    q = h * w
    fw = compute(flow, mask, query, key, radius, wide)
    T = F64 if wide else F32
    root = np.sqrt(T(c))
    G = np.asarray(g, F32).astype(F64).reshape(n, 2, q)
    idx, inside, part = fw['idx'], fw['inside'], fw['part']
    safe = np.where(inside, idx, 0)
    live = part & inside[None] & fw['valid'].reshape(n, q)[:, :, None]                       # pairs whose terms are not forced to +0
    with np.errstate(all='ignore'):
        tx_ = G[:, 0, :, None] * (fw['U'] - fw['ox'][:, :, None])
        ty_ = G[:, 1, :, None] * (fw['V'] - fw['oy'][:, :, None])
        t_ = tx_ + ty_
        wt = np.exp(fw['s'].astype(F64) - fw['m'].astype(F64)[:, :, None]) / fw['S'][:, :, None]
        dss = np.where(live, (wt * t_).astype(T) / root, T(0))
        tx = np.where(live, (wt * G[:, 0, :, None]).astype(T), T(0))
        ty = np.where(live, (wt * G[:, 1, :, None]).astype(T), T(0))
        qf, kf = qf.astype(T), kf.astype(T)
        names = ('d_query', 'd_key', 'd_flow')
        acc = {k: np.zeros((n, c if k != 'd_flow' else 2, q), T) for k in names}
        acc64 = {k: np.zeros(acc[k].shape, F64) for k in names}
        mag = {k: np.zeros(acc[k].shape, F64) for k in names}
        cnt = {k: np.zeros(acc[k].shape, np.int64) for k in names}

        def add(name, where, term):
            """one more term of every element of acc[name] selected by `where` [n?, ., q]"""
            acc[name] = np.where(where, acc[name] + term, acc[name])
            acc64[name] = np.where(where, acc64[name] + term.astype(F64), acc64[name])
            mag[name] = np.where(where, mag[name] + np.abs(term.astype(F64)), mag[name])
            cnt[name] = cnt[name] + np.broadcast_to(where, cnt[name].shape)
        for t in range(idx.shape[1]):                                                        # d query: the steps of p in order
            add('d_query', inside[None, None, :, t], dss[:, None, :, t] * kf[:, :, safe[:, t]])
        if radius is None:
            for pix in range(q):                                                             # p ascending, every q at once
                add('d_key', np.ones((1, 1, q), bool), dss[:, None, pix, :] * qf[:, :, pix, None])
                add('d_flow', np.ones((1, 1, q), bool), np.stack([tx[:, pix, :], ty[:, pix, :]], 1))
        else:
            for t in range(idx.shape[1] - 1, -1, -1):                                        # p = q - offset ascending: offsets descending
                ps = np.nonzero(inside[:, t])[0]
                if ps.size == 0:
                    continue
                qs = idx[ps, t]                                                              # (one p per q at a given offset)
                wh = np.zeros((1, 1, q), bool)
                wh[0, 0, qs] = True
                term = np.zeros((n, c, q), T)
                term[:, :, qs] = dss[:, None, ps, t] * qf[:, :, ps]
                add('d_key', wh, term)
                term2 = np.zeros((n, 2, q), T)
                term2[:, 0, qs] = tx[:, ps, t]
                term2[:, 1, qs] = ty[:, ps, t]
                add('d_flow', wh, term2)
    res = {}
    for k in names:
        shape = (n, acc[k].shape[1], h, w)
        res[k], res[k + '64'], res['mag_' + k], res['terms_' + k] = (a.reshape(shape) for a in (acc[k], acc64[k], mag[k], cnt[k]))
    return res


def forward_shift(t):
    """k of the forward's bar ulp32(want) + 2^-k A (the derivation of matching_oracle.forward_shift with values in place of
    coordinates): a term e differs by at most 2^-51 of itself per exp it has passed through, at most T of them in the global chain (the
    local form has one and stays inside); |value - out| enters A directly, so 2 A 2^-51 T with a margin of 16: k = 46 - ceil(log2 T)"""
    return 46 - np.ceil(np.log2(np.maximum(t, 1))).astype(int)


def grad_shift(t):
    """k of a gradient's bar ulp32(want) + 2^-k A against the float64 sum of the definition's float32 terms
    (matching_oracle.grad_shift): k = 20 - ceil(log2(T + 6)), T the number of terms of the element"""
    return 20 - np.ceil(np.log2(t + 6)).astype(int)


# ---- the textbook expressions ---------------------------------------------------------------------------------------------------------
def textbook_expression(flow, mask, query, key, radius):
    """softmax(Q K^T / sqrt(C)) flow over all positions (masked ones at -inf), or GMFlow's local form by unfold with zero padding, on torch
    tensors [n,.,h,w] of any floating dtype.  Pixels with nothing to attend to are not defined here (NaN)."""
    n, c, h, w = query.shape
    if radius is None:
        corr = torch.einsum('ncp,ncq->npq', query.reshape(n, c, h * w), key.reshape(n, c, h * w)) / (c ** 0.5)
        if mask is not None:
            corr = corr.masked_fill(~mask.reshape(n, 1, h * w), float('-inf'))
        out = torch.matmul(torch.softmax(corr, dim=2), flow.reshape(n, 2, h * w).permute(0, 2, 1))
        return out.permute(0, 2, 1).reshape(n, 2, h, w)
    k = 2 * radius + 1
    unf = lambda t: torch.nn.functional.unfold(t, k, padding=radius).reshape(n, t.shape[1], k * k, h * w)
    corr = (query.reshape(n, c, 1, h * w) * unf(key)).sum(1) / (c ** 0.5)                    # [n, D, P]
    if mask is not None:
        # an excluded position inside the frame: -inf; the padding stays at 0 (the mask is padded with True before it is unfolded)
        mk = torch.nn.functional.pad(mask[:, None].to(query.dtype), (radius,) * 4, value=1.0)
        corr = corr.masked_fill(torch.nn.functional.unfold(mk, k).reshape(n, k * k, h * w) == 0, float('-inf'))
    p = torch.softmax(corr, dim=1)
    return (p[:, None] * unf(flow)).sum(2).reshape(n, 2, h, w)


def textbook(flow, mask, query, key, radius, g=None):
    """{'out', and with g: 'd_query', 'd_key', 'd_flow'} in float64"""
    t64 = lambda a: torch.from_numpy(np.asarray(a, F32).astype(F64))
    fl, qt, kt = (t64(a).requires_grad_(g is not None) for a in (flow, query, key))
    mk = None if mask is None else torch.from_numpy(np.asarray(mask, bool))
    out = textbook_expression(fl, mk, qt, kt, radius)
    res = {'out': out.detach().numpy()}
    if g is not None:
        out.backward(t64(g))
        res['d_query'], res['d_key'], res['d_flow'] = qt.grad.numpy(), kt.grad.numpy(), fl.grad.numpy()
    return res


# ---- the bindings' stand-ins of the host tier -----------------------------------------------------------------------------------------
def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _four(a):
    return a[None] if a.ndim == 3 else a


def fake_flow_propagate(vecs, mask, query, key, radius=None, want_stats=False):
    r = compute(_np(vecs), _np(mask), _four(_np(query)), _four(_np(key)), radius)
    n, _, h, w = r['out'].shape
    return (torch.from_numpy(r['out32']), None if mask is None else torch.from_numpy(r['valid'].copy()),
            torch.zeros(28 * n * h * w, dtype=torch.uint8) if want_stats else None)


def fake_flow_propagate_grad(vecs, mask, query, key, radius, stats, grad_out, want_query=True, want_key=True, want_flow=True):
    assert stats.dtype == torch.uint8 and stats.numel() == 28 * grad_out.numel() // 2
    r = grads(_np(vecs), _np(mask), _four(_np(query)), _four(_np(key)), radius, _np(grad_out))
    return (torch.from_numpy(r['d_query']) if want_query else None, torch.from_numpy(r['d_key']) if want_key else None,
            torch.from_numpy(r['d_flow']) if want_flow else None)
