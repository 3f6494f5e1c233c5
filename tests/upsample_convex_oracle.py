"""The definition of Flow.upsample_convex in NumPy, vectorised over the pixels (a helper module, not a test; test
modules import it), the inputs the CPU and the GPU tier share, and RAFT's own expression in torch.

For the fine pixel (k y + i, k x + j), with the logits l_t = logits[n, t k^2 + i k + j, y, x], t = 3 (dy + 1) + (dx + 1):

    m        = the maximum of the nine logits by a running float32 compare: m = l_0; m = (l_t > m) ? l_t : m
    e_t      = exp(float64(l_t) - float64(m));  s = (((e_0 + e_1) + ...) + e_8);  w_t = e_t / s                    (float64)
    F_{c,t}  = k * float64(f_c(y + dy, x + dx)), exact; +0 where the neighbour lies outside the coarse frame (RAFT's zero padding)
    o_c      = sum_t w_t * F_{c,t} from +0, t ascending, product then sum;  out[n, c, k y + i, k x + j] = float32(o_c)
    d l_t    = float32( w_t * ((G_0 F_{0,t} + G_1 F_{1,t}) - (G_0 o_0 + G_1 o_1)) ),  G_c = float64(g_c) at the fine pixel
    d f_c(q) = float32( k * sum_t sum_i sum_j w_t(i, j; q - delta_t) * G_c(q - delta_t; i, j) ), one float64 sum from +0 in that order,
               over the taps whose coarse pixel q - delta_t lies in the frame

The mask does not enter the arithmetic: the result's mask is the coarse pixel's bit over its k x k block.  `raft_reference` is the
expression people mean, RAFT's upsample_flow: softmax(view(N,1,9,k,k,H,W), 2), unfold(k flow, 3, padding=1), sum,
permute(0,1,4,2,5,3), in torch float64, and its autograd.
"""
import functools
import os
import re

import numpy as np
import torch

F32, F64 = np.float32, np.float64
FACTORS = (2, 4, 8)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the kernel's geometry and the frames it gives the GPU tier ----------------------------------------------------------------------
def geometry():
    """{kTileW, kTileH} of ofl_upsample.hip: a block owns kTileW coarse pixels along x and kTileH FINE rows"""
    with open(os.path.join(ROOT, 'oflibpytorch_amd', 'csrc', 'ofl_upsample.hip')) as fh:
        text = fh.read()
    out = {}
    for name in ("kTileW", "kTileH"):
        m = re.search(r"constexpr int [^;\n]*\b%s = (\d+)[,;]" % name, text)
        assert m, name
        out[name] = int(m.group(1))
    return out


def frames():
    """(n, h, w), coarse, of the GPU tier: the kernel's tile minus one, itself, plus one, and two tiles plus one in both axes (kTileH fine
    rows are kTileH / k coarse rows: every one of these heights ends a block early at some k); 1 x 1, 1 x 5 and 5 x 1, where every or
    most taps are outside; a batch of 3"""
    g = geometry()
    tw, th = g["kTileW"], g["kTileH"]
    return [(1, th - 1, tw - 1), (1, th, tw), (1, th + 1, tw + 1), (1, 2 * th + 1, 2 * tw + 1), (1, 1, 1), (1, 1, 5), (1, 5, 1), (3, 5, 7)]


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(n, h, w):
    """(f float32 [n,2,h,w], mask bool [n,h,w]), read-only and computed once: the vectors are multiples of 2^-6 with |f| < 32, so the
    fp16-stored flow holds the same values; a fifth of the pixels are masked"""
    rng = np.random.RandomState(9001 + 1000 * n + 10 * h + w)
    f = (rng.randint(-32 * 64 + 1, 32 * 64, (n, 2, h, w)) / 64.0).astype(F32)
    mask = rng.uniform(size=(n, h, w)) >= 0.2
    assert np.abs(f).max() < 32 and np.array_equal(f.astype(np.float16).astype(F32), f)
    f.setflags(write=False)
    mask.setflags(write=False)
    return f, mask


@functools.lru_cache(maxsize=None)
def logits_general(n, k, h, w):
    """N(0, 4) rounded to multiples of 2^-6, float32 [n, 9 k^2, h, w]"""
    rng = np.random.RandomState(77 + 1000 * n + 100 * k + 10 * h + w)
    lg = (np.round(rng.normal(0.0, 2.0, (n, 9 * k * k, h, w)) * 64) / 64).astype(F32)
    lg.setflags(write=False)
    return lg


def _grids(n, k, h, w):
    t, i, j, y, x = np.meshgrid(np.arange(9), np.arange(k), np.arange(k), np.arange(h), np.arange(w), indexing='ij')
    return t, i, j, y, x


@functools.lru_cache(maxsize=None)
def logits_exact(kind, n, k, h, w):
    """Logits whose softmax is exact under any correct exp (exp(0) = 1, exp(-1000) = +0):
    'constant'  the nine logits of a fine pixel are equal: 0, 3.5 or -87, in different pixels -- every weight is 1 / 9
    'one-hot'   0 at one tap and -1000 at the others: tap t of fine pixel (i, j) of coarse pixel (y, x) is hot where
                (t + 3 i + 5 j + y + 2 x) mod 9 == 0 -- the output is k times ONE named neighbour
    'two-hot'   0 at that tap and at the next one (mod 9), -1000 at the others: two weights of exactly 1 / 2"""
    t, i, j, y, x = _grids(n, k, h, w)
    hot = (-(3 * i + 5 * j + y + 2 * x)) % 9
    if kind == 'constant':
        lg = np.choose((i + 2 * j + y + x) % 3, [0.0, 3.5, -87.0])
    elif kind == 'one-hot':
        lg = np.where(t == hot, 0.0, -1000.0)
    elif kind == 'two-hot':
        lg = np.where((t == hot) | (t == (hot + 1) % 9), 0.0, -1000.0)
    else:
        raise ValueError(kind)
    lg = np.broadcast_to(lg.reshape(1, 9 * k * k, h, w), (n, 9 * k * k, h, w)).astype(F32).copy()
    if n > 1:                                               # the images differ: image b is rolled by b taps
        for b in range(1, n):
            lg[b] = np.roll(lg[b].reshape(9, k * k, h, w), b, axis=0).reshape(9 * k * k, h, w)
    lg.setflags(write=False)
    return lg


def hot_tap(n, k, h, w):
    """[n, k, k, h, w]: the hot tap of logits_exact('one-hot', ...)"""
    _, i, j, y, x = (a[0] for a in _grids(n, k, h, w))
    hot = (-(3 * i + 5 * j + y + 2 * x)) % 9
    return np.stack([(hot + b) % 9 for b in range(n)])


@functools.lru_cache(maxsize=None)
def upstream(n, k, h, w):
    """The upstream gradient, float32 [n, 2, k h, k w], uniform in [-1, 1)"""
    g = (np.random.RandomState(433 + 1000 * n + 100 * k + 10 * h + w).uniform(size=(n, 2, k * h, k * w)) * 2.0 - 1.0).astype(F32)
    g.setflags(write=False)
    return g


# ---- the definition -------------------------------------------------------------------------------------------------------------------
def factor_of(channels):
    for k in FACTORS:
        if channels == 9 * k * k:
            return k
    raise ValueError("%d channels are not 9 k^2 with k in (2, 4, 8)" % channels)


def weights(logits, k):
    """(w float64 [n, 9, k, k, h, w], m, s): the softmax over the nine taps, in the order of the definition"""
    n, _, h, w = logits.shape
    lg = np.asarray(logits, F32).reshape(n, 9, k, k, h, w)
    with np.errstate(all='ignore'):
        m = lg[:, 0].copy()
        for t in range(1, 9):
            m = np.where(lg[:, t] > m, lg[:, t], m)
        e = np.exp(lg.astype(F64) - m.astype(F64)[:, None])
        s = e[:, 0] + e[:, 1]
        for t in range(2, 9):
            s = s + e[:, t]
        return e / s[:, None], m, s


def neighbours(f, k):
    """F float64 [n, 2, 9, h, w]: k times the 3 x 3 neighbourhood, +0 outside the frame"""
    f = np.asarray(f)
    n, _, h, w = f.shape
    pad = np.zeros((n, 2, h + 2, w + 2), F64)
    pad[:, :, 1:-1, 1:-1] = f.astype(F32).astype(F64)
    return np.stack([F64(k) * pad[:, :, 1 + t // 3 - 1:1 + t // 3 - 1 + h, 1 + t % 3 - 1:1 + t % 3 - 1 + w] for t in range(9)], 2)


def _fine(x, k):
    """[n, c, k, k, h, w] (i, j, y, x) -> [n, c, k h, k w]"""
    n, c, _, _, h, w = x.shape
    return np.ascontiguousarray(x.transpose(0, 1, 4, 2, 5, 3)).reshape(n, c, k * h, k * w)


def _blocks(x, k):
    """[n, c, k h, k w] -> [n, c, k, k, h, w]"""
    n, c, fh, fw = x.shape
    return x.reshape(n, c, fh // k, k, fw // k, k).transpose(0, 1, 3, 5, 2, 4)


def compute(f, logits, k, float64=False, swap_ij=False, dx_outer=False, over_k2=False):
    """{'out': float32 [n, 2, k h, k w] (float64 with float64=True: before the last rounding), 'mag': A = sum_t w_t |F_{c,t}|}.  The three
    flags are the MUTANTS the host tier must tell apart: a swapped i / j, a tap order with dx outermost, weights normalised over k^2"""
    wt, _, _ = weights(logits, k)
    if over_k2:
        n, _, h, w = logits.shape
        lg = np.asarray(logits, F64).reshape(n, 9, k * k, h, w)
        e = np.exp(lg - lg.max(2, keepdims=True))
        wt = (e / e.sum(2, keepdims=True)).reshape(n, 9, k, k, h, w)
    if swap_ij:
        wt = wt.transpose(0, 1, 3, 2, 4, 5)
    F = neighbours(f, k)
    if dx_outer:
        F = F[:, :, [3 * (t % 3) + t // 3 for t in range(9)]]
    with np.errstate(all='ignore'):
        o = np.zeros((F.shape[0], 2) + wt.shape[2:], F64)
        mag = np.zeros_like(o)
        for t in range(9):
            o = o + wt[:, None, t] * F[:, :, t, None, None]
            mag = mag + np.abs(wt[:, None, t]) * np.abs(F[:, :, t, None, None])
        out = _fine(o, k)
        return {'out': out if float64 else out.astype(F32), 'mag': _fine(mag, k)}


def mask_of(mask, k):
    """The coarse pixel's bit over its k x k block"""
    return None if mask is None else np.repeat(np.repeat(np.asarray(mask, bool), k, axis=1), k, axis=2)


def grads(f, logits, k, g, float64=False):
    """{'d_logits': float32 [n, 9 k^2, h, w], 'd_flow': float32 [n, 2, h, w], 'mag_logits', 'mag_flow': the sums of the absolute terms}"""
    n, _, h, w = logits.shape
    wt, _, _ = weights(logits, k)
    F = neighbours(f, k)
    G = _blocks(np.asarray(g, F32).astype(F64), k)                                            # [n, 2, k, k, h, w]
    with np.errstate(all='ignore'):
        o = np.zeros((n, 2, k, k, h, w), F64)
        for t in range(9):
            o = o + wt[:, None, t] * F[:, :, t, None, None]
        go = G[:, 0] * o[:, 0] + G[:, 1] * o[:, 1]
        ago = np.abs(G[:, 0] * o[:, 0]) + np.abs(G[:, 1] * o[:, 1])
        dl = np.empty((n, 9, k, k, h, w), F64)
        mag_l = np.empty_like(dl)
        for t in range(9):
            gf = G[:, 0] * F[:, 0, t, None, None] + G[:, 1] * F[:, 1, t, None, None]
            dl[:, t] = wt[:, t] * (gf - go)
            mag_l[:, t] = np.abs(wt[:, t]) * (np.abs(G[:, 0] * F[:, 0, t, None, None]) + np.abs(G[:, 1] * F[:, 1, t, None, None]) + ago)
        acc = np.zeros((n, 2, h, w), F64)
        mag_f = np.zeros_like(acc)
        for t in range(9):
            dy, dx = t // 3 - 1, t % 3 - 1
            y0, y1, x0, x1 = max(0, -dy), min(h, h - dy), max(0, -dx), min(w, w - dx)         # the pixels p with p + delta_t in the frame
            if y0 >= y1 or x0 >= x1:
                continue
            for i in range(k):
                for j in range(k):
                    term = wt[:, None, t, i, j, y0:y1, x0:x1] * G[:, :, i, j, y0:y1, x0:x1]
                    acc[:, :, y0 + dy:y1 + dy, x0 + dx:x1 + dx] = acc[:, :, y0 + dy:y1 + dy, x0 + dx:x1 + dx] + term
                    mag_f[:, :, y0 + dy:y1 + dy, x0 + dx:x1 + dx] += np.abs(term)
        df = F64(k) * acc
        dl = dl.reshape(n, 9 * k * k, h, w)
        return {'d_logits': dl if float64 else dl.astype(F32), 'd_flow': df if float64 else df.astype(F32),
                'mag_logits': mag_l.reshape(n, 9 * k * k, h, w), 'mag_flow': F64(k) * mag_f}


# ---- RAFT's own expression ------------------------------------------------------------------------------------------------------------
def raft_expression(flow, logits, k):
    """RAFT's upsample_flow on torch tensors of any floating dtype"""
    n, _, h, w = flow.shape
    mask = torch.softmax(logits.view(n, 1, 9, k, k, h, w), dim=2)
    up = torch.nn.functional.unfold(k * flow, [3, 3], padding=1).view(n, 2, 9, 1, 1, h, w)
    return torch.sum(mask * up, dim=2).permute(0, 1, 4, 2, 5, 3).reshape(n, 2, k * h, k * w)


def raft_reference(f, logits, k, g=None):
    """{'out', and with g: 'd_logits', 'd_flow'} in float64"""
    ft = torch.from_numpy(np.asarray(f, F32).astype(F64)).requires_grad_(g is not None)
    lt = torch.from_numpy(np.asarray(logits, F32).astype(F64)).requires_grad_(g is not None)
    out = raft_expression(ft, lt, k)
    res = {'out': out.detach().numpy()}
    if g is not None:
        out.backward(torch.from_numpy(np.asarray(g, F32).astype(F64)))
        res['d_logits'], res['d_flow'] = lt.grad.numpy(), ft.grad.numpy()
    return res


# ---- the bindings' stand-ins of the host tier -----------------------------------------------------------------------------------------
def fake_flow_upsample_convex(vecs, mask, logits, factor):
    out = torch.from_numpy(compute(vecs.detach().float().cpu().numpy(), logits.detach().cpu().numpy(), int(factor))['out'])
    om = None if mask is None else torch.from_numpy(mask_of(mask.cpu().numpy(), int(factor)))
    return out, om


def fake_flow_upsample_convex_grad(vecs, logits, factor, grad_out, want_logits=True, want_vecs=True):
    r = grads(vecs.detach().float().cpu().numpy(), logits.detach().cpu().numpy(), int(factor), grad_out.detach().cpu().numpy())
    return (torch.from_numpy(r['d_logits']) if want_logits else None, torch.from_numpy(r['d_flow']) if want_vecs else None)


def ulp32(x):
    """The spacing of float32 at |x| (float64 array), that of the smallest normal below it"""
    a = np.maximum(np.abs(np.asarray(x, F64)), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(a)) - 23)
