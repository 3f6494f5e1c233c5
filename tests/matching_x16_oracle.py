"""What the tests of Flow.from_matching on fp16 / bf16 features share (a helper module, not a test): the float64 evaluation
of the definition on the exact values of the 16-bit inputs -- `matching_oracle.compute(..., wide=True)` on the up-converted arrays --, the
geometry of ofl_matching_x16.hip and the frames and channel counts it gives the GPU tier, the exact families rebuilt on ITS borders, the
derived bars of the general tier, one more mutant, and a stand-in of the new binding for the host tier.

THE BARS (DESIGN.md 4 has the derivation; u = 2^-24).  A computed weight e_q stands for exp(s_q - m) with a relative error of at most
    eta = (C + 2) u max_q sum_c |feat_c(p) other_c(q)| / sqrt(C)      C float32 additions in the MFMA, the constant kInvRoot, the product
        + (2 + 3 d) u                                                 v_exp_f32 (1 ulp), and s - m, kLog2e and their product at |s - m| = d
        + (kLaneQ - 1) u                                              the float32 sum of a lane's kLaneQ weights of a chunk
        + 4 (Q / kChunkQ + 2) 2^-53                                   the float64 sums and rescales across chunks
with d the largest |s - m| of the pixel whose weight is not zero in float32 (at most 104), and a coordinate sum takes
    sigma = kLaneQ u                                                  one float32 product and kLaneQ - 1 float32 additions a chunk
so that  |o~ - o| <= eta A + sigma B,  A = sum_q w_q |q - o|,  B = sum_q w_q |q|  per axis, and the forward is held to
ulp32(want) + eta A + sigma B.  prob = 1 / S: ulp32(want) + 2 eta want (the maximum the sum is taken on moves by a logit's error too).
"""
import functools
import os
import re

import numpy as np
import torch

import matching_oracle as mo

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
DTYPES = {'fp16': torch.float16, 'bf16': torch.bfloat16}
MUTANTS = mo.MUTANTS + ("padded_zero",)


# ---- the kernel's geometry and the frames and channel counts it gives the GPU tier -----------------------------------------------------
@functools.lru_cache(maxsize=None)
def geometry():
    """{kTileP, kSubP, kChunkQ, kLaneQ, kKStep, kRegSteps, kQPad} of ofl_matching_x16.hip: a block owns kTileP pixels as sub-tiles of
    kSubP and walks the other frame kChunkQ positions at a time, kLaneQ of them in one lane; an MFMA takes kKStep channels, the pixels'
    fragments of up to kRegSteps of them stay in registers; the packed rows are padded to a multiple of kQPad"""
    with open(os.path.join(mo.ROOT, 'oflibpytorch_amd', 'csrc', 'ofl_matching_x16.hip')) as fh:
        text = fh.read()
    out = {}
    for name in ("kTileP", "kSubP", "kChunkQ", "kLaneQ", "kKStep", "kRegSteps", "kQPad"):
        m = re.search(r"constexpr int %s = (\d+);" % name, text)
        assert m, name
        out[name] = int(m.group(1))
    return out


def frames():
    """(n, h, w) of the GPU tier, by Q = h w: 1; 1 x 5 and 5 x 1; the pixel tile and the walked chunk, each minus one, exact, plus one and
    twice plus one; a batch of 3 at 5 x 7"""
    g = geometry()
    qs = []
    for t in (g["kTileP"], g["kChunkQ"]):
        qs += [t - 1, t, t + 1, 2 * t + 1]
    out = [(1, 1, 1), (1, 1, 5), (1, 5, 1)] + [(1,) + mo._shape_of(q) for q in sorted(set(qs))] + [(3, 5, 7)]
    assert all(f[1] * f[2] <= 1100 for f in out)
    return out


def channels():
    """C of the GPU tier: 1; the K step of an MFMA and twice it, each minus one, exact and plus one; the most channels whose fragments
    stay in registers, and a count above them (the kernel's other instantiation, more than two K loops)"""
    g = geometry()
    k, top = g["kKStep"], g["kKStep"] * g["kRegSteps"]
    return sorted(set([1, k - 1, k, k + 1, 2 * k - 1, 2 * k, 2 * k + 1, top, top + 2]))


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def to16(a, dtype):
    """(the torch tensor of `dtype`, rounded to nearest even as `Tensor.to` does; its exact values as float32 NumPy)"""
    t = torch.from_numpy(np.ascontiguousarray(a, F32).copy()).to(dtype)
    up = t.float().numpy()
    up.setflags(write=False)
    return t, up


def bf16_changes(a):
    """The elements of a multiple-of-2^-6 array that bfloat16 (8 significant bits) cannot hold: odd multiples at |x| >= 4 (even ones up
    to 8, multiples of 4 up to 16, ...)"""
    k = np.abs(np.round(np.asarray(a, F64) * 64)).astype(np.int64)
    low = k & -k                                                                              # the lowest set bit
    return (k >= 256) & (k // np.maximum(low, 1) >= 256)


@functools.lru_cache(maxsize=None)
def features_general(name, n, c, h, w):
    """(feat, other) as torch tensors of the dtype, and their exact values as float32 NumPy: mo.features_general, N(0, 1) on a grid of
    2^-6, cast.  Every such value below 4 in magnitude is exact in both dtypes; the cast to bfloat16 changes exactly the elements
    `bf16_changes` names (asserted), the cast to float16 none"""
    res = []
    for a in mo.features_general(n, c, h, w):
        t, up = to16(a, DTYPES[name])
        changed = up != a
        assert np.array_equal(changed, bf16_changes(a) if name == 'bf16' else np.zeros(a.shape, bool)), name
        res.append((t, up))
    return res[0][0], res[1][0], res[0][1], res[1][1]


def targets(kind, q, c):
    """mo.targets on the borders of ofl_matching_x16.hip: the first and the last position, both sides of the rows where a chunk passes
    from one half of the lanes to the other (4), of every chunk border and of every tile border"""
    g = geometry()
    k = len(mo.codes(c))
    if kind == 'one-hot':
        cand = [0, q - 1, 3, 4]
        for t in (g["kChunkQ"], g["kSubP"], g["kTileP"]):
            cand += [t - 1, t, 2 * t - 1, 2 * t]
        pos = sorted(set(p for p in cand if 0 <= p < q))
        pos = pos[:k - 2] + pos[-1:] if len(pos) > k - 1 else pos
        return {p: i for i, p in enumerate(pos)}
    if kind == 'two-hot':
        step = g["kChunkQ"] + 4                                                               # the second match: another chunk, the other half
        out = {}
        for i in range(k - 1):
            if i < q:
                out[i] = i
            if i + step < q:
                out[i + step] = i
        return out
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def features_exact(kind, n, c, h, w):
    """mo.features_exact with the targets above: float32 [n,c,h,w] in {0, +-32}, which both 16-bit dtypes hold exactly; every logit is 0
    or at most -1024 ('one-hot', 'two-hot', 'all-equal', 'rising': see there)"""
    q = h * w
    k = len(mo.codes(c))
    fcls = np.zeros((n, q), np.int64)
    ocls = np.zeros((n, q), np.int64)
    if kind in ('one-hot', 'two-hot'):
        tg = targets(kind, q, c)
        t = len(set(tg.values()))
        ocls[:] = k - 1
        for pos, cl in tg.items():
            ocls[:, pos] = cl
        for b in range(n):
            fcls[b] = (np.arange(q) + b) % t
    elif kind == 'rising':
        assert c == 16
        cw = mo.codes(c)
        comp = cw.index(tuple(1 - x for x in cw[0]))
        nb = next(i for i in range(k) if i not in (0, comp))
        ocls[:] = comp
        ocls[:, q // 3] = nb
        ocls[:, (2 * q) // 3] = 0
        for b in range(n):
            fcls[b] = np.where((np.arange(q) + b) % 2 == 0, 0, nb)
    elif kind != 'all-equal':
        raise ValueError(kind)
    feat = np.ascontiguousarray(mo._encode(fcls, c, 'feat').transpose(0, 2, 1)).reshape(n, c, h, w)
    other = np.ascontiguousarray(mo._encode(ocls, c, 'other').transpose(0, 2, 1)).reshape(n, c, h, w)
    feat.setflags(write=False)
    other.setflags(write=False)
    return feat, other


# ---- the float64 evaluation and the bars ------------------------------------------------------------------------------------------------
def _padded_zero(feat, other, flow_sign):
    """The mutant that counts the padded positions of the last chunk with a logit of 0, at the raster positions that follow the frame"""
    _, (n, c, h, w) = mo._flat(feat)
    s = mo.logits(feat, other, True)
    pad = -(h * w) % geometry()["kChunkQ"]
    s = np.concatenate([s, np.zeros((n, h * w, pad), F64)], 2)
    m, S, X, Y = mo.chain(s, w)
    px, py = (np.arange(h * w) % w).astype(F64), (np.arange(h * w) // w).astype(F64)
    return np.stack([(X / S - px) * F64(-flow_sign), (Y / S - py) * F64(-flow_sign)], 1).reshape(n, 2, h, w)


def compute(feat, other, flow_sign, mutant=None, ignore=None):
    """mo.compute(..., wide=True) on the exact values `feat`, `other` (float32 NumPy) of the 16-bit inputs, and the terms of the bars:
    'A', 'B' [n,2,h,w]; 'eta' [n,h,w]; 'bar' = ulp32(out) + eta A + sigma B; 'bar_prob'; 'loose' = eta A + sigma B, the deviation of the
    saved ox, oy.  `ignore`: a position whose logits stand for -inf (a weight of exactly 0) and enter no error term"""
    if mutant == 'padded_zero':
        return {'out': _padded_zero(feat, other, flow_sign)}
    r = mo.compute(feat, other, flow_sign, wide=True, mutant=mutant)
    if mutant is not None:
        return r
    g = geometry()
    f, (n, c, h, w) = mo._flat(feat)
    o, _ = mo._flat(other)
    q = h * w
    qx, qy = (np.arange(q) % w).astype(F64), (np.arange(q) // w).astype(F64)
    wt = r['w']
    with np.errstate(all='ignore'):
        A = np.stack([(wt * np.abs(qx[None, None, :] - r['ox'][:, :, None])).sum(2), (wt * np.abs(qy[None, None, :] - r['oy'][:, :, None])).sum(2)], 1)
        B = np.stack([(wt * qx).sum(2), (wt * qy).sum(2)], 1)
        absdot = np.einsum('ncp,ncq->npq', np.abs(f.astype(F64)), np.abs(o.astype(F64))) / np.sqrt(F64(c))
        absdot = np.where(np.isfinite(r['s']), absdot, 0.0)                                   # (a logit of -inf: a weight of exactly 0, no error)
        depth = r['m'][:, :, None] - r['s']                                                   # |s - m|
        if ignore is not None:                                                                # (a position that stands for such a logit)
            absdot[:, :, ignore] = 0.0
            depth[:, :, ignore] = 0.0
        d = np.where(depth < 104.0, depth, 0.0).max(2)
        eta = (c + 2) * U * absdot.max(2) + (2 + 3 * d) * U + (g["kLaneQ"] - 1) * U + 4 * (q / g["kChunkQ"] + 2) * 2.0 ** -53
        eta = eta / (1 - eta)
        sigma = g["kLaneQ"] * U
        loose = eta[:, None, :] * A + sigma * B
    r.update(A=A.reshape(n, 2, h, w), B=B.reshape(n, 2, h, w), eta=eta.reshape(n, h, w), loose=loose.reshape(n, 2, h, w), absdot=absdot)
    r['bar'] = mo.ulp32(r['out']) + r['loose']
    want_prob = (1.0 / r['S']).reshape(n, h, w)
    r['want_prob'] = want_prob
    r['bar_prob'] = mo.ulp32(want_prob) + 2 * r['eta'] * want_prob
    return r


def ulp16(x, name):
    """The spacing of the 16-bit dtype at |x| (float64 array), that of its smallest normal below it"""
    bits, emin = (10, -14) if name == 'fp16' else (7, -126)
    a = np.maximum(np.abs(np.asarray(x, F64)), 2.0 ** emin)
    return 2.0 ** (np.floor(np.log2(a)) - bits)


def grads(feat, other, flow_sign, g, name, fwd=None):
    """The float64 gradients of the exact 16-bit values (mo.grads(..., wide=True)) and their bars.  The device runs the float32 gradient
    kernels on the statistics of the 16-bit forward and rounds once to the dtype, so a term dss(p, q) = w t / sqrt(C) differs from the
    float64 one by at most
        |dss| (lambda + eta)           lambda(p, q) = (C + 1) u sum_c |feat_c(p) other_c(q)| / sqrt(C): the float32 logit of the gradient
                                       kernel (C - 1 additions of exact products, the root, the division); eta: the saved sum S
        + w T / sqrt(C)                T(p) = |G_x| E_x + |G_y| E_y, E = eta A + sigma B: the deviation of the saved ox, oy
    summed with |other_c(q)| (|feat_c(p)|) over the walk; to that the float32 route's own bar ulp32(want) + 2^-k A (DESIGN.md 4,
    mo.grad_shift) and half an ulp of the dtype at the value are added.  Returns {'d_feat', 'd_other': float64; 'bar_feat', 'bar_other'}"""
    fwd = compute(feat, other, flow_sign) if fwd is None else fwd
    gr = mo.grads(feat, other, flow_sign, g, wide=True)
    f, (n, c, h, w) = mo._flat(feat)
    o, _ = mo._flat(other)
    q = h * w
    root = np.sqrt(F64(c))
    G = np.abs(np.asarray(g, F32).astype(F64).reshape(n, 2, q))
    qx, qy = (np.arange(q) % w).astype(F64), (np.arange(q) // w).astype(F64)
    Gs = F64(-flow_sign) * np.asarray(g, F32).astype(F64).reshape(n, 2, q)
    t = Gs[:, 0, :, None] * (qx[None, None, :] - fwd['ox'][:, :, None]) + Gs[:, 1, :, None] * (qy[None, None, :] - fwd['oy'][:, :, None])
    dss = np.abs(fwd['w'] * t) / root
    loose = fwd['loose'].reshape(n, 2, q)
    T = G[:, 0] * loose[:, 0] + G[:, 1] * loose[:, 1]
    lam = (c + 1) * U * fwd['absdot']
    pair = dss * (lam + fwd['eta'].reshape(n, q)[:, :, None]) + fwd['w'] * (T / root)[:, :, None]
    af, ao = np.abs(f.astype(F64)), np.abs(o.astype(F64))
    extra_feat = np.einsum('npq,ncq->ncp', pair, ao).reshape(n, c, h, w)
    extra_other = np.einsum('npq,ncp->ncq', pair, af).reshape(n, c, h, w)
    res = {'d_feat': gr['d_feat'], 'd_other': gr['d_other']}
    for key, extra, mag in (('feat', extra_feat, gr['mag_feat']), ('other', extra_other, gr['mag_other'])):
        res['bar32_' + key] = mo.ulp32(gr['d_' + key]) + 2.0 ** -mo.grad_shift(q) * mag + extra
    return rounded_to(res, name)


def rounded_to(res, name):
    """The gradients' bars for the dtype `name`: the float32 part, which no dtype enters, plus half an ulp of the dtype at the value"""
    res = dict(res)
    for key in ('feat', 'other'):
        res['bar_' + key] = res['bar32_' + key] + 0.5 * ulp16(np.abs(res['d_' + key]) + res['bar32_' + key], name)
    return res


# ---- the binding's stand-in of the host tier --------------------------------------------------------------------------------------------
def fake_flow_global_match_x16(feat, other, flow_sign=-1.0, want_prob=False, want_stats=False):
    assert feat.dtype == other.dtype and feat.dtype in (torch.float16, torch.bfloat16)
    r = mo.compute(feat.detach().float().cpu().numpy(), other.detach().float().cpu().numpy(), float(flow_sign))
    n, _, h, w = r['out'].shape
    return (torch.from_numpy(r['out32']), torch.from_numpy(r['prob']) if want_prob else None,
            torch.zeros(28 * n * h * w, dtype=torch.uint8) if want_stats else None)
