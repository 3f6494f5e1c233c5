"""The definition of Flow.cost_volume in NumPy (a helper module, not a test; test modules import it), the inputs the CPU
and the GPU tier share, and the float64 reference of the whole backward pass.

The sample W = `other` where the flow points and the weight test mr > 0.99999 come from `oracle_backend.warp_bwd(..., want_valid=True)`
(the C oracle of the backward warp, which the reference pins).  W' is W where the pixel is usable (valid in the mask and the sample
inside the frame) and +0 elsewhere and outside the frame: selected, not multiplied.  Everything after it is np.float32 arithmetic, one
rounding per operation, in loops over the offsets o = (dy + r) (2 r + 1) + dx + r and the channels c in ascending order:

    V[o](p)          = (sum_c feat_c(p) * W'_c(p + o)) / float(C)                        from +0, each product rounded, then each sum
    gs               = g / float(C)
    d feat_c(p)      = sum_o gs[o](p) * W'_c(p + o)                                      from +0, o ascending
    d W_c(q)         = usable(q) ? sum_o gs[o](q - o) * feat_c(q - o) : +0               from +0, o ascending, q - o in the frame only

With `float64=True` the same steps run in float64 on the same float32 inputs and W'.  d other and d flow are the backward of the warp
applied to d W: `chain` evaluates them in float64 with `grad_oracle64.warp_grad`; `torch_reference` is the whole definition written out
as one differentiable float64 torch expression, whose autograd is the reference of both tiers.
"""
import functools

import numpy as np
import torch

import frame_sweep as fs
import grad_oracle64 as go
import oracle_backend as ob
import photometric_oracle as po

F32, F64 = np.float32, np.float64
RADII = (1, 2, 3, 4)
RADIUS = 4
REFS = po.REFS
sign_of = po.sign_of


def offsets(radius):
    return [(dy, dx) for dy in range(-radius, radius + 1) for dx in range(-radius, radius + 1)]


# ---- the kernel's geometry and the frames and channel counts it gives the GPU tier --------------------------------------------------
def geometry():
    """{kTileW, kTileH, kChanChunk} of ofl_cost_volume.hip"""
    text = fs._source("ofl_cost_volume.hip")
    return {k: fs._constant(text, k) for k in ("kTileW", "kTileH", "kChanChunk")}


def frames():
    """(n, h, w) of the GPU tier: 20 x 28; the kernel's tile minus one, itself, plus one and two tiles plus one in both axes, so that a
    window crosses every tile edge and the frame edge; a frame smaller than the largest window; a batch of 3 on two tiles"""
    g = geometry()
    tw, th = g["kTileW"], g["kTileH"]
    return [(2, 20, 28), (1, th - 1, tw - 1), (1, th, tw), (1, th + 1, tw + 1), (1, 2 * th + 1, 2 * tw + 1), (1, 3, 3), (3, th, 2 * tw)]


def channel_counts():
    """One channel, one fewer than a chunk, a chunk, one more, two chunks and three"""
    k = geometry()["kChanChunk"]
    return [1, k - 1, k, k + 1, 2 * k + 3]


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def features(n, c, h, w, ref):
    """(feat, other) float32 [n,c,h,w], uniform in [-1, 1) from a seeded generator, read-only and computed once"""
    rng = np.random.RandomState(9151 + 1000 * n + 100 * c + 10 * h + w + (0 if ref == 's' else 7))
    feat = (rng.uniform(size=(n, c, h, w)) * 2.0 - 1.0).astype(F32)
    other = (rng.uniform(size=(n, c, h, w)) * 2.0 - 1.0).astype(F32)
    for arr in (feat, other):
        assert arr.min() >= -1 and arr.max() < 1
        arr.setflags(write=False)
    return feat, other


@functools.lru_cache(maxsize=None)
def upstream(n, d, h, w):
    """The upstream gradient of the volume, float32 [n,d,h,w], uniform in [-1, 1)"""
    g = (np.random.RandomState(733 + 1000 * n + 100 * d + 10 * h + w).uniform(size=(n, d, h, w)) * 2.0 - 1.0).astype(F32)
    g.setflags(write=False)
    return g


def case(n, h, w, ref):
    """(a float32 [n,2,h,w], a_mask bool [n,h,w]) of `photometric_oracle.case`"""
    return po.case(n, h, w, ref)[:2]


# ---- the definition -------------------------------------------------------------------------------------------------------------------
def _as_feat(x, n):
    """float32 [n, C, H, W]; C-H-W broadcasts over the batch"""
    x = np.asarray(x)
    assert x.dtype == F32 and x.ndim in (3, 4) and x.shape[-3] >= 1
    if x.ndim == 3:
        x = x[None]
    assert x.shape[0] in (1, n)
    return np.ascontiguousarray(np.broadcast_to(x, (n,) + x.shape[1:]))


def _shifted(x, r, dy, dx):
    """x(p + (dy, dx)), the fill value 0 / False outside the frame: x [..., h, w]"""
    h, w = x.shape[-2:]
    pad = np.pad(x, [(0, 0)] * (x.ndim - 2) + [(r, r), (r, r)])
    return pad[..., r + dy:r + dy + h, r + dx:r + dx + w]


def warped(a, mask, other, ref):
    """(W' float32 [N,C,H,W], usable bool [N,H,W], inside bool [N,H,W])"""
    f = po._as_f32(a)
    n = f.shape[0]
    ot = _as_feat(other, n)
    assert ot.shape[2:] == f.shape[2:]
    out, valid, _, _ = ob.warp_bwd(torch.from_numpy(f.copy()), torch.from_numpy(ot.copy()), flow_sign=sign_of(ref), want_valid=True)
    inside = valid.numpy().astype(bool)
    usable = inside if mask is None else inside & np.asarray(mask, bool)
    wp = np.where(usable[:, None], out.numpy(), F32(0.0)).astype(F32)                         # selected, not multiplied
    return wp, usable, inside


def compute(a, mask, feat, other, ref, radius=RADIUS, float64=False):
    """dict: 'volume' [N,D,H,W] (float32, or float64 with `float64`); 'abs' float64 [N,D,H,W], (sum_c |feat * W'|) / C; 'warped'
    float32 [N,C,H,W], W'; 'usable', 'inside' bool [N,H,W]"""
    assert radius in RADII
    T = F64 if float64 else F32
    wp, usable, inside = warped(a, mask, other, ref)
    n, chan, h, w = wp.shape
    ft = _as_feat(feat, n)
    assert ft.shape == wp.shape
    offs = offsets(radius)
    vol, mag = np.zeros((n, len(offs), h, w), T), np.zeros((n, len(offs), h, w), F64)
    with np.errstate(all='ignore'):
        for o, (dy, dx) in enumerate(offs):
            acc = np.zeros((n, h, w), T)
            sh = _shifted(wp, radius, dy, dx)
            for c in range(chan):                                                             # channels ascending: product, then sum
                prod = ft[:, c].astype(T) * sh[:, c].astype(T)
                acc = acc + prod
                mag[:, o] += np.abs(ft[:, c].astype(F64) * sh[:, c].astype(F64))
            vol[:, o] = acc / T(chan)
            assert acc.dtype == T
    return {'volume': vol, 'abs': mag / chan, 'warped': wp, 'usable': usable, 'inside': inside}


def grads(a, mask, feat, other, ref, radius, g, float64=False, res=None):
    """(d feat [N,C,H,W], d W [N,C,H,W]) in the stated order, float32 (float64 with `float64`); a C-H-W `feat` still gets N images"""
    T = F64 if float64 else F32
    res = compute(a, mask, feat, other, ref, radius) if res is None else res
    wp, usable = res['warped'], res['usable']
    n, chan, h, w = wp.shape
    ft = _as_feat(feat, n)
    g = np.asarray(g)
    offs = offsets(radius)
    assert g.dtype == F32 and g.shape == (n, len(offs), h, w)
    frame = np.ones((h, w), bool)
    d_feat, d_w = np.zeros((n, chan, h, w), T), np.zeros((n, chan, h, w), T)
    with np.errstate(all='ignore'):
        gs = g.astype(T) / T(chan)
        for c in range(chan):
            acc_f, acc_w = np.zeros((n, h, w), T), np.zeros((n, h, w), T)
            for o, (dy, dx) in enumerate(offs):
                acc_f = acc_f + gs[:, o] * _shifted(wp[:, c], radius, dy, dx).astype(T)
                term = gs[:, o] * ft[:, c].astype(T)                                          # at q - o: where that lies in the frame
                acc_w = np.where(_shifted(frame, radius, -dy, -dx), acc_w + _shifted(term, radius, -dy, -dx), acc_w)
            d_feat[:, c] = acc_f
            d_w[:, c] = np.where(usable, acc_w, T(0.0))
    assert d_feat.dtype == T and d_w.dtype == T
    return d_feat, d_w


def chain(a, other, d_w, ref):
    """(d other [Ns,C,H,W], d flow [N,2,H,W]) float64: the backward of the warp applied to d W (`grad_oracle64.warp_grad`)"""
    f = po._as_f32(a)
    ot = np.asarray(other)
    res = go.warp_grad(f, ot[None] if ot.ndim == 3 else ot, np.asarray(d_w), sign_of(ref), 1.0)
    return res['grad_src'][0], res['grad_flow'][0]


def torch_reference(a, usable, feat, other, ref, radius, g):
    """The definition as one differentiable float64 torch expression (explicit bilinear sample at the float32 positions' float64
    values, `usable` piecewise constant and given, shifted slices, channel mean) and its autograd for the upstream gradient `g`:
    dict of float64 arrays 'volume', 'warped' (W'), 'd_feat', 'd_warped', 'd_other', 'd_flow', each of its operand's own shape"""
    f = po._as_f32(a)
    n, _, h, w = f.shape
    sign = sign_of(ref)
    u = torch.from_numpy(f).double().requires_grad_(True)
    ft = torch.from_numpy(np.asarray(feat).copy()).double().requires_grad_(True)
    ot = torch.from_numpy(np.asarray(other).copy()).double().requires_grad_(True)
    ft4 = (ft[None] if ft.dim() == 3 else ft).expand(n, -1, -1, -1)
    ot4 = (ot[None] if ot.dim() == 3 else ot).expand(n, -1, -1, -1)
    c = ot4.shape[1]
    # the positions carry the float32 values of the kernel (every floor and inside test is its own) and the derivative -sign
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
    wp = torch.where(us, iw, torch.zeros((), dtype=torch.float64))
    wp.retain_grad()
    r = radius
    pad = torch.nn.functional.pad(wp, (r, r, r, r))
    vol = torch.stack([(ft4 * pad[..., r + dy:r + dy + h, r + dx:r + dx + w]).sum(1) / c for dy, dx in offsets(r)], 1)
    (vol * torch.from_numpy(np.asarray(g).copy()).double()).sum().backward()
    # (d W is the gradient of the SAMPLE: what reaches W' where the pixel is not usable goes nowhere)
    return {'volume': vol.detach().numpy(), 'warped': wp.detach().numpy(), 'd_feat': ft.grad.numpy(),
            'd_warped': torch.where(us, wp.grad, torch.zeros((), dtype=torch.float64)).numpy(),
            'd_other': ot.grad.numpy(), 'd_flow': u.grad.numpy()}


# ---- the native calls served by this module (host-logic tests) ----------------------------------------------------------------------
def fake_flow_cost_volume(vecs, mask, feat, other, flow_sign=-1.0, radius=RADIUS):
    res = compute(vecs.detach().numpy(), None if mask is None else mask.numpy(), feat.detach().numpy(), other.detach().numpy(),
                  's' if flow_sign < 0 else 't', radius)
    return torch.from_numpy(res['volume'])


CHAIN_AWAY = F32(2.0 ** 31)


def chain_vectors(a, ref):
    """float32 [N,2,H,W]: the vectors the backward of the warp is run on -- the flow's own, and (sign * 2^31, 0) where a component is
    not finite"""
    f = np.asarray(a).astype(F32)
    bad = ~np.isfinite(f).all(1)
    f[:, 0][bad], f[:, 1][bad] = F32(sign_of(ref)) * CHAIN_AWAY, F32(0.0)
    return f


def usable_of(a, mask, ref):
    """bool [N,H,W]: `usable` of the definition, which no value of `other` enters"""
    f = po._as_f32(a)
    return warped(f, mask, np.zeros((f.shape[0], 1) + f.shape[2:], F32), ref)[1]


def fake_flow_cost_volume_chain(vecs, flow_sign):
    return torch.from_numpy(chain_vectors(vecs.detach().numpy(), 's' if flow_sign < 0 else 't'))


def fake_flow_cost_volume_gate(vecs, mask, flow_sign, grad_flow):
    usable = usable_of(vecs.detach().numpy(), None if mask is None else mask.numpy(), 's' if flow_sign < 0 else 't')
    grad_flow[torch.from_numpy(~np.broadcast_to(usable[:, None], tuple(grad_flow.shape)))] = 0.0
    return grad_flow


def fake_flow_cost_volume_grad(vecs, mask, feat, other, flow_sign, radius, grad_volume, want_feat=True, want_warped=True):
    d_feat, d_w = grads(vecs.detach().numpy(), None if mask is None else mask.numpy(), feat.detach().numpy(), other.detach().numpy(),
                        's' if flow_sign < 0 else 't', radius, grad_volume.detach().numpy())
    return (torch.from_numpy(d_feat) if want_feat else None), (torch.from_numpy(d_w) if want_warped else None)
