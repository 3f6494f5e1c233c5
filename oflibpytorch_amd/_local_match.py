"""ctypes binding of the local matching (ofl_local_match.hip; C ABI: include/oflib_hip.h).

A module of its own next to `_native`, whose helpers it uses: it declares the two entry points it calls and allocates its outputs, the
statistics, the workspace of the backward and the gradients under its own module-level name `torch`, which the dirty-memory tests
replace (tests/test_gpu_local_match_dirty_memory.py).  Nothing is read back.
"""
import ctypes

import torch

from ._native import _check, _on, _planes, _ptr, _stream, _vis_flow, _wants_grad, device, load_library

RADIUS = 4                    # the default: GMFlow's 9 x 9 window at 1/4 scale, D = 81
MAX_RADIUS = 4
STATS_BYTES = 28              # of the statistics, per pixel: S, ox, oy float64, m float32

_declared = None


def _library():
    """libofl_hip.so with the two entry points of this module declared."""
    global _declared
    lib = load_library()
    if _declared is not lib:
        p, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float
        ops = [p, i64, i32, p, i64, p, i64, p, i64, i32, f32, i32]
        lib.ofl_flow_local_match_f32.argtypes = ops + [p, p, p, i32, i32, i32, p]
        lib.ofl_flow_local_match_f32.restype = ctypes.c_int
        lib.ofl_flow_local_match_grad_f32.argtypes = ops + [p, p, p, p, p, i32, i32, i32, p]
        lib.ofl_flow_local_match_grad_f32.restype = ctypes.c_int
        _declared = lib
    return lib


def check_operands(vecs, feat, other, radius):
    """The checks every route shares: float32 feature tensors, C-H-W or N-C-H-W, the same C >= 1, the flow's H-W (at least 2 x 2) and
    batch; an integer radius 1 .. 4."""
    for t in (feat, other):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise TypeError("oflibpytorch_amd: the two feature tensors need to be float32 tensors")
        if t.dim() not in (3, 4):
            raise ValueError("oflibpytorch_amd: the two feature tensors need to be C-H-W or N-C-H-W")
        if tuple(t.shape[-2:]) != tuple(vecs.shape[-2:]) or (t.dim() == 4 and t.shape[0] != vecs.shape[0]):
            raise ValueError("oflibpytorch_amd: the two feature tensors need the flow's shape")
    if feat.shape[-3] != other.shape[-3] or feat.shape[-3] < 1:
        raise ValueError("oflibpytorch_amd: the two feature tensors need the same number of channels, at least 1")
    if vecs.shape[-2] < 2 or vecs.shape[-1] < 2:
        raise ValueError("oflibpytorch_amd: the flow needs to be at least 2 pixels high and wide")
    if isinstance(radius, bool) or not isinstance(radius, int):
        raise TypeError("oflibpytorch_amd: the radius needs to be an integer")
    if not 1 <= radius <= MAX_RADIUS:
        raise ValueError("oflibpytorch_amd: the radius needs to be 1, 2, 3 or 4")


def _operands(vecs, mask, feat, other, flow_sign, radius, dev, n):
    """(tensors to keep alive, the arguments both entry points begin with)"""
    v, vbs, half = _vis_flow(vecs.detach(), dev, n)
    m, mbs = (None, 0) if mask is None else _planes(mask, dev, torch.bool, n, "mask")
    ft, ot = feat.detach(), other.detach()
    ft, fbs = _planes(ft[None] if ft.dim() == 3 else ft, dev, torch.float32, n, "features")
    ot, obs = _planes(ot[None] if ot.dim() == 3 else ot, dev, torch.float32, n, "other features")
    return (v, m, ft, ot), (_ptr(v), vbs, half, _ptr(m), mbs, _ptr(ft), fbs, _ptr(ot), obs, int(ft.shape[1]), float(flow_sign),
                            int(radius))


def flow_local_match(vecs: torch.Tensor, mask: torch.Tensor, feat: torch.Tensor, other: torch.Tensor, flow_sign: float = -1.0,
                     radius: int = RADIUS, want_prob: bool = False, want_stats: bool = False):
    """The local matching of a flow (ofl_flow_local_match_f32): vectors [N,2,H,W] fp32 or fp16 as stored, mask [N,H,W]
    bool or None (all True), `feat` the features on the flow's grid and `other` those of the frame it points into, float32 [N,C,H,W] or
    [C,H,W], `flow_sign` -1 for 's' flows and +1 for 't' flows, `radius` 1 .. 4.  Returns (the refined vectors, fp32 [N,2,H,W]; the
    softmax weight of the best position, fp32 [N,H,W], or None; the statistics of every pixel's softmax for the backward, 28 bytes a
    pixel in one uint8 tensor, or None) on the HIP device: one launch; nothing is read back."""
    check_operands(vecs, feat, other, radius)
    lib, dev = _library(), device(vecs, mask, feat, other)
    n, _, h, w = vecs.shape
    with _on(dev):
        keep, args = _operands(vecs, mask, feat, other, flow_sign, radius, dev, n)
        out = torch.empty((n, 2, h, w), dtype=torch.float32, device=dev)
        prob = torch.empty((n, h, w), dtype=torch.float32, device=dev) if want_prob else None
        stats = torch.empty((STATS_BYTES * n * h * w,), dtype=torch.uint8, device=dev) if want_stats else None
        _check(lib.ofl_flow_local_match_f32(*args, _ptr(out), _ptr(prob), _ptr(stats), n, h, w, _stream(dev)), "ofl_flow_local_match_f32")
    del keep
    return out, prob, stats


def flow_local_match_grad(vecs: torch.Tensor, mask: torch.Tensor, feat: torch.Tensor, other: torch.Tensor, flow_sign: float, radius: int,
                          stats: torch.Tensor, grad_out: torch.Tensor, want_feat: bool = True, want_warped: bool = True):
    """The backward of the local matching (ofl_flow_local_match_grad_f32): `stats` as the forward returned it for these operands,
    `grad_out` [N,2,H,W], the upstream gradient.  Returns (the gradient with respect to `feat`, fp32 [N,C,H,W], or None; the gradient
    with respect to the warped tensor W, fp32 [N,C,H,W], or None) on the HIP device -- N images each, whatever the batch of `feat` and
    `other`.  The workspace, (2 radius + 1)^2 float32 per pixel for dss, lives for the call only."""
    if not (want_feat or want_warped):
        raise ValueError("oflibpytorch_amd: flow_local_match_grad needs at least one output")
    check_operands(vecs, feat, other, radius)
    lib, dev = _library(), device(vecs, mask, feat, other, grad_out)
    n, _, h, w = vecs.shape
    if stats.dtype != torch.uint8 or stats.numel() != STATS_BYTES * n * h * w or stats.device != dev or not stats.is_contiguous():
        raise ValueError("oflibpytorch_amd: the statistics need to be those the forward returned for these operands")
    with _on(dev):
        keep, args = _operands(vecs, mask, feat, other, flow_sign, radius, dev, n)
        c = args[9]
        g = grad_out.detach().to(dev, torch.float32).contiguous()
        if tuple(g.shape) != (n, 2, h, w):
            raise ValueError("oflibpytorch_amd: the gradient of the matched flow needs its shape")
        d_feat = torch.empty((n, c, h, w), dtype=torch.float32, device=dev) if want_feat else None
        d_warped = torch.empty((n, c, h, w), dtype=torch.float32, device=dev) if want_warped else None
        scratch = torch.empty((n, (2 * int(radius) + 1) ** 2, h, w), dtype=torch.float32, device=dev)
        _check(lib.ofl_flow_local_match_grad_f32(*args, _ptr(stats), _ptr(g), _ptr(scratch), _ptr(d_feat), _ptr(d_warped), n, h, w,
                                                 _stream(dev)), "ofl_flow_local_match_grad_f32")
        del scratch
    del keep, g
    return d_feat, d_warped


def local_match(vecs: torch.Tensor, mask: torch.Tensor, feat: torch.Tensor, other: torch.Tensor, flow_sign: float = -1.0,
                radius: int = RADIUS, want_prob: bool = False):
    """(the refined vectors, fp32 [N,2,H,W]; the probability, fp32 [N,H,W], or None).  When autograd is recording and the vectors, `feat`
    or `other` require a gradient, the call goes through `_autograd.LocalMatchFn`; the mask and the probability never carry one."""
    if _wants_grad(vecs, feat, other):
        from . import _autograd
        out, prob = _autograd.LocalMatchFn.apply(vecs, mask, feat, other, flow_sign, radius, want_prob)
        return out, prob
    out, prob, _ = flow_local_match(vecs, mask, feat, other, flow_sign, radius, want_prob, False)
    return out, prob
