"""ctypes binding of the fused cost volume (ofl_cost_volume.hip; C ABI: include/oflib_hip.h).

A module of its own next to `_native`, whose helpers it uses: it declares the four entry points it calls and allocates its outputs under
its own module-level name `torch`, which the dirty-memory tests replace (tests/test_gpu_cost_volume_dirty_memory.py).
"""
import ctypes

import torch

from ._native import _check, _on, _planes, _ptr, _stream, _vis_flow, _wants_grad, device, load_library

RADIUS = 4                    # the default: PWC-Net's 9 x 9 window, D = 81
MAX_RADIUS = 4

_declared = None


def _library():
    """libofl_hip.so with the four entry points of this module declared."""
    global _declared
    lib = load_library()
    if _declared is not lib:
        p, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float
        lib.ofl_flow_cost_volume_f32.argtypes = [p, i64, i32, p, i64, p, i64, p, i64, i32, f32, i32, p, i32, i32, i32, p]
        lib.ofl_flow_cost_volume_f32.restype = ctypes.c_int
        lib.ofl_flow_cost_volume_grad_f32.argtypes = [p, i64, i32, p, i64, p, i64, p, i64, i32, f32, i32, p, p, p, i32, i32, i32, p]
        lib.ofl_flow_cost_volume_grad_f32.restype = ctypes.c_int
        lib.ofl_flow_cost_volume_chain_f32.argtypes = [p, i64, i32, f32, p, i32, i32, i32, p]
        lib.ofl_flow_cost_volume_chain_f32.restype = ctypes.c_int
        lib.ofl_flow_cost_volume_gate_f32.argtypes = [p, i64, i32, p, i64, f32, p, i32, i32, i32, p]
        lib.ofl_flow_cost_volume_gate_f32.restype = ctypes.c_int
        _declared = lib
    return lib


def _operands(vecs, mask, feat, other, dev, n):
    """(tensors to keep alive, the arguments of both entry points up to `channels`).  `feat`, `other`: float32, C-H-W (broadcast over
    the batch) or N-C-H-W, the same C."""
    v, vbs, half = _vis_flow(vecs, dev, n)
    m, mbs = (None, 0) if mask is None else _planes(mask, dev, torch.bool, n, "mask")
    if feat.dtype != torch.float32 or other.dtype != torch.float32:
        raise TypeError("oflibpytorch_amd: the two feature tensors need to be float32")
    if feat.shape[-3] != other.shape[-3]:
        raise ValueError("oflibpytorch_amd: the two feature tensors need the same number of channels")
    ft, ot = feat.detach(), other.detach()
    ft, fbs = _planes(ft[None] if ft.dim() == 3 else ft, dev, torch.float32, n, "features")
    ot, obs = _planes(ot[None] if ot.dim() == 3 else ot, dev, torch.float32, n, "other features")
    return (v, m, ft, ot), (_ptr(v), vbs, half, _ptr(m), mbs, _ptr(ft), fbs, _ptr(ot), obs, int(ft.shape[1]))


def flow_cost_volume(vecs: torch.Tensor, mask: torch.Tensor, feat: torch.Tensor, other: torch.Tensor, flow_sign: float = -1.0,
                     radius: int = RADIUS) -> torch.Tensor:
    """The cost volume of a flow (ofl_flow_cost_volume_f32): vectors [N,2,H,W] fp32 or fp16 as stored, mask [N,H,W] bool
    or None (all True), `feat` the features on the flow's grid and `other` those of the frame it points into, float32 [N,C,H,W] or
    [C,H,W], `flow_sign` -1 for 's' flows and +1 for 't' flows, `radius` 1 .. 4.  Returns fp32 [N,(2 radius + 1)^2,H,W] on the HIP
    device; nothing is read back."""
    lib, dev = _library(), device(vecs, mask, feat, other)
    n, _, h, w = vecs.shape
    d = (2 * int(radius) + 1) ** 2
    with _on(dev):
        keep, args = _operands(vecs, mask, feat, other, dev, n)
        vol = torch.empty((n, d, h, w), dtype=torch.float32, device=dev)
        _check(lib.ofl_flow_cost_volume_f32(*args, float(flow_sign), int(radius), _ptr(vol), n, h, w, _stream(dev)),
               "ofl_flow_cost_volume_f32")
    del keep
    return vol


def flow_cost_volume_grad(vecs: torch.Tensor, mask: torch.Tensor, feat: torch.Tensor, other: torch.Tensor, flow_sign: float, radius: int,
                          grad_volume: torch.Tensor, want_feat: bool = True, want_warped: bool = True):
    """The backward of the cost volume (ofl_flow_cost_volume_grad_f32): `grad_volume` [N,D,H,W], the upstream gradient.  Returns (the
    gradient with respect to `feat`, fp32 [N,C,H,W], or None; the gradient with respect to the warped tensor W, fp32 [N,C,H,W], or None)
    on the HIP device -- N images each, whatever the batch of `feat` and `other`."""
    if not (want_feat or want_warped):
        raise ValueError("oflibpytorch_amd: flow_cost_volume_grad needs at least one output")
    lib, dev = _library(), device(vecs, mask, feat, other, grad_volume)
    n, _, h, w = vecs.shape
    with _on(dev):
        keep, args = _operands(vecs, mask, feat, other, dev, n)
        g = grad_volume.detach().to(dev, torch.float32).contiguous()
        if tuple(g.shape) != (n, (2 * int(radius) + 1) ** 2, h, w):
            raise ValueError("oflibpytorch_amd: the gradient of the volume needs the volume's shape")
        c = args[-1]
        g_feat = torch.empty((n, c, h, w), dtype=torch.float32, device=dev) if want_feat else None
        g_warped = torch.empty((n, c, h, w), dtype=torch.float32, device=dev) if want_warped else None
        _check(lib.ofl_flow_cost_volume_grad_f32(*args, float(flow_sign), int(radius), _ptr(g), _ptr(g_feat), _ptr(g_warped), n, h, w,
                                                 _stream(dev)), "ofl_flow_cost_volume_grad_f32")
    del keep
    return g_feat, g_warped


def flow_cost_volume_chain(vecs: torch.Tensor, flow_sign: float) -> torch.Tensor:
    """The vectors the backward of the warp is run on (ofl_flow_cost_volume_chain_f32): fp32 [N,2,H,W], the flow's own,
    and a vector that points out of the frame where a component is not finite, so that such a pixel -- never usable, its gradient of W
    +0 -- puts no NaN weight on that +0."""
    lib, dev = _library(), device(vecs)
    n, _, h, w = vecs.shape
    with _on(dev):
        v, vbs, half = _vis_flow(vecs, dev, n)
        chain = torch.empty((n, 2, h, w), dtype=torch.float32, device=dev)
        _check(lib.ofl_flow_cost_volume_chain_f32(_ptr(v), vbs, half, float(flow_sign), _ptr(chain), n, h, w, _stream(dev)),
               "ofl_flow_cost_volume_chain_f32")
    del v
    return chain


def flow_cost_volume_gate(vecs: torch.Tensor, mask: torch.Tensor, flow_sign: float, grad_flow: torch.Tensor) -> torch.Tensor:
    """`grad_flow` fp32 [N,2,H,W] contiguous, in place: +0 where the pixel is not usable (ofl_flow_cost_volume_gate_f32) -- selected, not
    multiplied, as in the forward.  Returns `grad_flow`; allocates nothing."""
    lib, dev = _library(), device(vecs, mask, grad_flow)
    n, _, h, w = vecs.shape
    if grad_flow.dtype != torch.float32 or tuple(grad_flow.shape) != (n, 2, h, w) or not grad_flow.is_contiguous():
        raise ValueError("oflibpytorch_amd: the gradient of the flow needs to be contiguous float32 of the flow's shape")
    with _on(dev):
        v, vbs, half = _vis_flow(vecs, dev, n)
        m, mbs = (None, 0) if mask is None else _planes(mask, dev, torch.bool, n, "mask")
        _check(lib.ofl_flow_cost_volume_gate_f32(_ptr(v), vbs, half, _ptr(m), mbs, float(flow_sign), _ptr(grad_flow), n, h, w,
                                                 _stream(dev)), "ofl_flow_cost_volume_gate_f32")
    del v, m
    return grad_flow


def cost_volume(vecs: torch.Tensor, mask: torch.Tensor, feat: torch.Tensor, other: torch.Tensor, flow_sign: float = -1.0,
                radius: int = RADIUS) -> torch.Tensor:
    """The cost volume, fp32 [N,D,H,W].  When autograd is recording and the vectors, `feat` or `other` require a gradient, the call goes
    through `_autograd.CostVolumeFn`; the mask never carries a gradient."""
    if _wants_grad(vecs, feat, other):
        from . import _autograd
        return _autograd.CostVolumeFn.apply(vecs, mask, feat, other, flow_sign, radius)
    return flow_cost_volume(vecs, mask, feat, other, flow_sign, radius)
