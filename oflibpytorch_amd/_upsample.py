"""ctypes binding of the convex upsampling (ofl_upsample.hip; C ABI: include/oflib_hip.h).

A module of its own next to `_native`, whose helpers it uses: it declares the two entry points it calls and allocates its outputs and the
workspace of the backward under its own module-level name `torch`, which the dirty-memory tests replace
(tests/test_gpu_upsample_convex_dirty_memory.py).  Nothing is read back.
"""
import ctypes

import torch

from ._native import _check, _on, _planes, _ptr, _stream, _vis_flow, _wants_grad, device, load_library

FACTORS = (2, 4, 8)

_declared = None


def _library():
    """libofl_hip.so with the two entry points of this module declared."""
    global _declared
    lib = load_library()
    if _declared is not lib:
        p, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
        lib.ofl_flow_upsample_convex_f32.argtypes = [p, i64, i32, p, i64, p, i32, p, p, i32, i32, i32, p]
        lib.ofl_flow_upsample_convex_f32.restype = ctypes.c_int
        lib.ofl_flow_upsample_convex_grad_f32.argtypes = [p, i64, i32, p, i32, p, p, p, p, i32, i32, i32, p]
        lib.ofl_flow_upsample_convex_grad_f32.restype = ctypes.c_int
        _declared = lib
    return lib


def factor_of(channels: int) -> int:
    """The factor k of 9 k^2 logit channels, k in 2, 4, 8"""
    for k in FACTORS:
        if channels == 9 * k * k:
            return k
    raise ValueError("oflibpytorch_amd: %d logit channels are not 9 k^2 with k in (2, 4, 8)" % channels)


def _logits(logits, factor, dev, n, h, w):
    """The checks both routes share; the logits on the device, contiguous"""
    if isinstance(factor, bool) or not isinstance(factor, int):
        raise TypeError("oflibpytorch_amd: the factor needs to be an integer")
    if factor not in FACTORS:
        raise ValueError("oflibpytorch_amd: the factor needs to be 2, 4 or 8")
    if logits.dtype != torch.float32:
        raise TypeError("oflibpytorch_amd: the logits need to be float32")
    if tuple(logits.shape) != (n, 9 * factor * factor, h, w):
        raise ValueError("oflibpytorch_amd: the logits need the shape [N, 9 k^2, H, W] of the flow")
    lg = logits.detach()
    if lg.device != dev:
        lg = lg.to(dev)
    return lg.contiguous()


def flow_upsample_convex(vecs: torch.Tensor, mask: torch.Tensor, logits: torch.Tensor, factor: int):
    """The convex upsampling of a flow (ofl_flow_upsample_convex_f32): vectors [N,2,H,W] fp32 or fp16 as stored, mask
    [N,H,W] bool or None, `logits` float32 [N, 9 k^2, H, W] in RAFT's channel order, `factor` k in 2, 4, 8.  Returns (fp32
    [N, 2, k H, k W], bool [N, k H, k W] -- the coarse pixel's bit over its k x k block -- or None without a mask) on the HIP device: one
    launch; nothing is read back."""
    lib, dev = _library(), device(vecs, mask, logits)
    n, _, h, w = vecs.shape
    with _on(dev):
        lg = _logits(logits, factor, dev, n, h, w)
        v, vbs, half = _vis_flow(vecs, dev, n)
        m, mbs = (None, 0) if mask is None else _planes(mask, dev, torch.bool, n, "mask")
        out = torch.empty((n, 2, factor * h, factor * w), dtype=torch.float32, device=dev)
        out_mask = None if mask is None else torch.empty((n, factor * h, factor * w), dtype=torch.bool, device=dev)
        _check(lib.ofl_flow_upsample_convex_f32(_ptr(v), vbs, half, _ptr(m), mbs, _ptr(lg), factor, _ptr(out), _ptr(out_mask), n, h, w,
                                                _stream(dev)), "ofl_flow_upsample_convex_f32")
    del v, m, lg
    return out, out_mask


def flow_upsample_convex_grad(vecs: torch.Tensor, logits: torch.Tensor, factor: int, grad_out: torch.Tensor, want_logits: bool = True,
                              want_vecs: bool = True):
    """The backward of the convex upsampling (ofl_flow_upsample_convex_grad_f32): `grad_out` [N, 2, k H, k W], the upstream gradient.
    Returns (the gradient with respect to the logits, fp32 [N, 9 k^2, H, W], or None; the gradient with respect to the vectors, fp32
    [N,2,H,W], or None) on the HIP device.  The per-fine-pixel pass writes d logits and, when the vectors want a gradient, the maximum
    and the sum of every fine pixel's softmax to a float64 workspace [N, 2, k H, k W], which the gather of d vecs then reads."""
    if not (want_logits or want_vecs):
        raise ValueError("oflibpytorch_amd: flow_upsample_convex_grad needs at least one output")
    lib, dev = _library(), device(vecs, logits, grad_out)
    n, _, h, w = vecs.shape
    with _on(dev):
        lg = _logits(logits, factor, dev, n, h, w)
        v, vbs, half = _vis_flow(vecs, dev, n)
        g = grad_out.detach().to(dev, torch.float32).contiguous()
        if tuple(g.shape) != (n, 2, factor * h, factor * w):
            raise ValueError("oflibpytorch_amd: the gradient of the upsampled flow needs its shape")
        if g.data_ptr() % 16:
            g = g.clone()                                   # (a view at an odd offset: the kernels load whole fine rows)
        d_logits = torch.empty((n, 9 * factor * factor, h, w), dtype=torch.float32, device=dev) if want_logits else None
        d_vecs = torch.empty((n, 2, h, w), dtype=torch.float32, device=dev) if want_vecs else None
        work = torch.empty((n, 2, factor * h, factor * w), dtype=torch.float64, device=dev) if want_vecs else None
        _check(lib.ofl_flow_upsample_convex_grad_f32(_ptr(v), vbs, half, _ptr(lg), factor, _ptr(g), _ptr(d_logits), _ptr(d_vecs), _ptr(work),
                                                     n, h, w, _stream(dev)), "ofl_flow_upsample_convex_grad_f32")
    del v, lg, g, work
    return d_logits, d_vecs


def upsample_convex(vecs: torch.Tensor, mask: torch.Tensor, logits: torch.Tensor, factor: int):
    """(the upsampled vectors, fp32 [N, 2, k H, k W]; their mask or None).  When autograd is recording and the logits or the vectors
    require a gradient, the call goes through `_autograd.UpsampleConvexFn`; the mask never carries one."""
    if _wants_grad(vecs, logits):
        from . import _autograd
        out, out_mask = _autograd.UpsampleConvexFn.apply(vecs, mask, logits, factor)
        return out, out_mask
    return flow_upsample_convex(vecs, mask, logits, factor)
