"""ctypes binding of the edge-aware smoothness penalty (ofl_smoothness.hip; C ABI: include/oflib_hip.h).

A module of its own next to `_native`, whose helpers it uses: it declares the three entry points it calls and allocates its outputs and
its workspace under its own module-level name `torch`, which the dirty-memory tests replace (tests/test_gpu_smoothness_dirty_memory.py).
"""
import ctypes

import torch

from ._native import _check, _on, _planes, _ptr, _stream, _vis_flow, _wants_grad, device, load_library

RECORD = 8                    # doubles per image: count_x, count_y, sum_x, sum_y, max over the valid terms, 0, 0, 0

_declared = None


def _library():
    """libofl_hip.so with the three entry points of this module declared."""
    global _declared
    lib = load_library()
    if _declared is not lib:
        p, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float
        lib.ofl_flow_smoothness_workspace_bytes.argtypes = [i32, i32, i32]
        lib.ofl_flow_smoothness_workspace_bytes.restype = ctypes.c_int64
        lib.ofl_flow_smoothness_f64.argtypes = [p, i64, i32, p, i64, p, i64, i32, i32, i32, f32, f32, p, p, p, i32, i32, i32, p]
        lib.ofl_flow_smoothness_f64.restype = ctypes.c_int
        lib.ofl_flow_smoothness_grad_f32.argtypes = [p, i64, i32, p, i64, p, i64, i32, i32, i32, f32, f32, p, p, i32, i32, i32, p]
        lib.ofl_flow_smoothness_grad_f32.restype = ctypes.c_int
        _declared = lib
    return lib


def _operands(vecs, mask, img, dev, n):
    """(tensors to keep alive, the arguments of both entry points up to img_u8).  `img`: None, or C-H-W (broadcast over the batch) or
    N-C-H-W, float32 or uint8."""
    v, vbs, half = _vis_flow(vecs, dev, n)
    m, mbs = (None, 0) if mask is None else _planes(mask, dev, torch.bool, n, "mask")
    im, ibs, chan, u8 = None, 0, 0, 0
    if img is not None:
        if img.dtype not in (torch.float32, torch.uint8):
            raise TypeError("oflibpytorch_amd: the guidance image needs to be float32 or uint8")
        im = img.detach()
        im, ibs = _planes(im[None] if im.dim() == 3 else im, dev, img.dtype, n, "image")
        chan, u8 = int(im.shape[1]), int(img.dtype == torch.uint8)
    return (v, m, im), (_ptr(v), vbs, half, _ptr(m), mbs, _ptr(im), ibs, chan, u8)


def flow_smoothness(vecs: torch.Tensor, mask: torch.Tensor = None, img: torch.Tensor = None, order: int = 1, alpha: float = 10.0,
                    eps: float = 0.001, want_map: bool = False):
    """The smoothness records of a flow (ofl_flow_smoothness_f64): vectors [N,2,H,W] fp32 or fp16 as stored, mask
    [N,H,W] bool or None (all True), guidance image [N,C,H,W] or [C,H,W] float32 or uint8, or None.  Returns (float64 [N,8] records,
    fp32 [N,H,W] map or None) on the HIP device; nothing is read back."""
    lib, dev = _library(), device(vecs, mask, img)
    n, _, h, w = vecs.shape
    with _on(dev):
        keep, args = _operands(vecs, mask, img, dev, n)
        nbytes = int(lib.ofl_flow_smoothness_workspace_bytes(n, h, w))
        _check(min(nbytes, 0), "ofl_flow_smoothness_workspace_bytes")
        ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
        rec = torch.empty((n, RECORD), dtype=torch.float64, device=dev)
        smap = torch.empty((n, h, w), dtype=torch.float32, device=dev) if want_map else None
        _check(lib.ofl_flow_smoothness_f64(*args, int(order), float(alpha), float(eps), _ptr(ws), _ptr(smap), _ptr(rec), n, h, w,
                                           _stream(dev)), "ofl_flow_smoothness_f64")
    del keep
    return rec, smap


def flow_smoothness_grad(vecs: torch.Tensor, mask: torch.Tensor, img: torch.Tensor, order: int, alpha: float, eps: float,
                         scale: torch.Tensor) -> torch.Tensor:
    """The backward of the per-image mean smoothness (ofl_flow_smoothness_grad_f32): `scale` fp32 [N] on the device (upstream gradient /
    total count).  Returns the gradient with respect to the vectors, fp32 [N,2,H,W] on the HIP device."""
    lib, dev = _library(), device(vecs, mask, img)
    n, _, h, w = vecs.shape
    with _on(dev):
        keep, args = _operands(vecs, mask, img, dev, n)
        sc = scale.detach().to(dev, torch.float32).contiguous()
        grad = torch.empty((n, 2, h, w), dtype=torch.float32, device=dev)
        _check(lib.ofl_flow_smoothness_grad_f32(*args, int(order), float(alpha), float(eps), _ptr(sc), _ptr(grad), n, h, w,
                                                _stream(dev)), "ofl_flow_smoothness_grad_f32")
    del keep
    return grad


def mean_of(rec: torch.Tensor) -> torch.Tensor:
    """The loss of a record: the float64 quotient (sum_x + sum_y) / (count_x + count_y) rounded once to fp32 (NaN without a valid term)."""
    return ((rec[:, 2] + rec[:, 3]) / (rec[:, 0] + rec[:, 1])).to(torch.float32)


def smoothness(vecs: torch.Tensor, mask: torch.Tensor = None, img: torch.Tensor = None, order: int = 1, alpha: float = 10.0,
               eps: float = 0.001) -> torch.Tensor:
    """The per-image smoothness loss, fp32 [N].  When autograd is recording and the vectors require a gradient, the call goes through
    `_autograd.SmoothnessFn`; the image never carries a gradient."""
    if _wants_grad(vecs):
        from . import _autograd
        return _autograd.SmoothnessFn.apply(vecs, mask, img, order, alpha, eps)
    return mean_of(flow_smoothness(vecs, mask, img, order, alpha, eps)[0])
