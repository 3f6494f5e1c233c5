"""ctypes binding of the fused photometric loss (ofl_photometric.hip; C ABI: include/oflib_hip.h).

A module of its own next to `_native`, whose helpers it uses: it declares the three entry points it calls and allocates its outputs and
its workspace under its own module-level name `torch`, which the dirty-memory tests replace (tests/test_gpu_photometric_dirty_memory.py).
"""
import ctypes

import torch

from ._native import _check, _on, _operands, _ptr, _stream, _wants_grad, device, load_library, mean_of

RECORD = 8                    # doubles per image: count of known pixels, sum rho, max rho over the known pixels, 0, 0, 0, 0, 0

_declared = None


def _library():
    """libofl_hip.so with the three entry points of this module declared."""
    global _declared
    lib = load_library()
    if _declared is not lib:
        p, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float
        lib.ofl_flow_photometric_workspace_bytes.argtypes = [i32, i32, i32]
        lib.ofl_flow_photometric_workspace_bytes.restype = ctypes.c_int64
        lib.ofl_flow_photometric_f64.argtypes = [p, i64, i32, p, i64, p, i64, p, i64, i32, i32, f32, f32, p, p, p, i32, i32, i32, p]
        lib.ofl_flow_photometric_f64.restype = ctypes.c_int
        lib.ofl_flow_photometric_grad_f32.argtypes = [p, i64, i32, p, i64, p, i64, p, i64, i32, i32, f32, f32, p, p, i32, i32, i32, p]
        lib.ofl_flow_photometric_grad_f32.restype = ctypes.c_int
        _declared = lib
    return lib


def flow_photometric(vecs: torch.Tensor, mask: torch.Tensor, img: torch.Tensor, other: torch.Tensor, flow_sign: float = -1.0,
                     eps: float = 0.001, want_map: bool = False, want_record: bool = True):
    """The photometric records of a flow (ofl_flow_photometric_f64): vectors [N,2,H,W] fp32 or fp16 as stored, mask
    [N,H,W] bool or None (all True), `img` the frame on the flow's grid and `other` the frame it points into, [N,C,H,W] or [C,H,W],
    float32 or uint8, `flow_sign` -1 for 's' flows and +1 for 't' flows.  Returns (float64 [N,8] records or None, fp32 [N,H,W] map or
    None) on the HIP device; nothing is read back."""
    lib, dev = _library(), device(vecs, mask, img, other)
    n, _, h, w = vecs.shape
    if not (want_map or want_record):
        raise ValueError("oflibpytorch_amd: flow_photometric needs at least one output")
    with _on(dev):
        keep, args = _operands(vecs, mask, img, other, dev, n)
        ws = rec = None
        if want_record:
            nbytes = int(lib.ofl_flow_photometric_workspace_bytes(n, h, w))
            _check(min(nbytes, 0), "ofl_flow_photometric_workspace_bytes")
            ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
            rec = torch.empty((n, RECORD), dtype=torch.float64, device=dev)
        pmap = torch.empty((n, h, w), dtype=torch.float32, device=dev) if want_map else None
        _check(lib.ofl_flow_photometric_f64(*args, float(flow_sign), float(eps), _ptr(ws), _ptr(pmap), _ptr(rec), n, h, w,
                                            _stream(dev)), "ofl_flow_photometric_f64")
    del keep
    return rec, pmap


def flow_photometric_grad(vecs: torch.Tensor, mask: torch.Tensor, img: torch.Tensor, other: torch.Tensor, flow_sign: float, eps: float,
                          scale: torch.Tensor) -> torch.Tensor:
    """The backward of the per-image mean photometric penalty (ofl_flow_photometric_grad_f32): `scale` fp32 [N] on the device (upstream
    gradient / count).  Returns the gradient with respect to the vectors, fp32 [N,2,H,W] on the HIP device."""
    lib, dev = _library(), device(vecs, mask, img, other)
    n, _, h, w = vecs.shape
    with _on(dev):
        keep, args = _operands(vecs, mask, img, other, dev, n)
        sc = scale.detach().to(dev, torch.float32).contiguous()
        grad = torch.empty((n, 2, h, w), dtype=torch.float32, device=dev)
        _check(lib.ofl_flow_photometric_grad_f32(*args, float(flow_sign), float(eps), _ptr(sc), _ptr(grad), n, h, w, _stream(dev)),
               "ofl_flow_photometric_grad_f32")
    del keep
    return grad


def photometric(vecs: torch.Tensor, mask: torch.Tensor, img: torch.Tensor, other: torch.Tensor, flow_sign: float = -1.0,
                eps: float = 0.001) -> torch.Tensor:
    """The per-image photometric loss, fp32 [N].  When autograd is recording and the vectors require a gradient, the call goes through
    `_autograd.PhotometricFn`; the images never carry a gradient."""
    if _wants_grad(vecs):
        from . import _autograd
        return _autograd.PhotometricFn.apply(vecs, mask, img, other, flow_sign, eps)
    return mean_of(flow_photometric(vecs, mask, img, other, flow_sign, eps)[0])
