"""ctypes binding of the flow propagation by attention (ofl_propagate.hip; C ABI: include/oflib_hip.h).

A module of its own next to `_native`, whose helpers it uses: it declares the four entry points it calls and allocates its outputs, the
result mask, the statistics and the scratch of the backward and the gradients under its own module-level name `torch`, which the
dirty-memory tests replace (tests/test_gpu_propagate_dirty_memory.py).  Nothing is read back.
"""
import ctypes

import torch

from ._native import _check, _on, _planes, _ptr, _stream, _wants_grad, device, load_library

STATS_BYTES = 28              # of the workspace, per pixel: S, ox, oy float64, m float32
MAX_RADIUS = 4

_declared = None


def _library():
    """libofl_hip.so with the four entry points of this module declared."""
    global _declared
    lib = load_library()
    if _declared is not lib:
        p, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
        ops = [p, i64, p, i64, i32, p, i64, p, i64]
        lib.ofl_flow_propagate_global_f32.argtypes = ops + [p, p, p, i32, i32, i32, p]
        lib.ofl_flow_propagate_global_f32.restype = ctypes.c_int
        lib.ofl_flow_propagate_global_grad_f32.argtypes = ops + [p, p, p, p, p, i32, i32, i32, p]
        lib.ofl_flow_propagate_global_grad_f32.restype = ctypes.c_int
        lib.ofl_flow_propagate_local_f32.argtypes = ops + [i32, p, p, p, i32, i32, i32, p]
        lib.ofl_flow_propagate_local_f32.restype = ctypes.c_int
        lib.ofl_flow_propagate_local_grad_f32.argtypes = ops + [i32, p, p, p, p, p, p, i32, i32, i32, p]
        lib.ofl_flow_propagate_local_grad_f32.restype = ctypes.c_int
        _declared = lib
    return lib


def check_operands(vecs, mask, query, key, radius):
    """The checks every route shares: float32 query and key, C-H-W or N-C-H-W, the same C, the flow's H-W and batch; radius None or
    1 .. 4."""
    for t in (query, key):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise TypeError("oflibpytorch_amd: query and key need to be float32 tensors")
        if t.dim() not in (3, 4):
            raise ValueError("oflibpytorch_amd: query and key need to be C-H-W or N-C-H-W")
        if tuple(t.shape[-2:]) != tuple(vecs.shape[-2:]) or (t.dim() == 4 and t.shape[0] != vecs.shape[0]):
            raise ValueError("oflibpytorch_amd: query and key need the flow's shape")
    if query.shape[-3] != key.shape[-3] or query.shape[-3] < 1:
        raise ValueError("oflibpytorch_amd: query and key need the same number of channels, at least 1")
    if radius is not None:
        if isinstance(radius, bool) or not isinstance(radius, int):
            raise TypeError("oflibpytorch_amd: the radius needs to be an integer or None")
        if not 1 <= radius <= MAX_RADIUS:
            raise ValueError("oflibpytorch_amd: the radius needs to be 1, 2, 3 or 4")


def _operands(vecs, mask, query, key, dev, n):
    """(tensors to keep alive, the arguments all four entry points begin with)"""
    v, vbs = _planes(vecs.detach(), dev, torch.float32, n, "flow")
    m, mbs = (None, 0) if mask is None else _planes(mask, dev, torch.bool, n, "mask")
    qt, kt = query.detach(), key.detach()
    qt, qbs = _planes(qt[None] if qt.dim() == 3 else qt, dev, torch.float32, n, "query")
    kt, kbs = _planes(kt[None] if kt.dim() == 3 else kt, dev, torch.float32, n, "key")
    return (v, m, qt, kt), (_ptr(qt), qbs, _ptr(kt), kbs, int(qt.shape[1]), _ptr(v), vbs, _ptr(m), mbs)


def flow_propagate(vecs: torch.Tensor, mask: torch.Tensor, query: torch.Tensor, key: torch.Tensor, radius=None, want_stats: bool = False):
    """The propagation of a flow by attention (ofl_flow_propagate_global_f32 with `radius` None, ofl_flow_propagate_local_f32 with 1 .. 4;
    DESIGN.md 3.28): vectors [N,2,H,W], mask [N,H,W] bool or None (nothing excluded), `query` and `key` float32 [N,C,H,W] or [C,H,W].
    Returns (the vectors, fp32 [N,2,H,W]; the result mask, bool [N,H,W], False at the empty pixels, or None without a mask; the
    statistics of every pixel's softmax for the backward, 28 bytes a pixel in one uint8 tensor, or None) on the HIP device: one launch;
    nothing is read back."""
    check_operands(vecs, mask, query, key, radius)
    lib, dev = _library(), device(vecs, mask, query, key)
    n, _, h, w = vecs.shape
    with _on(dev):
        keep, args = _operands(vecs, mask, query, key, dev, n)
        out = torch.empty((n, 2, h, w), dtype=torch.float32, device=dev)
        valid = None if mask is None else torch.empty((n, h, w), dtype=torch.bool, device=dev)
        stats = torch.empty((STATS_BYTES * n * h * w,), dtype=torch.uint8, device=dev) if want_stats else None
        if radius is None:
            _check(lib.ofl_flow_propagate_global_f32(*args, _ptr(out), _ptr(valid), _ptr(stats), n, h, w, _stream(dev)),
                   "ofl_flow_propagate_global_f32")
        else:
            _check(lib.ofl_flow_propagate_local_f32(*args, int(radius), _ptr(out), _ptr(valid), _ptr(stats), n, h, w, _stream(dev)),
                   "ofl_flow_propagate_local_f32")
    del keep
    return out, valid, stats


def flow_propagate_grad(vecs: torch.Tensor, mask: torch.Tensor, query: torch.Tensor, key: torch.Tensor, radius, stats: torch.Tensor,
                        grad_out: torch.Tensor, want_query: bool = True, want_key: bool = True, want_flow: bool = True):
    """The backward of the propagation (ofl_flow_propagate_global_grad_f32 / ofl_flow_propagate_local_grad_f32): `stats` as the forward
    returned it for these operands, `grad_out` [N,2,H,W], the upstream gradient.  Returns (the gradient with respect to `query`, fp32
    [N,C,H,W], or None; with respect to `key`, likewise; with respect to the vectors, fp32 [N,2,H,W], or None) on the HIP device -- N
    images each, whatever the batch of `query` and `key`.  The local form's scratch, (2 radius + 1)^2 float32 per pixel for dss and
    twice as many again when the vectors want a gradient, lives for the call only."""
    if not (want_query or want_key or want_flow):
        raise ValueError("oflibpytorch_amd: flow_propagate_grad needs at least one output")
    check_operands(vecs, mask, query, key, radius)
    lib, dev = _library(), device(vecs, mask, query, key, grad_out)
    n, _, h, w = vecs.shape
    if stats.dtype != torch.uint8 or stats.numel() != STATS_BYTES * n * h * w or stats.device != dev or not stats.is_contiguous():
        raise ValueError("oflibpytorch_amd: the statistics need to be those the forward returned for these operands")
    with _on(dev):
        keep, args = _operands(vecs, mask, query, key, dev, n)
        c = args[4]
        g = grad_out.detach().to(dev, torch.float32).contiguous()
        if tuple(g.shape) != (n, 2, h, w):
            raise ValueError("oflibpytorch_amd: the gradient of the propagated flow needs its shape")
        d_query = torch.empty((n, c, h, w), dtype=torch.float32, device=dev) if want_query else None
        d_key = torch.empty((n, c, h, w), dtype=torch.float32, device=dev) if want_key else None
        d_flow = torch.empty((n, 2, h, w), dtype=torch.float32, device=dev) if want_flow else None
        if radius is None:
            _check(lib.ofl_flow_propagate_global_grad_f32(*args, _ptr(stats), _ptr(g), _ptr(d_query), _ptr(d_key), _ptr(d_flow), n, h, w,
                                                          _stream(dev)), "ofl_flow_propagate_global_grad_f32")
        else:
            d = (2 * int(radius) + 1) ** 2
            scratch = torch.empty((n, 3 if want_flow else 1, d, h, w), dtype=torch.float32, device=dev)
            _check(lib.ofl_flow_propagate_local_grad_f32(*args, int(radius), _ptr(stats), _ptr(g), _ptr(scratch), _ptr(d_query), _ptr(d_key),
                                                         _ptr(d_flow), n, h, w, _stream(dev)), "ofl_flow_propagate_local_grad_f32")
            del scratch
    del keep, g
    return d_query, d_key, d_flow


def propagate(vecs: torch.Tensor, mask: torch.Tensor, query: torch.Tensor, key: torch.Tensor, radius=None):
    """(the propagated vectors, fp32 [N,2,H,W]; the result mask or None).  When autograd is recording and the vectors, `query` or `key`
    require a gradient, the call goes through `_autograd.PropagateFn`; the mask never carries one."""
    if _wants_grad(vecs, query, key):
        from . import _autograd
        out, valid = _autograd.PropagateFn.apply(vecs, mask, query, key, radius)
        return out, valid
    out, valid, _ = flow_propagate(vecs, mask, query, key, radius, False)
    return out, valid
