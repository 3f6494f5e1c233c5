"""ctypes binding of the global matching (ofl_matching.hip, DESIGN.md 3.27, and ofl_matching_x16.hip, DESIGN.md 3.32, for two fp16 or two
bf16 tensors; C ABI: include/oflib_hip.h).

A module of its own next to `_native`, whose helpers it uses: it declares the entry points it calls and allocates its outputs, the
matching probability, the workspace of the backward, the packed rows of the 16-bit route and the gradients under its own module-level
name `torch`, which the dirty-memory tests replace (tests/test_gpu_matching_dirty_memory.py, tests/test_gpu_matching_x16_dirty_memory.py).
Nothing is read back.
"""
import ctypes

import torch

from ._native import _check, _on, _planes, _ptr, _stream, _wants_grad, device, load_library

STATS_BYTES = 28              # of the workspace, per pixel: S, ox, oy float64, m float32
X16 = {torch.float16: 0, torch.bfloat16: 1}          # OFL_X16_HALF, OFL_X16_BFLOAT (include/oflib_hip.h)

_declared = None


def _library():
    """libofl_hip.so with the entry points of this module declared."""
    global _declared
    lib = load_library()
    if _declared is not lib:
        p, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float
        lib.ofl_flow_global_match_f32.argtypes = [p, i64, p, i64, i32, f32, p, p, p, i32, i32, i32, p]
        lib.ofl_flow_global_match_f32.restype = ctypes.c_int
        lib.ofl_flow_global_match_grad_f32.argtypes = [p, i64, p, i64, i32, f32, p, p, p, p, i32, i32, i32, p]
        lib.ofl_flow_global_match_grad_f32.restype = ctypes.c_int
        lib.ofl_flow_global_match_x16.argtypes = [p, i64, p, i64, i32, i32, f32, p, p, p, p, i32, i32, i32, p]
        lib.ofl_flow_global_match_x16.restype = ctypes.c_int
        lib.ofl_flow_global_match_x16_pack_bytes.argtypes = [i32, i32, i32, i32]
        lib.ofl_flow_global_match_x16_pack_bytes.restype = ctypes.c_int64
        _declared = lib
    return lib


def check_features(feat, other):
    """The checks every route shares: two float32 tensors, or two tensors of ONE 16-bit dtype (float16, bfloat16), of one shape, C-H-W
    or N-C-H-W, no empty axis."""
    for t in (feat, other):
        if not isinstance(t, torch.Tensor) or (t.dtype != torch.float32 and t.dtype not in X16):
            raise TypeError("oflibpytorch_amd: the feature tensors need to be float32 tensors, or both float16 or both bfloat16")
    if feat.dtype != other.dtype:
        raise TypeError("oflibpytorch_amd: the feature tensors need to be float32 tensors, or both float16 or both bfloat16, not a "
                        "mixed pair")
    if feat.dim() not in (3, 4):
        raise ValueError("oflibpytorch_amd: the feature tensors need to be C-H-W or N-C-H-W")
    if tuple(feat.shape) != tuple(other.shape):
        raise ValueError("oflibpytorch_amd: the feature tensors need the same shape")
    if min(feat.shape) < 1:
        raise ValueError("oflibpytorch_amd: the feature tensors are empty")


def _features(t, dev, n, what, dtype=torch.float32):
    t = t.detach()
    return _planes(t[None] if t.dim() == 3 else t, dev, dtype, n, what)


def _frame(feat):
    """(n, c, h, w) of a C-H-W or N-C-H-W tensor"""
    return (1,) + tuple(int(s) for s in feat.shape) if feat.dim() == 3 else tuple(int(s) for s in feat.shape)


def flow_global_match(feat: torch.Tensor, other: torch.Tensor, flow_sign: float = -1.0, want_prob: bool = False, want_stats: bool = False):
    """The global matching of two feature tensors (ofl_flow_global_match_f32): `feat` and `other` float32 [N,C,H,W] or
    [C,H,W] of one shape, `flow_sign` -1 for an 's' flow and +1 for a 't' flow.  Returns (the vectors, fp32 [N,2,H,W]; the matching
    probability, fp32 [N,H,W], or None; the statistics of every pixel's softmax for the backward, 28 bytes a pixel in one uint8 tensor, or
    None) on the HIP device: one launch; nothing is read back."""
    check_features(feat, other)
    lib, dev = _library(), device(feat, other)
    n, c, h, w = _frame(feat)
    with _on(dev):
        ft, fbs = _features(feat, dev, n, "features")
        ot, obs = _features(other, dev, n, "other features")
        out = torch.empty((n, 2, h, w), dtype=torch.float32, device=dev)
        prob = torch.empty((n, h, w), dtype=torch.float32, device=dev) if want_prob else None
        stats = torch.empty((STATS_BYTES * n * h * w,), dtype=torch.uint8, device=dev) if want_stats else None
        _check(lib.ofl_flow_global_match_f32(_ptr(ft), fbs, _ptr(ot), obs, c, float(flow_sign), _ptr(out), _ptr(prob), _ptr(stats), n, h, w,
                                             _stream(dev)), "ofl_flow_global_match_f32")
    del ft, ot
    return out, prob, stats


def flow_global_match_x16(feat: torch.Tensor, other: torch.Tensor, flow_sign: float = -1.0, want_prob: bool = False, want_stats: bool = False):
    """The global matching of two fp16 or two bf16 feature tensors on the matrix cores (ofl_flow_global_match_x16): the
    arguments and the results of `flow_global_match` -- the vectors and the probability float32, the statistics in the same layout, so
    that `flow_global_match_grad` reads them.  Two launches (the tensors to pixel-major rows, then the walk); the packed rows are a
    workspace of this call; nothing is read back."""
    check_features(feat, other)
    if feat.dtype not in X16:
        raise TypeError("oflibpytorch_amd: flow_global_match_x16 needs float16 or bfloat16 feature tensors")
    lib, dev = _library(), device(feat, other)
    n, c, h, w = _frame(feat)
    with _on(dev):
        ft, fbs = _features(feat, dev, n, "features", feat.dtype)
        ot, obs = _features(other, dev, n, "other features", feat.dtype)
        size = int(lib.ofl_flow_global_match_x16_pack_bytes(c, n, h, w))
        if size < 0:
            _check(size, "ofl_flow_global_match_x16_pack_bytes")
        out = torch.empty((n, 2, h, w), dtype=torch.float32, device=dev)
        prob = torch.empty((n, h, w), dtype=torch.float32, device=dev) if want_prob else None
        stats = torch.empty((STATS_BYTES * n * h * w,), dtype=torch.uint8, device=dev) if want_stats else None
        pack = torch.empty((size,), dtype=torch.uint8, device=dev)
        _check(lib.ofl_flow_global_match_x16(_ptr(ft), fbs, _ptr(ot), obs, c, X16[feat.dtype], float(flow_sign), _ptr(out), _ptr(prob),
                                             _ptr(stats), _ptr(pack), n, h, w, _stream(dev)), "ofl_flow_global_match_x16")
    del ft, ot, pack
    return out, prob, stats


def flow_global_match_grad(feat: torch.Tensor, other: torch.Tensor, flow_sign: float, stats: torch.Tensor, grad_out: torch.Tensor,
                           want_feat: bool = True, want_other: bool = True):
    """The backward of the global matching (ofl_flow_global_match_grad_f32): `stats` as the forward returned it for these operands,
    `grad_out` [N,2,H,W], the upstream gradient.  Returns (the gradient with respect to `feat`, fp32 [N,C,H,W], or None; with respect to
    `other`, likewise) on the HIP device: one launch per gradient, each recomputing the logits on the saved maximum and sum."""
    if not (want_feat or want_other):
        raise ValueError("oflibpytorch_amd: flow_global_match_grad needs at least one output")
    check_features(feat, other)
    n, c, h, w = _frame(feat)
    lib, dev = _library(), device(feat, other, grad_out)
    if stats.dtype != torch.uint8 or stats.numel() != STATS_BYTES * n * h * w or stats.device != dev or not stats.is_contiguous():
        raise ValueError("oflibpytorch_amd: the statistics need to be those the forward returned for these operands")
    with _on(dev):
        ft, fbs = _features(feat, dev, n, "features")
        ot, obs = _features(other, dev, n, "other features")
        g = grad_out.detach().to(dev, torch.float32).contiguous()
        if tuple(g.shape) != (n, 2, h, w):
            raise ValueError("oflibpytorch_amd: the gradient of the matched flow needs its shape")
        d_feat = torch.empty((n, c, h, w), dtype=torch.float32, device=dev) if want_feat else None
        d_other = torch.empty((n, c, h, w), dtype=torch.float32, device=dev) if want_other else None
        _check(lib.ofl_flow_global_match_grad_f32(_ptr(ft), fbs, _ptr(ot), obs, c, float(flow_sign), _ptr(stats), _ptr(g), _ptr(d_feat),
                                                  _ptr(d_other), n, h, w, _stream(dev)), "ofl_flow_global_match_grad_f32")
    del ft, ot, g
    return d_feat, d_other


def global_match(feat: torch.Tensor, other: torch.Tensor, flow_sign: float = -1.0, want_prob: bool = False):
    """(the vectors, fp32 [N,2,H,W]; the matching probability, fp32 [N,H,W], or None).  Two float32 tensors take ofl_matching.hip, two
    float16 or two bfloat16 tensors ofl_matching_x16.hip.  When autograd is recording and `feat` or `other` requires a gradient, the call
    goes through `_autograd.GlobalMatchFn`; the probability never carries one."""
    check_features(feat, other)
    if _wants_grad(feat, other):
        from . import _autograd
        return _autograd.GlobalMatchFn.apply(feat, other, flow_sign, want_prob)
    forward = flow_global_match_x16 if feat.dtype in X16 else flow_global_match
    out, prob, _ = forward(feat, other, flow_sign, want_prob, False)
    return out, prob
