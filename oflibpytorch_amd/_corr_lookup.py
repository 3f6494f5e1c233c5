"""ctypes binding of the correlation lookup (ofl_corr_lookup.hip; C ABI: include/oflib_hip.h).

A module of its own next to `_native`, whose helpers it uses: it declares the five entry points it calls and allocates its outputs, the
workspace of the backward and the keys under its own module-level name `torch`, which the dirty-memory tests replace
(tests/test_gpu_corr_lookup_dirty_memory.py).  The ordering of the keys between the two launches of the gradient of a level is plumbing
on the device: `torch.sort` (the keys are unique, so the order is determined) and `torch.searchsorted`; nothing is read back.
"""
import ctypes

import torch

from ._native import _check, _on, _planes, _ptr, _stream, _vis_flow, _wants_grad, device, load_library

RADIUS = 4                    # the default: RAFT's 9 x 9 window, D = 81
MAX_RADIUS = 4
LEVELS = 4                    # the default: RAFT's pyramid
MAX_LEVELS = 6

_declared = None


def _library():
    """libofl_hip.so with the five entry points of this module declared."""
    global _declared
    lib = load_library()
    if _declared is not lib:
        p, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float
        lib.ofl_flow_corr_lookup_cells.argtypes = [i32, i32, i32]
        lib.ofl_flow_corr_lookup_cells.restype = ctypes.c_int64
        lib.ofl_flow_corr_lookup_f32.argtypes = [p, i64, i32, p, i64, p, i64, p, i64, i32, f32, i32, i32, i32, i32, p, i64, i32, i32, i32, p]
        lib.ofl_flow_corr_lookup_f32.restype = ctypes.c_int
        lib.ofl_flow_corr_lookup_nodes_f32.argtypes = [p, i64, i32, p, i64, i32, f32, i32, i32, i32, i32, p, i64, p, p, i32, i32, i32, p]
        lib.ofl_flow_corr_lookup_nodes_f32.restype = ctypes.c_int
        lib.ofl_flow_corr_lookup_grad_feat_f32.argtypes = [p, i64, i32, p, i64, p, i64, i32, f32, i32, i32, i32, i32, p, p, i32, i32, i32,
                                                           i32, p]
        lib.ofl_flow_corr_lookup_grad_feat_f32.restype = ctypes.c_int
        lib.ofl_flow_corr_lookup_grad_other_f32.argtypes = [p, i64, i32, i32, i32, i32, p, p, p, p, i32, i32, i32, p]
        lib.ofl_flow_corr_lookup_grad_other_f32.restype = ctypes.c_int
        _declared = lib
    return lib


def check_levels(feat, levels):
    """The checks every route shares: float32 features, one C, levels of at least 1 x 1, batches of 1 or the flow's."""
    if not isinstance(levels, (list, tuple)) or not 1 <= len(levels) <= MAX_LEVELS:
        raise ValueError("oflibpytorch_amd: the lookup needs 1 to %d levels" % MAX_LEVELS)
    for t in (feat,) + tuple(levels):
        if t.dtype != torch.float32:
            raise TypeError("oflibpytorch_amd: the feature tensors need to be float32")
        if t.dim() not in (3, 4):
            raise ValueError("oflibpytorch_amd: the feature tensors need to be C-H-W or N-C-H-W")
    for lv in levels:
        if lv.shape[-3] != feat.shape[-3]:
            raise ValueError("oflibpytorch_amd: the feature tensors need the same number of channels")
        if lv.shape[-2] < 1 or lv.shape[-1] < 1:
            raise ValueError("oflibpytorch_amd: a level of the pyramid is empty")


def corr_pyramid(other: torch.Tensor, levels: int = LEVELS) -> list:
    """The levels of the lookup from one feature tensor, [N,C,H,W] or [C,H,W]: other_0 = other, other_l = avg_pool2d(other_{l-1}, 2, 2)
    (odd sizes are floored, as in RAFT).  Plain torch, so autograd carries the gradient of a level back to `other`.  A training loop
    calls this once for the lookups of all its iterations."""
    if not isinstance(levels, int) or isinstance(levels, bool):
        raise TypeError("oflibpytorch_amd: levels needs to be an integer")
    if not 1 <= levels <= MAX_LEVELS:
        raise ValueError("oflibpytorch_amd: levels needs to be 1 to %d" % MAX_LEVELS)
    if not isinstance(other, torch.Tensor) or other.dim() not in (3, 4):
        raise ValueError("oflibpytorch_amd: the feature tensor needs to be a tensor, C-H-W or N-C-H-W")
    out = [other]
    for _ in range(levels - 1):
        if out[-1].shape[-2] < 2 or out[-1].shape[-1] < 2:
            raise ValueError("oflibpytorch_amd: a level of the pyramid is empty")
        out.append(torch.nn.functional.avg_pool2d(out[-1], 2, 2))
    return out


def _flow_operands(vecs, mask, dev, n):
    v, vbs, half = _vis_flow(vecs, dev, n)
    m, mbs = (None, 0) if mask is None else _planes(mask, dev, torch.bool, n, "mask")
    return (v, m), (_ptr(v), vbs, half, _ptr(m), mbs)


def _features(t, dev, n, what):
    t = t.detach()
    return _planes(t[None] if t.dim() == 3 else t, dev, torch.float32, n, what)


def flow_corr_lookup(vecs: torch.Tensor, mask: torch.Tensor, feat: torch.Tensor, levels, flow_sign: float = -1.0,
                     radius: int = RADIUS) -> torch.Tensor:
    """The lookup of a flow (ofl_flow_corr_lookup_f32): vectors [N,2,H,W] fp32 or fp16 as stored, mask [N,H,W] bool or
    None (all True), `feat` float32 [N,C,H,W] or [C,H,W] on the flow's grid, `levels` a sequence of L float32 tensors [N,C,H_l,W_l] or
    [C,H_l,W_l] of the frame the flow points into, `flow_sign` -1 for 's' flows and +1 for 't' flows, `radius` 1 .. 4.  Returns fp32
    [N, L (2 radius + 1)^2, H, W] on the HIP device: one launch per level into its channel slice; nothing is read back."""
    check_levels(feat, levels)
    lib, dev = _library(), device(vecs, mask, feat, *levels)
    n, _, h, w = vecs.shape
    d = (2 * int(radius) + 1) ** 2
    with _on(dev):
        keep, flow_args = _flow_operands(vecs, mask, dev, n)
        ft, fbs = _features(feat, dev, n, "features")
        out = torch.empty((n, len(levels) * d, h, w), dtype=torch.float32, device=dev)
        for l, lv in enumerate(levels):
            ot, obs = _features(lv, dev, n, "level features")
            _check(lib.ofl_flow_corr_lookup_f32(*flow_args, _ptr(ft), fbs, _ptr(ot), obs, int(ft.shape[1]), float(flow_sign), int(radius), l,
                                                int(ot.shape[2]), int(ot.shape[3]), ctypes.c_void_p(out.data_ptr() + 4 * l * d * h * w),
                                                len(levels) * d * h * w, n, h, w, _stream(dev)), "ofl_flow_corr_lookup_f32")
            del ot
    del keep, ft
    return out


def flow_corr_lookup_grad(vecs: torch.Tensor, mask: torch.Tensor, feat: torch.Tensor, levels, flow_sign: float, radius: int,
                          grad_out: torch.Tensor, want_feat: bool = True, want_levels=None):
    """The backward of the lookup: `grad_out` [N, L D, H, W], the upstream gradient; `want_levels`: one bool per level (None: all).
    Returns (the gradient with respect to `feat`, fp32 [N,C,H,W], or None; a list with the gradient of each level, fp32 [N,C,H_l,W_l],
    or None) on the HIP device -- N images each, whatever the batch of the operand.  Per level: the nodes pass
    (ofl_flow_corr_lookup_nodes_f32) into one workspace that all levels share, then d feat, which continues the sums of the level
    before, and -- after torch.sort and torch.searchsorted of the keys -- the gather of d other."""
    check_levels(feat, levels)
    want_levels = [True] * len(levels) if want_levels is None else [bool(x) for x in want_levels]
    if len(want_levels) != len(levels):
        raise ValueError("oflibpytorch_amd: flow_corr_lookup_grad needs one flag per level")
    if not (want_feat or any(want_levels)):
        raise ValueError("oflibpytorch_amd: flow_corr_lookup_grad needs at least one output")
    lib, dev = _library(), device(vecs, mask, feat, grad_out, *levels)
    n, _, h, w = vecs.shape
    r = int(radius)
    d, nodes = (2 * r + 1) ** 2, (2 * r + 2) ** 2
    with _on(dev):
        keep, flow_args = _flow_operands(vecs, mask, dev, n)
        ft, fbs = _features(feat, dev, n, "features")
        c = int(ft.shape[1])
        g = grad_out.detach().to(dev, torch.float32).contiguous()
        if tuple(g.shape) != (n, len(levels) * d, h, w):
            raise ValueError("oflibpytorch_amd: the gradient of the lookup needs the lookup's shape")
        gn = torch.empty((n, nodes, h, w), dtype=torch.float32, device=dev)
        keys = torch.empty((n * h * w,), dtype=torch.int64, device=dev) if any(want_levels) else None
        g_feat = torch.empty((n, c, h, w), dtype=torch.float32, device=dev) if want_feat else None
        g_levels = []
        stream = _stream(dev)
        for l, lv in enumerate(levels):
            ot, obs = _features(lv, dev, n, "level features")
            hl, wl = int(ot.shape[2]), int(ot.shape[3])
            _check(lib.ofl_flow_corr_lookup_nodes_f32(*flow_args, c, float(flow_sign), r, l, hl, wl,
                                                      ctypes.c_void_p(g.data_ptr() + 4 * l * d * h * w), len(levels) * d * h * w, _ptr(gn),
                                                      _ptr(keys if want_levels[l] else None), n, h, w, stream),
                   "ofl_flow_corr_lookup_nodes_f32")
            if want_feat:
                _check(lib.ofl_flow_corr_lookup_grad_feat_f32(*flow_args, _ptr(ot), obs, c, float(flow_sign), r, l, hl, wl, _ptr(gn),
                                                              _ptr(g_feat), int(l > 0), n, h, w, stream),
                       "ofl_flow_corr_lookup_grad_feat_f32")
            if want_levels[l]:
                cells = int(lib.ofl_flow_corr_lookup_cells(hl, wl, r))
                if cells < 0:
                    raise RuntimeError("oflibpytorch_amd: ofl_flow_corr_lookup_cells failed with status %d" % cells)
                ordered, order = torch.sort(keys)
                bounds = torch.arange(n * cells + 1, dtype=torch.int64, device=dev) * (h * w)
                starts = torch.searchsorted(ordered, bounds).contiguous()
                g_other = torch.empty((n, c, hl, wl), dtype=torch.float32, device=dev)
                _check(lib.ofl_flow_corr_lookup_grad_other_f32(_ptr(ft), fbs, c, r, hl, wl, _ptr(gn), _ptr(order), _ptr(starts),
                                                               _ptr(g_other), n, h, w, stream), "ofl_flow_corr_lookup_grad_other_f32")
                g_levels.append(g_other)
                del ordered, order, bounds, starts
            else:
                g_levels.append(None)
            del ot
    del keep, ft
    return g_feat, g_levels


def corr_lookup(vecs: torch.Tensor, mask: torch.Tensor, feat: torch.Tensor, levels, flow_sign: float = -1.0,
                radius: int = RADIUS) -> torch.Tensor:
    """The lookup, fp32 [N, L D, H, W].  When autograd is recording and `feat` or a level requires a gradient, the call goes through
    `_autograd.CorrLookupFn`; the vectors and the mask never carry a gradient (RAFT detaches the coordinates before every lookup)."""
    if _wants_grad(feat, *levels):
        from . import _autograd
        return _autograd.CorrLookupFn.apply(vecs.detach(), mask, feat, flow_sign, radius, *levels)
    return flow_corr_lookup(vecs, mask, feat, levels, flow_sign, radius)
