"""ctypes binding of the forward-backward consistency check (ofl_consistency.hip; C ABI: include/oflib_hip.h).

A module of its own next to `_native`, whose helpers it uses: it declares the two entry points it calls and allocates its outputs and
its workspace under its own module-level name `torch`, which the dirty-memory tests replace (tests/test_gpu_consistency_dirty_memory.py).
"""
import ctypes

import torch

from ._native import _check, _on, _planes, _ptr, _stream, _vis_flow, device, load_library

RECORD = 8                    # doubles per image: known, consistent, sum e over known, max e over known, sum e over consistent, 0, 0, 0

_declared = None


def _library():
    """libofl_hip.so with the two entry points of this module declared."""
    global _declared
    lib = load_library()
    if _declared is not lib:
        p, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float
        lib.ofl_flow_consistency_workspace_bytes.argtypes = [i32, i32, i32]
        lib.ofl_flow_consistency_workspace_bytes.restype = ctypes.c_int64
        lib.ofl_flow_consistency_f32.argtypes = [p, i64, i32, p, i64, i32, p, i64, p, i64, f32, f32, f32, p, p, p, p, p, i32, i32, i32, p]
        lib.ofl_flow_consistency_f32.restype = ctypes.c_int
        _declared = lib
    return lib


def flow_consistency(a: torch.Tensor, back: torch.Tensor, a_mask: torch.Tensor = None, back_mask: torch.Tensor = None,
                     flow_sign: float = -1.0, alpha: float = 0.01, beta: float = 0.5, want_error: bool = True,
                     want_consistent: bool = True, want_known: bool = True, want_record: bool = True):
    """The forward-backward check of flow `a` against the flow `back` (ofl_flow_consistency_f32): vectors [N,2,H,W]
    fp32 or fp16 as stored, masks [N,H,W] bool or None (all True), `flow_sign` -1 for 's' flows and +1 for 't' flows.  Returns (fp32
    [N,H,W] error, bool [N,H,W] consistent, bool [N,H,W] known, float64 [N,8] records) on the HIP device, None for what is not
    wanted; nothing is read back."""
    lib, dev = _library(), device(a, back)
    n, _, h, w = a.shape
    if not (want_error or want_consistent or want_known or want_record):
        raise ValueError("oflibpytorch_amd: flow_consistency needs at least one output")
    with _on(dev):
        av, abs_, ahalf = _vis_flow(a, dev, n)
        bv, bbs, bhalf = _vis_flow(back, dev, n)
        am, ambs = (None, 0) if a_mask is None else _planes(a_mask, dev, torch.bool, n, "mask")
        bm, bmbs = (None, 0) if back_mask is None else _planes(back_mask, dev, torch.bool, n, "mask of the flow back")
        ws = rec = None
        if want_record:
            nbytes = int(lib.ofl_flow_consistency_workspace_bytes(n, h, w))
            _check(min(nbytes, 0), "ofl_flow_consistency_workspace_bytes")
            ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
            rec = torch.empty((n, RECORD), dtype=torch.float64, device=dev)
        err = torch.empty((n, h, w), dtype=torch.float32, device=dev) if want_error else None
        cons = torch.empty((n, h, w), dtype=torch.bool, device=dev) if want_consistent else None
        known = torch.empty((n, h, w), dtype=torch.bool, device=dev) if want_known else None
        _check(lib.ofl_flow_consistency_f32(_ptr(av), abs_, ahalf, _ptr(bv), bbs, bhalf, _ptr(am), ambs, _ptr(bm), bmbs,
                                            float(flow_sign), float(alpha), float(beta), _ptr(ws), _ptr(err), _ptr(cons), _ptr(known),
                                            _ptr(rec), n, h, w, _stream(dev)), "ofl_flow_consistency_f32")
    return err, cons, known, rec
