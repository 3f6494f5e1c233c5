"""ctypes binding of the composition of a sequence of flows (ofl_chain.hip; C ABI: include/oflib_hip.h).

A module of its own next to `_native`, whose helpers it uses: it declares the entry point it calls and allocates its two outputs with
`torch.empty` under its own module-level name `torch`, which the dirty-memory tests replace (tests/test_gpu_chain_dirty_memory.py).
Nothing is read back.
"""
import ctypes

import torch

from ._native import _check, _on, _planes, _ptr, _stream, _vis_flow, device, load_library

MAX_T = 32                    # OFL_CHAIN_MAX_T
ERR = "Error chaining flows: "

_declared = None


def _library():
    """libofl_hip.so with the entry point of this module declared."""
    global _declared
    lib = load_library()
    if _declared is not lib:
        p, i32, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_float
        lib.ofl_flow_chain_f32.argtypes = [p, p, p, p, p, i32, f32, p, p, i32, i32, i32, i32, p]
        lib.ofl_flow_chain_f32.restype = ctypes.c_int
        _declared = lib
    return lib


def flow_chain(vecs, masks, flow_sign: float = -1.0, want_all: bool = False):
    """The chain of T flows in the order of time (ofl_flow_chain_f32): `vecs` a sequence of 2 to 32 tensors [N,2,H,W]
    fp32 or fp16 as stored, `masks` a sequence of as many tensors [N,H,W] bool or None (all True), `flow_sign` -1 for 's' flows and +1
    for 't' flows.  Returns (fp32 [N,2,H,W] vectors, bool [N,H,W] mask) of the whole chain, or with `want_all` (fp32 [T-1,N,2,H,W],
    bool [T-1,N,H,W]): slot j the chain of the first j + 2 flows ('s') or of the flows from j on ('t').  One launch on the HIP device;
    the device pointers, strides and storage kinds travel as host arrays, which the library copies into the kernel arguments."""
    lib, dev = _library(), device(*vecs)
    t = len(vecs)
    n, _, h, w = vecs[0].shape
    with _on(dev):
        keep = []
        ptrs, strides, halves = (ctypes.c_void_p * t)(), (ctypes.c_int64 * t)(), (ctypes.c_int32 * t)()
        mptrs, mstrides = (ctypes.c_void_p * t)(), (ctypes.c_int64 * t)()
        for i in range(t):
            v, vbs, half = _vis_flow(vecs[i], dev, n)
            m, mbs = (None, 0) if masks[i] is None else _planes(masks[i], dev, torch.bool, n, "mask")
            keep += [v, m]
            ptrs[i], strides[i], halves[i] = v.data_ptr(), vbs, half
            mptrs[i], mstrides[i] = (None if m is None else m.data_ptr()), mbs
        lead = (t - 1,) if want_all else ()
        out = torch.empty(lead + (n, 2, h, w), dtype=torch.float32, device=dev)
        out_mask = torch.empty(lead + (n, h, w), dtype=torch.bool, device=dev)
        _check(lib.ofl_flow_chain_f32(ptrs, strides, halves, mptrs, mstrides, t, float(flow_sign), _ptr(out), _ptr(out_mask),
                                      1 if want_all else 0, n, h, w, _stream(dev)), "ofl_flow_chain_f32")
    del keep
    return out, out_mask
