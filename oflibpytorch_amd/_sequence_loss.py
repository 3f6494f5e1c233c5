"""ctypes binding of the sequence loss (ofl_sequence_loss.hip; C ABI: include/oflib_hip.h).

A module of its own next to `_native`, whose helpers it uses: it declares the three entry points it calls and allocates the workspace and
the records (`flow_sequence_loss`: two allocations) and one gradient per prediction that wants one (`flow_sequence_loss_grad`) with
`torch.empty` under its own module-level name `torch`, which the dirty-memory tests replace
(tests/test_gpu_sequence_loss_dirty_memory.py).  The loss, the scale of the backward and the statistics are formed from the records by
torch float64 operations on the device.  Nothing is read back.
"""
import ctypes
import math

import torch

from ._native import _check, _on, _planes, _ptr, _stream, _vis_flow, _wants_grad, device, load_library

MAX_T = 32                    # OFL_SEQUENCE_LOSS_MAX_T
CHUNK = 2048                  # OFL_SEQUENCE_LOSS_CHUNK: pixels a block owns
GAMMA, MAX_FLOW = 0.8, 400.0  # RAFT's defaults
PENALTIES = {'l1': 0, 'l2': 1}
NORMALISE = {'all': 0, 'valid': 1}
ERR = "Error scoring flow sequence: "

_declared = None


def _library():
    """libofl_hip.so with the three entry points of this module declared."""
    global _declared
    lib = load_library()
    if _declared is not lib:
        p, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float
        lib.ofl_flow_sequence_loss_workspace_bytes.argtypes = [i32, i32, i32, i32]
        lib.ofl_flow_sequence_loss_workspace_bytes.restype = ctypes.c_int64
        lib.ofl_flow_sequence_loss_f64.argtypes = [p, p, p, i32, p, i64, i32, p, i64, f32, i32, i32, p, p, i32, i32, i32, p]
        lib.ofl_flow_sequence_loss_f64.restype = ctypes.c_int
        lib.ofl_flow_sequence_loss_grad_f32.argtypes = [p, p, p, i32, p, i64, i32, p, i64, f32, i32, i32, p, p, i32, i32, i32, p]
        lib.ofl_flow_sequence_loss_grad_f32.restype = ctypes.c_int
        _declared = lib
    return lib


def record_length(t: int) -> int:
    """doubles per image: count, t sums of the penalty, t sums of the end-point error, the pixels of the last prediction under 1, 3, 5 px"""
    return 2 * t + 4


def check_params(gamma, max_flow, penalty, normalise):
    """The defaults and checks of the four parameters every route shares; returns them as (float, float, str, str)."""
    gamma = GAMMA if gamma is None else gamma
    max_flow = MAX_FLOW if max_flow is None else max_flow
    penalty = 'l1' if penalty is None else penalty
    normalise = 'all' if normalise is None else normalise
    for name, value in (("Gamma", gamma), ("Max_flow", max_flow)):
        if not isinstance(value, (int, float)) or isinstance(value, bool):
            raise TypeError(ERR + name + " needs to be an integer or a float")
    if not (math.isfinite(gamma) and gamma > 0):
        raise ValueError(ERR + "Gamma needs to be finite and larger than 0")
    if not max_flow > 0:                                       # (NaN fails the test; inf passes)
        raise ValueError(ERR + "Max_flow needs to be larger than 0 and not NaN")
    if not isinstance(penalty, str) or penalty not in PENALTIES:
        raise ValueError(ERR + "Penalty needs to be 'l1' or 'l2'")
    if not isinstance(normalise, str) or normalise not in NORMALISE:
        raise ValueError(ERR + "Normalise needs to be 'all' or 'valid'")
    return float(gamma), float(max_flow), penalty, normalise


def check_count(t: int):
    if not 1 <= t <= MAX_T:
        raise ValueError(ERR + "The sequence needs to hold 1 to {} predictions".format(MAX_T))


def _operands(preds, gt, gt_mask, dev, n):
    """(tensors to keep alive until the launch is queued, the arguments of both entry points up to gt_mask_bs): the predictions' device
    pointers, batch strides and storage kinds as host arrays, which the library copies into the kernel arguments."""
    t = len(preds)
    keep, ptrs, strides, halves = [], (ctypes.c_void_p * t)(), (ctypes.c_int64 * t)(), (ctypes.c_int32 * t)()
    for i, pr in enumerate(preds):
        v, vbs, half = _vis_flow(pr, dev, n)
        keep.append(v)
        ptrs[i], strides[i], halves[i] = v.data_ptr(), vbs, half
    g, gbs, ghalf = _vis_flow(gt, dev, n)
    gm, gmbs = (None, 0) if gt_mask is None else _planes(gt_mask, dev, torch.bool, n, "ground-truth mask")
    keep += [g, gm, ptrs, strides, halves]
    return keep, (ptrs, strides, halves, t, _ptr(g), gbs, ghalf, _ptr(gm), gmbs)


def flow_sequence_loss(preds, gt: torch.Tensor, gt_mask: torch.Tensor = None, max_flow: float = MAX_FLOW, penalty: str = 'l1',
                       normalise: str = 'all') -> torch.Tensor:
    """The records of T predictions against one ground truth (ofl_flow_sequence_loss_f64): `preds` a sequence of 1 to 32
    tensors [N,2,H,W] fp32 or fp16 as stored, `gt` likewise, `gt_mask` [N,H,W] bool or None (all True).  Returns float64 [N, 2 T + 4] on
    the HIP device -- count, T sums of the penalty, T sums of the end-point error, the pixels of the last prediction under 1, 3 and 5 px;
    two launches for all T predictions, nothing is read back."""
    lib, dev = _library(), device(gt, *preds)
    n, _, h, w = gt.shape
    t = len(preds)
    with _on(dev):
        keep, args = _operands(preds, gt, gt_mask, dev, n)
        nbytes = int(lib.ofl_flow_sequence_loss_workspace_bytes(t, n, h, w))
        _check(min(nbytes, 0), "ofl_flow_sequence_loss_workspace_bytes")
        ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
        rec = torch.empty((n, record_length(t)), dtype=torch.float64, device=dev)
        _check(lib.ofl_flow_sequence_loss_f64(*args, float(max_flow), PENALTIES[penalty], NORMALISE[normalise], _ptr(ws), _ptr(rec),
                                              n, h, w, _stream(dev)), "ofl_flow_sequence_loss_f64")
    del keep
    return rec


def flow_sequence_loss_grad(preds, gt: torch.Tensor, gt_mask: torch.Tensor, max_flow: float, penalty: str, normalise: str,
                            scale: torch.Tensor, wants):
    """The backward of the sequence loss (ofl_flow_sequence_loss_grad_f32): `scale` fp32 [N,T] on the device (upstream gradient * weight /
    divisor), `wants` one bool per prediction.  Returns a list of T entries: the gradient fp32 [N,2,H,W] on the HIP device, or None where
    not wanted (neither allocated nor written); one launch for all of them."""
    lib, dev = _library(), device(gt, *preds)
    n, _, h, w = gt.shape
    t = len(preds)
    if len(wants) != t or not any(wants):
        raise ValueError("oflibpytorch_amd: flow_sequence_loss_grad needs one flag per prediction and at least one gradient")
    with _on(dev):
        keep, args = _operands(preds, gt, gt_mask, dev, n)
        sc = scale.detach().to(dev, torch.float32).contiguous()
        if tuple(sc.shape) != (n, t):
            raise ValueError("oflibpytorch_amd: the scale of the sequence loss needs the shape [N,T]")
        grads = []
        for want in wants:                    # (a loop, not a comprehension: the allocations are this function's own)
            grads.append(torch.empty((n, 2, h, w), dtype=torch.float32, device=dev) if want else None)
        gptrs = (ctypes.c_void_p * t)(*[None if g is None else g.data_ptr() for g in grads])
        _check(lib.ofl_flow_sequence_loss_grad_f32(*args, float(max_flow), PENALTIES[penalty], NORMALISE[normalise], _ptr(sc), gptrs,
                                                   n, h, w, _stream(dev)), "ofl_flow_sequence_loss_grad_f32")
    del keep, sc
    return grads


def weights_of(t: int, gamma: float):
    """w_i = gamma ** (T - 1 - i), Python floats: the last prediction weighs 1"""
    return [gamma ** (t - 1 - i) for i in range(t)]


_weight_tensors = {}


def _weights_on(t: int, gamma: float, dev) -> torch.Tensor:
    """`weights_of` as a float64 tensor on `dev`, kept: a copy from pageable host memory in every call would make the host wait for the
    kernels queued in front of it"""
    key = (t, gamma, str(dev))
    w = _weight_tensors.get(key)
    if w is None:
        if len(_weight_tensors) >= 64:
            _weight_tensors.clear()
        w = _weight_tensors[key] = torch.tensor(weights_of(t, gamma), dtype=torch.float64, device=dev)
    return w


def divisor_of(rec: torch.Tensor, hw: int, penalty: str, normalise: str) -> torch.Tensor:
    """D_n, float64 [N]: the number of terms of the mean -- 2 H W ('l1') or H W ('l2') under 'all', 2 count or count under 'valid'"""
    per_pixel = 2.0 if penalty == 'l1' else 1.0
    if normalise == 'all':
        return torch.full_like(rec[:, 0], per_pixel * hw)
    return rec[:, 0] * per_pixel


def loss_of(rec: torch.Tensor, hw: int, gamma: float, penalty: str, normalise: str) -> torch.Tensor:
    """loss_n = (float)((sum_i w_i S_{n,i}) / D_n), fp32 [N]: float64 operations on the device of the records, rounded once"""
    t = (rec.shape[1] - 4) // 2
    w = _weights_on(t, gamma, rec.device)
    return ((rec[:, 1:1 + t] * w).sum(dim=1) / divisor_of(rec, hw, penalty, normalise)).to(torch.float32)


def scale_of(g: torch.Tensor, rec: torch.Tensor, hw: int, gamma: float, penalty: str, normalise: str) -> torch.Tensor:
    """scale[n,i] = (float)(g_n w_i / D_n), fp32 [N,T] on the device of the records"""
    t = (rec.shape[1] - 4) // 2
    w = _weights_on(t, gamma, rec.device)
    g = g.to(rec.device, torch.float64)
    return ((g[:, None] * w[None, :]) / divisor_of(rec, hw, penalty, normalise)[:, None]).to(torch.float32)


def stats_of(rec: torch.Tensor, hw: int, gamma: float, penalty: str, normalise: str) -> dict:
    """The dict of Flow.sequence_stats from the records, on their device"""
    t = (rec.shape[1] - 4) // 2
    count = rec[:, 0]
    return {'count': count.to(torch.int64), 'loss': loss_of(rec, hw, gamma, penalty, normalise),
            'weights': _weights_on(t, gamma, rec.device).clone(),
            'terms': rec[:, 1:1 + t] / divisor_of(rec, hw, penalty, normalise)[:, None],
            'epe': rec[:, 1 + t:1 + 2 * t] / count[:, None], 'within': rec[:, 1 + 2 * t:4 + 2 * t] / count[:, None]}


def sequence_loss(preds, gt: torch.Tensor, gt_mask: torch.Tensor = None, gamma: float = GAMMA, max_flow: float = MAX_FLOW,
                  penalty: str = 'l1', normalise: str = 'all') -> torch.Tensor:
    """The sequence loss, fp32 [N].  When autograd is recording and a prediction requires a gradient, the call goes through
    `_autograd.SequenceLossFn`; the ground truth and the mask never carry one."""
    if _wants_grad(*preds):
        from . import _autograd
        return _autograd.SequenceLossFn.apply(gt, gt_mask, gamma, max_flow, penalty, normalise, *preds)
    rec = flow_sequence_loss([pr.detach() for pr in preds], gt.detach(), gt_mask, max_flow, penalty, normalise)
    return loss_of(rec, int(gt.shape[-2]) * int(gt.shape[-1]), gamma, penalty, normalise)


def sequence_stats(preds, gt: torch.Tensor, gt_mask: torch.Tensor = None, gamma: float = GAMMA, max_flow: float = MAX_FLOW,
                   penalty: str = 'l1', normalise: str = 'all') -> dict:
    """The dict of Flow.sequence_stats (`stats_of`) from one pass; never differentiable."""
    rec =flow_sequence_loss([pr.detach() for pr in preds], gt.detach(), gt_mask, max_flow, penalty, normalise)
    return stats_of(rec, int(gt.shape[-2]) * int(gt.shape[-1]), gamma, penalty, normalise)
