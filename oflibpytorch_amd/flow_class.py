"""`Flow`: host-side mirror of the reference's flow object for the warp / compose hot path.

Same constructor, properties, operators and method signatures as ``oflibpytorch.Flow`` (reference
``src/oflibpytorch/flow_class.py``; cited per method).  The object is a thin container -- `vecs`
N-2-H-W fp32, `mask` N-H-W bool, `ref` 's'/'t', `device` -- and every warp / splat / composition is
one fused launch of the HIP kernels in ``libofl_hip.so`` (see :mod:`oflibpytorch_amd._native`).

Differences from the reference that do not change results:
  * validation is one fused reduction (finiteness + the four zero tests) per tensor version,
    cached on the object, instead of a pass per predicate per call;
  * an all-True default mask is kept implicit (`None`) until somebody asks for `.mask`;
  * intermediates produced by the kernels are not re-validated eagerly.
"""
import math
import warnings
import weakref
from typing import Tuple, Union

import numpy as np
import torch
import torch.nn.functional as F

from . import (_census, _chain, _consistency, _corr_lookup, _cost_volume, _local_match, _matching, _native, _photometric, _propagate, _sequence_loss,
               _smoothness, _ssim, _upsample, distributed)
from .utils import (get_valid_vecs, get_valid_ref, get_valid_mask, get_valid_device, get_valid_padding,
                    get_valid_shape, get_pure_pytorch, move_axis, from_matrix, from_transforms, resize_flow,
                    apply_flow, _flags_to_host, _host_flags, _griddata_unavailable, track_pts, get_half_flow_outputs,
                    interpolate_bilinear, _mesh_mode)

FlowAlias = 'Flow'
_VALID_THR = 0.99999   # flow_class.py:922
_COMBINE_FUSED = True  # False (tests / tools/bench_combine.py): Flow.combine runs its plan through the public operators, one launch per operator


class _NeverEqual(object):
    """Key component that matches nothing, not even itself: a flag word cached under it is never taken as current."""
    __slots__ = ()

    def __eq__(self, other):
        return False

    def __ne__(self, other):
        return True

    __hash__ = None


# -- the reference's per-call zero / finiteness tests, on demand ---------------------------------------------------------------
# The reference re-computes `is_zero` / `isfinite().all()` inside EVERY apply / combine_with (utils.py:497-498, flow_class.py:
# 1226-1244, 1729-1744).  Here the flag word of a tensor is cached under its version counter, which sees every in-place edit torch
# itself makes -- but not a write through a NumPy array that shares the memory (`torch.from_numpy`), through `.data`, by a foreign
# kernel, or by a c10d in-place collective on the tensor (those leave `_version` alone; `distributed.broadcast_operand` bumps it
# itself).  Two ways to tell the library that such a write happened:
#   * `Flow.invalidate()` drops the cached word of one flow;
#   * `set_revalidate_every_call(True)` makes every PUBLIC call (apply, combine_with, switch_ref, is_zero, ...) start a new epoch
#     that no cached word belongs to: each call looks at its operands again, exactly as the reference does (within a call the words
#     are still shared between the steps of that call).
_reval_on = False
_reval_epoch = 0
_reval_depth = 0


def set_revalidate_every_call(on: bool = True):
    """True: every public `Flow` method re-runs the fused validation / zero-test reduction on the flows it reads (the reference's
    behaviour, utils.py:497-498); False (default): the flag word is cached per tensor version.  Turn it on when flow storage is
    written behind torch's back (NumPy views, `.data`, custom kernels, in-place collectives), or call `Flow.invalidate()`."""
    global _reval_on, _reval_epoch
    _reval_on = bool(on)
    _reval_epoch += 1


def get_revalidate_every_call() -> bool:
    return _reval_on


def _public(fn):
    """Entry point of the public API: with `set_revalidate_every_call(True)` the outermost public call starts a new epoch."""
    import functools

    @functools.wraps(fn)
    def entry(*args, **kwargs):
        global _reval_epoch, _reval_depth
        if not _reval_on:
            return fn(*args, **kwargs)
        if _reval_depth == 0:
            _reval_epoch += 1
        _reval_depth += 1
        try:
            return fn(*args, **kwargs)
        finally:
            _reval_depth -= 1
    return entry


def _ver(t: torch.Tensor, private: bool = False):
    """Version counter of a tensor (see below; the common case is one attribute read).  Inference tensors have none (reading `_version` raises) yet CAN be edited in place inside
    `torch.inference_mode()`: nothing tells an edited one from an untouched one, so their flag words are never cached
    across calls (a FRESH key component that compares unequal to everything -- fresh because tuple comparison short-cuts on
    identity) -- UNLESS the tensor is `private`: a kernel output that only this Flow object has ever held (nobody
    else has a reference through which to edit it; ADVICE r3: inference_mode is the usual deployment mode, and re-running the
    reduction for every kernel output cost a pass and a host wait per call there)."""
    try:
        return t._version
    except RuntimeError:          # "Inference tensors do not track version counter."
        return 0 if private else _NeverEqual()


def _storage_ptr(t):
    try:
        return t.untyped_storage().data_ptr()
    except Exception:  # noqa: BLE001
        return id(t)


_private_flows = weakref.WeakSet()   # the flows whose `_private` is set: kernel outputs that are inference tensors (empty outside inference mode)


def _sharing_ends_privacy(vecs, mask):
    """`vecs` / `mask` are about to be wrapped by another flow object (a copy, a view, a relabelled or negated flow that keeps
    the mask): whoever held their storage privately no longer does -- an in-place edit through the new object must not meet
    the old one's cached flag word.  Costs nothing unless private flows exist (inference mode only)."""
    if not _private_flows:
        return
    ptrs = set(_storage_ptr(t) for t in (vecs, mask) if t is not None)
    for f in list(_private_flows):
        if _storage_ptr(f._fv) in ptrs or (f._mask is not None and _storage_ptr(f._mask) in ptrs):
            f._release_private()


class Flow(object):
    # ------------------------------------------------------------------------------------------
    # construction / properties (flow_class.py:37-236)
    # ------------------------------------------------------------------------------------------
    # -- vector storage -------------------------------------------------------------------------
    # `_vecs` is what the reference holds: N-2-H-W fp32.  A flow handed over as an fp16 tensor on a HIP device (BASELINE
    # config 5) STAYS in fp16 (`_half`): the kernels that take fp16 operands read it directly (ofl_splat_tiled_f16,
    # ofl_warp_bwd_h_f32: exact up-conversion in registers, fp32 arithmetic, the reference's `vecs.float()` of utils.py:95,118
    # without the fp32 copy), and the fp32 tensor is only made when somebody asks for it (`.vecs`, arithmetic, ...).
    @property
    def _vecs(self) -> torch.Tensor:
        if self._v32 is None:
            self._v32 = self._half.float()
        return self._v32

    @_vecs.setter
    def _vecs(self, t: torch.Tensor):
        if t.dtype == torch.float16 and t.device.type == 'cuda':
            self._half, self._v32 = t, None
        else:
            self._half, self._v32 = None, t

    @property
    def _fv(self) -> torch.Tensor:
        """The vectors as stored: fp16 if the flow was handed over (or, by option, produced) in fp16, else fp32."""
        return self._half if self._half is not None else self._v32

    def __init__(self, flow_vectors, ref: str = None, mask=None, device=None):
        self._flag_cache = None
        self._pending_flags = None
        self._mask = None
        self._vecs = get_valid_vecs(flow_vectors, error_string="Error setting flow vectors: ", _check_finite=False,
                                    _keep_half=True)
        self._device = self._fv.device
        try:
            self.ref = ref
            if mask is not None:
                m = get_valid_mask(mask, desired_shape=self.shape, error_string="Error setting flow mask: ")
                self._mask = m.to(self._fv.device)
        except (TypeError, ValueError):
            self._mask = None
            self._from_half()
            self._require_finite("Error setting flow vectors: ")   # the vecs error comes first in the reference
            raise
        self._from_half()
        _sharing_ends_privacy(self._fv, self._mask)
        self._require_finite("Error setting flow vectors: ")
        self.device = device

    def _from_half(self):
        """fp16-stored vectors on a HIP device (BASELINE config 5): the reference's `.float()` (utils.py:95,118) and the
        validation reduction run as one kernel, now that the mask is known."""
        if self._half is not None:
            self._set_pending_flags(_native.flow_flags(self._half, self._mask))     # (flags only: 5 B/px, the flow stays fp16)

    _private = False     # the vectors and the mask are kernel outputs no one else holds (see _ver); cleared when they are handed out

    @classmethod
    def _wrap(cls, vecs: torch.Tensor, ref: str, mask, device=None, flags: torch.Tensor = None,
              like: FlowAlias = None, fresh: bool = False, made_from: tuple = None, borrowed: bool = False) -> FlowAlias:
        """Internal: wrap tensors that are valid by construction (kernel outputs, views of validated flows).
        `flags` is the device-side flag word a kernel produced as a by-product, read lazily.  `fresh`: vecs and mask were
        allocated by the call that produced them; `made_from`: ... unless they share storage with one of these tensors (the
        early exits hand their inputs through).  `borrowed`: a temporary that never leaves the method that makes it (the same
        tensors under another reference): whoever holds them privately still does."""
        obj = cls.__new__(cls)
        obj._vecs, obj._ref, obj._mask = vecs, ref, mask
        obj._device = vecs.device if device is None else device
        obj._flag_cache, obj._pending_flags = None, None
        if made_from is not None:
            theirs = set(_storage_ptr(t) for t in made_from if t is not None)
            fresh = _storage_ptr(vecs) not in theirs and (mask is None or _storage_ptr(mask) not in theirs)
        if not fresh and not borrowed:
            _sharing_ends_privacy(vecs, mask)
        elif vecs.is_inference():                # (only inference tensors need it: the others carry version counters)
            obj._private = True
            _private_flows.add(obj)
        if obj._fv.device != obj._device:
            obj._vecs = obj._fv.to(obj._device)
        if obj._mask is not None and obj._mask.device != obj._device:
            obj._mask = obj._mask.to(obj._device)
        if flags is not None:
            obj._set_pending_flags(flags)
        if like is not None:
            obj._inherit_flags(like)
        return obj

    def _inherit_flags(self, src: FlowAlias):
        """`self` holds the vectors of `src` or their exact negation, under the same mask: every flag (finiteness, the
        symmetric zero / threshold tests) carries over, no reduction needed."""
        if src._flags_known() and (self._mask is src._mask):
            key = self._key()
            self._flag_cache = (key, src._flag_cache[1])

    def _negated(self, ref: str) -> FlowAlias:
        return Flow._wrap(self._vecs * -1.0, ref, self._mask, self._device, like=self)

    @classmethod
    def _deferred(cls, flow_vectors, ref: str = None, mask=None, device=None) -> FlowAlias:
        """Internal: like the public constructor (same structural checks and errors) but the finiteness test is not
        run yet -- the first kernel that reads the vectors produces the flag word as a by-product and the same
        ValueError is raised then (tensor-level wrappers: the error surfaces inside the same call)."""
        obj = cls.__new__(cls)
        obj._flag_cache, obj._pending_flags, obj._mask = None, None, None
        obj._vecs = get_valid_vecs(flow_vectors, error_string="Error setting flow vectors: ", _check_finite=False)
        obj._device = obj._vecs.device
        obj.ref = ref
        if mask is not None:
            m = get_valid_mask(mask, desired_shape=obj.shape, error_string="Error setting flow mask: ")
            obj._mask = m.to(obj._vecs.device)
        obj.device = device
        return obj

    def _key(self) -> tuple:
        """Cache key of the flag word: tensor versions (in-place edits invalidate it).  Tensors created under
        torch.inference_mode() carry no version counter: their key never matches, i.e. every call that needs the flags of
        such a flow runs the (cheap, fused) reduction again -- an in-place edit inside inference mode must not meet a
        stale 'all zero' / 'finite' word."""
        return (_ver(self._fv, self._private), None if self._mask is None else (id(self._mask), _ver(self._mask, self._private)), _reval_epoch)

    def _flags_known(self) -> bool:
        key = self._key()
        return self._flag_cache is not None and self._flag_cache[0] == key

    # -- flags: finiteness + zero tests, one fused reduction per tensor version ------------------
    def _flags(self) -> list:
        key = self._key()
        if self._flag_cache is None or self._flag_cache[0] != key:
            dev_flags = None
            if self._pending_flags is not None and self._pending_flags[0] == key:
                dev_flags = self._pending_flags[1]
            self._pending_flags = None
            sharded = distributed.is_enabled()
            if dev_flags is None and (not sharded or distributed.host_exchange_active()):
                # a tensor nobody has looked at yet (the constructor's validation): reduction + read-back in one launch.
                # Batch sharding on one node: the same launch, then the OR of the batch word over the ranks through
                # shared memory (distributed._HostExchange) -- the sharded wait is the unsharded one plus microseconds
                words = _host_flags(self._fv, self._mask)
                self._flag_cache = (key, words)
                if sharded:
                    local = 0
                    for f in words:
                        local |= f
                    self._flag_cache = (key, words, (True, distributed.reduce_flags(local, self._fv.device)))
                return self._flag_cache[1]
            if dev_flags is None:
                dev_flags = _native.flow_flags(self._fv, self._mask)
            if sharded and distributed.host_exchange_active():
                words = _flags_to_host(dev_flags)                     # (a kernel's by-product words: copy + polled event)
                local = 0
                for f in words:
                    local |= f
                self._flag_cache = (key, words, (True, distributed.reduce_flags(local, self._fv.device)))
            elif sharded:
                # batch sharding: the OR over every rank's shard is formed on the device (one small all-reduce) and read
                # together with the local words -- one host sync per tensor version, as without sharding
                words, glob = distributed.split_global_or(_flags_to_host(distributed.with_global_or(dev_flags)))
                self._flag_cache = (key, words, (True, glob))
            else:
                self._flag_cache = (key, _flags_to_host(dev_flags))
        return self._flag_cache[1]

    def _set_pending_flags(self, dev_flags):
        if dev_flags is not None:
            key = self._key()
            self._pending_flags = (key, dev_flags)

    def _batch_flags(self) -> int:
        """OR of the flag words over the whole batch -- over every rank's shard when batch sharding is on
        (the reference's early exits are batch-global, distributed.py)."""
        flags = self._flags()
        if len(self._flag_cache) < 3 or self._flag_cache[2][0] != distributed.is_enabled():
            local = 0
            for f in flags:
                local |= f
            glob = distributed.reduce_flags(local, self._fv.device)
            self._flag_cache = (self._flag_cache[0], self._flag_cache[1], (distributed.is_enabled(), glob))
        return self._flag_cache[2][1]

    def invalidate(self) -> FlowAlias:
        """Forget what is known about the vectors (finite / all zero / below the threshold, plain and under the mask): the next call
        that needs it looks again.  For writes torch's version counter does not see -- a NumPy array sharing the memory
        (`torch.from_numpy`), `tensor.data`, a custom kernel, an in-place collective on the tensor.  The reference needs no such call
        because it runs the tests inside every apply / combine_with (utils.py:497-498, flow_class.py:1226-1244); see also
        `set_revalidate_every_call`.  Returns the flow itself."""
        self._flag_cache, self._pending_flags = None, None
        return self

    def _require_finite(self, error_string: str):
        if self._batch_flags() & _native.FLAG_NONFINITE:                              # utils.py:98
            raise ValueError(error_string + "Input contains NaN, Inf or -Inf values")

    def _all_zero(self, bit: int) -> bool:
        return not (self._batch_flags() & bit)

    @property
    def vecs(self) -> torch.Tensor:
        """Flow vectors N-2-H-W, fp32 (flow_class.py:68-80).  As in the reference the tensor handed out IS the flow's
        storage: an in-place edit of it edits the flow.  A flow kept in fp16 (`_half`) therefore gives up its fp16 planes
        the moment its fp32 tensor is handed out -- from then on there is one store, the fp32 one, and the kernels read
        that (the flag word carries over: the up-conversion is exact; a later in-place edit bumps the tensor's version and
        invalidates it like any other)."""
        v = self._vecs
        self._release_private()
        if self._half is not None:
            flags = self._flag_cache[1:] if self._flags_known() else None
            pending = self._pending_flags[1] if (self._pending_flags is not None and self._pending_flags[0] == self._key()) else None
            self._half = None
            self._flag_cache = None if flags is None else (self._key(),) + tuple(flags)
            self._pending_flags = None if pending is None else (self._key(), pending)
        return v

    @vecs.setter
    def vecs(self, input_vecs):
        v = get_valid_vecs(input_vecs, error_string="Error setting flow vectors: ", _check_finite=False)
        old = self._vecs
        # the caller's tensor may be stored as it is (an fp32 tensor on the device passes through get_valid_vecs): a flow
        # that was private to its object is not any more, so an inference tensor's key must stop matching
        self._release_private()
        self._vecs, self._flag_cache, self._pending_flags = v, None, None
        try:
            self._require_finite("Error setting flow vectors: ")
        except ValueError:
            self._vecs, self._flag_cache = old, None
            raise

    @property
    def vecs_numpy(self) -> np.ndarray:
        """N-H-W-2 float32 numpy view of the vectors (flow_class.py:95-110)"""
        self._release_private()               # (a CPU-resident flow hands out shared memory here)
        return np.moveaxis(self._vecs.detach().cpu().numpy(), 1, -1)

    @property
    def ref(self) -> str:
        """'s' (source) or 't' (target) reference (flow_class.py:112-148)"""
        return self._ref

    @ref.setter
    def ref(self, input_ref: str = None):
        self._ref = get_valid_ref(input_ref)

    @property
    def mask(self) -> torch.Tensor:
        """Validity mask N-H-W bool (flow_class.py:159-172).  An all-True default is materialised on first use."""
        if self._mask is None:
            self._mask = torch.ones(self.shape, dtype=torch.bool, device=self._fv.device)
            self._flag_cache = None if self._flag_cache is None else (self._key(), self._flag_cache[1])
        self._release_private()
        return self._mask

    def _release_private(self):
        """The storage is about to be handed out: from now on somebody else can edit it in place.  Tensors that track versions
        keep their key (an edit bumps it); an inference tensor's key stops matching, so its next use runs the reduction again."""
        if self._private:
            self._private = False
            _private_flows.discard(self)

    @mask.setter
    def mask(self, input_mask=None):
        self._release_private()               # (the caller's mask may be stored as it is: see the vecs setter)
        if input_mask is None:
            self._mask = None
        else:
            m = get_valid_mask(input_mask, desired_shape=self.shape, error_string="Error setting flow mask: ")
            self._mask = m.to(self._fv.device)
        self._flag_cache, self._pending_flags = None, None

    @property
    def mask_numpy(self) -> np.ndarray:
        """flow_class.py:188-205"""
        return self.mask.detach().cpu().numpy()

    @property
    def device(self) -> torch.device:
        """flow_class.py:207-213"""
        return self._device

    @device.setter
    def device(self, input_device=None):
        device = self._fv.device if input_device is None else get_valid_device(input_device)
        self._device = device
        if self._fv.device != device or (self._mask is not None and self._mask.device != device):
            self._release_private()           # storage is replaced: the privacy of the old tensors says nothing about the new ones
        if self._fv.device != device:
            self._vecs = self._fv.to(device) if device.type == 'cuda' else self._vecs.to(device)
            self._flag_cache = None if self._flag_cache is None else \
                ((_ver(self._fv),) + tuple(self._flag_cache[0][1:]), self._flag_cache[1])
        if self._mask is not None and self._mask.device != device:
            flags = None if self._flag_cache is None else self._flag_cache[1]
            self._mask = self._mask.to(device)
            if flags is not None:
                self._flag_cache = (self._key(), flags)

    @property
    def shape(self) -> tuple:
        """(N, H, W) (flow_class.py:228-236)"""
        return (self._fv.shape[0],) + tuple(self._fv.shape[2:])

    @classmethod
    def zero(cls, shape, ref: str = None, mask=None, device=None) -> FlowAlias:
        """All-zero flow of shape (H, W) or (N, H, W) (flow_class.py:238-258)"""
        dims = get_valid_shape(shape)
        return cls(torch.zeros(dims[0], 2, dims[1], dims[2]), ref, mask, device)

    @classmethod
    def from_matrix(cls, matrix, shape, ref: str = None, mask=None, device=None, matrix_is_inverse: bool = None) -> FlowAlias:
        """flow_class.py:260-292"""
        device = get_valid_device(device) if device is not None else None
        on = device if (device is not None and device.type == 'cuda') else None        # generate the field where it is wanted
        return cls(from_matrix(matrix, shape, ref, matrix_is_inverse, _device=on), ref, mask, device)

    @classmethod
    def from_transforms(cls, transform_list: list, shape, ref: str = None, mask=None, device=None,
                        padding: list = None) -> FlowAlias:
        """flow_class.py:294-328"""
        device = get_valid_device(device) if device is not None else None
        on = device if (device is not None and device.type == 'cuda') else None
        return cls(from_transforms(transform_list, shape, ref, padding, _device=on), ref, mask, device)

    @classmethod
    def from_matching(cls, feat, other, ref: str = None, mask=None, return_prob: bool = None):
        """The flow between two frames by global matching of their features, as in GMFlow, UniMatch and the matching heads of tracking
        and stereo networks: `feat` and `other` are float32 tensors of one shape, C-H-W or N-C-H-W -- or both float16 or both bfloat16,
        as a network under autocast has them (below).  For every pixel p of `feat` the
        softmax over ALL positions q of `other` of feat(p) . other(q) / sqrt(C) gives the expected position of its match; the vector
        of an 's' flow at p is that position minus p, the vector of a 't' flow (the default `ref`) its negation, with the meaning the
        reference has in `Flow.corr_lookup`.  Returns a flow of shape N-H-W on the features' device with `mask` handed to the constructor
        unchanged; with `return_prob` True a tuple of that flow and the matching probability, float32 N-H-W: the softmax weight of the
        best match of every pixel, the value GMFlow returns as `prob`.  One launch of ofl_matching.hip that streams `other` past tiles of
        pixels with a running maximum and three running float64 sums per pixel: the (H W)^2 volume is never formed and no logit is
        written to memory; every sum has a fixed order, bitwise reproducible and independent of the batch.
        Differentiable with respect to `feat` and `other`, by kernels that recompute the logits, without atomics;
        NOT through the probability.  Two float16 or two bfloat16 tensors take ofl_matching_x16.hip: the logits are
        formed on the matrix cores from the 16-bit values (products exact, float32 sums in the hardware's order), the weights are
        float32 exponentials, summed in float32 inside a chunk of the walk and in float64 across chunks; the flow and the probability
        are float32 as before and agree with the float64 evaluation within the bar DESIGN.md 4 derives, not bit for bit with the
        float32 route; the gradients come from the float32 gradient kernels on transient up-conversions and are rounded once to the
        features' dtype.  A mixed pair of dtypes, channels_last features, a mask over the positions of `other`, a local window,
        another temperature and the 1-D variant are not supported."""
        err = "Error matching flow: "
        for name, ft in (("Feat", feat), ("Other", other)):
            if not isinstance(ft, torch.Tensor):
                raise TypeError(err + name + " needs to be a torch tensor")
            if ft.dtype not in (torch.float32, torch.float16, torch.bfloat16):
                raise TypeError(err + name + " needs to be of dtype float32, float16 or bfloat16")
        if feat.dtype != other.dtype:
            raise TypeError(err + "Feat and other need to be both float32, both float16 or both bfloat16, not a mixed pair")
        return_prob = False if return_prob is None else return_prob
        if not isinstance(return_prob, bool):
            raise TypeError(err + "Return_prob needs to be boolean")
        if feat.dim() not in (3, 4):
            raise ValueError(err + "Feat needs to have 3 or 4 dimensions, C-H-W or N-C-H-W")
        if tuple(feat.shape) != tuple(other.shape):
            raise ValueError(err + "Feat and other need to have the same shape")
        if min(feat.shape) < 1:
            raise ValueError(err + "Feat and other must not be empty")
        if ref is not None and (not isinstance(ref, str) or ref not in ('s', 't')):
            raise ValueError(err + "Ref needs to be 's' or 't', but got {}".format(ref))
        ref = 't' if ref is None else ref
        if other.device != feat.device:
            other = other.to(feat.device)                   # (keeps its grad_fn)
        out, prob = _matching.global_match(feat, other, -1.0 if ref == 's' else 1.0, return_prob)
        flow = cls(out, ref, mask, device=feat.device)
        return (flow, prob.to(feat.device)) if return_prob else flow

    @classmethod
    def from_kitti(cls, path, load_valid: bool = None, device=None) -> FlowAlias:
        """flow_class.py:330-355: the flow of a KITTI ``uint16`` .png file as an 's' flow, the valid pixels as its mask unless
        `load_valid` is False.  The file's raw samples are decoded on the HIP device by one kernel that also leaves the flag word,
        so no validation pass follows.  Extension: `path` may be a list / tuple of paths of equally sized
        frames, which come back as one N-batch flow from one launch."""
        load_valid = True if load_valid is None else load_valid
        if not isinstance(load_valid, bool):
            raise TypeError("Error loading flow from KITTI data: Load_valid needs to be boolean")
        device = get_valid_device(device) if device is not None else torch.device('cpu')
        from . import _loaders
        vecs, mask, flags, _ = _loaders.kitti(path, load_valid)
        return cls._wrap(vecs, 's', mask, device, flags=flags, fresh=True)

    @classmethod
    def from_sintel(cls, path, inv_path=None, device=None) -> FlowAlias:
        """flow_class.py:357-374: the flow of a Sintel .flo file as an 's' flow; with `inv_path` the mask is False where that
        .png's grey value is non-zero.  Decoded as `from_kitti`; NaN / Inf in the file raise the constructor's ValueError.
        Extension: `path` (and `inv_path`) may be lists / tuples of equal length."""
        device = get_valid_device(device) if device is not None else torch.device('cpu')
        from . import _loaders
        vecs, mask, flags, _, mask_error = _loaders.sintel(path, inv_path)
        flow = cls._wrap(vecs, 's', mask, device, flags=flags, fresh=True)
        flow._require_finite("Error setting flow vectors: ")
        if mask_error is not None:                # (after the vectors' own error, as in the constructor)
            raise ValueError(mask_error)
        return flow

    # ------------------------------------------------------------------------------------------
    # copies, indexing (flow_class.py:376-448)
    # ------------------------------------------------------------------------------------------
    def copy(self) -> FlowAlias:
        """flow_class.py:376-383.  The copy aliases the same (already validated) tensors: its flag word is inherited
        instead of recomputed (no launch, no host sync)."""
        return Flow._wrap(self._fv, self._ref, self._mask, self._device, like=self)

    def to_device(self, device) -> FlowAlias:
        device = get_valid_device(device)
        return Flow(self._vecs.to(device), self._ref, None if self._mask is None else self._mask.to(device), device)

    def __str__(self) -> str:
        return "Flow object, reference {}, batch size {}, shape {}*{}, device {}; ".format(
            self._ref, *self.shape, self._device) + self.__repr__()

    def select(self, item: int = None) -> FlowAlias:
        if item is None:
            return self
        if not isinstance(item, int):
            raise TypeError("Error selecting from flow object: item needs to be an integer")
        try:
            return self._subset(self._vecs[item], self.mask[item])
        except IndexError:
            raise IndexError("Error selecting from flow object: item {} out of bounds for flow with batch size {}"
                             .format(item, self.shape[0]))

    def __getitem__(self, item) -> FlowAlias:
        # index H, W (then N, 2) the way a tensor of shape H-W-N-2 would be indexed (flow_class.py:433-448)
        vecs = self._vecs.permute(2, 3, 0, 1).__getitem__(item).permute(2, 3, 0, 1)
        mask = self.mask.permute(1, 2, 0).__getitem__(item).permute(2, 0, 1)
        return self._subset(vecs, mask)

    def _subset(self, vecs: torch.Tensor, mask: torch.Tensor) -> FlowAlias:
        """A slice of this (validated) flow as a flow object: the constructor's shape checks (flow_class.py:60-99) without its
        finiteness reduction -- a subset of finite values is finite (no kernel launch, no host sync)."""
        v = get_valid_vecs(vecs, error_string="Error setting flow vectors: ", _check_finite=False)
        m = get_valid_mask(mask, desired_shape=(v.shape[0], v.shape[2], v.shape[3]), error_string="Error setting flow mask: ")
        return Flow._wrap(v, self._ref, m, self._device)

    # ------------------------------------------------------------------------------------------
    # arithmetic (flow_class.py:450-692)
    # ------------------------------------------------------------------------------------------
    def _binary_operand(self, other, verb_ing: str, names: tuple):
        if isinstance(other, (np.ndarray, torch.Tensor)):
            ov = get_valid_vecs(other, desired_shape=self.shape, error_string="Error adding to flow: ")
            om = None
        elif isinstance(other, Flow):
            ov, om = other._vecs, other._mask
        else:
            raise TypeError("Error {}: {} is not a flow object, numpy array, or torch tensor".format(verb_ing, names[0]))
        if self.shape[0] != ov.shape[0] and self.shape[0] != 1 and ov.shape[0] != 1:
            raise ValueError("Error {}: {} batch dimensions don't match, and neither is 1".format(verb_ing, names[1]))
        if self.shape[1:] != tuple(ov.shape[2:]):
            raise ValueError("Error {}: {} flow objects are not the same shape".format(verb_ing, names[1]))
        return ov.to(self._device), (None if om is None else om.to(self._device))

    def _and_masks(self, other_mask):
        if self._mask is None and other_mask is None:
            return None
        if self._mask is None:
            return other_mask if other_mask.shape[0] >= self.shape[0] else other_mask.expand(self.shape).clone()
        if other_mask is None:
            return self._mask
        return self._mask & other_mask

    def __add__(self, other) -> FlowAlias:
        """Vector sum, masks ANDed -- not a composition (flow_class.py:450-488)"""
        ov, om = self._binary_operand(other, "adding to flow", ("Addend", "Augend and addend"))
        vecs = self._vecs + ov
        mask = self._and_masks(om)
        if mask is not None and mask.shape[0] != vecs.shape[0]:
            mask = mask.expand(vecs.shape[0], -1, -1)
        return Flow._wrap(vecs, self._ref, mask, self._device)

    def __sub__(self, other) -> FlowAlias:
        """flow_class.py:490-531"""
        ov, om = self._binary_operand(other, "subtracting from flow", ("Subtrahend", "Minuend and subtrahend"))
        vecs = self._vecs - ov
        mask = self._and_masks(om)
        if mask is not None and mask.shape[0] != vecs.shape[0]:
            mask = mask.expand(vecs.shape[0], -1, -1)
        return Flow._wrap(vecs, self._ref, mask, self._device)

    def _scalar_or_field(self, other, verb_ing: str, noun: str):
        """Operand of * / **: number, list of 2, or array of shape 2, H-W, 2-H-W, H-W-2, N-2-H-W."""
        try:
            return float(other)
        except (TypeError, ValueError):
            pass
        if isinstance(other, list):
            if len(other) != 2:
                raise ValueError("Error {} flow: {} list not length 2".format(verb_ing, noun))
            other = torch.tensor(other)
        elif isinstance(other, np.ndarray):
            other = torch.tensor(other)
        if not isinstance(other, torch.Tensor):
            raise TypeError("Error {} flow: {} cannot be converted to float, or isn't a list, numpy array, or torch "
                            "tensor".format(verb_ing, noun))
        hw = self.shape[1:]
        if other.dim() == 1 and other.shape[0] == 2:
            other = other.view(1, 2, 1, 1)
        elif other.dim() == 2 and tuple(other.shape) == hw:
            other = other.view(1, 1, *hw)
        elif other.dim() == 3 and tuple(other.shape) == (2,) + hw:
            other = other.unsqueeze(0)
        elif other.dim() == 3 and tuple(other.shape) == hw + (2,):
            other = move_axis(other, -1, 0).unsqueeze(0)
        elif other.dim() == 4 and tuple(other.shape[2:]) == hw and other.shape[1] == 2 and \
                (self.shape[0] == 1 or other.shape[0] == 1 or self.shape[0] == other.shape[0]):
            pass
        else:
            raise ValueError("Error {} flow: {} array or tensor needs to be of size 2, of the shape of the flow object "
                             "(H-W), or 2-H-W or H-W-2, or N-2-H-W".format(verb_ing, noun))
        return other.to(self._device)

    def _result_of(self, vecs) -> FlowAlias:
        mask = self._mask
        if mask is not None and vecs.shape[0] != self.shape[0]:
            mask = mask.repeat(vecs.shape[0], 1, 1)
        return Flow(vecs, self._ref, mask, self._device)

    def __mul__(self, other) -> FlowAlias:
        """flow_class.py:533-580"""
        o = self._scalar_or_field(other, "multiplying", "Multiplier")
        if isinstance(o, float):
            if o == -1.0 or o == 1.0:
                return Flow._wrap(self._vecs * o, self._ref, self._mask, self._device, like=self)
            return Flow._wrap(self._vecs * o, self._ref, self._mask, self._device) if np.isfinite(o) \
                else Flow(self._vecs * o, self._ref, self._mask, self._device)
        return self._result_of(self._vecs * o)

    def __truediv__(self, other) -> FlowAlias:
        """flow_class.py:582-629.  A Python-number divisor is handed to ATen as a DEVICE scalar tensor: with a host scalar
        ATen's GPU kernel multiplies by the reciprocal instead of dividing, which differs from the reference's (CPU) quotient
        in the last bit for a third of the values; tensor / tensor is the correctly rounded division on either device."""
        o = self._scalar_or_field(other, "dividing", "Divisor")
        if isinstance(o, float) and self._vecs.device.type == 'cuda':
            o = torch.tensor(o, dtype=self._vecs.dtype, device=self._vecs.device)
        return self._result_of(self._vecs / o)

    def __pow__(self, other) -> FlowAlias:
        """flow_class.py:631-678"""
        return self._result_of(self._vecs ** self._scalar_or_field(other, "exponentiating", "Exponent"))

    def __neg__(self) -> FlowAlias:
        """flow_class.py:680-692"""
        return self * -1

    # ------------------------------------------------------------------------------------------
    # resize / pad (flow_class.py:694-753) -- thin PyTorch wrappers, not on the kernel path
    # ------------------------------------------------------------------------------------------
    def resize(self, scale) -> FlowAlias:
        """flow_class.py:694-714: bilinear interpolation (`align_corners=False`) of the vectors (scaled along) and of the mask
        (then rounded).  On a HIP device `ofl_resize_bilinear_f32` restates the arithmetic of ATen's CPU kernels, so the result is
        the reference's PyTorch-CPU result bit for bit; on the host it is ATen itself.  The mask goes through the reference's own
        `.squeeze(0).squeeze(0)`, so -- exactly like the reference -- a batch of more than one flow raises the mask's shape error."""
        resized = resize_flow(self._vecs, scale)
        sc = [scale, scale] if isinstance(scale, (float, int)) else scale
        m = interpolate_bilinear(self.mask.float().unsqueeze(1), sc).squeeze(0).squeeze(0)
        return Flow(resized, self._ref, torch.round(m), device=self._device)

    def pad(self, padding: list = None, mode: str = None) -> FlowAlias:
        mode = 'constant' if mode is None else mode
        if mode not in ('constant', 'reflect', 'replicate'):
            raise ValueError("Error padding flow: Mode should be one of "
                             "'constant', 'reflect', or 'replicate', but instead got '{}'".format(mode))
        padding = get_valid_padding(padding, "Error padding flow: ")
        lrtb = (padding[2], padding[3], padding[0], padding[1])
        return Flow._wrap(F.pad(self._vecs, lrtb, mode=mode), self._ref,
                          F.pad(self.mask.unsqueeze(1), lrtb).squeeze(1), self._device)

    def unpad(self, padding: list = None) -> FlowAlias:
        padding = get_valid_padding(padding, "Error padding flow: ")
        h, w = self.shape[1:3]
        if sum(padding[0:2]) > h - 1 or sum(padding[2:4]) > w - 1:
            raise ValueError("Error unpadding flow: one or more dimensions cut to zero or less")
        return self[padding[0]:h - padding[1], padding[2]:w - padding[3]]

    # ------------------------------------------------------------------------------------------
    # apply (flow_class.py:755-959)
    # ------------------------------------------------------------------------------------------
    def apply(self, target, target_mask: torch.Tensor = None, return_valid_area: bool = None,
              consider_mask: bool = None, padding: list = None, cut: bool = None):
        """Warp `target` (tensor H-W / C-H-W / N-C-H-W, or a Flow) with this flow.  One fused kernel launch: the
        target's mask rides along as an extra channel, is thresholded at 0.99999 and ANDed with the flow mask in
        the same pass (reference: cat + apply_flow + gt + and, flow_class.py:896-934)."""
        return_valid_area = False if return_valid_area is None else return_valid_area
        if not isinstance(return_valid_area, bool):
            raise TypeError("Error applying flow: Return_valid_area needs to be a boolean")
        consider_mask = True if consider_mask is None else consider_mask
        if not isinstance(consider_mask, bool):
            raise TypeError("Error applying flow: Consider_mask needs to be a boolean")
        cut = True if cut is None else cut
        if not isinstance(cut, bool):
            raise TypeError("Error applying flow: Cut needs to be a boolean")
        if padding is not None:
            padding = get_valid_padding(padding, "Error applying flow: ")
            if self.shape[1] + padding[0] + padding[1] != target.shape[-2] or \
                    self.shape[2] + padding[2] + padding[3] != target.shape[-1]:
                raise ValueError("Error applying flow: Padding values do not match flow and target shape difference")

        return_dtype, return_2d, return_3d = torch.float, False, False
        if isinstance(target, Flow):
            return_flow = True
            t, tmask = target._fv, target._mask
        elif isinstance(target, torch.Tensor):
            return_flow = False
            if target.dim() == 4:
                t = target
            elif target.dim() == 3:
                t, return_3d = target.unsqueeze(0), True
            elif target.dim() == 2:
                t, return_2d = target.unsqueeze(0).unsqueeze(0), True
            else:
                raise ValueError("Error applying flow: Target needs to have the shape H-W (2 dimensions)"
                                 ", C-H-W (3 dimensions), or N-C-H-W (4 dimensions)")
            tmask = None
            if target_mask is not None:
                if not isinstance(target_mask, torch.Tensor):
                    raise TypeError("Error applying flow: Target_mask needs to be a torch tensor")
                if target_mask.dim() == 2:
                    target_mask = target_mask.unsqueeze(0)
                if tuple(target_mask.shape) != (t.shape[0],) + tuple(t.shape[2:]):
                    raise ValueError("Error applying flow: Target_mask needs to match the target shape")
                if target_mask.dtype != torch.bool:
                    raise TypeError("Error applying flow: Target_mask needs to have dtype 'bool'")
                if not return_valid_area:
                    warnings.warn("Warning applying flow: a mask is passed, but return_valid_area is False - so the "
                                  "mask passed will not affect the output, but possibly make the function slower.")
                tmask = target_mask
            return_dtype = target.dtype
        else:
            raise TypeError("Error applying flow: Target needs to be either a flow object or a torch tensor")
        need_valid = return_flow or return_valid_area

        rm = _native.ROUND_NONE
        if not return_flow and not return_dtype.is_floating_point:
            rm = _native.ROUND_U8 if return_dtype == torch.uint8 else _native.ROUND_RINT
        if padding is None:
            if tuple(target.shape[-2:]) != self.shape[-2:]:
                raise ValueError("Error applying flow: Flow and target have to have the same shape")
            warped, valid, dflags = self._warp(t, tmask, need_valid, consider_mask, rm, keep16=not return_flow)
        else:
            warped, valid, dflags = self._warp_padded(t, tmask, need_valid, consider_mask, rm, padding)

        if padding is not None and not cut and need_valid and self._ref == 't' and warped.shape[0] < self.shape[0]:
            # an all-zero 't' flow of batch N, padded and NOT cut, over a batch-1 target: the reference's mask is still batch 1 (the target
            # went through apply_flow untouched, utils.py:497-498) when it assigns the batch-N `tmp & self._mask` into its flow-area
            # window (flow_class.py:929-932) -- torch refuses, with this message (found by tests/golden/fuzz_vs_reference.py)
            raise RuntimeError("The expanded size of the tensor (%d) must match the existing size (%d) at non-singleton dimension 0.  "
                               "Target sizes: [%d, %d, %d].  Tensor sizes: [%d, %d, %d]"
                               % (warped.shape[0], self.shape[0], warped.shape[0], self.shape[1], self.shape[2], self.shape[0], self.shape[1], self.shape[2]))
        if padding is not None and cut:
            win = (slice(padding[0], padding[0] + self.shape[1]), slice(padding[2], padding[2] + self.shape[2]))
            warped = warped[..., win[0], win[1]]
            if valid is not None:
                valid = valid[..., win[0], win[1]]
            dflags = None                                # (they describe the whole padded frame)

        if return_flow:
            if valid is not None and valid.shape[0] != warped.shape[0]:
                # an all-zero 't' flow of batch N over a batch-1 Flow target: apply_flow hands the batch-1 target through
                # (utils.py:497-498) while the mask is ANDed with this flow's N masks (:934) -- the reference's Flow(...) of the two
                # (:938) then fails in its mask setter, with this message (found by tests/golden/fuzz_vs_reference.py)
                raise ValueError("Error setting flow mask: Input shape does not match the desired shape")
            return Flow._wrap(warped, target._ref, valid, self._device, flags=dflags, made_from=(t, tmask, self._mask))
        if not return_dtype.is_floating_point:
            if not get_pure_pytorch():
                warped = warped.to(return_dtype)         # PURE_PYTORCH keeps the rounded values as floats (:943-949)
        else:
            warped = warped.to(return_dtype)
        if (return_2d or return_3d) and warped.shape[0] == 1:
            warped = warped[0, 0] if return_2d else warped[0]
        return (warped, valid) if return_valid_area else warped

    def _warp_padded(self, t: torch.Tensor, tmask, need_valid: bool, consider_mask: bool, round_mode: int, padding: list):
        """`apply` with a target larger than the flow by `padding` (flow_class.py:830-834, 880-895, 901-913, 924-932): the
        reference pads the flow to the target's size first -- zeros for 't', replicated border for 's', mask False -- and
        warps the whole frame.  Here the kernels read the un-padded flow through a window (`ofl_warp_bwd_win_f32`,
        `ofl_splat_tiled_win_f32`): no padded copy of the flow or its mask is made.  The all-zero early exit, narrow frames
        the gather kernels do not take, and tensors that want a gradient go through the padded copy (rare / plumbing)."""
        window = (padding[0], padding[2])
        # The reference's padded 's' branch walks the TARGET's batch (flow_class.py:884-894: `for i in range(mask.shape[0])`): with a
        # batch-1 target under a batch-N flow it ANDs element 0's flow mask -- and only that one -- into the mask channel, which every
        # element of the flow then warps; and because `mask` keeps batch 1 the target is not expanded (:896-897), so an all-zero flow
        # hands the batch-1 target (and that batch-1 mask) straight through (utils.py:497-498).  Reproduced: results are what the
        # reference returns on the same inputs, quirk included (fixtures tests/golden/padbc.npz).
        quirk = self._ref == 's' and need_valid and t.shape[0] < self.shape[0]
        chan_b = self._mask if not quirk else self.mask[:1]
        direct = not self._all_zero(_native.FLAG_NZ_THR) and \
            not _native._wants_grad(self._vecs, t) and (self._ref == 't' or get_pure_pytorch())
        if direct:
            self._require_finite("Error applying flow to a target: ")
            if self._ref == 't':
                warped, valid = _native.warp_bwd_win(self._vecs, t, window, src_mask=tmask,
                                                     flow_mask=self._mask if need_valid else None, want_valid=need_valid,
                                                     round_mode=round_mode)
                return warped.to(self._device), (None if valid is None else valid.to(self._device)), None
            res = _native.splat_fwd_win(self._vecs, t, window, weight_mask=self.mask if consider_mask else None,
                                        chan_mask_a=tmask, chan_mask_b=chan_b, want_valid=need_valid, occlude=True,
                                        round_mode=round_mode)
            if res is not None:
                return res[0].to(self._device), (None if res[1] is None else res[1].to(self._device)), None
        # 't': zero padding is irrelevant outside the flow area; 's': replicate avoids artefacts at the border of the flow area
        # (flow_class.py:906-913).  The padded mask is False, so the un-padded formulas hold for the padded flow as they stand.
        flow = self.pad(padding, mode='constant' if self._ref == 't' else 'replicate')
        if quirk:
            return flow._warp(t, tmask, need_valid, consider_mask, round_mode, mask_chan_b=flow.mask[:1])
        return flow._warp(t, tmask, need_valid, consider_mask, round_mode)

    def _warp(self, t: torch.Tensor, tmask, need_valid: bool, consider_mask: bool, round_mode: int = 0,
              flow_sign: float = 1.0, data_sign: float = 1.0, t_minus: torch.Tensor = None, mask_chan_b: torch.Tensor = None,
              keep16: bool = False):
        """Core of `apply`: t [Nt,C,H,W] any dtype, tmask [Nt,H,W] bool or None (all True).
        Returns (warped fp32 [N,C,H,W], valid bool [N,H,W] | None) on self.device.
        `flow_sign` / `data_sign` = -1 (forward flows only) restate `(-self)` as the warper / `-t` as the target inside the
        kernel (exact negations; finiteness and zero tests do not depend on the sign), so that switch_ref / invert need
        no negated copy and no second flag reduction.  `t_minus` (past the early exit only): the target is t - t_minus,
        subtracted inside the kernel (modes 1 't' / 2 's': target `flow - self`; `tmask` / the two channel masks carry
        m_flow & m_self).  `mask_chan_b` ('s' only; the padded batch-1-target case of `_warp_padded`): the batch-1 flow mask
        that goes into the mask channel instead of this flow's own, and keeps an all-zero flow's result at batch 1.
        `keep16` ('t' only; a TENSOR target of `apply`): fp16 / bf16 data on the device is warped from and to its 16-bit planes
        and `warped` comes back in that dtype (`_native.warp_bwd_keep16`); fp32 / fp16 / bf16 data stored channels_last on the device
        is warped from and to that storage and `warped` comes back channels_last in that dtype (`_native.warp_bwd_nhwc`)."""
        mesh = self._ref == 's' and _mesh_mode("Flow.apply(ref='s')")
        batch_flags = self._batch_flags()                                             # (one look at the cached word for both tests)
        if batch_flags & _native.FLAG_NONFINITE:                                      # utils.py:98
            raise ValueError("Error applying flow to a target: Input contains NaN, Inf or -Inf values")
        if not (batch_flags & _native.FLAG_NZ_THR):
            # apply_flow's early exit (utils.py:497-498): every |component| < 1e-3 -> the target (and its mask
            # channel) pass through unchanged; batch broadcasting as in flow_class.py:895-898, 922-934
            warped = t.to(torch.float).to(self._device)
            if data_sign != 1.0:
                warped = warped * data_sign
            valid = None
            if need_valid:
                valid = torch.ones((t.shape[0],) + tuple(t.shape[2:]), dtype=torch.bool, device=self._device) \
                    if tmask is None else tmask.to(self._device)
                if self._ref == 's' and mask_chan_b is not None:      # padded, batch-1 target: element 0's mask only, batch stays 1 (:884-897)
                    valid = valid & mask_chan_b.to(self._device)
                elif self._ref == 's':                                # mask & self._mask before the warp (:895)
                    valid = valid & self.mask if self._mask is not None or valid.shape[0] < self.shape[0] else valid
                if valid.shape[0] != warped.shape[0]:                 # :896-897
                    warped = warped.expand(valid.shape[0], -1, -1, -1)
                if self._ref == 't':                                  # ... or after it (:934)
                    valid = valid & self.mask if self._mask is not None or valid.shape[0] < self.shape[0] else valid
            if round_mode:
                warped = torch.round(warped)
                if round_mode == _native.ROUND_U8:
                    warped = torch.clamp(warped, 0, 255)
            return warped, valid, None
        dflags = None
        if mesh:
            warped, valid = self._warp_mesh(t, tmask, need_valid, consider_mask, round_mode, flow_sign, data_sign, t_minus, mask_chan_b)
        elif self._ref == 't':
            res = None
            if keep16 and t_minus is None and round_mode == _native.ROUND_NONE:
                # a channels_last feature tensor on the device: warped from and to its N-H-W-C storage (None: not of that kind)
                res = _native.warp_bwd_nhwc(self._fv, t, src_mask=tmask, flow_mask=self._mask if need_valid else None,
                                            want_valid=need_valid)
            if res is None and keep16 and t_minus is None and t.dtype in _native._X16_DTYPES:
                res = _native.warp_bwd_keep16(self._fv, t, src_mask=tmask, flow_mask=self._mask if need_valid else None,
                                              want_valid=need_valid, round_mode=round_mode)
            if res is None:
                res = _native.warp_bwd(self._fv, t, src_mask=tmask,
                                       flow_mask=self._mask if need_valid else None,
                                       want_valid=need_valid, round_mode=round_mode, src_b=t_minus,
                                       out_uint8=not get_pure_pytorch())   # (:943-949: only then is it cast back)
            warped, valid = res[0], res[1]
        else:
            # a warped FLOW (2 channels, with its valid mask) brings its flag word along: the splat produces it as a
            # by-product, so that using the result as a warper needs no validation pass of its own
            want_f = need_valid and t.shape[1] == 2 and round_mode == 0
            res = _native.splat_fwd(self._fv, t, weight_mask=self._mask if consider_mask else None,
                                    chan_mask_a=tmask, chan_mask_b=self._mask if mask_chan_b is None else mask_chan_b,
                                    want_valid=need_valid, occlude=True, round_mode=round_mode,
                                    flow_sign=flow_sign, data_sign=data_sign, want_dst_flags=want_f, data_b=t_minus,
                                    out_half=get_half_flow_outputs())
            warped, valid = res[0], res[1]
            dflags = res[4] if want_f else None
        return warped.to(self._device), (None if valid is None else valid.to(self._device)), dflags

    def _warp_mesh(self, t, tmask, need_valid, consider_mask, round_mode, flow_sign, data_sign, t_minus, mask_chan_b):
        """`_warp` of an 's' flow with PURE_PYTORCH unset and the mesh interpolator on: the reference's own
        composition (flow_class.py:878-934) around `apply_flow` -- the target as floats, the mask (target's AND flow's) as one
        more channel, interpolated together, the channel thresholded at 0.99999.  Rounding follows on the fp32 result (:943-946).
        Nothing here is differentiable, as in the reference (utils.py:577-600 goes through NumPy)."""
        dev = self._device
        data = t.detach().to(dev).float()
        if t_minus is not None:
            data = data - t_minus.detach().to(dev).float()
        if data_sign != 1.0:
            data = data * data_sign
        if need_valid:
            m = torch.ones((t.shape[0],) + tuple(t.shape[2:]), dtype=torch.bool, device=dev) if tmask is None else tmask.to(dev)
            m = m & (self.mask if mask_chan_b is None else mask_chan_b.to(dev))                  # :895
            if m.shape[0] != data.shape[0]:                                                      # :896-897
                data = data.expand(m.shape[0], -1, -1, -1)
            data = torch.cat((data, m.unsqueeze(1).float()), dim=1)
        out = _native.mesh_apply(self._vecs, data, mask=self.mask if consider_mask and self._mask is not None else None,
                                 flow_sign=flow_sign)[0].to(dev)
        valid = None
        if need_valid:
            valid, out = out[:, -1] > _VALID_THR, out[:, :-1]
        if round_mode:
            out = torch.round(out)
            if round_mode == _native.ROUND_U8:
                out = torch.clamp(out, 0, 255)
        return out, valid

    # ------------------------------------------------------------------------------------------
    # track (flow_class.py:961-1020)
    # ------------------------------------------------------------------------------------------
    def track(self, pts: torch.Tensor, int_out: bool = None, get_valid_status: bool = None):
        """Warp points (y, x) of shape M-2 or N-M-2; optionally the status of each point = `valid_source()` at its
        (rounded) position.  Differentiable wrt the flow vectors and the points."""
        input_2d = pts.dim() == 2
        get_valid_status = False if get_valid_status is None else get_valid_status
        if not isinstance(get_valid_status, bool):
            raise TypeError("Error tracking points: Get_tracked needs to be a boolean")
        warped_pts = track_pts(flow=self._vecs, ref=self._ref, pts=pts, int_out=int_out)
        if input_2d and self.shape[0] == 1:
            warped_pts = warped_pts.squeeze(0)
        if not get_valid_status:
            return warped_pts
        if pts.dtype.is_floating_point:
            pts = torch.round(pts)
        pts2 = pts.unsqueeze(0) if input_2d else pts
        if pts2.shape[0] != self.shape[0]:
            pts2 = pts2.expand(self.shape[0], -1, -1)
        valid_source = self.valid_source().view(self.shape[0], -1)
        pts2 = (pts2[..., 0] * self.shape[-1] + pts2[..., 1]).to(valid_source.device)
        status_array = torch.gather(valid_source, 1, pts2.long())
        if warped_pts.dim() == 2:
            status_array = status_array.squeeze(0)
        return warped_pts, status_array

    # ------------------------------------------------------------------------------------------
    # switch_ref / invert (flow_class.py:1022-1086)
    # ------------------------------------------------------------------------------------------
    def switch_ref(self, mode: str = None) -> FlowAlias:
        mode = 'valid' if mode is None else mode
        if mode == 'invalid':
            return Flow._wrap(self._fv, 't' if self._ref == 's' else 's', self._mask, self._device, like=self)
        if mode != 'valid':
            raise ValueError("Error switching flow reference: Mode not recognised, should be 'valid' or 'invalid'")
        if self._all_zero(_native.FLAG_NZ_MASKED):                                   # flow_class.py:1046
            return self.switch_ref(mode='invalid')
        if self._ref == 's':
            out = self.apply(self)                                                    # one splat: P(f, f||[m], m)
            out._ref = 't'
            return out
        # (-as_s).apply(as_s) with as_s = this flow read as 's' (flow_class.py:1060-1062): one splat P(-f, f||[m], m),
        # the negation folded into the kernel's end points
        as_s = Flow._wrap(self._fv, 's', self._mask, self._device, like=self, borrowed=True)
        warped, valid, dflags = as_s._warp(self._fv, self._mask, True, True, flow_sign=-1.0)
        return Flow._wrap(warped, 's', valid, self._device, flags=dflags, made_from=(self._fv, self._mask))

    def invert(self, ref: str = None) -> FlowAlias:
        ref = self._ref if ref is None else get_valid_ref(ref)
        if self._ref == 's':
            if ref == 's':                                      # self.apply(-self): P(f, -f||[m], m)
                warped, valid, dflags = self._warp(self._fv, self._mask, True, True, data_sign=-1.0)
                return Flow._wrap(warped, 's', valid, self._device, flags=dflags, made_from=(self._fv, self._mask))
            return self._negated('t')
        if ref == 's':
            return self._negated('s')
        # self.invert('s').switch_ref(): with g = -f read as 's', g.apply(g) = P(-f, -f||[m], m)   (flow_class.py:1084-1086)
        if self._all_zero(_native.FLAG_NZ_MASKED):              # switch_ref's early exit (:1046) on g
            return self._negated('t')
        warped, valid, dflags = Flow._wrap(self._fv, 's', self._mask, self._device, like=self, borrowed=True)._warp(
            self._fv, self._mask, True, True, flow_sign=-1.0, data_sign=-1.0)
        return Flow._wrap(warped, 't', valid, self._device, flags=dflags, made_from=(self._fv, self._mask))

    # ------------------------------------------------------------------------------------------
    # valid areas (flow_class.py:1088-1172)
    # ------------------------------------------------------------------------------------------
    def valid_target(self, consider_mask: bool = None) -> torch.Tensor:
        consider_mask = True if consider_mask is None else consider_mask
        if not isinstance(consider_mask, bool):
            raise TypeError("Error applying flow: Consider_mask needs to be a boolean")
        if self._ref == 's':
            return self._splat_mask_is_one(1.0, consider_mask)
        return self._warped_ones_valid(1.0)

    def valid_source(self, consider_mask: bool = None) -> torch.Tensor:
        consider_mask = True if consider_mask is None else consider_mask
        if not isinstance(consider_mask, bool):
            raise TypeError("Error applying flow: Consider_mask needs to be a boolean")
        if self._ref == 's':
            return self._warped_ones_valid(-1.0)
        return self._splat_mask_is_one(-1.0, consider_mask)

    def _warped_ones_valid(self, sign: float) -> torch.Tensor:
        """(apply_flow(sign * vecs, ones, 't') > 0.9999) & mask (flow_class.py:1119-1122, 1151-1157) as ONE launch that reads the
        flow and its mask and writes the area (`ofl_warp_valid_f32`): no all-ones image, no warped copy of it, no compare and
        AND passes."""
        self._require_finite("Error applying flow to a target: ")
        if self._all_zero(_native.FLAG_NZ_THR):                      # apply_flow's early exit (utils.py:497-498): ones > 0.9999
            return self.mask.clone()
        return _native.warp_valid(self._vecs, self._mask, sign, 0.9999).to(self._device)

    def _splat_mask_is_one(self, sign: float, consider_mask: bool) -> torch.Tensor:
        """apply_flow(sign * vecs, mask.float(), 's', mask if consider_mask else None) == 1 (flow_class.py:1116-1118,
        1165-1169): the flow mask splatted as data, through the kernels' mask channel so that "every contributor
        valid" is exactly 1 whatever order the accumulation ran in."""
        mesh = _mesh_mode("valid_target / valid_source")
        self._require_finite("Error applying flow to a target: ")
        if self._all_zero(_native.FLAG_NZ_THR):                      # apply_flow's early exit: the mask itself
            return self.mask.clone()
        if mesh:
            # the same composition through the mesh interpolator: the mask as fp32 data; a pixel whose
            # triangle has three valid corners gets float32(w0 + w1 + w2) = 1
            area = _native.mesh_apply(self._vecs, self.mask.unsqueeze(1).float(), flow_sign=sign,
                                      mask=self._mask if consider_mask else None)[0]
            return (area[:, 0] == 1).to(self._device)
        dummy = self._vecs[:, :1]
        _, mch, _, _ = _native.splat_fwd(self._vecs, dummy, flow_sign=sign, chan_mask_a=self._mask,
                                         weight_mask=self._mask if consider_mask else None, occlude=True,
                                         want_mask_chan=True)
        return (mch == 1).to(self._device)

    # ------------------------------------------------------------------------------------------
    # padding needed (flow_class.py:1174-1224)
    # ------------------------------------------------------------------------------------------
    def get_padding(self, item: int = None) -> list:
        """[top, bottom, left, right] (per batch element, or of element `item`) by which a source image ('t') or the
        flow itself ('s') must be padded so that no valid vector reaches outside.  One masked min / max reduction
        kernel (`ofl_flow_extents_f32`) over the thresholded positions instead of clone + 4 elementwise passes + 4
        boolean-indexed reductions per batch element."""
        flow = self.select(item=item)
        ext = _native.flow_extents(flow._vecs, flow._mask, 1.0 if flow._ref == 't' else -1.0).cpu().tolist()
        h, w = flow.shape[1:]
        padding = []
        for lo_y, hi_y, lo_x, hi_x, any_valid in ext:
            if not any_valid:        # torch.min of an empty selection raises in the reference as well
                raise RuntimeError("Error getting padding: the flow mask is False everywhere")
            pad = [max(-lo_y, 0), max(hi_y - (h - 1), 0), max(-lo_x, 0), max(hi_x - (w - 1), 0)]
            padding.append([int(np.ceil(p)) for p in pad])
        return padding[0] if item is not None else padding

    # ------------------------------------------------------------------------------------------
    # zero test (flow_class.py:1226-1244)
    # ------------------------------------------------------------------------------------------
    def is_zero(self, thresholded: bool = None, masked: bool = None) -> torch.Tensor:
        masked = True if masked is None else masked
        if not isinstance(masked, bool):
            raise TypeError("Error checking whether flow is zero: Masked needs to be a boolean")
        thresholded = True if thresholded is None else thresholded
        if not isinstance(thresholded, bool):
            raise TypeError("Error checking whether flow is zero: Thresholded needs to be a boolean")
        if masked:
            bit = _native.FLAG_NZ_THR_MASKED if thresholded else _native.FLAG_NZ_MASKED
        else:
            bit = _native.FLAG_NZ_THR if thresholded else _native.FLAG_NZ
        return torch.tensor([(f & bit) == 0 for f in self._flags()], dtype=torch.bool, device=self._device)

    # ------------------------------------------------------------------------------------------
    # visualisation (flow_class.py:1246-1356)
    # ------------------------------------------------------------------------------------------
    def visualise(self, mode: str, show_mask: bool = None, show_mask_borders: bool = None,
                  range_max: Union[float, int, list, tuple] = None, return_tensor: bool = None):
        """The flow as an 'rgb' / 'bgr' / 'hsv' image (hue: direction, saturation: magnitude / range_max, value 180 outside
        the mask if `show_mask`, mask borders black if `show_mask_borders`).  `range_max` defaults to the 99th percentile of
        the magnitudes per batch element (under the mask if `show_mask`).  Returns a uint8 tensor N-3-H-W on the flow's
        device, or a NumPy array N-H-W-3 if `return_tensor` is False; 'hsv' is always a NumPy array N-H-W-3, as in the
        reference.  Computed by two HIP kernels (ofl_visualise.hip), bit-exact with the reference's NumPy / OpenCV host code;
        not differentiable, as in the reference."""
        show_mask = False if show_mask is None else show_mask
        show_mask_borders = False if show_mask_borders is None else show_mask_borders
        return_tensor = True if return_tensor is None else return_tensor
        if not isinstance(show_mask, bool):
            raise TypeError("Error visualising flow: Show_mask needs to be boolean")
        if not isinstance(show_mask_borders, bool):
            raise TypeError("Error visualising flow: Show_mask_borders needs to be boolean")
        if not isinstance(return_tensor, bool):
            raise TypeError("Error visualising flow: Return_tensor needs to be boolean")
        self._require_finite("Error visualising flow: ")
        vecs, mask = self._fv, self._mask            # (no mask: all True, never materialised)
        n = self.shape[0]
        if range_max is None:
            rng, counts = _native.visualise_range(vecs, mask if show_mask else None)
            if show_mask and mask is not None and int(counts.min()) == 0:
                # np.percentile of an empty selection (flow_class.py:1304)
                raise IndexError("index -1 is out of bounds for axis 0 with size 0")
        else:
            # flow_class.py:1310-1320, the same NumPy expressions on the N values
            if isinstance(range_max, (list, tuple)):
                if len(range_max) != n:
                    raise TypeError("Error visualising flow: Range_max list or tuple length ({}) needs to match the flow "
                                    "batch size ({})".format(len(range_max), n))
                range_max = np.array(range_max)
            elif isinstance(range_max, (float, int)):
                range_max = np.array([range_max for _ in range(n)])
            else:
                raise TypeError("Error visualising flow: Range_max needs to be an integer, a float, a list, or a tuple")
            if any(range_max <= 0):
                raise ValueError("Error visualising flow: Range_max needs to be larger than zero")
            rng = np.asarray(range_max, dtype=np.float64)
        if not isinstance(mode, str) or mode not in _native.VIS_MODES:
            raise ValueError("Error visualising flow: Mode needs to be either 'bgr', 'rgb', or 'hsv'")
        kw = dict(mask=mask, show_mask=show_mask and mask is not None, show_mask_borders=show_mask_borders)
        if mode == 'hsv' or not return_tensor:
            return _native.visualise(vecs, rng, mode, layout=_native.VIS_INTERLEAVED, **kw).cpu().numpy()
        return _native.visualise(vecs, rng, mode, layout=_native.VIS_PLANES, **kw).to(self._device)

    def visualise_arrows(self, grid_dist: int = None, img: Union[np.ndarray, torch.Tensor] = None,
                         scaling: Union[float, int] = None, show_mask: bool = None, show_mask_borders: bool = None,
                         colour: tuple = None, thickness: int = None, return_tensor: bool = None):
        """The flow as arrows on a grid of points `grid_dist` apart (default 20), over `img` (BGR uint8: NumPy H-W-3 / N-H-W-3
        or torch 3-H-W / N-3-H-W; default white), scaled by `scaling` (default: the 99th percentile of the arrow lengths over
        the whole batch equals `grid_dist`), coloured by direction as in :meth:`visualise` or with `colour` (b, g, r), with
        the area outside the mask halved (`show_mask`) and the mask borders black (`show_mask_borders`).  Returns a uint8
        tensor N-3-H-W on the flow's device, or a NumPy array N-H-W-3 if `return_tensor` is False.  Computed by the HIP kernels
        of ofl_arrows.hip.  Everything but the line drawing follows the reference bit for bit; the anti-aliased arrows are
        those of DESIGN.md 3.11 (own rasteriser and hue table, not OpenCV's).  As in the reference an 's' flow is drawn with
        thickness 1 whatever `thickness` (which still sizes the tip).  Differences: `img` is never written to, must be uint8,
        and arrows whose scaled length is not finite or beyond 2^20 pixels are skipped.  Not differentiable."""
        n, h, w = self.shape
        # flow_class.py:1395-1446, in the reference's order
        grid_dist = 20 if grid_dist is None else grid_dist
        if not isinstance(grid_dist, int):
            raise TypeError("Error visualising flow arrows: Grid_dist needs to be an integer value")
        if grid_dist > min(h, w) // 2:
            print("Warning: grid_dist in visualise_arrows is '{}', which is too large for a flow field of shape "
                  "({}, {}). grid_dist will be reset to '{}'.".format(grid_dist, h, w, min(h, w) // 2))
            grid_dist = min(h, w) // 2
        if not grid_dist > 0:
            raise ValueError("Error visualising flow arrows: Grid_dist needs to be an integer larger than zero")
        interleaved = False
        if img is not None:
            if not isinstance(img, (np.ndarray, torch.Tensor)):
                raise TypeError("Error visualising flow arrows: Img needs to be a numpy array or a torch tensor")
            interleaved = isinstance(img, np.ndarray)
            if len(img.shape) == 3:
                img = img[None]
            want = (h, w, 3) if interleaved else (3, h, w)
            if len(img.shape) != 4 or img.shape[0] not in (1, n) or tuple(img.shape[1:]) != want:
                raise ValueError("Error visualising flow arrows: Img needs to have 3 or 4 channels and the same "
                                 "shape as the flow, including the batch size")
            if img.dtype not in (np.uint8, torch.uint8):
                raise TypeError("Error visualising flow arrows: Img needs to be of dtype uint8")
        if scaling is not None:
            if not isinstance(scaling, (float, int)):
                raise TypeError("Error visualising flow arrows: Scaling needs to be a float or an integer")
            if scaling <= 0:
                raise ValueError("Error visualising flow arrows: Scaling needs to be larger than zero")
        show_mask = False if show_mask is None else show_mask
        show_mask_borders = False if show_mask_borders is None else show_mask_borders
        return_tensor = True if return_tensor is None else return_tensor
        if not isinstance(show_mask, bool):
            raise TypeError("Error visualising flow: Show_mask needs to be boolean")
        if not isinstance(show_mask_borders, bool):
            raise TypeError("Error visualising flow: Show_mask_borders needs to be boolean")
        if not isinstance(return_tensor, bool):
            raise TypeError("Error visualising flow: Return_tensor needs to be boolean")
        if colour is not None:
            if not isinstance(colour, tuple):
                raise TypeError("Error visualising flow: Colour needs to be a tuple")
            if len(colour) != 3:
                raise ValueError("Error visualising flow arrows: Colour list or tuple needs to have length 3")
            # (OpenCV saturates a colour to 8 bits: round half to even, clamp)
            colour = tuple(int(c) for c in np.clip(np.rint(np.asarray(colour, np.float64)), 0, 255))
        thickness = 1 if thickness is None else thickness
        if not isinstance(thickness, int):
            raise TypeError("Error visualising flow: Thickness needs to be an integer")
        if thickness <= 0:
            raise ValueError("Error visualising flow: Thickness needs to be a integer larger than zero")
        if thickness > 32767:                                     # (OpenCV's MAX_THICKNESS: the reference fails inside cv2)
            raise ValueError("Error visualising flow: Thickness needs to be at most 32767")
        self._require_finite("Error visualising flow arrows: ")
        vecs, mask = self._fv, self._mask            # (no mask: all True, never materialised)
        if isinstance(img, np.ndarray):
            img = torch.from_numpy(np.ascontiguousarray(img))    # (read only: the kernels never write to it)
        if scaling is None:
            scaling = _native.arrows_scale(vecs, grid_dist)
        out = _native.arrows(vecs, self._ref, grid_dist, scaling, thickness, colour=colour, img=img, img_interleaved=interleaved,
                             mask=mask, show_mask=show_mask and mask is not None, show_mask_borders=show_mask_borders,
                             layout=_native.VIS_PLANES if return_tensor else _native.VIS_INTERLEAVED)
        return out.to(self._device) if return_tensor else out.cpu().numpy()

    def matrix(self, dof: int = None, method: str = None, masked: bool = None) -> torch.Tensor:
        """Fit a transformation matrix to the flow field: `dof` 4 (rotation, translation, scaling), 6 (affine) or 8
        (homography; default), `method` 'lms', 'ransac' (default) or 'lmeds', `masked` (default True): only pixels inside
        the flow mask take part.  Returns a float64 tensor N-3-3 on the flow's device.  Fitted on the device by the kernels
        of ofl_matrix.hip; the reference calls OpenCV's estimators, the numerics here are those of DESIGN.md 3.10.  Raises
        ValueError for an image with too few usable points (the reference fails with an unrelated TypeError there).  Not
        differentiable, as in the reference."""
        dof = 8 if dof is None else dof
        if dof not in [4, 6, 8]:
            raise ValueError("Error fitting transformation matrix to flow: Dof needs to be 4, 6 or 8")
        method = 'ransac' if method is None else method
        if method not in ['lms', 'ransac', 'lmeds']:
            raise ValueError("Error fitting transformation matrix to flow: "
                             "Method needs to be 'lms', 'ransac', or 'lmeds'")
        masked = True if masked is None else masked
        if not isinstance(masked, bool):
            raise TypeError("Error fitting transformation matrix to flow: Masked needs to be boolean")
        if dof in [4, 6] and method == 'lms':
            method = 'ransac'
            warnings.warn("Method 'lms' (least mean squares) not supported for fitting a transformation matrix with 4 "
                          "or 6 degrees of freedom to the flow - defaulting to 'ransac'")
        mats, info = _native.matrix_fit(self._fv, self._ref, self._mask if masked else None, dof, method)
        status = info[:, 3].cpu()                                 # the only host read: N words
        if bool((status != 0).any()):
            i = int(torch.nonzero(status)[0])
            why = {_native.MATRIX_FEW_POINTS: "fewer than {} valid flow vectors".format(dof // 2),
                   _native.MATRIX_NO_HYPOTHESIS: "no non-degenerate point sample found",
                   _native.MATRIX_REFIT_SINGULAR: "the inlier points are degenerate"}[int(status[i])]
            raise ValueError("Error fitting transformation matrix to flow: batch element {}: {}".format(i, why))
        return mats.to(self._device)

    # ------------------------------------------------------------------------------------------
    # scoring against a ground truth (an extension: the reference has no such methods)
    # ------------------------------------------------------------------------------------------
    def _error_operands(self, gt: FlowAlias, consider_mask: bool):
        """The checks the three scoring methods share; returns (gt on this flow's device, this flow's mask, gt's mask) with None for
        a mask that does not count."""
        if not isinstance(gt, Flow):
            raise TypeError("Error scoring flow: Gt needs to be of type 'Flow'")
        if self.shape != gt.shape:
            raise ValueError("Error scoring flow: Flow fields need to have the same shape, including batch size")
        if self.ref != gt.ref:
            raise ValueError("Error scoring flow: Flow fields need to have the same reference")
        consider_mask = True if consider_mask is None else consider_mask
        if not isinstance(consider_mask, bool):
            raise TypeError("Error scoring flow: Consider_mask needs to be boolean")
        if self._device != gt._device:
            gt = gt.to_device(self._device)
        return gt, (self._mask if consider_mask else None), (gt._mask if consider_mask else None)

    def error_stats(self, gt: FlowAlias, consider_mask: bool = None, thresholds: Union[list, tuple] = None) -> dict:
        """Score this flow as an estimate of the ground truth `gt` (equal shape and reference), per batch element over the pixels
        valid in both masks (every pixel if `consider_mask` is False).  Returns a dict of tensors on the flow's device:
        'count' int64 [N]; 'epe' float64 [N], the mean end-point error (NaN where count is 0); 'max' float64 [N]; 'outliers' float64
        [N,K], the share of pixels whose error is over (strictly) each of the K `thresholds` (1 to 4, default (1, 3, 5) px); 'fl'
        float64 [N], KITTI's outlier rate (error over 3 px and over 5 % of the true speed); 'speed_count' int64 [N,3] and
        'speed_epe' float64 [N,3], the pixels and their mean error by true speed in [0, 10), [10, 40), [40, inf) px.  One pass of
        ofl_metrics.hip over both flows, float64 sums in a fixed order (bitwise reproducible, independent of the batch; DESIGN.md
        3.16); nothing is read back to the host.  Not differentiable: see :meth:`epe`."""
        gt, mask, gt_mask = self._error_operands(gt, consider_mask)
        thresholds = (1, 3, 5) if thresholds is None else thresholds
        if not isinstance(thresholds, (list, tuple)):
            raise TypeError("Error scoring flow: Thresholds needs to be a list or a tuple")
        if not 1 <= len(thresholds) <= _native.ERROR_MAX_THRESHOLDS:
            raise ValueError("Error scoring flow: Thresholds list or tuple needs to have length 1 to 4")
        if not all(isinstance(t, (int, float)) and not isinstance(t, bool) for t in thresholds):
            raise TypeError("Error scoring flow: Thresholds needs to hold integers or floats")
        if not all(math.isfinite(t) and t >= 0 for t in thresholds):
            raise ValueError("Error scoring flow: Thresholds need to be finite and not negative")
        k = len(thresholds)
        rec, _ = _native.flow_error(self._fv, gt._fv, mask, gt_mask, tuple(thresholds), False)
        rec = rec.to(self._device)
        count = rec[:, 0]
        return {'count': count.to(torch.int64), 'epe': rec[:, 1] / count, 'max': rec[:, 2].clone(),
                'outliers': rec[:, 3:3 + k] / count[:, None], 'fl': rec[:, 7] / count,
                'speed_count': rec[:, 8:11].to(torch.int64), 'speed_epe': rec[:, 11:14] / rec[:, 8:11]}

    def epe_map(self, gt: FlowAlias, consider_mask: bool = None) -> torch.Tensor:
        """The end-point error of every pixel against the ground truth `gt`: float32 N-H-W on the flow's device, 0 where a pixel is
        not valid in both masks (every pixel counts if `consider_mask` is False).  Not differentiable: see :meth:`epe`."""
        gt, mask, gt_mask = self._error_operands(gt, consider_mask)
        return _native.flow_error(self._fv, gt._fv, mask, gt_mask, (), True)[1].to(self._device)

    def epe(self, gt: FlowAlias, consider_mask: bool = None) -> torch.Tensor:
        """The mean end-point error against the ground truth `gt` per batch element: float32 [N] on the flow's device (the float64
        mean of :meth:`error_stats` rounded once; NaN for an element without a valid pixel).  Differentiable with respect to the
        vectors of either flow -- the supervised loss of a flow network; an element without a valid pixel has gradient 0."""
        gt, mask, gt_mask = self._error_operands(gt, consider_mask)
        return _native.flow_epe(self._fv, gt._fv, mask, gt_mask).to(self._device)

    # ------------------------------------------------------------------------------------------
    # the sequence loss of a refinement network (an extension: the reference has no such methods)
    # ------------------------------------------------------------------------------------------
    @staticmethod
    def _sequence_operands(preds, gt, gamma, max_flow, penalty, normalise, consider_mask):
        """The checks the two sequence methods share; returns the arguments of `_sequence_loss.sequence_loss` and the device of the
        result."""
        err = _sequence_loss.ERR
        if not isinstance(preds, (list, tuple)) or not all(isinstance(f, Flow) for f in preds):
            raise TypeError(err + "Preds needs to be a list or a tuple of flow objects")
        if not isinstance(gt, Flow):
            raise TypeError(err + "Gt needs to be of type 'Flow'")
        _sequence_loss.check_count(len(preds))
        if any(f.shape != gt.shape for f in preds):
            raise ValueError(err + "Flow fields need to have the same shape, including batch size")
        if any(f.ref != gt.ref for f in preds):
            raise ValueError(err + "Flow fields need to have the same reference")
        gamma, max_flow, penalty, normalise = _sequence_loss.check_params(gamma, max_flow, penalty, normalise)
        consider_mask = True if consider_mask is None else consider_mask
        if not isinstance(consider_mask, bool):
            raise TypeError(err + "Consider_mask needs to be boolean")
        dev = preds[0]._device
        if gt._device != dev:
            gt = gt.to_device(dev)
        return ([f._fv for f in preds], gt._fv, gt._mask if consider_mask else None, gamma, max_flow, penalty, normalise), dev

    @staticmethod
    def sequence_loss(preds: Union[list, tuple], gt: FlowAlias, gamma: float = None, max_flow: float = None, penalty: str = None,
                      normalise: str = None, consider_mask: bool = None) -> torch.Tensor:
        """The sequence loss of RAFT, GMA, CRAFT, GMFlow, UniMatch and FlowFormer per batch element, float32 [N] on the device of the
        first prediction: `preds` is a list or tuple of the 1 to 32 refinement outputs of a network, flows of the shape and reference
        of the ground truth `gt`, and loss_n = sum_i gamma^(T-1-i) * mean_i, the last prediction weighing 1 (`gamma` default 0.8).  A
        pixel is VALID where `gt.mask` is True (with `consider_mask` False: everywhere) and the magnitude of the ground truth is
        below `max_flow` (default 400, inf allowed; a NaN or infinite ground truth is never valid).  The masks of the predictions
        are NOT read: the outputs of a network carry none, and T masks would give T different counts.  `penalty` 'l1' (default)
        sums |du| + |dv| over the valid pixels, 'l2' the end-point error; `normalise` 'all' (default, RAFT's) divides by all 2 H W
        ('l2': H W) terms of the image, 'valid' by those of the valid pixels (NaN for an element without one, whose gradient is
        0).  `loss.mean()` under ('l1', 'all') is RAFT's scalar.  One pass of ofl_sequence_loss.hip reads the ground truth and its mask
        once for all T predictions; float64 sums in a fixed order (bitwise reproducible, independent of the batch);
        nothing is read back to the host.  Differentiable with respect to the vectors of the predictions that require a gradient --
        one more launch writes all of them -- not the ground truth or any mask."""
        args, dev = Flow._sequence_operands(preds, gt, gamma, max_flow, penalty, normalise, consider_mask)
        return _sequence_loss.sequence_loss(*args).to(dev)

    @staticmethod
    def sequence_stats(preds: Union[list, tuple], gt: FlowAlias, gamma: float = None, max_flow: float = None, penalty: str = None,
                       normalise: str = None, consider_mask: bool = None) -> dict:
        """What :meth:`sequence_loss` is made of, from the same pass, as a dict of tensors on the device of the first prediction:
        'count' int64 [N], the valid pixels; 'loss' float32 [N]; 'weights' float64 [T]; 'terms' float64 [N,T], the mean penalty of
        every prediction (loss = sum_i weights_i terms_i); 'epe' float64 [N,T], the mean end-point error of every prediction over the
        valid pixels (NaN where count is 0) -- the convergence curve over the iterations; 'within' float64 [N,3], the share of valid
        pixels whose end-point error of the LAST prediction is below (strictly, unlike the `>` of :meth:`error_stats`) 1, 3 and 5
        px, RAFT's 1px / 3px / 5px metrics.  The masks of the predictions are not read.  Not differentiable."""
        args, dev = Flow._sequence_operands(preds, gt, gamma, max_flow, penalty, normalise, consider_mask)
        return {k: v.to(dev) for k, v in _sequence_loss.sequence_stats(*args).items()}

    # ------------------------------------------------------------------------------------------
    # the composition of a clip's flows (an extension: the reference composes two flows at a time)
    # ------------------------------------------------------------------------------------------
    @staticmethod
    def chain(flows: Union[list, tuple], return_all: bool = None) -> Union[FlowAlias, list]:
        """The flow from the first frame of a clip to its last, composed from the 1 to 32 frame-to-frame flows `flows`, a list or
        tuple ordered in time (`flows[k]` runs from frame k to frame k + 1) of flows of one shape and one reference.  For 's' flows
        the result lives on the grid of frame 0 and is the left fold `(((f_1 (+) f_2) (+) f_3) ...)` of :meth:`combine_with` mode 3; for
        't' flows it lives on the grid of the last frame and is the right fold `(f_1 (+) (... (f_{T-1} (+) f_T)))`.  The vectors and the
        mask carry the bits of that fold wherever the fold takes none of its early exits (an operand that is all zero under its mask,
        an accumulated flow under the threshold of :meth:`apply`); where it would, the general formula is the definition (DESIGN.md
        3.31): the vectors agree, the mask is the one the sampling gives.  One launch of ofl_chain.hip whatever T is: every pixel walks
        through the flows with its running vector and mask bit in registers, no intermediate flow is written, read back, wrapped or
        validated.  With `return_all` True a list of T flows: for 's' flows `out[k]` is the chain of `flows[:k + 1]` -- the dense
        trajectories of the pixels of frame 0, the whole chain last -- for 't' flows the chain of `flows[k:]`, the whole chain first; the
        element that is a single input flow is that object, the others are views of one allocation the same launch writes.  A single
        flow is returned as it is.  The result is on the device of the first flow.  When autograd is recording and the vectors of a
        flow require a gradient, the call runs the fold of :meth:`combine_with` instead and keeps its gradients: the fused kernel has
        no backward."""
        err = _chain.ERR
        if not isinstance(flows, (list, tuple)) or not all(isinstance(f, Flow) for f in flows):
            raise TypeError(err + "Flows needs to be a list or a tuple of flow objects")
        if not 1 <= len(flows) <= _chain.MAX_T:
            raise ValueError(err + "The sequence needs to hold 1 to {} flows".format(_chain.MAX_T))
        first = flows[0]
        if any(f.shape != first.shape for f in flows):
            raise ValueError(err + "Flow fields need to have the same shape, including batch size")
        if any(f.ref != first.ref for f in flows):
            raise ValueError(err + "Flow fields need to have the same reference: switch_ref the others")
        if first.shape[1] < 2 or first.shape[2] < 2:
            raise ValueError(err + "Flow fields need to be at least 2 pixels high and wide")
        return_all = False if return_all is None else return_all
        if not isinstance(return_all, bool):
            raise TypeError(err + "Return_all needs to be boolean")
        t, ref, dev = len(flows), first._ref, first._device
        if t == 1:
            return [first] if return_all else first
        flows = [f if f._device == dev else f.to_device(dev) for f in flows]
        if _native._wants_grad(*[f._fv for f in flows]):
            return Flow._chain_fold(flows, return_all)
        vecs, mask = _chain.flow_chain([f._fv.detach() for f in flows], [f._mask for f in flows], -1.0 if ref == 's' else 1.0, return_all)
        if not return_all:
            return Flow._wrap(vecs, ref, mask, dev, fresh=True)
        parts = [Flow._wrap(vecs[j], ref, mask[j], dev, fresh=True) for j in range(t - 1)]
        return [flows[0]] + parts if ref == 's' else parts + [flows[-1]]

    @staticmethod
    def _chain_fold(flows: list, return_all: bool) -> Union[FlowAlias, list]:
        """:meth:`chain` as the fold of :meth:`combine_with` mode 3 it is defined by -- T - 1 launches, early exits included: the route
        of flows whose vectors require a gradient."""
        if flows[0]._ref == 's':
            out = [flows[0]]
            for f in flows[1:]:
                out.append(out[-1].combine_with(f, 3))
            return out if return_all else out[-1]
        out = [flows[-1]]
        for f in reversed(flows[:-1]):
            out.insert(0, f.combine_with(out[0], 3))
        return out if return_all else out[0]

    # ------------------------------------------------------------------------------------------
    # forward-backward consistency (an extension: the reference has no such methods)
    # ------------------------------------------------------------------------------------------
    def _consistency_operands(self, back: FlowAlias, alpha, beta, consider_mask: bool):
        """The checks the three consistency methods share; returns the arguments of `_consistency.flow_consistency` up to beta."""
        err = "Error checking flow consistency: "
        if not isinstance(back, Flow):
            raise TypeError(err + "Back needs to be of type 'Flow'")
        if self.shape != back.shape:
            raise ValueError(err + "Flow fields need to have the same shape, including batch size")
        if self.ref != back.ref:
            raise ValueError(err + "Flow fields need to have the same reference: switch_ref one of them")
        if self.shape[1] < 2 or self.shape[2] < 2:
            raise ValueError(err + "Flow fields need to be at least 2 pixels high and wide")
        alpha = 0.01 if alpha is None else alpha
        beta = 0.5 if beta is None else beta
        for name, value in (("Alpha", alpha), ("Beta", beta)):
            if not isinstance(value, (int, float)) or isinstance(value, bool):
                raise TypeError(err + name + " needs to be an integer or a float")
            if not (math.isfinite(value) and value >= 0):
                raise ValueError(err + name + " needs to be finite and not negative")
        consider_mask = True if consider_mask is None else consider_mask
        if not isinstance(consider_mask, bool):
            raise TypeError(err + "Consider_mask needs to be boolean")
        if self._device != back._device:
            back = back.to_device(self._device)
        return (self._fv, back._fv, self._mask if consider_mask else None, back._mask if consider_mask else None,
                -1.0 if self._ref == 's' else 1.0, float(alpha), float(beta))

    def consistency(self, back: FlowAlias, alpha: float = None, beta: float = None, consider_mask: bool = None) -> dict:
        """The forward-backward check of this flow (frame 1 to frame 2) against `back`, a flow from frame 2 to frame 1 of equal shape
        and reference.  The partner of a pixel is `back` sampled bilinearly where this flow points -- at p + self(p) for 's' flows, at
        x - self(x) for 't' flows, the arithmetic of :meth:`combine_with` mode 3.  A pixel is KNOWN where the partner's taps lie in
        the frame and are valid in `back.mask` and the pixel is valid in this flow's mask (with `consider_mask` False: the frame test
        alone); its error e is the length of the round trip self + partner; it is CONSISTENT where it is known and
        e^2 <= alpha (|self|^2 + |partner|^2) + beta (inclusive; defaults 0.01 and 0.5 as in UnFlow).  Returns a dict of tensors on
        the flow's device: 'error' float32 [N,H,W] (0 where not known), 'consistent' and 'known' bool [N,H,W], 'count' and
        'consistent_count' int64 [N], 'rate' float64 [N] (consistent / known, NaN without a known pixel), 'mean_error' (over the
        known pixels), 'max_error' and 'mean_error_consistent' float64 [N].  One pass of ofl_consistency.hip: the composed flow is
        never written, float64 sums in a fixed order (bitwise reproducible, independent of the batch), nothing is
        read back to the host.  Not differentiable: the call runs on the detached vectors."""
        err, cons, known, rec = _consistency.flow_consistency(*self._consistency_operands(back, alpha, beta, consider_mask))
        err, cons, known, rec = (t.to(self._device) for t in (err, cons, known, rec))
        count, ccount = rec[:, 0], rec[:, 1]
        return {'error': err, 'consistent': cons, 'known': known, 'count': count.to(torch.int64),
                'consistent_count': ccount.to(torch.int64), 'rate': ccount / count, 'mean_error': rec[:, 2] / count,
                'max_error': rec[:, 3].clone(), 'mean_error_consistent': rec[:, 4] / ccount}

    def consistency_mask(self, back: FlowAlias, alpha: float = None, beta: float = None, consider_mask: bool = None) -> torch.Tensor:
        """The 'consistent' map of :meth:`consistency` alone: bool N-H-W on the flow's device (the kernel writes nothing else).  Not
        differentiable."""
        ops = self._consistency_operands(back, alpha, beta, consider_mask)
        return _consistency.flow_consistency(*ops, want_error=False, want_known=False, want_record=False)[1].to(self._device)

    def filter_consistent(self, back: FlowAlias, alpha: float = None, beta: float = None, consider_mask: bool = None) -> FlowAlias:
        """This flow with its mask narrowed to the pixels :meth:`consistency_mask` finds consistent with `back`: same vectors (the
        same tensor, not a copy) and reference, mask = self.mask & consistent.  Not differentiable with respect to `back`."""
        mask = self._and_masks(self.consistency_mask(back, alpha, beta, consider_mask))
        out = Flow._wrap(self._fv, self._ref, mask, self._device)
        if self._flags_known():
            # the vectors are this flow's: finiteness and the unmasked zero tests carry over; the masked ones can only lose bits under a
            # narrower mask, so a word that has none of them set stays exact
            word = self._flag_cache[1]
            if not any(f & (_native.FLAG_NZ_MASKED | _native.FLAG_NZ_THR_MASKED) for f in word):
                out._flag_cache = (out._key(), word)
        return out

    # ------------------------------------------------------------------------------------------
    # edge-aware smoothness (an extension: the reference has no such methods)
    # ------------------------------------------------------------------------------------------
    def _smoothness_operands(self, img, order, alpha, eps, consider_mask: bool):
        """The checks the three smoothness methods share; returns the arguments of `_smoothness.flow_smoothness` up to eps."""
        err = "Error computing flow smoothness: "
        if img is not None:
            if isinstance(img, np.ndarray):
                if img.dtype not in (np.float32, np.uint8):
                    raise TypeError(err + "Img needs to be of dtype float32 or uint8")
                img = torch.from_numpy(img)
            if not isinstance(img, torch.Tensor):
                raise TypeError(err + "Img needs to be a torch tensor or a numpy array")
            if img.dtype not in (torch.float32, torch.uint8):
                raise TypeError(err + "Img needs to be of dtype float32 or uint8")
            if img.dim() not in (3, 4):
                raise ValueError(err + "Img needs to have 3 or 4 dimensions, C-H-W or N-C-H-W")
            if not 1 <= img.shape[-3] <= 4:
                raise ValueError(err + "Img needs to have 1 to 4 channels")
            if tuple(img.shape[-2:]) != tuple(self.shape[1:]):
                raise ValueError(err + "Img needs to have the H-W shape of the flow")
            if img.dim() == 4 and img.shape[0] != self.shape[0]:
                raise ValueError(err + "Img needs to have the batch size of the flow")
        order = 1 if order is None else order
        if not isinstance(order, int) or isinstance(order, bool):
            raise TypeError(err + "Order needs to be an integer")
        if order not in (1, 2):
            raise ValueError(err + "Order needs to be 1 or 2")
        alpha = 10.0 if alpha is None else alpha
        eps = 0.001 if eps is None else eps
        for name, value in (("Alpha", alpha), ("Eps", eps)):
            if not isinstance(value, (int, float)) or isinstance(value, bool):
                raise TypeError(err + name + " needs to be an integer or a float")
            if not (math.isfinite(value) and value >= 0):
                raise ValueError(err + name + " needs to be finite and not negative")
        consider_mask = True if consider_mask is None else consider_mask
        if not isinstance(consider_mask, bool):
            raise TypeError(err + "Consider_mask needs to be boolean")
        if img is not None:
            img = img.detach()
            if img.device != self._device:
                img = img.to(self._device)
            img = img.contiguous()
        return self._fv, (self._mask if consider_mask else None), img, order, float(alpha), float(eps)

    def smoothness_stats(self, img=None, order: int = None, alpha: float = None, eps: float = None, consider_mask: bool = None) -> dict:
        """The edge-aware smoothness penalty of this flow, per batch element.  A term is a first (`order` 1, the default) or second
        (`order` 2) difference d of the vectors along x or along y, penalised as sqrt(du^2 + eps^2) + sqrt(dv^2 + eps^2) (`eps`
        default 0.001) and, with a guidance image `img` (tensor or array, float32 or uint8 read as s / 255, C-H-W or N-C-H-W with 1 to 4
        channels), weighted by exp(-alpha g) (`alpha` default 10), g being the mean over the channels of the absolute image difference
        across the same pixels.  A term counts where every pixel it reads is valid in the mask (every term that exists if
        `consider_mask` is False).  Returns a dict of tensors on the flow's device: 'count_x', 'count_y' int64 [N]; 'sum_x', 'sum_y',
        'max' float64 [N]; 'smoothness' float64 [N], (sum_x + sum_y) / (count_x + count_y), NaN without a valid term.  One pass of
        ofl_smoothness.hip, float64 sums in a fixed order (bitwise reproducible, independent of the batch); nothing is
        read back to the host.  Not differentiable: see :meth:`smoothness`."""
        rec, _ = _smoothness.flow_smoothness(*self._smoothness_operands(img, order, alpha, eps, consider_mask))
        rec = rec.to(self._device)
        return {'count_x': rec[:, 0].to(torch.int64), 'count_y': rec[:, 1].to(torch.int64), 'sum_x': rec[:, 2].clone(),
                'sum_y': rec[:, 3].clone(), 'max': rec[:, 4].clone(), 'smoothness': (rec[:, 2] + rec[:, 3]) / (rec[:, 0] + rec[:, 1])}

    def smoothness_map(self, img=None, order: int = None, alpha: float = None, eps: float = None, consider_mask: bool = None) -> torch.Tensor:
        """The x term plus the y term of :meth:`smoothness_stats` at every pixel: float32 N-H-W on the flow's device, a term being
        attributed to its left / upper pixel (order 1) or its centre pixel (order 2); a term that is not valid is 0.  Not
        differentiable: see :meth:`smoothness`."""
        ops = self._smoothness_operands(img, order, alpha, eps, consider_mask)
        return _smoothness.flow_smoothness(*ops, want_map=True)[1].to(self._device)

    def smoothness(self, img=None, order: int = None, alpha: float = None, eps: float = None, consider_mask: bool = None) -> torch.Tensor:
        """The mean of the valid terms of :meth:`smoothness_stats` per batch element: float32 [N] on the flow's device (the float64
        quotient rounded once; NaN for an element without a valid term).  Differentiable with respect to the flow vectors ONLY -- the
        smoothness term of an unsupervised flow loss.  The image is guidance and carries no gradient, even if it requires one; an
        element without a valid term has gradient 0.  The backward pass gathers (no atomics): it is bitwise reproducible."""
        return _smoothness.smoothness(*self._smoothness_operands(img, order, alpha, eps, consider_mask)).to(self._device)

    # ------------------------------------------------------------------------------------------
    # photometric loss (an extension: the reference has no such methods)
    # ------------------------------------------------------------------------------------------
    def _photometric_operands(self, img, other, eps, consider_mask: bool):
        """The checks the three photometric methods share; returns the arguments of `_photometric.flow_photometric` up to eps."""
        err = "Error computing photometric loss: "
        images = []
        for name, im in (("Img", img), ("Other", other)):
            if isinstance(im, np.ndarray):
                if im.dtype not in (np.float32, np.uint8):
                    raise TypeError(err + name + " needs to be of dtype float32 or uint8")
                im = torch.from_numpy(im)
            if not isinstance(im, torch.Tensor):
                raise TypeError(err + name + " needs to be a torch tensor or a numpy array")
            if im.dtype not in (torch.float32, torch.uint8):
                raise TypeError(err + name + " needs to be of dtype float32 or uint8")
            images.append(im)
        img, other = images
        if img.dtype != other.dtype:
            raise TypeError(err + "Img and other need to be of the same dtype")
        for name, im in (("Img", img), ("Other", other)):
            if im.dim() not in (3, 4):
                raise ValueError(err + name + " needs to have 3 or 4 dimensions, C-H-W or N-C-H-W")
            if not 1 <= im.shape[-3] <= 4:
                raise ValueError(err + name + " needs to have 1 to 4 channels")
        if img.shape[-3] != other.shape[-3]:
            raise ValueError(err + "Img and other need to have the same number of channels")
        for name, im in (("Img", img), ("Other", other)):
            if tuple(im.shape[-2:]) != tuple(self.shape[1:]):
                raise ValueError(err + name + " needs to have the H-W shape of the flow")
            if im.dim() == 4 and im.shape[0] != self.shape[0]:
                raise ValueError(err + name + " needs to have the batch size of the flow")
        if self.shape[1] < 2 or self.shape[2] < 2:
            raise ValueError(err + "Flow field needs to be at least 2 pixels high and wide")
        eps = 0.001 if eps is None else eps
        if not isinstance(eps, (int, float)) or isinstance(eps, bool):
            raise TypeError(err + "Eps needs to be an integer or a float")
        if not (math.isfinite(eps) and eps >= 0):
            raise ValueError(err + "Eps needs to be finite and not negative")
        consider_mask = True if consider_mask is None else consider_mask
        if not isinstance(consider_mask, bool):
            raise TypeError(err + "Consider_mask needs to be boolean")
        images = []
        for im in (img, other):
            im = im.detach()
            if im.device != self._device:
                im = im.to(self._device)
            images.append(im.contiguous())
        return (self._fv, (self._mask if consider_mask else None), images[0], images[1], -1.0 if self._ref == 's' else 1.0,
                float(eps))

    def photometric_stats(self, img, other, eps: float = None, consider_mask: bool = None) -> dict:
        """The photometric penalty of this flow between two frames, per batch element.  `img` is the frame on the flow's own grid,
        `other` the frame the flow points into: for an 's' flow from frame 1 to frame 2, `img` is frame 1 and `other` frame 2; for a
        't' flow, `img` is frame 2 and `other` frame 1.  Both are tensors or arrays of one dtype, float32 or uint8 (read as s / 255),
        C-H-W or N-C-H-W with the same 1 to 4 channels.  `other` is sampled bilinearly where the flow points -- at p + self(p) for 's'
        flows, at p - self(p) for 't' flows, the arithmetic of :meth:`apply` on a 't' flow -- and compared with `img` under the
        Charbonnier penalty sqrt(d^2 + eps^2) (`eps` default 0.001), averaged over the channels.  A pixel is KNOWN where the sample's
        taps lie in the frame and the pixel is valid in this flow's mask (with `consider_mask` False: the frame test alone).  Returns a
        dict of tensors on the flow's device: 'count' int64 [N], the known pixels; 'sum', 'max' float64 [N] over them; 'photometric'
        float64 [N], sum / count, NaN without a known pixel.  One pass of ofl_photometric.hip: the warped image is never written,
        float64 sums in a fixed order (bitwise reproducible, independent of the batch), nothing is read back to the
        host.  Not differentiable: see :meth:`photometric`."""
        rec, _ = _photometric.flow_photometric(*self._photometric_operands(img, other, eps, consider_mask))
        rec = rec.to(self._device)
        return {'count': rec[:, 0].to(torch.int64), 'sum': rec[:, 1].clone(), 'max': rec[:, 2].clone(), 'photometric': rec[:, 1] / rec[:, 0]}

    def photometric_map(self, img, other, eps: float = None, consider_mask: bool = None) -> torch.Tensor:
        """The penalty of :meth:`photometric_stats` at every pixel: float32 N-H-W on the flow's device, 0 where the pixel is not
        known (the kernel writes nothing else).  Not differentiable: see :meth:`photometric`."""
        ops = self._photometric_operands(img, other, eps, consider_mask)
        return _photometric.flow_photometric(*ops, want_map=True, want_record=False)[1].to(self._device)

    def photometric(self, img, other, eps: float = None, consider_mask: bool = None) -> torch.Tensor:
        """The mean of :meth:`photometric_stats` over the known pixels per batch element: float32 [N] on the flow's device (the
        float64 quotient rounded once; NaN for an element without a known pixel).  Differentiable with respect to the flow vectors
        ONLY -- the photometric term of an unsupervised flow loss.  The images carry no gradient, even if they require one; an
        element without a known pixel has gradient 0.  The backward pass gathers (no atomics): it is bitwise reproducible."""
        return _photometric.photometric(*self._photometric_operands(img, other, eps, consider_mask)).to(self._device)

    # ------------------------------------------------------------------------------------------
    # census loss (an extension: the reference has no such methods)
    # ------------------------------------------------------------------------------------------
    def _census_operands(self, img, other, patch, thresh, eps, q, consider_mask: bool):
        """The checks the three census methods share; returns the arguments of `_census.flow_census` up to q."""
        err = "Error computing census loss: "
        images = []
        for name, im in (("Img", img), ("Other", other)):
            if isinstance(im, np.ndarray):
                if im.dtype not in (np.float32, np.uint8):
                    raise TypeError(err + name + " needs to be of dtype float32 or uint8")
                im = torch.from_numpy(im)
            if not isinstance(im, torch.Tensor):
                raise TypeError(err + name + " needs to be a torch tensor or a numpy array")
            if im.dtype not in (torch.float32, torch.uint8):
                raise TypeError(err + name + " needs to be of dtype float32 or uint8")
            images.append(im)
        img, other = images
        if img.dtype != other.dtype:
            raise TypeError(err + "Img and other need to be of the same dtype")
        for name, im in (("Img", img), ("Other", other)):
            if im.dim() not in (3, 4):
                raise ValueError(err + name + " needs to have 3 or 4 dimensions, C-H-W or N-C-H-W")
            if im.shape[-3] not in (1, 3):
                raise ValueError(err + name + " needs to have 1 or 3 channels")
        if img.shape[-3] != other.shape[-3]:
            raise ValueError(err + "Img and other need to have the same number of channels")
        for name, im in (("Img", img), ("Other", other)):
            if tuple(im.shape[-2:]) != tuple(self.shape[1:]):
                raise ValueError(err + name + " needs to have the H-W shape of the flow")
            if im.dim() == 4 and im.shape[0] != self.shape[0]:
                raise ValueError(err + name + " needs to have the batch size of the flow")
        if self.shape[1] < 2 or self.shape[2] < 2:
            raise ValueError(err + "Flow field needs to be at least 2 pixels high and wide")
        patch = _census.PATCH if patch is None else patch
        if not isinstance(patch, int) or isinstance(patch, bool):
            raise TypeError(err + "Patch needs to be an integer")
        if patch not in (3, 5, 7):
            raise ValueError(err + "Patch needs to be 3, 5 or 7")
        values = []
        for name, val, default in (("Thresh", thresh, _census.THRESH), ("Eps", eps, _census.EPS), ("Q", q, _census.Q)):
            val = default if val is None else val
            if not isinstance(val, (int, float)) or isinstance(val, bool):
                raise TypeError(err + name + " needs to be an integer or a float")
            # (the kernels take float32: a value that rounds to 0 or to infinity there is out of range)
            if not (math.isfinite(val) and val > 0 and 0 < float(np.float32(val)) < float('inf')):
                raise ValueError(err + name + " needs to be finite and larger than 0")
            values.append(float(val))
        if values[2] > 1:
            raise ValueError(err + "Q needs to be at most 1")
        consider_mask = True if consider_mask is None else consider_mask
        if not isinstance(consider_mask, bool):
            raise TypeError(err + "Consider_mask needs to be boolean")
        images = []
        for im in (img, other):
            im = im.detach()
            if im.device != self._device:
                im = im.to(self._device)
            images.append(im.contiguous())
        return (self._fv, (self._mask if consider_mask else None), images[0], images[1], -1.0 if self._ref == 's' else 1.0,
                patch, values[0], values[1], values[2])

    def census_stats(self, img, other, patch: int = None, thresh: float = None, eps: float = None, q: float = None,
                     consider_mask: bool = None) -> dict:
        """The census penalty of this flow between two frames, per batch element: the data term unsupervised flow training uses in
        place of a brightness difference, because it survives a change of illumination.  `img` is the frame on the flow's own grid,
        `other` the frame the flow points into, as in :meth:`photometric_stats`: tensors or arrays of one dtype, float32 (scale 0 .. 1)
        or uint8, C-H-W or N-C-H-W with the same 1 or 3 channels.  `other` is sampled bilinearly where the flow points, both frames
        are turned into grey on the scale 0 .. 255, and for every neighbour o of a pixel p in its `patch` x `patch` window (3, 5 or
        7, default 7) the soft signs t = d / sqrt(0.81 + d^2) of the grey differences d = G(p + o) - G(p) are compared:
        f = (ti - tw)^2 / (`thresh` + (ti - tw)^2), `thresh` default 0.1.  The penalty of p is (mean of f + `eps`)^`q`, `eps` default
        0.01, `q` default 0.4.  A pixel is USABLE where it is valid in this flow's mask (with `consider_mask` False: everywhere) and
        its sample's taps lie in the frame; only usable neighbours are terms, and a pixel is KNOWN where it is usable and has at
        least one.  Returns a dict of tensors on the flow's device: 'count' int64 [N], the known pixels; 'sum', 'max' float64 [N]
        over them; 'census' float64 [N], sum / count, NaN without a known pixel; 'fill' float64 [N], the share of the patch
        neighbours of the known pixels that were terms.  One pass of ofl_census.hip from LDS tiles: neither the warped image nor a
        tensor of patch^2 - 1 channels is written, float64 sums in a fixed order (bitwise reproducible, independent of the batch;
        DESIGN.md 3.21), nothing is read back to the host.  Not differentiable: see :meth:`census`."""
        ops = self._census_operands(img, other, patch, thresh, eps, q, consider_mask)
        rec, _ = _census.flow_census(*ops)
        rec = rec.to(self._device)
        return {'count': rec[:, 0].to(torch.int64), 'sum': rec[:, 1].clone(), 'max': rec[:, 2].clone(), 'census': rec[:, 1] / rec[:, 0],
                'fill': rec[:, 3] / (rec[:, 0] * float(ops[5] * ops[5] - 1))}

    def census_map(self, img, other, patch: int = None, thresh: float = None, eps: float = None, q: float = None,
                   consider_mask: bool = None) -> torch.Tensor:
        """The penalty of :meth:`census_stats` at every pixel: float32 N-H-W on the flow's device, 0 where the pixel is not known
        (the kernel writes nothing else).  Not differentiable: see :meth:`census`."""
        ops = self._census_operands(img, other, patch, thresh, eps, q, consider_mask)
        return _census.flow_census(*ops, want_map=True, want_record=False)[1].to(self._device)

    def census(self, img, other, patch: int = None, thresh: float = None, eps: float = None, q: float = None,
               consider_mask: bool = None) -> torch.Tensor:
        """The mean of :meth:`census_stats` over the known pixels per batch element: float32 [N] on the flow's device (the float64
        quotient rounded once; NaN for an element without a known pixel).  Differentiable with respect to the flow vectors ONLY --
        the census term of an unsupervised flow loss.  The images carry no gradient, even if they require one; an element without a
        known pixel has gradient 0.  The backward pass gathers (no atomics): it is bitwise reproducible."""
        return _census.census(*self._census_operands(img, other, patch, thresh, eps, q, consider_mask)).to(self._device)

    # ------------------------------------------------------------------------------------------
    # SSIM loss (an extension: the reference has no such methods)
    # ------------------------------------------------------------------------------------------
    def _ssim_operands(self, img, other, window, c1, c2, consider_mask: bool):
        """The checks the three SSIM methods share; returns the arguments of `_ssim.flow_ssim` up to c2."""
        err = "Error computing SSIM loss: "
        images = []
        for name, im in (("Img", img), ("Other", other)):
            if isinstance(im, np.ndarray):
                if im.dtype not in (np.float32, np.uint8):
                    raise TypeError(err + name + " needs to be of dtype float32 or uint8")
                im = torch.from_numpy(im)
            if not isinstance(im, torch.Tensor):
                raise TypeError(err + name + " needs to be a torch tensor or a numpy array")
            if im.dtype not in (torch.float32, torch.uint8):
                raise TypeError(err + name + " needs to be of dtype float32 or uint8")
            images.append(im)
        img, other = images
        if img.dtype != other.dtype:
            raise TypeError(err + "Img and other need to be of the same dtype")
        for name, im in (("Img", img), ("Other", other)):
            if im.dim() not in (3, 4):
                raise ValueError(err + name + " needs to have 3 or 4 dimensions, C-H-W or N-C-H-W")
            if im.shape[-3] not in (1, 3):
                raise ValueError(err + name + " needs to have 1 or 3 channels")
        if img.shape[-3] != other.shape[-3]:
            raise ValueError(err + "Img and other need to have the same number of channels")
        for name, im in (("Img", img), ("Other", other)):
            if tuple(im.shape[-2:]) != tuple(self.shape[1:]):
                raise ValueError(err + name + " needs to have the H-W shape of the flow")
            if im.dim() == 4 and im.shape[0] != self.shape[0]:
                raise ValueError(err + name + " needs to have the batch size of the flow")
        if self.shape[1] < 2 or self.shape[2] < 2:
            raise ValueError(err + "Flow field needs to be at least 2 pixels high and wide")
        window = _ssim.WINDOW if window is None else window
        if not isinstance(window, int) or isinstance(window, bool):
            raise TypeError(err + "Window needs to be an integer")
        if window not in (3, 5, 7):
            raise ValueError(err + "Window needs to be 3, 5 or 7")
        values = []
        for name, val, default in (("C1", c1, _ssim.C1), ("C2", c2, _ssim.C2)):
            val = default if val is None else val
            if not isinstance(val, (int, float)) or isinstance(val, bool):
                raise TypeError(err + name + " needs to be an integer or a float")
            # (the kernels take float32: a value that rounds to 0 or to infinity there is out of range)
            if not (math.isfinite(val) and val > 0 and 0 < float(np.float32(val)) < float('inf')):
                raise ValueError(err + name + " needs to be finite and larger than 0")
            values.append(float(val))
        consider_mask = True if consider_mask is None else consider_mask
        if not isinstance(consider_mask, bool):
            raise TypeError(err + "Consider_mask needs to be boolean")
        images = []
        for im in (img, other):
            im = im.detach()
            if im.device != self._device:
                im = im.to(self._device)
            images.append(im.contiguous())
        return (self._fv, (self._mask if consider_mask else None), images[0], images[1], -1.0 if self._ref == 's' else 1.0,
                window, values[0], values[1])

    def ssim_stats(self, img, other, window: int = None, c1: float = None, c2: float = None, consider_mask: bool = None) -> dict:
        """The structural-similarity penalty of this flow between two frames, per batch element: the data term ARFlow, UFlow and the
        monodepth line weight against the brightness difference.  `img` is the frame on the flow's own grid, `other` the frame the
        flow points into, as in :meth:`photometric_stats`: tensors or arrays of one dtype, float32 (scale 0 .. 1) or uint8 (read as
        s / 255), C-H-W or N-C-H-W with the same 1 or 3 channels.  `other` is sampled bilinearly where the flow points; per channel,
        over the `window` x `window` box around a pixel (3, 5 or 7, default 3), the means, variances and the covariance of the two
        frames give SSIM = (2 mx my + `c1`) (2 sxy + `c2`) / ((mx^2 + my^2 + `c1`) (sxx + syy + `c2`)), `c1` default 1e-4, `c2`
        default 9e-4, and the penalty of the pixel is the mean over the channels of clamp((1 - SSIM) / 2, 0, 1).  A pixel is USABLE
        where it is valid in this flow's mask (with `consider_mask` False: everywhere) and its sample's taps lie in the frame; a
        window holds its usable pixels only and is normalised by their number, and a pixel is KNOWN where it is usable.  Returns a
        dict of tensors on the flow's device: 'count' int64 [N], the known pixels; 'sum', 'max' float64 [N] over them; 'ssim' float64
        [N], sum / count, NaN without a known pixel; 'fill' float64 [N], the share of the window pixels of the known pixels that were
        usable.  One pass of ofl_ssim.hip from LDS tiles: neither the warped image nor a pooled tensor is written, float64 sums in a
        fixed order (bitwise reproducible, independent of the batch), nothing is read back to the host.  Not
        differentiable: see :meth:`ssim`."""
        ops = self._ssim_operands(img, other, window, c1, c2, consider_mask)
        rec, _ = _ssim.flow_ssim(*ops)
        rec = rec.to(self._device)
        return {'count': rec[:, 0].to(torch.int64), 'sum': rec[:, 1].clone(), 'max': rec[:, 2].clone(), 'ssim': rec[:, 1] / rec[:, 0],
                'fill': rec[:, 3] / (rec[:, 0] * float(ops[5] * ops[5]))}

    def ssim_map(self, img, other, window: int = None, c1: float = None, c2: float = None, consider_mask: bool = None) -> torch.Tensor:
        """The penalty of :meth:`ssim_stats` at every pixel: float32 N-H-W on the flow's device, 0 where the pixel is not known (the
        kernel writes nothing else).  Not differentiable: see :meth:`ssim`."""
        ops = self._ssim_operands(img, other, window, c1, c2, consider_mask)
        return _ssim.flow_ssim(*ops, want_map=True, want_record=False)[1].to(self._device)

    def ssim(self, img, other, window: int = None, c1: float = None, c2: float = None, consider_mask: bool = None) -> torch.Tensor:
        """The mean of :meth:`ssim_stats` over the known pixels per batch element: float32 [N] on the flow's device (the float64
        quotient rounded once; NaN for an element without a known pixel).  Differentiable with respect to the flow vectors ONLY --
        the SSIM term of an unsupervised flow loss.  The images carry no gradient, even if they require one; an element without a
        known pixel has gradient 0.  The backward pass gathers (no atomics): it is bitwise reproducible."""
        return _ssim.ssim(*self._ssim_operands(img, other, window, c1, c2, consider_mask)).to(self._device)

    # ------------------------------------------------------------------------------------------
    # cost volume (an extension: the reference has no such method)
    # ------------------------------------------------------------------------------------------
    def cost_volume(self, feat, other, radius: int = None, consider_mask: bool = None) -> torch.Tensor:
        """The local cost volume of PWC-Net, LiteFlowNet, ARFlow and UFlow: the features `feat` on this flow's own grid correlated with
        the features `other` of the frame the flow points into, warped by this flow, over a (2 `radius` + 1)^2 window.  `feat` and
        `other` are float32 tensors or arrays, C-H-W (one image for the whole batch) or N-C-H-W, with the same C >= 1; `radius` is 1,
        2, 3 or 4 (default 4: 81 offsets).  `other` is sampled bilinearly where the flow points, as :meth:`apply` does on a 't' flow;
        a pixel is USABLE where it is valid in this flow's mask (with `consider_mask` False: everywhere) and its sample's taps lie in
        the frame, and the warped value W' is the sample where the pixel is usable and 0 elsewhere and outside the frame (PWC-Net's
        warp with its mask).  Returns float32 N-D-H-W on the flow's device, D = (2 `radius` + 1)^2: entry o = (dy + radius) (2 `radius`
        + 1) + dx + radius at pixel p is the mean over the channels of feat(p) * W'(p + (dy, dx)).  One pass of ofl_cost_volume.hip
        from LDS tiles: the warped tensor is never written, every sum runs in a fixed float32 order (bitwise reproducible, independent
        of the batch), nothing is read back to the host.  Differentiable with respect to `feat`, `other` and the flow
        vectors (not the mask); the gradients of `feat` and of the warped tensor are gathers without atomics.  Stride, dilation,
        16-bit and channels_last features are not supported."""
        err = "Error computing cost volume: "
        feats = []
        for name, ft in (("Feat", feat), ("Other", other)):
            if isinstance(ft, np.ndarray):
                if ft.dtype != np.float32:
                    raise TypeError(err + name + " needs to be of dtype float32")
                ft = torch.from_numpy(ft)
            if not isinstance(ft, torch.Tensor):
                raise TypeError(err + name + " needs to be a torch tensor or a numpy array")
            if ft.dtype != torch.float32:
                raise TypeError(err + name + " needs to be of dtype float32")
            feats.append(ft)
        for name, ft in zip(("Feat", "Other"), feats):
            if ft.dim() not in (3, 4):
                raise ValueError(err + name + " needs to have 3 or 4 dimensions, C-H-W or N-C-H-W")
            if ft.shape[-3] < 1:
                raise ValueError(err + name + " needs to have at least 1 channel")
        if feats[0].shape[-3] != feats[1].shape[-3]:
            raise ValueError(err + "Feat and other need to have the same number of channels")
        for name, ft in zip(("Feat", "Other"), feats):
            if tuple(ft.shape[-2:]) != tuple(self.shape[1:]):
                raise ValueError(err + name + " needs to have the H-W shape of the flow")
            if ft.dim() == 4 and ft.shape[0] != self.shape[0]:
                raise ValueError(err + name + " needs to have the batch size of the flow")
        if self.shape[1] < 2 or self.shape[2] < 2:
            raise ValueError(err + "Flow field needs to be at least 2 pixels high and wide")
        radius = _cost_volume.RADIUS if radius is None else radius
        if not isinstance(radius, int) or isinstance(radius, bool):
            raise TypeError(err + "Radius needs to be an integer")
        if not 1 <= radius <= _cost_volume.MAX_RADIUS:
            raise ValueError(err + "Radius needs to be 1, 2, 3 or 4")
        consider_mask = True if consider_mask is None else consider_mask
        if not isinstance(consider_mask, bool):
            raise TypeError(err + "Consider_mask needs to be boolean")
        feats = [(ft if ft.device == self._device else ft.to(self._device)).contiguous() for ft in feats]      # (they keep their grad_fn)
        return _cost_volume.cost_volume(self._fv, (self._mask if consider_mask else None), feats[0], feats[1],
                                        -1.0 if self._ref == 's' else 1.0, radius).to(self._device)

    def corr_lookup(self, feat, other, radius: int = None, levels: int = None, consider_mask: bool = None) -> torch.Tensor:
        """The correlation lookup of RAFT-style networks (RAFT, GMA, SEA-RAFT, CRAFT), computed on the fly at the looked-up positions:
        the all-pairs volume is never formed.  `feat` holds the features on this flow's own grid, float32 C-H-W (one image for the
        whole batch) or N-C-H-W.  `other` holds the features of the frame the flow points into: either one tensor like `feat`, with the
        same C and H-W, from which `levels` levels (1 to 6, default 4) are made by `corr_pyramid` (avg_pool2d(2, 2), in torch, so that
        the gradient flows back through the pooling), or a sequence of level tensors N-C-H_l-W_l / C-H_l-W_l of any sizes of at least
        1 x 1 with the same C (`levels` is then ignored).  `radius` r is 1, 2, 3 or 4 (default 4).  Returns float32 N-(L D)-H-W on the
        flow's device, D = (2 r + 1)^2: entry l D + (dx + r) (2 r + 1) + dy + r at pixel p is the bilinear sample (zeros outside the
        level) of the correlation feat(p) . other_l / sqrt(C) at (p + flow(p)) / 2^l + (dx, dy) for an 's' flow, p - flow(p) for a 't'
        flow -- the x offset is the outer index, RAFT's channel order.  All entries of a pixel are 0 where it is not valid in this
        flow's mask (with `consider_mask` False: the mask is ignored) or a vector component is not finite.  One launch of
        ofl_corr_lookup.hip per level, every sum in a fixed float32 order (bitwise reproducible, independent of the batch; DESIGN.md
        3.25), nothing is read back to the host.  Differentiable with respect to `feat` and `other` (or each level tensor), by gathers
        without atomics; NOT differentiable with respect to the flow vectors or the mask: RAFT detaches the coordinates before every
        lookup.  16-bit and channels_last features are not supported."""
        err = "Error computing correlation lookup: "

        def as_tensor(name, ft):
            if isinstance(ft, np.ndarray):
                if ft.dtype != np.float32:
                    raise TypeError(err + name + " needs to be of dtype float32")
                ft = torch.from_numpy(ft)
            if not isinstance(ft, torch.Tensor):
                raise TypeError(err + name + " needs to be a torch tensor or a numpy array")
            if ft.dtype != torch.float32:
                raise TypeError(err + name + " needs to be of dtype float32")
            if ft.dim() not in (3, 4):
                raise ValueError(err + name + " needs to have 3 or 4 dimensions, C-H-W or N-C-H-W")
            if ft.shape[-3] < 1:
                raise ValueError(err + name + " needs to have at least 1 channel")
            if ft.dim() == 4 and ft.shape[0] != self.shape[0]:
                raise ValueError(err + name + " needs to have the batch size of the flow")
            return ft
        feat = as_tensor("Feat", feat)
        if tuple(feat.shape[-2:]) != tuple(self.shape[1:]):
            raise ValueError(err + "Feat needs to have the H-W shape of the flow")
        pyramid = isinstance(other, (list, tuple))
        if pyramid:
            if not 1 <= len(other) <= _corr_lookup.MAX_LEVELS:
                raise ValueError(err + "Other needs to hold 1 to 6 levels")
            level_list = [as_tensor("Other level %d" % l, lv) for l, lv in enumerate(other)]
            for l, lv in enumerate(level_list):
                if lv.shape[-2] < 1 or lv.shape[-1] < 1:
                    raise ValueError(err + "Other level %d is empty" % l)
        else:
            other = as_tensor("Other", other)
            if tuple(other.shape[-2:]) != tuple(self.shape[1:]):
                raise ValueError(err + "Other needs to have the H-W shape of the flow")
            level_list = [other]
        for lv in level_list:
            if lv.shape[-3] != feat.shape[-3]:
                raise ValueError(err + "Feat and other need to have the same number of channels")
        radius = _corr_lookup.RADIUS if radius is None else radius
        if not isinstance(radius, int) or isinstance(radius, bool):
            raise TypeError(err + "Radius needs to be an integer")
        if not 1 <= radius <= _corr_lookup.MAX_RADIUS:
            raise ValueError(err + "Radius needs to be 1, 2, 3 or 4")
        if not pyramid:
            levels = _corr_lookup.LEVELS if levels is None else levels
            if not isinstance(levels, int) or isinstance(levels, bool):
                raise TypeError(err + "Levels needs to be an integer")
            if not 1 <= levels <= _corr_lookup.MAX_LEVELS:
                raise ValueError(err + "Levels needs to be 1 to 6")
            if min(other.shape[-2:]) >> (levels - 1) < 1:
                raise ValueError(err + "Other level %d is empty" % (levels - 1))
        consider_mask = True if consider_mask is None else consider_mask
        if not isinstance(consider_mask, bool):
            raise TypeError(err + "Consider_mask needs to be boolean")
        to_dev = lambda ft: (ft if ft.device == self._device else ft.to(self._device)).contiguous()      # (they keep their grad_fn)
        feat = to_dev(feat)
        level_list = [to_dev(lv) for lv in level_list] if pyramid else _corr_lookup.corr_pyramid(to_dev(other), levels)
        return _corr_lookup.corr_lookup(self._fv, (self._mask if consider_mask else None), feat, level_list,
                                        -1.0 if self._ref == 's' else 1.0, radius).to(self._device)

    def upsample_convex(self, weights, factor: int = None, consider_mask: bool = None) -> FlowAlias:
        """The learned convex upsampling that ends every refinement iteration of RAFT-style networks (RAFT, GMA, CRAFT, SEA-RAFT,
        FlowFormer, RAFT-Stereo): `weights` holds the 9 k^2 logits the network predicts per pixel of this (coarse) flow, float32
        N-(9 k^2)-H-W, or (9 k^2)-H-W for a batch of 1, in RAFT's channel order -- channel t k^2 + i k + j belongs to tap
        t = 3 (dy + 1) + (dx + 1), sub-row i and sub-column j.  `factor` k is 2, 4 or 8 and is inferred from the channel count when None.
        Returns a flow of shape N-(k H)-(k W) with the same reference and device: fine pixel (k y + i, k x + j) is the mix of the 3 x 3
        neighbourhood of k flow(y, x), zeros outside the frame, under the softmax of its nine logits.  Its mask is this flow's, every bit
        replicated over its k x k block (with `consider_mask` False: no mask, i.e. all True); masked pixels still lend their vectors to
        their neighbours.  One launch of ofl_upsample.hip, float64 arithmetic in a fixed order rounded once, bitwise
        reproducible and independent of the batch.  Differentiable with respect to the logits and the flow vectors, without atomics;
        not with respect to the mask.  16-bit and channels_last logits, other factors and other neighbourhoods are not supported: under
        autocast the caller casts the logits, as RAFT's own `.float()` does."""
        err = "Error upsampling flow: "
        if isinstance(weights, np.ndarray):
            if weights.dtype != np.float32:
                raise TypeError(err + "Weights need to be of dtype float32")
            weights = torch.from_numpy(weights)
        if not isinstance(weights, torch.Tensor):
            raise TypeError(err + "Weights need to be a torch tensor or a numpy array")
        if weights.dtype != torch.float32:
            raise TypeError(err + "Weights need to be of dtype float32")
        if weights.dim() not in (3, 4):
            raise ValueError(err + "Weights need to have 3 or 4 dimensions, (9 k^2)-H-W or N-(9 k^2)-H-W")
        if weights.dim() == 3:
            weights = weights.unsqueeze(0)
        channels = int(weights.shape[1])
        if channels not in [9 * k * k for k in _upsample.FACTORS]:
            raise ValueError(err + "Weights need to have 9 k^2 channels with k 2, 4 or 8, but got {}".format(channels))
        if factor is not None:
            if isinstance(factor, bool) or not isinstance(factor, int):
                raise TypeError(err + "Factor needs to be an integer")
            if factor not in _upsample.FACTORS:
                raise ValueError(err + "Factor needs to be 2, 4 or 8")
            if 9 * factor * factor != channels:
                raise ValueError(err + "Factor {} contradicts the {} channels of the weights".format(factor, channels))
        factor = _upsample.factor_of(channels)
        if weights.shape[0] != self.shape[0]:
            raise ValueError(err + "Weights need to have the batch size of the flow")
        if tuple(weights.shape[-2:]) != tuple(self.shape[1:]):
            raise ValueError(err + "Weights need to have the H-W shape of the flow")
        consider_mask = True if consider_mask is None else consider_mask
        if not isinstance(consider_mask, bool):
            raise TypeError(err + "Consider_mask needs to be boolean")
        if weights.device != self._device:
            weights = weights.to(self._device)              # (keeps its grad_fn)
        out, out_mask = _upsample.upsample_convex(self._fv, (self._mask if consider_mask else None), weights, factor)
        return Flow(out, self._ref, out_mask, device=self._device)

    def propagate(self, query, key=None, radius: int = None, consider_mask: bool = None) -> FlowAlias:
        """The flow propagation by self-attention of GMFlow, UniMatch and their stereo and depth siblings, which carries matched vectors
        into occluded and out-of-frame regions: the vector at p becomes sum_q softmax_q(query(p) . key(q) / sqrt(C)) flow(q).  `query`
        and `key` are float32 tensors, C-H-W (one image for the whole batch) or N-C-H-W, with this flow's H-W and the same C >= 1;
        `key` None means `key` = `query` (the projections of the network are the caller's layers).  `radius` None is the global form,
        over ALL positions q, as at 1/8 scale; `radius` 1, 2, 3 or 4 is the local form over the (2 `radius` + 1)^2 window of p, as at
        1/4 scale, in which a position outside the frame takes part with the logit 0 and the vector (0, 0): the zero padding of
        `unfold`, which the trained networks expect.  A position that is not valid in this flow's mask is EXCLUDED from the softmax
        (with `consider_mask` False: none is), so the flow's invalid pixels are filled from its valid ones by feature similarity.
        Returns a flow of the same shape, reference and device; its mask is True everywhere but at the EMPTY pixels, for which no
        position inside the frame takes part (the whole image masked; locally, the whole window masked) and whose vector is (0, 0).
        One launch of ofl_propagate.hip: the global form streams the key past tiles of pixels with a running maximum and three running
        float64 sums per pixel, so that the (H W)^2 volume is never formed; the local form computes the window's logits from LDS tiles
        without an unfold; every sum has a fixed order, bitwise reproducible and independent of the batch.
        Differentiable with respect to `query`, `key` and the flow vectors, without atomics; not with respect to the mask.  16-bit and
        channels_last features, another temperature, another border rule and a double backward are not supported."""
        err = "Error propagating flow: "
        key = query if key is None else key
        feats = []
        for name, ft in (("Query", query), ("Key", key)):
            if isinstance(ft, np.ndarray):
                if ft.dtype != np.float32:
                    raise TypeError(err + name + " needs to be of dtype float32")
                ft = torch.from_numpy(ft)
            if not isinstance(ft, torch.Tensor):
                raise TypeError(err + name + " needs to be a torch tensor or a numpy array")
            if ft.dtype != torch.float32:
                raise TypeError(err + name + " needs to be of dtype float32")
            feats.append(ft)
        for name, ft in zip(("Query", "Key"), feats):
            if ft.dim() not in (3, 4):
                raise ValueError(err + name + " needs to have 3 or 4 dimensions, C-H-W or N-C-H-W")
            if ft.shape[-3] < 1:
                raise ValueError(err + name + " needs to have at least 1 channel")
        if feats[0].shape[-3] != feats[1].shape[-3]:
            raise ValueError(err + "Query and key need to have the same number of channels")
        for name, ft in zip(("Query", "Key"), feats):
            if tuple(ft.shape[-2:]) != tuple(self.shape[1:]):
                raise ValueError(err + name + " needs to have the H-W shape of the flow")
            if ft.dim() == 4 and ft.shape[0] != self.shape[0]:
                raise ValueError(err + name + " needs to have the batch size of the flow")
        if radius is not None:
            if not isinstance(radius, int) or isinstance(radius, bool):
                raise TypeError(err + "Radius needs to be an integer or None")
            if not 1 <= radius <= _propagate.MAX_RADIUS:
                raise ValueError(err + "Radius needs to be None, 1, 2, 3 or 4")
        consider_mask = True if consider_mask is None else consider_mask
        if not isinstance(consider_mask, bool):
            raise TypeError(err + "Consider_mask needs to be boolean")
        feats = [(ft if ft.device == self._device else ft.to(self._device)).contiguous() for ft in feats]      # (they keep their grad_fn)
        out, out_mask = _propagate.propagate(self._fv, (self._mask if consider_mask else None), feats[0], feats[1], radius)
        return Flow(out, self._ref, out_mask, device=self._device)

    def match_local(self, feat, other, radius: int = None, consider_mask: bool = None, return_prob: bool = None):
        """The local matching of the refinement stage of GMFlow and UniMatch, as at 1/4 scale: the features `other` of the frame this
        flow points into are warped by the flow, every pixel p of `feat` -- the features on the flow's own grid -- is correlated with
        the (2 `radius` + 1)^2 window of the warped features around it, the softmax of feat(p) . W'(p + o) / sqrt(C) over the window
        gives the expected offset E[o], and the vector at p becomes flow(p) + E[o] for an 's' flow, flow(p) - E[o] for a 't' flow
        (whose sample position is p - flow(p)).  `feat` and `other` are float32 tensors or arrays, C-H-W (one image for the whole
        batch) or N-C-H-W, with this flow's H-W and the same C >= 1; `radius` is 1, 2, 3 or 4 (default 4: 81 offsets).  The warp is
        that of :meth:`cost_volume`: a pixel is USABLE where it is valid in this flow's mask (with `consider_mask` False: everywhere)
        and its sample's taps lie in the frame, and the warped value W' is the sample where the pixel is usable and 0 elsewhere.  A
        window position OUTSIDE the frame takes no part in the softmax (GMFlow's rule); one inside always does, with W' = 0 if it is
        not usable.  Returns a flow of the same shape, reference, device and mask; with `return_prob` True a tuple of that flow and the
        softmax weight of the best position of every pixel, float32 N-H-W.  One launch of ofl_local_match.hip from LDS tiles: the
        warped tensor and the D planes of the volume are never written, the softmax runs in float64 in a fixed order (bitwise
        reproducible, independent of the batch), nothing is read back to the host.  Differentiable with respect to
        `feat`, `other` and the flow vectors (not the mask, not through the probability): the gradients of `feat` and of the warped
        tensor are gathers without atomics, those of `other` and of the warp's part of the vectors follow from the latter through the
        backward of :meth:`cost_volume`'s warp, with that backward's own properties; pass a flow with detached vectors for GMFlow's
        detached warp.  The 1-D stereo variant, another
        temperature, the full match probability, 16-bit and channels_last features and a double backward are not supported."""
        err = "Error matching flow locally: "
        feats = []
        for name, ft in (("Feat", feat), ("Other", other)):
            if isinstance(ft, np.ndarray):
                if ft.dtype != np.float32:
                    raise TypeError(err + name + " needs to be of dtype float32")
                ft = torch.from_numpy(ft)
            if not isinstance(ft, torch.Tensor):
                raise TypeError(err + name + " needs to be a torch tensor or a numpy array")
            if ft.dtype != torch.float32:
                raise TypeError(err + name + " needs to be of dtype float32")
            feats.append(ft)
        for name, ft in zip(("Feat", "Other"), feats):
            if ft.dim() not in (3, 4):
                raise ValueError(err + name + " needs to have 3 or 4 dimensions, C-H-W or N-C-H-W")
            if ft.shape[-3] < 1:
                raise ValueError(err + name + " needs to have at least 1 channel")
        if feats[0].shape[-3] != feats[1].shape[-3]:
            raise ValueError(err + "Feat and other need to have the same number of channels")
        for name, ft in zip(("Feat", "Other"), feats):
            if tuple(ft.shape[-2:]) != tuple(self.shape[1:]):
                raise ValueError(err + name + " needs to have the H-W shape of the flow")
            if ft.dim() == 4 and ft.shape[0] != self.shape[0]:
                raise ValueError(err + name + " needs to have the batch size of the flow")
        if self.shape[1] < 2 or self.shape[2] < 2:
            raise ValueError(err + "Flow field needs to be at least 2 pixels high and wide")
        radius = _local_match.RADIUS if radius is None else radius
        if not isinstance(radius, int) or isinstance(radius, bool):
            raise TypeError(err + "Radius needs to be an integer")
        if not 1 <= radius <= _local_match.MAX_RADIUS:
            raise ValueError(err + "Radius needs to be 1, 2, 3 or 4")
        consider_mask = True if consider_mask is None else consider_mask
        if not isinstance(consider_mask, bool):
            raise TypeError(err + "Consider_mask needs to be boolean")
        return_prob = False if return_prob is None else return_prob
        if not isinstance(return_prob, bool):
            raise TypeError(err + "Return_prob needs to be boolean")
        feats = [(ft if ft.device == self._device else ft.to(self._device)).contiguous() for ft in feats]      # (they keep their grad_fn)
        out, prob = _local_match.local_match(self._fv, (self._mask if consider_mask else None), feats[0], feats[1],
                                             -1.0 if self._ref == 's' else 1.0, radius, return_prob)
        flow = Flow(out, self._ref, self._mask, device=self._device)
        return (flow, prob.to(self._device)) if return_prob else flow

    # ------------------------------------------------------------------------------------------
    # composition (flow_class.py:1648-1810)
    # ------------------------------------------------------------------------------------------
    def combine_with(self, flow: FlowAlias, mode: int, thresholded: bool = None) -> FlowAlias:
        """flow_1 (+) flow_2 = flow_3 for two flows of equal shape and reference; `mode` names the unknown.
        Mode 3 is ONE fused launch (gather of (u, v, mask) + vector add + mask AND)."""
        if not isinstance(flow, Flow):
            raise TypeError("Error combining flows: Flow need to be of type 'Flow'")
        if self.shape != flow.shape:
            raise ValueError("Error combining flows: Flow fields need to have the same shape, including batch size")
        if self.ref != flow.ref:
            raise ValueError("Error combining flows: Flow fields need to have the same reference")
        if self._device != flow._device:
            flow = flow.to_device(self._device)
        if mode not in [1, 2, 3]:
            raise ValueError("Error combining flows: Mode needs to be 1, 2 or 3")
        thresholded = False if thresholded is None else thresholded
        if not isinstance(thresholded, bool):
            raise TypeError("Error combining flows: Thresholded needs to be a boolean")
        speculative = None
        if mode == 3 and not (self._flags_known() and flow._flags_known()):
            # flags not known yet: launch the fused composition right away; it returns both operands' flag words as a
            # by-product, and the reference's validation / early-exit decisions are taken afterwards (result discarded
            # if one of them fires).  One pass over the data instead of validation passes + the composition.
            speculative = self._combine3(flow, speculative=True)
        self._require_finite("Error setting flow vectors: " if speculative is not None else "Error combining flows: ")
        flow._require_finite("Error setting flow vectors: " if speculative is not None else "Error combining flows: ")

        bit = _native.FLAG_NZ_THR_MASKED if thresholded else _native.FLAG_NZ_MASKED
        if self._all_zero(bit):                                                      # flow_class.py:1729-1737
            return flow
        if flow._all_zero(bit):                                                      # :1738-1744
            return self if mode == 3 else self.invert()

        ref = self._ref
        if mode == 3:
            if speculative is not None and not (flow if ref == 't' else self)._all_zero(_native.FLAG_NZ_THR):
                return speculative
            return self._combine3(flow)
        if mode == 1:
            if ref == 's':                                                           # :1759-1760
                # flow - (flow_inv_t + flow_inv_t.apply(self.switch_ref())).apply(self) with flow_inv_t = flow.invert('t') =
                # Flow(-flow.vecs, 't'): the inner sum is the fused mode-3 launch (the negation folded into its signs), the
                # outer difference the epilogue of the second gather
                return flow._minus_applied(self.switch_ref()._combine3(flow, result_is_warper=True, negated_warper=True), self)
            # self.invert().apply(flow - self)   (:1763): the difference is formed while the source box is staged
            inv = self.invert()
            if inv._all_zero(_native.FLAG_NZ_THR):
                return inv.apply(flow - self)
            warped, valid, _ = inv._warp(flow._fv, flow._and_masks(self._mask), True, True, t_minus=self._vecs)
            return Flow._wrap(warped, 't', valid, self._device, made_from=(flow._fv, flow._mask, self._mask, inv._mask))
        if ref == 's':                                                               # mode 2, :1768
            # self.apply(flow - self): the difference (and the AND of the two masks) is formed inside the splat
            if self._all_zero(_native.FLAG_NZ_THR) or not get_pure_pytorch():        # (apply's early exit / griddata gate)
                return self.apply(flow - self)
            warped, valid, dflags = self._warp(flow._vecs, flow._mask, True, True, t_minus=self._vecs)
            return Flow._wrap(warped, 's', valid, self._device, flags=dflags, made_from=(flow._fv, flow._mask, self._mask))
        if not get_pure_pytorch():
            # the reference resamples (vectors, mask) at the float positions grid - flow of a SECOND flow with a griddata call of its own
            # (:1776-1796): a whole-frame point query over C channels, which the mesh kernels do not have
            _griddata_unavailable("combine_with(mode=2, ref='t')")
        return flow._minus_applied(flow, self.invert().apply(self))                  # :1773  flow - flow.apply(...)

    def _minus_applied(self, warper: FlowAlias, target: FlowAlias) -> FlowAlias:
        """self - warper.apply(target) for a 't'-referenced `warper` and a flow `target`: one launch, the subtraction is
        the gather's epilogue (1 * self + (-1) * G: the same fp32 operation as the reference's `-`); masks AND as in
        flow_class.py:490-531 / 921-934.  The thresholded early exit of `apply` takes the plain path."""
        if warper._ref != 't' or warper._all_zero(_native.FLAG_NZ_THR) or self.shape[0] != warper.shape[0] \
                or target.shape[0] != warper.shape[0]:
            return self - warper.apply(target)
        warper._require_finite("Error applying flow to a target: ")
        vecs, valid, _, _ = _native.warp_bwd(warper._vecs, target._vecs, src_mask=target._mask, flow_mask=warper._mask,
                                             want_valid=True, addend=self._vecs, a_sign=1.0, g_sign=-1.0)
        if self._mask is not None and self._mask is not warper._mask:
            valid = valid & self._mask
        return Flow._wrap(vecs, self._ref, valid, self._device, fresh=True)

    def _combine3(self, flow: FlowAlias, speculative: bool = False, result_is_warper: bool = False,
                  negated_warper: bool = False) -> FlowAlias:
        """mode 3: 't'  f3 = f2 + G(f2, f1),  m3 = m2 & theta(G(f2, [m1]))           (flow_class.py:1808)
                   's'  f3 = f1 + G(-f1, f2), m3 = m1 & theta(G(-f1, [m2]))          (flow_class.py:1804)
        `negated_warper` ('t' only): `flow` stands for Flow(-flow.vecs, 't', flow.mask) -- `flow.invert('t')` of a
        forward flow -- without the negated copy: positions and addend change sign in the kernel, flags do not."""
        a_sign = 1.0
        if self._ref == 't':
            warper, sign, src = flow, 1.0, self
            if negated_warper:
                sign, a_sign = -1.0, -1.0
        else:
            warper, sign, src = self, -1.0, flow
        if not speculative and warper._all_zero(_native.FLAG_NZ_THR):
            # apply_flow's thresholded early exit inside .apply (utils.py:497): the gather is the identity
            w_ = warper._negated('t') if a_sign < 0 else warper
            return w_ + Flow._wrap(src._vecs, src._ref, src._and_masks(warper._mask), self._device)
        # (`result_is_warper`: the result will warp something next, so its own flag word is worth the ~5 % it costs here)
        res = _native.warp_bwd(warper._vecs, src._vecs, flow_sign=sign, src_mask=src._mask,
                               flow_mask=warper._mask, want_valid=True, addend=warper._vecs, a_sign=a_sign,
                               want_flags=speculative, want_src_flags=speculative, want_dst_flags=result_is_warper)
        vecs, valid, wf, sf = res[:4]
        if speculative:
            if not warper._flags_known():
                warper._set_pending_flags(wf)
            if not src._flags_known():
                src._set_pending_flags(sf)
        return Flow._wrap(vecs, self._ref, valid, self._device, flags=res[4] if result_is_warper else None, fresh=True)

    # ------------------------------------------------------------------------------------------
    # general composition (flow_class.py:1812-1939)
    # ------------------------------------------------------------------------------------------
    def combine(self, other: FlowAlias, mode: int, ref: str = None) -> FlowAlias:
        """flow_1 (+) flow_2 = flow_3 for two flows of equal shape and ANY references, result in reference `ref`
        (default: that of self); `mode` names the unknown.  Same results as the reference (flow_class.py:1812-1939, every
        (mode, self.ref, other.ref, ref) cell pinned by fixtures), computed from a per-cell PLAN (`_combine_plan`): at most
        one `switch_ref`, then ONE fused launch -- the linear combination of the two fields rides the epilogue of the
        backward gather (`a_sign * close + g_sign * G(+-close, far)`) or is formed inside the forward splat (`data - data_b`),
        and the `invert` of the carrying flow is a sign of the kernel's sample positions / end points."""
        if not isinstance(other, Flow):
            raise TypeError("Error combining flows: Flow need to be of type 'Flow'")
        if self.shape != other.shape:
            raise ValueError("Error combining flows: Flow fields need to have the same shape, including batch size")
        if self._device != other._device:
            other = other.to_device(self._device)
        if mode not in [1, 2, 3]:
            raise ValueError("Error combining flows: Mode needs to be 1, 2 or 3")
        ref = self._ref if ref is None else get_valid_ref(ref)
        plan = _combine_plan(mode, self._ref, other._ref, ref)
        close, far = (self, other) if plan.close_is_self else (other, self)
        if plan.switch_far:                                  # the far field onto the pivot grid (a splat, or a relabel)
            far = far.switch_ref()
        if plan.close_on_goal:
            result = close._carry_back_and_add(far, plan.carry_sign, plan.sign_close, plan.sign_far)
        else:
            result = close._add_and_carry_forward(far, plan.carry_sign, plan.sign_close, plan.sign_far)
        result._ref = ref
        return result

    def _carry_back_and_add(self, field: FlowAlias, carry_sign: float, sign_self: float, sign_field: float) -> FlowAlias:
        """sign_self * self + sign_field * W(field), with W the backward warp of `field` (a flow on another grid) onto this
        flow's grid along `self` (carry_sign +1: self is 't'-referenced) or along Flow(-self.vecs, 't') (carry_sign -1: self
        is 's'-referenced and `invert('t')`-ed, flow_class.py:1081).  Vectors `s_self * self + s_field * G`, mask
        `theta(G(mask channel)) & self.mask` -- the reference's apply + two scalings + add (flow_class.py:921-934, 450-488,
        533-549), as the addend epilogue of one gather."""
        warper_zero = self._all_zero(_native.FLAG_NZ_THR)      # apply_flow's early exit (utils.py:497-498): W is the identity
        if warper_zero or self.shape[0] != field.shape[0] or not _COMBINE_FUSED:
            carrier = self if carry_sign > 0 else self._negated('t')
            return carrier.apply(field) * sign_field + self * sign_self
        self._require_finite("Error applying flow to a target: ")
        res = _native.warp_bwd(self._vecs, field._vecs, flow_sign=carry_sign, src_mask=field._mask, flow_mask=self._mask,
                               want_valid=True, addend=self._vecs, a_sign=sign_self, g_sign=sign_field)
        return Flow._wrap(res[0], self._ref, res[1], self._device, fresh=True)

    def _add_and_carry_forward(self, field: FlowAlias, carry_sign: float, sign_self: float, sign_field: float) -> FlowAlias:
        """P(sign_self * self + sign_field * field): the combination of two fields on one grid, carried to the other end of
        `self` by a forward splat along `self` (carry_sign +1: self is 's'-referenced) or along Flow(-self.vecs, 's')
        (carry_sign -1: self is 't'-referenced and `invert('s')`-ed, flow_class.py:1084).  A difference is formed inside the
        splat (`data - data_b`, the same fp32 subtraction: a + (-b) == a - b); a sum takes one elementwise pass first."""
        if sign_self > 0 and sign_field > 0:
            total, minus = self + field, None
        elif sign_self > 0:
            total, minus = self, field                       # self - field
        else:
            total, minus = field, self                       # field - self
        warper = self if carry_sign > 0 else Flow._wrap(self._fv, 's', self._mask, self._device, like=self, borrowed=True)
        if warper._all_zero(_native.FLAG_NZ_THR) or not get_pure_pytorch() or self.shape[0] != field.shape[0] or not _COMBINE_FUSED:
            carrier = self if carry_sign > 0 else self._negated('s')
            return carrier.apply(total if minus is None else total - minus)
        tmask = total._mask if minus is None else total._and_masks(minus._mask)
        warped, valid, dflags = warper._warp(total._fv if minus is None else total._vecs, tmask, True, True, flow_sign=carry_sign,
                                             t_minus=None if minus is None else minus._vecs)
        return Flow._wrap(warped, self._ref, valid, self._device, flags=dflags, made_from=(total._fv, tmask, self._mask))


class _CombinePlan(object):
    """How `Flow.combine` computes one (mode, self.ref, other.ref, ref) cell."""
    __slots__ = ("close_is_self", "switch_far", "close_on_goal", "carry_sign", "sign_close", "sign_far")

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)


_PLANS = {}


def _combine_plan(mode: int, self_ref: str, other_ref: str, out_ref: str) -> _CombinePlan:
    """The 24 plans of `Flow.combine`, derived from the geometry rather than tabulated by hand.

    Three instants 0, 1, 2; flow_1 spans (0, 1), flow_2 (1, 2), flow_3 (0, 2).  A flow lives on the pixel grid of its
    earlier instant when referenced 's', of its later one when 't'.  The unknown flow spans (a, b); the third instant is the
    PIVOT: both known flows touch it, and the unknown is the vector sum of the hop a -> pivot and the hop pivot -> b once
    both hops sit on one grid.  The result is wanted on the GOAL grid (a for 's', b for 't').  The known flow that touches
    the goal is CLOSE, the other FAR.  A known flow counts +1 for a hop that runs with it (earlier -> later), -1 against it.
      1. FAR must sit on the pivot grid: `switch_ref` if it sits on the unknown's far end instead.
      2. CLOSE on the goal grid: FAR is carried pivot -> goal by a backward warp along CLOSE (negated when CLOSE runs
         goal -> pivot), then the two hops are added there.   CLOSE on the pivot grid: the hops are added there, and the
         sum is carried pivot -> goal by a forward warp along CLOSE (negated when CLOSE runs goal -> pivot)."""
    key = (mode, self_ref, other_ref, out_ref)
    plan = _PLANS.get(key)
    if plan is not None:
        return plan
    spans = {1: (0, 1), 2: (1, 2), 3: (0, 2)}
    a, b = spans[mode]
    pivot = 3 - a - b
    goal = a if out_ref == 's' else b
    known = [k for k in (1, 2, 3) if k != mode]            # self is the lower-numbered known flow, other the higher
    grid = lambda span, r: span[0] if r == 's' else span[1]
    self_span, other_span = spans[known[0]], spans[known[1]]
    close_is_self = goal in self_span
    close_span, close_ref = (self_span, self_ref) if close_is_self else (other_span, other_ref)
    far_span, far_ref = (other_span, other_ref) if close_is_self else (self_span, self_ref)
    along = lambda u, v: 1.0 if u < v else -1.0           # a hop u -> v measured against a flow that runs earlier -> later
    hop_in, hop_out = along(a, pivot), along(pivot, b)     # a -> pivot, pivot -> b
    plan = _CombinePlan(
        close_is_self=close_is_self,
        switch_far=grid(far_span, far_ref) != pivot,
        close_on_goal=grid(close_span, close_ref) == goal,
        carry_sign=along(pivot, goal),
        sign_close=hop_out if goal == b else hop_in,       # CLOSE spans pivot-goal: the hop that ends (starts) at the goal
        sign_far=hop_in if goal == b else hop_out)
    _PLANS[key] = plan
    return plan


# the public methods that read a flow's flag word: each starts a new validation epoch under set_revalidate_every_call(True)
for _name in ('apply', 'track', 'switch_ref', 'invert', 'valid_target', 'valid_source', 'get_padding', 'is_zero', 'combine_with',
              'combine', 'visualise', 'visualise_arrows', 'error_stats', 'epe_map', 'epe', 'consistency', 'consistency_mask',
              'filter_consistent'):
    setattr(Flow, _name, _public(getattr(Flow, _name)))
del _name
