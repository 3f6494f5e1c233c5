"""Tensor-level wrappers round the `Flow` methods of the hot path (reference
``src/oflibpytorch/flow_operations.py:84-277, 306-409, 458-483``): same signatures, 3-D in -> 3-D out."""
from typing import Union

import numpy as np
import torch

from . import _chain, _sequence_loss
from ._corr_lookup import corr_pyramid  # noqa: F401  (exported by the package)
from .flow_class import Flow
from .utils import get_valid_ref

FlowAlias = 'Flow'


def _unwrap(result: Flow, like) -> torch.Tensor:
    return result.vecs if len(like.shape) > 3 else result.vecs.squeeze(0)


def combine_flows(input_1, input_2, mode: int, ref: str = None, thresholded: bool = None):
    """flow_1 (+) flow_2 = flow_3; `mode` (1, 2 or 3) names the unknown (flow_operations.py:84-188).
    Arrays / tensors of shape (N-)2-H-W or (N-)H-W-2 in, torch tensor (N-)2-H-W out."""
    if isinstance(input_1, Flow) and isinstance(input_2, Flow):
        print("AVOID - future deprecation warning: using combine_flows(flow_obj1, flow_obj2) is deprecated and may "
              "not work anymore in future versions - use flow_obj1.combine_with(flow_obj2) instead. combine_flows() "
              "will be reserved for use with Torch tensors and NumPy arrays only.")
        return input_1.combine_with(input_2, mode=mode, thresholded=thresholded)
    # deferred validation: the composition kernel reports finiteness / zero flags of both operands as a by-product
    result = Flow._deferred(input_1, ref).combine_with(Flow._deferred(input_2, ref), mode=mode, thresholded=thresholded)
    return _unwrap(result, input_1)


def switch_flow_ref(flow, input_ref: str) -> torch.Tensor:
    """flow_operations.py:191-207"""
    return _unwrap(Flow(flow, input_ref).switch_ref(), flow)


def invert_flow(flow, input_ref: str, output_ref: str = None) -> torch.Tensor:
    """flow_operations.py:210-228"""
    output_ref = input_ref if output_ref is None else output_ref
    return _unwrap(Flow(flow, input_ref).invert(output_ref), flow)


def valid_target(flow, ref: str, consider_mask: bool = None) -> torch.Tensor:
    """flow_operations.py:231-254"""
    area = Flow(flow, ref).valid_target(consider_mask)
    return area if len(flow.shape) > 3 else area.squeeze(0)


def valid_source(flow, ref: str, consider_mask: bool = None) -> torch.Tensor:
    """flow_operations.py:257-277"""
    area = Flow(flow, ref).valid_source(consider_mask)
    return area if len(flow.shape) > 3 else area.squeeze(0)


def get_flow_padding(flow, ref: str) -> list:
    """[top, bottom, left, right] per batch member (one list for 3-D input): Flow(flow, ref).get_padding()
    (flow_operations.py:280-303)"""
    p = Flow(flow, ref).get_padding()
    return p if len(flow.shape) > 3 else p[0]


def visualise_flow(flow, mode: str, range_max: float = None, return_tensor: bool = None):
    """Flow(flow).visualise(mode, range_max=..., return_tensor=...), 3-D in -> 3-D out (flow_operations.py:339-367)"""
    v = Flow(flow).visualise(mode=mode, range_max=range_max, return_tensor=return_tensor)
    return v if len(flow.shape) > 3 else v.squeeze(0)


def visualise_flow_arrows(flow, ref: str, grid_dist: int = None, img=None, scaling: Union[float, int] = None, colour: tuple = None,
                          thickness: int = None, return_tensor: bool = None):
    """Flow(flow, ref).visualise_arrows(...), 3-D in -> 3-D out (flow_operations.py:370-409)"""
    a = Flow(flow, ref).visualise_arrows(grid_dist=grid_dist, img=img, scaling=scaling, colour=colour, thickness=thickness,
                                         return_tensor=return_tensor)
    return a if len(flow.shape) > 3 else a.squeeze(0)


def get_flow_matrix(flow, ref: str, dof: int = None, method: str = None) -> torch.Tensor:
    """Flow(flow, ref).matrix(dof, method): float64 (N-)3-3, 3-D in -> 3 x 3 out (flow_operations.py:306-336)"""
    m = Flow(flow, ref).matrix(dof=dof, method=method)
    return m if len(flow.shape) > 3 else m.squeeze(0)


def flow_error_stats(flow, gt, mask=None, gt_mask=None, thresholds: Union[list, tuple] = None) -> dict:
    """Flow(flow, mask=mask).error_stats(Flow(gt, mask=gt_mask), thresholds=thresholds): the dict of Flow.error_stats for arrays /
    tensors (N-)2-H-W or (N-)H-W-2 with optional masks (N-)H-W; 3-D in -> entries without the batch dimension.  An extension
    (DESIGN.md 3.16): the reference has no such function."""
    stats = Flow(flow, 't', mask).error_stats(Flow(gt, 't', gt_mask), thresholds=thresholds)
    return stats if len(flow.shape) > 3 else {k: v.squeeze(0) for k, v in stats.items()}


def flow_epe(flow, gt, mask=None, gt_mask=None) -> torch.Tensor:
    """Flow(flow, mask=mask).epe(Flow(gt, mask=gt_mask)): the mean end-point error, float32 [N] (a scalar tensor for 3-D input),
    differentiable with respect to tensor inputs.  An extension."""
    e = Flow(flow, 't', mask).epe(Flow(gt, 't', gt_mask))
    return e if len(flow.shape) > 3 else e.squeeze(0)


def flow_consistency(flow, back, ref: str, mask=None, back_mask=None, alpha: float = None, beta: float = None) -> dict:
    """Flow(flow, ref, mask).consistency(Flow(back, ref, back_mask), alpha, beta): the dict of Flow.consistency for arrays / tensors
    (N-)2-H-W or (N-)H-W-2 with optional masks (N-)H-W; 3-D in -> entries without the batch dimension.  An extension:
    the reference has no such function."""
    res = Flow(flow, ref, mask).consistency(Flow(back, ref, back_mask), alpha=alpha, beta=beta)
    return res if len(flow.shape) > 3 else {k: v.squeeze(0) for k, v in res.items()}


def flow_smoothness(flow, img=None, mask=None, order: int = None, alpha: float = None, eps: float = None) -> torch.Tensor:
    """Flow(flow, mask=mask).smoothness(img, order, alpha, eps): the edge-aware smoothness loss, float32 [N] (a scalar tensor for 3-D
    input), differentiable with respect to a tensor `flow`.  An extension: the reference has no such function."""
    s = Flow(flow, 't', mask).smoothness(img, order=order, alpha=alpha, eps=eps)
    return s if len(flow.shape) > 3 else s.squeeze(0)


def flow_smoothness_stats(flow, img=None, mask=None, order: int = None, alpha: float = None, eps: float = None) -> dict:
    """Flow(flow, mask=mask).smoothness_stats(img, order, alpha, eps): the dict of Flow.smoothness_stats for arrays / tensors
    (N-)2-H-W or (N-)H-W-2 with an optional mask (N-)H-W; 3-D in -> entries without the batch dimension.  An extension (DESIGN.md
    3.19)."""
    stats = Flow(flow, 't', mask).smoothness_stats(img, order=order, alpha=alpha, eps=eps)
    return stats if len(flow.shape) > 3 else {k: v.squeeze(0) for k, v in stats.items()}


def flow_photometric(flow, img, other, ref: str, mask=None, eps: float = None) -> torch.Tensor:
    """Flow(flow, ref, mask).photometric(img, other, eps): the photometric loss between the frame `img` on the flow's grid and the
    frame `other` it points into, float32 [N] (a scalar tensor for 3-D input), differentiable with respect to a tensor `flow`.  An
    extension: the reference has no such function."""
    p = Flow(flow, ref, mask).photometric(img, other, eps=eps)
    return p if len(flow.shape) > 3 else p.squeeze(0)


def flow_photometric_stats(flow, img, other, ref: str, mask=None, eps: float = None) -> dict:
    """Flow(flow, ref, mask).photometric_stats(img, other, eps): the dict of Flow.photometric_stats for arrays / tensors (N-)2-H-W or
    (N-)H-W-2 with an optional mask (N-)H-W; 3-D in -> entries without the batch dimension.  An extension."""
    stats = Flow(flow, ref, mask).photometric_stats(img, other, eps=eps)
    return stats if len(flow.shape) > 3 else {k: v.squeeze(0) for k, v in stats.items()}


def flow_census(flow, img, other, ref: str, mask=None, patch: int = None, thresh: float = None, eps: float = None,
                q: float = None) -> torch.Tensor:
    """Flow(flow, ref, mask).census(img, other, patch, thresh, eps, q): the census loss between the frame `img` on the flow's grid and
    the frame `other` it points into, float32 [N] (a scalar tensor for 3-D input), differentiable with respect to a tensor `flow`.  An
    extension: the reference has no such function."""
    c = Flow(flow, ref, mask).census(img, other, patch=patch, thresh=thresh, eps=eps, q=q)
    return c if len(flow.shape) > 3 else c.squeeze(0)


def flow_census_stats(flow, img, other, ref: str, mask=None, patch: int = None, thresh: float = None, eps: float = None,
                      q: float = None) -> dict:
    """Flow(flow, ref, mask).census_stats(img, other, patch, thresh, eps, q): the dict of Flow.census_stats for arrays / tensors
    (N-)2-H-W or (N-)H-W-2 with an optional mask (N-)H-W; 3-D in -> entries without the batch dimension.  An extension (DESIGN.md
    3.21)."""
    stats = Flow(flow, ref, mask).census_stats(img, other, patch=patch, thresh=thresh, eps=eps, q=q)
    return stats if len(flow.shape) > 3 else {k: v.squeeze(0) for k, v in stats.items()}


def flow_ssim(flow, img, other, ref: str, mask=None, window: int = None, c1: float = None, c2: float = None) -> torch.Tensor:
    """Flow(flow, ref, mask).ssim(img, other, window, c1, c2): the SSIM loss between the frame `img` on the flow's grid and the frame
    `other` it points into, float32 [N] (a scalar tensor for 3-D input), differentiable with respect to a tensor `flow`.  An extension
    (DESIGN.md 3.22): the reference has no such function."""
    s = Flow(flow, ref, mask).ssim(img, other, window=window, c1=c1, c2=c2)
    return s if len(flow.shape) > 3 else s.squeeze(0)


def flow_ssim_stats(flow, img, other, ref: str, mask=None, window: int = None, c1: float = None, c2: float = None) -> dict:
    """Flow(flow, ref, mask).ssim_stats(img, other, window, c1, c2): the dict of Flow.ssim_stats for arrays / tensors (N-)2-H-W or
    (N-)H-W-2 with an optional mask (N-)H-W; 3-D in -> entries without the batch dimension.  An extension."""
    stats = Flow(flow, ref, mask).ssim_stats(img, other, window=window, c1=c1, c2=c2)
    return stats if len(flow.shape) > 3 else {k: v.squeeze(0) for k, v in stats.items()}


def flow_cost_volume(flow, feat, other, ref: str, mask=None, radius: int = None) -> torch.Tensor:
    """Flow(flow, ref, mask).cost_volume(feat, other, radius): the local cost volume between the features `feat` on the flow's grid and
    the features `other` of the frame it points into, float32 N-D-H-W with D = (2 radius + 1)^2 (D-H-W for 3-D input), differentiable
    with respect to tensor `flow`, `feat` and `other`.  An extension: the reference has no such function."""
    v = Flow(flow, ref, mask).cost_volume(feat, other, radius=radius)
    return v if len(flow.shape) > 3 else v.squeeze(0)


def flow_corr_lookup(flow, feat, other, ref: str, mask=None, radius: int = None, levels: int = None) -> torch.Tensor:
    """Flow(flow, ref, mask).corr_lookup(feat, other, radius, levels): RAFT's correlation lookup between the features `feat` on the
    flow's grid and the features `other` (one tensor, pooled into `levels` levels, or a sequence of level tensors, e.g. from
    `corr_pyramid`) of the frame it points into, float32 N-(L D)-H-W with D = (2 radius + 1)^2 ((L D)-H-W for 3-D input),
    differentiable with respect to tensor `feat` and `other`, not `flow`.  An extension: the reference has no such
    function."""
    v = Flow(flow, ref, mask).corr_lookup(feat, other, radius=radius, levels=levels)
    return v if len(flow.shape) > 3 else v.squeeze(0)


def upsample_flow_convex(flow, weights, factor: int = None) -> torch.Tensor:
    """Flow(flow).upsample_convex(weights, factor).vecs: RAFT's learned convex upsampling of the vectors `flow` (2-H-W or N-2-H-W,
    tensor or array) under the 9 k^2 logits `weights` per pixel, float32 N-2-(k H)-(k W) (2-(k H)-(k W) for 3-D input), differentiable
    with respect to tensor `flow` and `weights`.  The arithmetic does not depend on the flow's reference.  An extension (DESIGN.md
    3.26): the reference has no such function."""
    v = Flow(flow).upsample_convex(weights, factor=factor, consider_mask=False).vecs
    return v if len(flow.shape) > 3 else v.squeeze(0)


def global_matching_flow(feat, other, ref: str, return_prob: bool = None):
    """Flow.from_matching(feat, other, ref).vecs: the flow between two frames by global matching of their float32 features `feat` and
    `other` (C-H-W or N-C-H-W, one shape), GMFlow's softmax over all positions, float32 N-2-H-W (2-H-W for 3-D input), differentiable
    with respect to both tensors.  With `return_prob` True a tuple of the vectors and the matching probability, N-H-W (H-W for 3-D
    input).  Two float16 or two bfloat16 tensors are matched on the matrix cores: the vectors and the probability
    stay float32, the gradients have the features' dtype.  An extension: the reference has no such function."""
    res = Flow.from_matching(feat, other, ref, return_prob=return_prob)
    flow, prob = res if isinstance(res, tuple) else (res, None)
    v = flow.vecs if feat.dim() > 3 else flow.vecs.squeeze(0)
    if prob is None:
        return v
    return v, (prob if feat.dim() > 3 else prob.squeeze(0))


def propagate_flow(flow, query, key=None, radius: int = None, mask=None):
    """Flow(flow, mask=mask).propagate(query, key, radius).vecs: the vectors `flow` (2-H-W or N-2-H-W, tensor or array) propagated by
    attention between the float32 features `query` and `key` (None: `query`), GMFlow's softmax over all positions (`radius` None) or
    over the zero-padded (2 radius + 1)^2 window, float32 N-2-H-W (2-H-W for 3-D input), differentiable with respect to tensor `flow`,
    `query` and `key`.  With `mask` (N-)H-W the positions where it is False are excluded from the softmax, and the result is a tuple of
    the vectors and the result mask, bool N-H-W (H-W for 3-D input), False where nothing was left to take part.  The arithmetic does
    not depend on the flow's reference.  An extension: the reference has no such function."""
    res = Flow(flow, mask=mask).propagate(query, key, radius=radius, consider_mask=mask is not None)
    v = res.vecs if len(flow.shape) > 3 else res.vecs.squeeze(0)
    if mask is None:
        return v
    return v, (res.mask if len(flow.shape) > 3 else res.mask.squeeze(0))


def local_matching_flow(flow, feat, other, ref: str, radius: int = None, mask=None, return_prob: bool = None):
    """Flow(flow, ref, mask).match_local(feat, other, radius).vecs: the vectors `flow` (2-H-W or N-2-H-W, tensor or array) refined by
    local matching between the float32 features `feat` on the flow's grid and the features `other` of the frame it points into, warped by
    the flow -- GMFlow's softmax over the (2 radius + 1)^2 window of the warped features, the positions outside the frame excluded, and
    the expected offset added to the flow -- float32 N-2-H-W (2-H-W for 3-D input), differentiable with respect to tensor `flow`,
    `feat` and `other`.  With `return_prob` True a tuple of the vectors and the weight of the best position, N-H-W (H-W for 3-D
    input).  An extension: the reference has no such function."""
    res = Flow(flow, ref, mask).match_local(feat, other, radius=radius, return_prob=return_prob)
    out, prob = res if isinstance(res, tuple) else (res, None)
    v = out.vecs if len(flow.shape) > 3 else out.vecs.squeeze(0)
    if prob is None:
        return v
    return v, (prob if len(flow.shape) > 3 else prob.squeeze(0))


def flow_sequence_loss(flows, gt, gt_mask=None, gamma: float = None, max_flow: float = None, penalty: str = None,
                       normalise: str = None) -> torch.Tensor:
    """Flow.sequence_loss for the raw outputs of a network: `flows` is a list or tuple of 1 to 32 float32 or float16 tensors 2-H-W or
    N-2-H-W, or ONE stacked tensor [T,(N,)2,H,W], which is unbound along axis 0 and whose slices are used in place; `gt` (tensor or
    array, with the optional mask `gt_mask`) is the ground truth of that shape.  Returns the loss, float32 [N] (a scalar tensor for 3-D
    input) on the device of the predictions, differentiable with respect to them (the gradient of a stacked tensor has the stack's
    shape).  The predictions are NOT validated and no flow object is made of them: T validation passes would cost more than the loss, and
    a non-finite prediction shows up as a NaN loss.  An extension: the reference has no such function."""
    err = _sequence_loss.ERR
    if isinstance(flows, torch.Tensor):
        if flows.dim() not in (4, 5):
            raise ValueError(err + "A stacked tensor of predictions needs to have 4 or 5 dimensions, T-2-H-W or T-N-2-H-W")
        flows = flows.unbind(0)
    if not isinstance(flows, (list, tuple)) or not all(isinstance(f, torch.Tensor) for f in flows):
        raise TypeError(err + "Flows needs to be a list or a tuple of tensors, or one stacked tensor")
    _sequence_loss.check_count(len(flows))
    if any(f.dtype not in (torch.float32, torch.float16) for f in flows):
        raise TypeError(err + "Flows need to be of dtype float32 or float16")
    if flows[0].dim() not in (3, 4) or flows[0].shape[-3] != 2 or min(flows[0].shape) < 1:
        raise ValueError(err + "Flows need to be of shape 2-H-W or N-2-H-W")
    if any(f.shape != flows[0].shape for f in flows):
        raise ValueError(err + "Flows need to have the same shape, including batch size")
    gamma, max_flow, penalty, normalise = _sequence_loss.check_params(gamma, max_flow, penalty, normalise)
    batched = flows[0].dim() == 4
    truth = Flow(gt, 't', gt_mask)
    if (truth.shape[0],) + tuple(truth.shape[1:]) != ((flows[0].shape[0] if batched else 1),) + tuple(flows[0].shape[-2:]):
        raise ValueError(err + "Gt needs to have the shape of the flows, including batch size")
    preds = [f if batched else f[None] for f in flows]
    loss = _sequence_loss.sequence_loss(preds, truth._fv, truth._mask, gamma, max_flow, penalty, normalise).to(flows[0].device)
    return loss if batched else loss.squeeze(0)


def batch_flows(flows: Union[list, tuple]) -> FlowAlias:
    """Concatenate flow objects of equal H, W, ref and device along the batch axis (flow_operations.py:458-483)"""
    if not isinstance(flows, (list, tuple)):
        raise TypeError("Error batching flows: Input needs to be a tuple or a list of flow objects")
    if not all(isinstance(f, Flow) for f in flows):
        raise TypeError("Error batching flows: Input needs to be a tuple or a list of flow objects")
    if len({f.shape[1:] for f in flows}) != 1:
        raise ValueError("Error batching flows: Flow objects need to have the same H-W shape")
    if len({f.ref for f in flows}) != 1:
        raise ValueError("Error batching flows: Flow objects need to have the same reference")
    if len({str(f.device) for f in flows}) != 1:
        raise ValueError("Error batching flows: Flow objects need to be on the same device")
    return Flow(torch.cat([f.vecs for f in flows], dim=0), flows[0].ref, torch.cat([f.mask for f in flows], dim=0))


def chain_flows(flows, ref: str, masks=None, return_all: bool = None):
    """Flow.chain for arrays / tensors: `flows` is a list or tuple of 1 to 32 arrays or tensors 2-H-W or N-2-H-W of one shape, ordered in
    time, `ref` their common reference, `masks` None or a list or tuple of as many masks (N-)H-W, of which single entries may be None.
    Returns the vectors of the chain, float32 (N-)2-H-W, 3-D in -> 3-D out; with `masks` given a tuple of the vectors and the mask, bool
    (N-)H-W; with `return_all` True a list of T such results (Flow.chain says which).  An extension: the reference has
    no such function."""
    err = _chain.ERR
    if not isinstance(flows, (list, tuple)) or not all(isinstance(f, (np.ndarray, torch.Tensor)) for f in flows):
        raise TypeError(err + "Flows needs to be a list or a tuple of numpy arrays or torch tensors")
    if not 1 <= len(flows) <= _chain.MAX_T:
        raise ValueError(err + "The sequence needs to hold 1 to {} flows".format(_chain.MAX_T))
    if masks is not None and (not isinstance(masks, (list, tuple)) or len(masks) != len(flows)):
        raise TypeError(err + "Masks needs to be None or a list or a tuple of one mask, or None, per flow")
    ref = get_valid_ref(ref)
    objs = [Flow(f, ref, None if masks is None else masks[i]) for i, f in enumerate(flows)]
    res = Flow.chain(objs, return_all=return_all)
    batched = len(flows[0].shape) > 3

    def unwrap(r: Flow):
        v = r.vecs if batched else r.vecs.squeeze(0)
        if masks is None:
            return v
        return v, (r.mask if batched else r.mask.squeeze(0))

    return [unwrap(r) for r in res] if isinstance(res, list) else unwrap(res)
