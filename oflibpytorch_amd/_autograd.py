"""Autograd for the two primitives of the path.

The reference's outputs are differentiable with respect to flow vectors and warped data (README.rst:7-10; 't' branch
through ``F.grid_sample`` and ``normalise_coords``, utils.py:462-465, 549-555; 's' branch through the weights and
``scatter_add_`` of ``grid_from_unstructured_data``, utils.py:1098-1144; its tests assert ``grad_fn``, e.g.
test_utils.py:500, 1113-1114).  Here the forward passes are the fused HIP kernels, so the backward passes are HIP
kernels too (``ofl_warp_bwd_grad_f32``, ``ofl_splat_grad_f32``, ``ofl_sample_pts_grad_f32``); the fused epilogues of
the forward launch (signs, `src_b` / `data_b`, addend) are chained here.  Boolean outputs (valid masks, flag words)
are non-differentiable, as the comparisons that produce them are in the reference.  Double backward is not
implemented (`once_differentiable` raises).
"""
import torch
from torch.autograd.function import once_differentiable

from . import (_census, _corr_lookup, _cost_volume, _local_match, _matching, _native, _photometric, _propagate, _sequence_loss, _smoothness,
               _ssim, _upsample)


def _reduce_to(g: torch.Tensor, like: torch.Tensor) -> torch.Tensor:
    """Gradient of a batch-broadcast operand: sum over the batch axis (the reference's `expand`, utils.py:527-537)."""
    if g.shape[0] != like.shape[0]:
        g = g.sum(0, keepdim=True)
    return g.to(like.device).to(like.dtype) if like.dtype.is_floating_point else g


class WarpFn(torch.autograd.Function):
    """dst = a_sign * addend + g_sign * G(flow_sign * flow, src - src_b)"""

    @staticmethod
    def forward(ctx, flow, src, addend, src_b, kw):
        d = lambda t: None if t is None else t.detach()
        kw = dict(kw)
        res = None
        nhwc, keep16 = kw.pop("nhwc", False), kw.pop("keep16", False)
        if nhwc:
            # a feature tensor stored channels_last: the native N-H-W-C launch (the output is channels_last whether or not a gradient is
            # wanted); a launch the library declines goes on below, on the planar route
            res = _native._warp_bwd_nhwc(d(flow), d(src), addend=d(addend), src_b=d(src_b), **kw)
        ctx.nhwc = res is not None
        if res is None and keep16:
            # a feature tensor stored in fp16 / bf16: the native 16-bit launch, and the 16-BIT source is what is saved (the
            # backward up-converts it transiently for the fp32 backward kernels); a launch the library declines is converted
            # here, so that the output has the source's dtype either way
            res = _native._warp_bwd_x16(d(flow), d(src), addend=d(addend), src_b=d(src_b), **kw)
            if res is None:
                with _native._on(_native.device(flow, src)):
                    res = _native._warp_bwd_raw(d(flow), d(src).float(), addend=d(addend), src_b=d(src_b), **kw)
                res = (res[0].to(src.dtype),) + tuple(res[1:])
        if res is None:
            with _native._on(_native.device(flow, src)):
                res = _native._warp_bwd_raw(d(flow), d(src), addend=d(addend), src_b=d(src_b), **kw)
        ctx.save_for_backward(flow, src, src_b)
        ctx.addend_meta = None if addend is None else (addend.shape[0], addend.device, addend.dtype)
        ctx.signs = (float(kw.get("flow_sign", 1.0)), float(kw.get("a_sign", 1.0)), float(kw.get("g_sign", 1.0)))
        ctx.mark_non_differentiable(*[r for r in res[1:] if r is not None])
        return tuple(res)

    @staticmethod
    @once_differentiable
    def backward(ctx, g, *_unused):
        flow, src, src_b = ctx.saved_tensors
        flow_sign, a_sign, g_sign = ctx.signs
        need_flow, need_src, need_add, need_b = ctx.needs_input_grad[:4]
        if getattr(ctx, "nhwc", False) and src_b is None and ctx.addend_meta is None and (need_flow or need_src):
            # the forward ran on N-H-W-C storage and the upstream gradient arrived channels_last too: the flow gradient from both as they
            # are stored, the source gradient through the library's own layout copies (DESIGN.md 3.14 "Autograd"); a planar gradient, a
            # source broadcast over the batch or a launch the library declines goes on below
            res = _native.warp_bwd_grad_nhwc(flow, src, g, flow_sign=flow_sign, g_scale=g_sign, want_src=bool(need_src), want_flow=bool(need_flow))
            if res is not None:
                return (_reduce_to(res[1], flow) if need_flow else None), (res[0] if need_src else None), None, None, None
        dense = g.is_contiguous()                        # (a strided upstream gradient -- channels-last -- keeps the present route)
        g = g.contiguous()
        as_stored = lambda t: t
        if getattr(ctx, "nhwc", False):
            # the forward ran on N-H-W-C storage but the upstream gradient is not of that kind (or the launch was declined above): the saved
            # source and the gradient as planes, then the planar route's own backward kernels on the same values; the source gradient goes
            # back channels_last, as the source is stored
            src, dense = src.contiguous(), True
            as_stored = lambda t: t.contiguous(memory_format=torch.channels_last)
        if (dense and src.dtype in _native._X16_DTYPES and src.device.type == 'cuda' and g.dtype == src.dtype and src_b is None
                and ctx.addend_meta is None and src.shape[0] == g.shape[0] and (need_flow or need_src)):
            # a 16-bit source that took the native forward: both gradients from the 16-bit planes (no fp32 copy of the source, of g or of
            # the source gradient); a source broadcast over the batch sums its gradient in fp32 below, as does a launch the library declines
            res = _native.warp_bwd_grad_x16(flow, src, g, flow_sign=flow_sign, g_scale=g_sign, want_src=bool(need_src), want_flow=bool(need_flow))
            if res is not None:
                return (_reduce_to(res[1], flow) if need_flow else None), (as_stored(res[0]) if need_src else None), None, None, None
        gathered = src.detach().float()
        if src_b is not None:
            gathered = gathered.to(g.device) - src_b.detach().float().to(g.device)
        gs, gf = _native.warp_bwd_grad(flow, gathered, g, flow_sign=flow_sign, g_scale=g_sign,
                                       want_src=bool(need_src or need_b), want_flow=bool(need_flow))
        g_flow = _reduce_to(gf, flow) if need_flow else None
        g_src = as_stored(_reduce_to(gs, src)) if need_src else None
        g_b = _reduce_to(-gs, src_b) if (need_b and src_b is not None) else None
        g_add = None
        if need_add and ctx.addend_meta is not None:
            nb, adev, adt = ctx.addend_meta
            g_add = g * a_sign if a_sign != 1.0 else g
            if g_add.shape[0] != nb:
                g_add = g_add.sum(0, keepdim=True)
            g_add = g_add.to(adev).to(adt)
        return g_flow, g_src, g_add, g_b, None


def warp(flow, src, **kw):
    """`_native.warp_bwd` with a grad_fn.  Integer rounding modes have no gradient in the reference either
    (`torch.round`, then a cast back to the integer dtype: flow_class.py:943-951, utils.py:613-618)."""
    if int(kw.get("round_mode", 0)) != 0:
        d = lambda t: None if t is None else t.detach()
        kw = dict(kw)
        kw.pop("keep16", None)
        kw.pop("nhwc", None)
        kw["addend"], kw["src_b"] = d(kw.get("addend")), d(kw.get("src_b"))
        with _native._on(_native.device(flow, src)):
            return _native._warp_bwd_raw(flow.detach(), src.detach(), **kw)
    kw = dict(kw)
    addend, src_b = kw.pop("addend", None), kw.pop("src_b", None)
    kw.pop("out_uint8", None)
    if not (addend is None and src_b is None):
        kw.pop("keep16", None)
        kw.pop("nhwc", None)
    if src.dtype == torch.uint8:          # (only the flow can want a gradient: the backward kernel reads float planes)
        src = src.float()
    return WarpFn.apply(flow, src, addend, src_b, kw)


class SplatFn(torch.autograd.Function):
    """dst = P(flow_sign * flow | (xs, ys), data_sign * (data - data_b))"""

    @staticmethod
    def forward(ctx, flow, xs, ys, data, data_b, kw):
        d = lambda t: None if t is None else t.detach()
        kw = dict(kw)
        user_density = bool(kw.get("want_density", False))
        kw["want_density"] = True                      # the backward pass needs D
        with _native._on(_native.device(flow, data, xs)):
            res = list(_native._splat_fwd_raw(d(flow), d(data), xs=d(xs), ys=d(ys), data_b=d(data_b), **kw))
        dst, density = res[0], res[2]
        ctx.save_for_backward(flow, xs, ys, data, data_b, dst, density)
        ctx.kw = (float(kw.get("flow_sign", 1.0)), float(kw.get("data_sign", 1.0)), kw.get("weight_mask"),
                  bool(kw.get("occlude", True)))
        if not user_density:
            res[2] = None
        nd = [r for i, r in enumerate(res) if r is not None and i not in (0, 2)]
        ctx.mark_non_differentiable(*nd)
        ctx.user_density = user_density
        return tuple(res)

    @staticmethod
    @once_differentiable
    def backward(ctx, g, *rest):
        flow, xs, ys, data, data_b, dst, density = ctx.saved_tensors
        flow_sign, data_sign, weight_mask, occlude = ctx.kw
        need_flow, need_x, need_y, need_data, need_b = ctx.needs_input_grad[:5]
        g_den = rest[1] if (ctx.user_density and len(rest) > 1) else None
        dev = g.device
        eff = data.detach().float().to(dev)
        if data_b is not None:
            eff = eff - data_b.detach().float().to(dev)
        if data_sign != 1.0:
            eff = eff * data_sign
        gd, gxy = _native.splat_grad(flow, eff, dst, density, g.contiguous(), xs=xs, ys=ys, flow_sign=flow_sign,
                                     weight_mask=weight_mask, occlude=occlude, grad_density=g_den,
                                     want_data=bool(need_data or need_b), want_xy=bool(need_flow or need_x or need_y))
        g_flow = g_x = g_y = g_data = g_b = None
        if need_flow and flow is not None:
            g_flow = _reduce_to(gxy * flow_sign if flow_sign != 1.0 else gxy, flow)
        if need_x and xs is not None:
            g_x = _reduce_to(gxy[:, 0], xs)
        if need_y and ys is not None:
            g_y = _reduce_to(gxy[:, 1], ys)
        if need_data:
            g_data = _reduce_to(gd * data_sign if data_sign != 1.0 else gd, data)
        if need_b and data_b is not None:
            g_b = _reduce_to(gd * (-data_sign), data_b)
        return g_flow, g_x, g_y, g_data, g_b, None


def splat(flow, data, **kw):
    """`_native.splat_fwd` with a grad_fn (see `warp` for the rounding modes)."""
    kw = dict(kw)
    xs, ys, data_b = kw.pop("xs", None), kw.pop("ys", None), kw.pop("data_b", None)
    if int(kw.get("round_mode", 0)) != 0:
        d = lambda t: None if t is None else t.detach()
        with _native._on(_native.device(flow, data, xs)):
            return _native._splat_fwd_raw(d(flow), d(data), xs=d(xs), ys=d(ys), data_b=d(data_b), **kw)
    if not data.dtype.is_floating_point:
        data = data.float()
    return SplatFn.apply(flow, xs, ys, data, data_b, kw)


class SamplePtsFn(torch.autograd.Function):
    """out = pts + bilinear(flow, pts)   (track_pts, utils.py:1004-1015)"""

    @staticmethod
    def forward(ctx, flow, pts):
        ctx.save_for_backward(flow, pts)
        return _native.sample_pts(flow.detach(), pts.detach())

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        flow, pts = ctx.saved_tensors
        need_flow, need_pts = ctx.needs_input_grad
        gf, gp = _native.sample_pts_grad(flow, pts, g.contiguous(), want_flow=bool(need_flow), want_pts=bool(need_pts))
        return (_reduce_to(gf, flow) if need_flow else None), (_reduce_to(gp, pts) if need_pts else None)


def sample_pts(flow, pts):
    if _native._wants_grad(flow, pts):
        return SamplePtsFn.apply(flow, pts)
    return _native.sample_pts(flow, pts)


class EpeFn(torch.autograd.Function):
    """epe[n] = mean over the valid pixels of |est - gt|   (Flow.epe): fp32, rounded once from the float64 quotient of
    the kernel's sum and count; NaN for an image without a valid pixel, whose gradient is 0."""

    @staticmethod
    def forward(ctx, est, gt, est_mask, gt_mask):
        rec, _ = _native.flow_error(est.detach(), gt.detach(), est_mask, gt_mask, (), False)
        ctx.save_for_backward(est, gt, rec)
        ctx.masks = (est_mask, gt_mask)
        return (rec[:, 1] / rec[:, 0]).to(torch.float32)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        est, gt, rec = ctx.saved_tensors
        need_est, need_gt = ctx.needs_input_grad[:2]
        scale = (g.to(rec.device, torch.float64) / rec[:, 0]).to(torch.float32)          # on the device: nothing is read back
        g_est, g_gt = _native.flow_epe_grad(est.detach(), gt.detach(), ctx.masks[0], ctx.masks[1], scale, want_est=bool(need_est),
                                            want_gt=bool(need_gt))
        return (_reduce_to(g_est, est) if need_est else None), (_reduce_to(g_gt, gt) if need_gt else None), None, None


class SequenceLossFn(torch.autograd.Function):
    """loss[n] = (sum_i gamma^(T-1-i) S[n, i]) / D[n], S the sums of the penalty of T predictions against one ground truth over its valid
    pixels (Flow.sequence_loss): fp32, rounded once from the float64 combination of the kernel's records; the predictions
    follow the parameters as further arguments.  Differentiable with respect to the predictions that require a gradient -- one launch
    writes all of them, the others are neither allocated nor written --, not the ground truth or the mask.  An fp16-stored prediction is
    saved as it is stored.  The binding is looked up by name at every call: the host tests replace it."""

    @staticmethod
    def forward(ctx, gt, gt_mask, gamma, max_flow, penalty, normalise, *preds):
        gt = gt.detach()
        rec = _sequence_loss.flow_sequence_loss([pr.detach() for pr in preds], gt, gt_mask, max_flow, penalty, normalise)
        ctx.save_for_backward(gt, rec, *preds)
        ctx.params = (gt_mask, gamma, max_flow, penalty, normalise)
        return _sequence_loss.loss_of(rec, int(gt.shape[-2]) * int(gt.shape[-1]), gamma, penalty, normalise)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        gt, rec = ctx.saved_tensors[:2]
        preds = ctx.saved_tensors[2:]
        gt_mask, gamma, max_flow, penalty, normalise = ctx.params
        wants = [bool(need) for need in ctx.needs_input_grad[6:]]
        scale = _sequence_loss.scale_of(g, rec, int(gt.shape[-2]) * int(gt.shape[-1]), gamma, penalty, normalise)   # on the device
        grads = _sequence_loss.flow_sequence_loss_grad([pr.detach() for pr in preds], gt, gt_mask, max_flow, penalty, normalise, scale,
                                                       wants)
        return (None,) * 6 + tuple(None if grad is None else _reduce_to(grad, pr) for grad, pr in zip(grads, preds))


class SmoothnessFn(torch.autograd.Function):
    """smoothness[n] = mean over the valid terms of the edge-aware smoothness penalty   (Flow.smoothness): fp32, rounded
    once from the float64 quotient of the kernel's sums and counts; NaN for an image without a valid term, whose gradient is 0.
    Differentiable with respect to the vectors only: the image is guidance.  An fp16-stored flow is saved as it is stored."""

    @staticmethod
    def forward(ctx, vecs, mask, img, order, alpha, eps):
        img = None if img is None else img.detach()
        rec, _ = _smoothness.flow_smoothness(vecs.detach(), mask, img, order, alpha, eps)
        ctx.save_for_backward(vecs, rec)
        ctx.guides = (mask, img, order, alpha, eps)
        return _smoothness.mean_of(rec)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        vecs, rec = ctx.saved_tensors
        mask, img, order, alpha, eps = ctx.guides
        scale = (g.to(rec.device, torch.float64) / (rec[:, 0] + rec[:, 1])).to(torch.float32)      # on the device: nothing is read back
        grad = _smoothness.flow_smoothness_grad(vecs.detach(), mask, img, order, alpha, eps, scale)
        return _reduce_to(grad, vecs), None, None, None, None, None


class _PairLossFn(torch.autograd.Function):
    """loss[n] = mean over the known pixels of a penalty between `img` and `other` sampled where the flow points (the image-pair losses,
    DESIGN.md 3.20 to 3.22): fp32, rounded once from the float64 quotient of the kernel's sum and count; NaN for an image without a known
    pixel, whose gradient is 0.  Differentiable with respect to the vectors only: the images carry no gradient.  An fp16-stored flow is
    saved as it is stored.  A subclass names its binding: the module and its two functions.  They are looked up by name at every call,
    not held as callables, because the host tests replace `module.flow_*` with fakes after this class exists; forward and backward
    are static, so the subclass is reached through `ctx._forward_cls`, which torch sets on the context class of every Function."""
    binding = None                                 # (module, name of flow_*, name of flow_*_grad)

    @staticmethod
    def forward(ctx, vecs, mask, img, other, *params):
        module, fwd, _ = ctx._forward_cls.binding
        img, other = img.detach(), other.detach()
        rec, _ = getattr(module, fwd)(vecs.detach(), mask, img, other, *params)
        ctx.save_for_backward(vecs, mask, img, other, rec)
        ctx.params = params
        return _native.mean_of(rec)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        vecs, mask, img, other, rec = ctx.saved_tensors
        module, _, bwd = ctx._forward_cls.binding
        scale = (g.to(rec.device, torch.float64) / rec[:, 0]).to(torch.float32)                      # on the device: nothing is read back
        grad = getattr(module, bwd)(vecs.detach(), mask, img, other, *ctx.params, scale)
        return (_reduce_to(grad, vecs), None, None, None) + (None,) * len(ctx.params)


class PhotometricFn(_PairLossFn):
    """photometric[n]: the Charbonnier penalty (Flow.photometric); params: flow_sign, eps"""
    binding = (_photometric, "flow_photometric", "flow_photometric_grad")


class CensusFn(_PairLossFn):
    """census[n]: the census penalty (Flow.census); params: flow_sign, patch, thresh, eps, q"""
    binding = (_census, "flow_census", "flow_census_grad")


class SsimFn(_PairLossFn):
    """ssim[n]: the SSIM penalty (Flow.ssim); params: flow_sign, window, c1, c2"""
    binding = (_ssim, "flow_ssim", "flow_ssim_grad")


class CostVolumeFn(torch.autograd.Function):
    """volume[n, o] = mean over the channels of feat(p) * W'(p + o), W' being `other` sampled where the flow points and +0 where the
    pixel is not usable (Flow.cost_volume); params: flow_sign, radius.  Differentiable with respect to the vectors, `feat`
    and `other`, not the mask: the gradient kernels give d feat and d W (gathers, bitwise reproducible), and the backward of the warp
    (`_native.warp_bwd_grad`) turns d W into d other and d flow -- a call that is skipped when neither is needed; d flow is +0 wherever
    the pixel is not usable (`flow_cost_volume_gate`), whatever `other` holds there.  The binding is looked
    up by name at every call: the host tests replace `_cost_volume.flow_*` with fakes after this class exists."""

    @staticmethod
    def forward(ctx, vecs, mask, feat, other, flow_sign, radius):
        vol = _cost_volume.flow_cost_volume(vecs.detach(), mask, feat.detach(), other.detach(), flow_sign, radius)
        ctx.save_for_backward(vecs, mask, feat, other)
        ctx.params = (flow_sign, radius)
        return vol

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        vecs, mask, feat, other = ctx.saved_tensors
        flow_sign, radius = ctx.params
        need_flow, _, need_feat, need_other = ctx.needs_input_grad[:4]
        need_warped = need_flow or need_other
        g_feat, g_warped = _cost_volume.flow_cost_volume_grad(vecs.detach(), mask, feat.detach(), other.detach(), flow_sign, radius, g,
                                                              want_feat=bool(need_feat), want_warped=bool(need_warped))
        g_flow = g_other = None
        if need_warped:
            # the rule of 3.24: d flow is +0 wherever the pixel is not usable, and a value of `other` that no usable pixel samples
            # reaches no gradient.  The warp's backward knows nothing of `usable`: it runs on vectors that are finite everywhere
            # (`chain`), and its d flow is gated by a kernel of the cost volume -- selected, not multiplied, as in the forward
            src = other.detach()
            chain = _cost_volume.flow_cost_volume_chain(vecs.detach(), flow_sign)
            g_other, g_flow = _native.warp_bwd_grad(chain, src[None] if src.dim() == 3 else src, g_warped, flow_sign=flow_sign,
                                                    want_src=bool(need_other), want_flow=bool(need_flow))
            if need_flow:
                g_flow = _cost_volume.flow_cost_volume_gate(vecs.detach(), mask, flow_sign, g_flow)
        like = lambda grad, t: _reduce_to(grad, t[None])[0] if t.dim() == 3 else _reduce_to(grad, t)      # C-H-W: summed over the batch
        return (_reduce_to(g_flow, vecs) if need_flow else None, None, like(g_feat, feat) if need_feat else None,
                like(g_other, other) if need_other else None, None, None)


class CorrLookupFn(torch.autograd.Function):
    """lookup[n, l D + (dx + r)(2 r + 1) + dy + r] = the bilinear sample, at (p + flow(p)) / 2^l + (dx, dy), of the correlation of feat(p)
    with level l, over sqrt(C) (Flow.corr_lookup); params: flow_sign, radius; the levels follow as further arguments.
    Differentiable with respect to `feat` and every level, not the vectors or the mask (RAFT detaches the coordinates before every
    lookup): both gradients are gathers in a fixed order, bitwise reproducible.  The binding is looked up by name at every call: the
    host tests replace `_corr_lookup.flow_*` with fakes after this class exists."""

    @staticmethod
    def forward(ctx, vecs, mask, feat, flow_sign, radius, *levels):
        out = _corr_lookup.flow_corr_lookup(vecs.detach(), mask, feat.detach(), [lv.detach() for lv in levels], flow_sign, radius)
        ctx.save_for_backward(vecs, mask, feat, *levels)
        ctx.params = (flow_sign, radius)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        vecs, mask, feat = ctx.saved_tensors[:3]
        levels = ctx.saved_tensors[3:]
        flow_sign, radius = ctx.params
        need_feat, need_levels = ctx.needs_input_grad[2], ctx.needs_input_grad[5:]
        g_feat, g_levels = _corr_lookup.flow_corr_lookup_grad(vecs.detach(), mask, feat.detach(), [lv.detach() for lv in levels], flow_sign,
                                                              radius, g, want_feat=bool(need_feat), want_levels=need_levels)
        like = lambda grad, t: _reduce_to(grad, t[None])[0] if t.dim() == 3 else _reduce_to(grad, t)      # C-H-W: summed over the batch
        return (None, None, like(g_feat, feat) if need_feat else None, None, None) + tuple(
            like(gl, lv) if need else None for gl, lv, need in zip(g_levels, levels, need_levels))


class UpsampleConvexFn(torch.autograd.Function):
    """out[n, c, k y + i, k x + j] = sum_t softmax_t(logits[n, t k^2 + i k + j, y, x]) * k * vecs_c(y + dy, x + dx), RAFT's convex
    upsampling (Flow.upsample_convex), and the mask of the coarse pixel over its k x k block (or None).  Differentiable
    with respect to the logits and the vectors, not the mask: d logits is local to the fine pixel, d vecs a gather in a fixed order, both
    bitwise reproducible.  The binding is looked up by name at every call: the host tests replace `_upsample.flow_*` with fakes after
    this class exists."""

    @staticmethod
    def forward(ctx, vecs, mask, logits, factor):
        out, out_mask = _upsample.flow_upsample_convex(vecs.detach(), mask, logits.detach(), factor)
        ctx.save_for_backward(vecs, logits)
        ctx.factor = factor
        if out_mask is not None:
            ctx.mark_non_differentiable(out_mask)
        return out, out_mask

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _g_mask=None):
        vecs, logits = ctx.saved_tensors
        need_vecs, need_logits = ctx.needs_input_grad[0], ctx.needs_input_grad[2]
        d_logits, d_vecs = _upsample.flow_upsample_convex_grad(vecs.detach(), logits.detach(), ctx.factor, g, want_logits=bool(need_logits),
                                                               want_vecs=bool(need_vecs))
        return (_reduce_to(d_vecs, vecs) if need_vecs else None, None, _reduce_to(d_logits, logits) if need_logits else None, None)


class GlobalMatchFn(torch.autograd.Function):
    """flow(p) = -flow_sign * (sum_q softmax_q(feat(p) . other(q) / sqrt(C)) q - p) and the matching probability 1 / S of every pixel
    (or None), GMFlow's global matching (Flow.from_matching).  Differentiable with respect to `feat` and `other`, not
    through the probability: both gradients recompute the logits on the saved maximum and sum, every sum in a fixed order, bitwise
    reproducible.  The binding is looked up by name at every call: the host tests replace `_matching.flow_*` with fakes after this
    class exists.

    Two float16 or two bfloat16 tensors take the matrix-core forward.  The graph keeps the 16-bit tensors and the
    statistics, no float32 copy; the backward forms the exact float32 up-conversions for the length of its call, runs the float32
    gradient kernels on the 16-bit forward's statistics and rounds each gradient once to the features' dtype."""

    @staticmethod
    def forward(ctx, feat, other, flow_sign, want_prob):
        forward = _matching.flow_global_match_x16 if feat.dtype in _matching.X16 else _matching.flow_global_match
        out, prob, stats = forward(feat.detach(), other.detach(), flow_sign, want_prob, True)
        ctx.save_for_backward(feat, other, stats)
        ctx.flow_sign = flow_sign
        if prob is not None:
            ctx.mark_non_differentiable(prob)
        return out, prob

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _g_prob=None):
        feat, other, stats = ctx.saved_tensors
        need_feat, need_other = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        d_feat, d_other = _matching.flow_global_match_grad(feat.detach().float(), other.detach().float(), ctx.flow_sign, stats, g,
                                                           want_feat=bool(need_feat), want_other=bool(need_other))
        # (`.float()` of a float32 tensor is that tensor; `_reduce_to` rounds a gradient once to the dtype of its operand)
        like = lambda grad, t: _reduce_to(grad, t[None])[0] if t.dim() == 3 else _reduce_to(grad, t)      # C-H-W: the batch of one
        return (like(d_feat, feat) if need_feat else None, like(d_other, other) if need_other else None, None, None)


class PropagateFn(torch.autograd.Function):
    """flow'(p) = sum_q softmax_q(query(p) . key(q) / sqrt(C)) flow(q) over the positions the mask does not exclude -- all of them
    (radius None) or the zero-padded (2 radius + 1)^2 window of p -- and the result mask (or None), GMFlow's flow propagation by
    attention (Flow.propagate).  Differentiable with respect to the vectors, `query` and `key`, not the mask: every
    gradient is a sum in a fixed order with one owner, bitwise reproducible.  The binding is looked up by name at every call: the host
    tests replace `_propagate.flow_*` with fakes after this class exists."""

    @staticmethod
    def forward(ctx, vecs, mask, query, key, radius):
        out, valid, stats = _propagate.flow_propagate(vecs.detach(), mask, query.detach(), key.detach(), radius, True)
        ctx.save_for_backward(vecs, mask, query, key, stats)
        ctx.radius = radius
        if valid is not None:
            ctx.mark_non_differentiable(valid)
        return out, valid

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _g_valid=None):
        vecs, mask, query, key, stats = ctx.saved_tensors
        need_vecs, _, need_query, need_key = ctx.needs_input_grad[:4]
        d_query, d_key, d_vecs = _propagate.flow_propagate_grad(vecs.detach(), mask, query.detach(), key.detach(), ctx.radius, stats, g,
                                                                want_query=bool(need_query), want_key=bool(need_key),
                                                                want_flow=bool(need_vecs))
        like = lambda grad, t: _reduce_to(grad, t[None])[0] if t.dim() == 3 else _reduce_to(grad, t)      # C-H-W: summed over the batch
        return (_reduce_to(d_vecs, vecs) if need_vecs else None, None, like(d_query, query) if need_query else None,
                like(d_key, key) if need_key else None, None)


class LocalMatchFn(torch.autograd.Function):
    """flow'(p) = flow(p) - flow_sign * E[o] under softmax_o(feat(p) . W'(p + o) / sqrt(C)) over the positions of the (2 radius + 1)^2
    window of p that lie inside the frame, W' being `other` sampled where the flow points and +0 where the pixel is not usable, and the
    weight 1 / S of the best position (or None): the local matching of GMFlow's refinement (Flow.match_local); params:
    flow_sign, radius, want_prob.  Differentiable with respect to the vectors, `feat` and `other`, not the mask and not through the
    probability: the gradient kernels give d feat and d W (gathers, bitwise reproducible), and the backward of the cost volume's warp
    (`flow_cost_volume_chain`, `_native.warp_bwd_grad`, `flow_cost_volume_gate`) turns d W into d other and the warp's part of d flow
    -- launches that are not made when neither is needed; d flow is the upstream gradient plus that part, one float32 addition, the
    upstream gradient itself wherever the pixel is not usable.  The binding is looked up by name at every call: the host tests replace
    `_local_match.flow_*` with fakes after this class exists."""

    @staticmethod
    def forward(ctx, vecs, mask, feat, other, flow_sign, radius, want_prob):
        out, prob, stats = _local_match.flow_local_match(vecs.detach(), mask, feat.detach(), other.detach(), flow_sign, radius, want_prob,
                                                         True)
        ctx.save_for_backward(vecs, mask, feat, other, stats)
        ctx.params = (flow_sign, radius)
        if prob is not None:
            ctx.mark_non_differentiable(prob)
        return out, prob

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _g_prob=None):
        vecs, mask, feat, other, stats = ctx.saved_tensors
        flow_sign, radius = ctx.params
        need_flow, _, need_feat, need_other = ctx.needs_input_grad[:4]
        need_warped = need_flow or need_other
        g_feat = g_other = g_flow = None
        if need_feat or need_warped:
            g_feat, g_warped = _local_match.flow_local_match_grad(vecs.detach(), mask, feat.detach(), other.detach(), flow_sign, radius,
                                                                  stats, g, want_feat=bool(need_feat), want_warped=bool(need_warped))
        if need_warped:
            # the rule of 3.24, through its own launches (CostVolumeFn.backward)
            src = other.detach()
            chain = _cost_volume.flow_cost_volume_chain(vecs.detach(), flow_sign)
            g_other, g_flow = _native.warp_bwd_grad(chain, src[None] if src.dim() == 3 else src, g_warped, flow_sign=flow_sign,
                                                    want_src=bool(need_other), want_flow=bool(need_flow))
            if need_flow:
                g_flow = _cost_volume.flow_cost_volume_gate(vecs.detach(), mask, flow_sign, g_flow)
                g_flow = g.to(g_flow.device, torch.float32) + g_flow                        # the identity term first: g + (the warp's part)
        like = lambda grad, t: _reduce_to(grad, t[None])[0] if t.dim() == 3 else _reduce_to(grad, t)      # C-H-W: summed over the batch
        return (_reduce_to(g_flow, vecs) if need_flow else None, None, like(g_feat, feat) if need_feat else None,
                like(g_other, other) if need_other else None, None, None, None)
