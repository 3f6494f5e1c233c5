"""oflibpytorch_amd -- MI355X-native (gfx950) dense optical-flow warping & composition.

Drop-in for the warp / compose hot path of oflibpytorch (`Flow.apply`, `Flow.combine_with` /
`combine_flows`, `Flow.switch_ref` / `invert`, `apply_flow`, `apply_s_flow`,
`grid_from_unstructured_data`) and the flow visualisation (`Flow.visualise`, `visualise_flow`; `Flow.visualise_arrows`, `visualise_flow_arrows`: the
reference's steps bit for bit, but the arrows by the package's own anti-aliased rasteriser and hue table, not
OpenCV's; an 's' flow keeps the reference's thickness 1; `img` is never written to and must be uint8; arrows longer than 2^20
pixels are skipped) and matrix fitting (`Flow.matrix`, `get_flow_matrix`): the
reference's Python surface (reference `__init__.py:14-18`) over hand-written HIP kernels.  `Flow.from_kitti` / `Flow.from_sintel` and
`load_kitti` / `load_sintel` / `load_sintel_mask` read the dataset files without OpenCV and decode them on the device (DESIGN.md 3.15;
a list of paths gives one batch).  `Flow.error_stats` / `epe_map` / `epe` and `flow_error_stats` / `flow_epe` score an estimate against
a ground truth on the device (not in the reference).  `Flow.consistency` / `consistency_mask` / `filter_consistent` and
`flow_consistency` run the forward-backward check of a flow pair in one pass (not in the reference).  `Flow.smoothness` / `smoothness_map` /
`smoothness_stats` and `flow_smoothness` / `flow_smoothness_stats` give the edge-aware smoothness loss of a flow, differentiable with
respect to its vectors (not in the reference).  `Flow.photometric` / `photometric_map` / `photometric_stats` and
`flow_photometric` / `flow_photometric_stats` give the photometric loss between two frames, warp and comparison in one pass,
differentiable with respect to the vectors (not in the reference).  `Flow.census` / `census_map` / `census_stats` and
`flow_census` / `flow_census_stats` give the census loss between two frames -- soft ternary census signatures over a 3, 5 or 7 pixel
patch, warped and compared from LDS tiles in one pass -- differentiable with respect to the vectors (not in the
reference).  `Flow.ssim` / `ssim_map` / `ssim_stats` and `flow_ssim` / `flow_ssim_stats` give the structural-similarity loss between two
frames -- windowed means, variances and covariance over a 3, 5 or 7 pixel box that holds the usable pixels only, warped and compared
from LDS tiles in one pass -- differentiable with respect to the vectors (not in the reference).  `Flow.cost_volume` and
`flow_cost_volume` give the local cost volume of a flow network -- the features of one frame correlated with the warped features of the
other over a window of radius 1 to 4, warp and correlation from LDS tiles in one pass -- differentiable with respect to both feature
tensors and the vectors (not in the reference).  `Flow.corr_lookup`, `flow_corr_lookup` and
`corr_pyramid` give the correlation lookup of RAFT-style networks -- feat(p) . other_l / sqrt(C) sampled bilinearly around
(p + flow(p)) / 2^l on every pyramid level, computed on the fly without the all-pairs volume -- differentiable with respect to both
feature tensors, not the vectors (not in the reference).  `Flow.upsample_convex` and `upsample_flow_convex` give the
learned convex upsampling that ends every refinement iteration of such a network -- each of the k x k fine pixels of a coarse pixel mixes
the 3 x 3 neighbourhood of k flow under the softmax of its nine predicted logits, k = 2, 4 or 8, in one streaming pass --
differentiable with respect to the logits and the vectors (not in the reference).  `Flow.from_matching` and
`global_matching_flow` give the first flow of a matching-style network (GMFlow, UniMatch) -- for every pixel the softmax over ALL
positions of the other frame of feat(p) . other(q) / sqrt(C), the expected position minus p, and the matching probability, streamed
without the (H W)^2 volume -- differentiable with respect to both feature tensors (not in the reference); two float16
or two bfloat16 feature tensors, as a network under autocast has them, are matched on the matrix cores without a float32 copy, with
float32 results and gradients in the features' dtype.
`Flow.propagate` and `propagate_flow` give the flow propagation by attention that follows it -- the vector at p becomes the softmax over
all positions q, or over a zero-padded window of radius 1 to 4, of query(p) . key(q) / sqrt(C), times flow(q), with the positions the
flow's mask excludes left out, so that matched vectors fill occluded regions -- differentiable with respect to both feature tensors and
the vectors (not in the reference).  `Flow.match_local` and `local_matching_flow` give the local matching of the
refinement stage that follows -- the other frame's features warped by the flow, the softmax over the window of radius 1 to 4 of
feat(p) . W'(p + o) / sqrt(C) with the positions outside the frame excluded, and the expected offset added to the flow, in one pass
without the warped tensor or the volume -- differentiable with respect to both feature tensors and the vectors (not in
the reference).  `Flow.sequence_loss` / `sequence_stats` and `flow_sequence_loss` give the objective all of these networks train on --
the gamma-weighted sum over the T refinement outputs of the masked L1 (or end-point) distance to one ground truth, which is read once
for all T -- differentiable with respect to the predictions (not in the reference).  `Flow.chain` and `chain_flows` compose the 1 to
32 frame-to-frame flows of a clip into the flow from its first frame to its last -- the fold of `combine_with` mode 3, bit for bit where that fold takes no early
exit, as one walk per pixel in one launch, with every partial chain (the dense trajectories) on request (not in the reference).  No
CPU fallback: see
`_native.NativeUnavailable`.
"""
from .flow_class import Flow, set_revalidate_every_call, get_revalidate_every_call
from .flow_operations import (combine_flows, switch_flow_ref, invert_flow, valid_target, valid_source, batch_flows,
                              get_flow_padding, visualise_flow, visualise_flow_arrows, get_flow_matrix,
                              flow_error_stats, flow_epe, flow_consistency, flow_smoothness, flow_smoothness_stats,
                              flow_photometric, flow_photometric_stats, flow_census, flow_census_stats,
                              flow_ssim, flow_ssim_stats, flow_cost_volume, flow_corr_lookup, corr_pyramid, upsample_flow_convex,
                              global_matching_flow, propagate_flow, local_matching_flow, flow_sequence_loss, chain_flows)
from .utils import (from_matrix, from_transforms, load_kitti, load_sintel, load_sintel_mask, resize_flow, apply_flow, is_zero_flow, get_pure_pytorch,
                    set_pure_pytorch, unset_pure_pytorch, to_numpy, to_tensor, move_axis, apply_s_flow,
                    grid_from_unstructured_data, get_flow_endpoints, threshold_vectors, normalise_coords, track_pts,
                    set_half_flow_outputs, get_half_flow_outputs, set_mesh_interpolation, get_mesh_interpolation)
from ._native import NativeUnavailable

__version__ = "0.1.0"
