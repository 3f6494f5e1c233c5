/*
 * oflib_hip.h -- C ABI of libofl_hip.so: the MI355X (gfx950) kernels behind the dense
 * flow warp / compose hot path of oflibpytorch.
 *
 * The reference (oflibpytorch v2.1.1) is pure Python and has no FFI layer of its own; the
 * arithmetic of this path lives in two ATen call sites.  The entry points below are what a
 * binding for exactly that path replaces:
 *
 *   ofl_warp_bwd_f32        <- F.grid_sample(target, normalise_coords(grid - flow))
 *                              src/oflibpytorch/utils.py:541-555 (+ normalise_coords :445-466),
 *                              with the mask channel / threshold / AND of Flow.apply
 *                              (flow_class.py:896-898, 921-934) and the vector add of
 *                              combine_with mode 3 (flow_class.py:1804, 1808; __add__ :450-488)
 *                              fused in.
 *   ofl_splat_fwd_f32 +     <- density.scatter_add_ / grid_data.scatter_add_ and the normalise
 *   ofl_splat_finalize_f32     pass of grid_from_unstructured_data (utils.py:1061-1154), with
 *                              get_flow_endpoints (:1045-1058), the zero-flow occlusion rule and
 *                              un-occlude fill of apply_s_flow (:1157-1205) and Flow.apply's mask
 *                              channel (flow_class.py:880-898, 921-923) fused in.
 *   ofl_flow_flags_f32      <- get_valid_vecs' isfinite().all() (utils.py:98), threshold_vectors
 *                              (:623-643), is_zero_flow (:919-938), Flow.is_zero
 *                              (flow_class.py:1226-1244): the data-dependent early-exit tests.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HIP); nothing is allocated or freed inside;
 *   - images are planar N-C-H-W, rows contiguous (stride_w = 1, stride_h = W, channel stride
 *     = H*W); the batch stride of every input is explicit, in ELEMENTS, and may be 0 to
 *     broadcast one batch element (the reference's 1<->N `expand`, utils.py:527-537);
 *   - masks are 1 byte per pixel, 0 = False, anything else = True (torch.bool storage);
 *   - `stream` is a hipStream_t passed as void*; launches are asynchronous on it;
 *   - return value: 0 on success, OFL_E_* (< 0) for rejected arguments, or a positive
 *     hipError_t from the launch.
 *   - all arithmetic is IEEE fp32 in the reference's operation order (no fast-math, no
 *     implicit contraction); masks are bit-exact with the reference's PyTorch-CPU path.
 */
#ifndef OFLIB_HIP_H
#define OFLIB_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OFL_OK 0
#define OFL_E_NULL -1      /* a required pointer is NULL */
#define OFL_E_SHAPE -2     /* n, c, h or w out of range (all must be >= 1; h*w < 2^24, utils.py:1118) */
#define OFL_E_ARG -3       /* inconsistent optional arguments */
#define OFL_E_UNSUPPORTED -4 /* this entry point cannot take the launch (alignment / channel count): use the general one */

/* library / build identification: returns e.g. 11 for 0.1.1 */
int ofl_version(void);

/* Process-wide options (testing / benchmarking aids; defaults are what production uses).
 *   OFL_OPT_WARP_PATH: 0 = auto (LDS-staged kernel when the launch is eligible: W >= 4, H >= 2; > 3 channels in ONE launch that loops over them;
 *                          generic direct-gather kernel otherwise -- both restate the same arithmetic),
 *                      1 = generic direct-gather kernel only,
 *                      3 / 4 = like auto, but the staged kernel with two tiles / one tile per block whatever the launch size
 *                          (auto picks by size: one tile per block for tiny launches, two for small ones, columns of four
 *                          from ~B = 8 at 1080p; all three run the same device code per tile -- tests compare them),
 *                      5 = like auto, but a warp of more than 3 channels runs as separate launches of 3 channels instead of the
 *                          channel-loop kernel (one launch that walks the channels in groups of 4 inside the block; W % 4 == 0),
 *                      6 = like auto, but the four-tile column kernel of large launches stages ONE y-sheared rectangle per tile instead of
 *                          per-row extents (the default for plain warps of 1..3 channels with W % 4 == 0 and no rounding: every source row
 *                          a 64 x 16 tile touches has its own first chunk and length; small launches run it with 1 or 2 tiles per block),
 *                      7 = like auto, but plain lean launches take the four-tile row-table columns whatever their size (tests). */
#define OFL_OPT_WARP_PATH 1
/*   OFL_OPT_WARP_SHEAR: 1 = the LDS-staged warp kernel stages a y-sheared box (default), 0 = plain bounding box
 *   (speed only; the results are identical). */
#define OFL_OPT_WARP_SHEAR 3
/*   OFL_OPT_SPLAT_PASS_IMAGES: upper bound on the images ofl_splat_tiled_f32 handles per pass (0 = automatic: one pass
 *   unless the fallback accumulator of a pass would pass 2^31 floats; tests use small values to exercise the multi-pass
 *   code on small inputs). */
#define OFL_OPT_SPLAT_PASS_IMAGES 4
/*   OFL_OPT_SPLAT_FALLBACK_SLOTS: images the two-pass fallback accumulator of ofl_splat_tiled_f32 holds (0 = automatic: the
 *   pass, capped at 1 GiB); tests use 1 to exercise the rounds.
 *   All options are PROCESS-GLOBAL, unsynchronised testing / benchmarking aids: set them before any concurrent use of the
 *   library, never from two threads; production code leaves them alone. */
#define OFL_OPT_SPLAT_FALLBACK_SLOTS 5
/*   OFL_OPT_SPLAT_EXTRA_LDS: bytes of dynamic LDS added to the round-6 gather kernel's launches (0 = none) -- a measuring aid: it
 *   lowers the blocks a CU holds (28 672: two, 65 536: one) without changing a single instruction (tools/splat_occupancy.py). */
#define OFL_OPT_SPLAT_EXTRA_LDS 7
int ofl_set_option(int32_t key, int32_t value);
/* the (mangled) name of the kernel the library launched LAST, as the loaded code object spells it ("" before the first launch) --
 * a diagnostic: bench.py reports the instantiation the launchers actually picked for its roofline kernel.  Process-global, like
 * the options; the pointer stays valid while the library is loaded. */
const char* ofl_last_kernel_name(void);

/* rounding applied to the warped channels before the store (apply_flow utils.py:613-618,
 * Flow.apply flow_class.py:943-946): 0 none, 1 round-half-even, 2 round then clamp to [0,255] */
#define OFL_ROUND_NONE 0
#define OFL_ROUND_RINT 1
#define OFL_ROUND_U8 2

/*
 * Backward ("t"-reference) bilinear warp, zero padding, align_corners=True.
 *
 *   p        = (gx, gy) - flow_sign * flow[n]                       (fp32)
 *   G[n,c]   = bilinear(src[n,c], p)                                 (taps outside the image = 0)
 *   dst[n,c] = addend ? a_sign * addend[n,c] + g_sign * G[n,c] : G[n,c]      (then `round_mode`)
 *   valid[n] = (bilinear(src_mask ? src_mask[n] : 1, p) > 0.99999f) & (flow_mask ? flow_mask[n] : 1)
 *
 * flow      [*,2,H,W] fp32, flow_sign = +1 or -1 (exact negation; Flow.invert('t') of an 's' flow)
 * src       [*,C,H,W] fp32
 * src_b     [*,C,H,W] fp32 or NULL: the field gathered is src - src_b (ONE fp32 subtraction per value: the reference's
 *           `flow - self` in combine_with mode 1, flow_class.py:1763).  Only for C == 2 with `valid` wanted, no addend and
 *           no flag outputs on frames the staged kernel takes (W >= 4, H >= 2); otherwise OFL_E_UNSUPPORTED and the
 *           caller passes the materialised difference
 * src_mask  [*,H,W] u8 or NULL (all True)      -- the mask warped as an extra channel
 * flow_mask [*,H,W] u8 or NULL (all True)      -- ANDed after the warp
 * addend    [*,C,H,W] fp32 or NULL; may alias `flow` (mode-3 composition, C = 2)
 * dst       [N,C,H,W] fp32, contiguous         -- must not alias an input
 * valid     [N,H,W] u8 or NULL (not wanted)
 * flow_flags / src_flags: optional int32[N] / int32[N] (or NULL): flag words (see
 *           ofl_flow_flags_f32) of the `flow` operand (with flow_mask) and, when C == 2 and
 *           src is itself a flow field, of `src` (with src_mask), OR-ed in as a by-product of the
 *           same pass.  The caller zeroes them beforehand.
 * dst_flags: optional int32[N] (C == 2 and `valid` wanted, else OFL_E_ARG; zeroed in-stream): the flag word of the
 *           OUTPUT read as a flow under `valid` -- spares the validation pass over an intermediate flow.
 */
int ofl_warp_bwd_f32(const float* flow, int64_t flow_bs, float flow_sign,
                     const float* src, int64_t src_bs,
                     const float* src_b, int64_t src_b_bs,
                     const uint8_t* src_mask, int64_t src_mask_bs,
                     const uint8_t* flow_mask, int64_t flow_mask_bs,
                     const float* addend, int64_t addend_bs, float a_sign, float g_sign,
                     float* dst, uint8_t* valid,
                     int32_t* flow_flags, int32_t* src_flags, int32_t* dst_flags,
                     int32_t n, int32_t c, int32_t h, int32_t w,
                     int32_t round_mode, void* stream);

/*
 * The same warp with a flow that covers a WINDOW of the frame -- Flow.apply(target, padding=[top, bottom, left, right]) with a
 * 't' flow (flow_class.py:901-913, 924-932): the reference zero-pads the flow to the target's size and pads its mask with
 * False before the warp; here flow [*,2,fh,fw] and flow_mask [*,fh,fw] stay as they are and cover rows foy .. foy + fh - 1,
 * columns fox .. fox + fw - 1 of the h x w frame of src / dst: outside the window the flow reads 0 and the flow mask False
 * (no padded copies).  Generic direct-gather kernel; no addend / src_b / flag outputs.  `cut` is a view of dst.
 */
int ofl_warp_bwd_win_f32(const float* flow, int64_t flow_bs, float flow_sign,
                         int32_t fh, int32_t fw, int32_t foy, int32_t fox,
                         const float* src, int64_t src_bs,
                         const uint8_t* src_mask, int64_t src_mask_bs,
                         const uint8_t* flow_mask, int64_t flow_mask_bs,
                         float* dst, uint8_t* valid,
                         int32_t n, int32_t c, int32_t h, int32_t w,
                         int32_t round_mode, void* stream);

/*
 * The same warp for 8-bit images (Flow.apply / apply_flow on uint8 targets, flow_class.py:943-951, utils.py:613-618):
 * src [*,C,H,W] uint8 is read as it is (no float copy); dst is fp32 [N,C,H,W] (dst_is_u8 = 0, any round_mode) or uint8
 * (dst_is_u8 = 1, round_mode must be OFL_ROUND_U8: round half to even, clamp to [0, 255] -- the values the reference's
 * `torch.round` / `clamp` / `.to(uint8)` produce).  17 instead of 35 bytes per pixel for C = 3 with masks, and no
 * conversion passes around the kernel.  Staged kernel only (W >= 4, H >= 2), else OFL_E_UNSUPPORTED: convert and
 * use ofl_warp_bwd_f32.
 */
int ofl_warp_bwd_u8(const float* flow, int64_t flow_bs, float flow_sign,
                    const uint8_t* src, int64_t src_bs,
                    const uint8_t* src_mask, int64_t src_mask_bs,
                    const uint8_t* flow_mask, int64_t flow_mask_bs,
                    void* dst, int32_t dst_is_u8, uint8_t* valid,
                    int32_t n, int32_t c, int32_t h, int32_t w,
                    int32_t round_mode, void* stream);

/*
 * Forward ("s"-reference) splat, pass 1: scatter-add of weight * value into `accum`.
 *
 *   (x, y)  = xy ? (xy_x[n], xy_y[n]) : (gx, gy) + flow_sign * flow[n]
 *   zero    = occlude && |flow_u| < 1e-3f && |flow_v| < 1e-3f         (strict, per component)
 *   wmask   = (weight_mask ? weight_mask[n] : 1) && !zero
 *   accum[n,0]       += w_corner * wmask                              (density)
 *   accum[n,1+c]     += w_corner * wmask * data_sign * data[n,c]
 *   accum[n,1+C]     += w_corner * wmask * !(chan_mask_a & chan_mask_b)  (only if with_mask_chan: the
 *                       INVALID weight; pass 2 forms density - invalid, which is exactly the density --
 *                       ratio exactly 1 -- when every contributor is valid, in any accumulation order)
 *
 * accum [N, 1 + C + with_mask_chan, H, W] fp32 workspace, zeroed by the caller.
 * Either `flow` (endpoints computed in-kernel, get_flow_endpoints) or `xs`/`ys` (explicit
 * positions, grid_from_unstructured_data) must be given; occlude requires `flow`.
 */
int ofl_splat_fwd_f32(const float* flow, int64_t flow_bs, float flow_sign,
                      const float* xs, const float* ys, int64_t xy_bs,
                      const float* data, int64_t data_bs, float data_sign,
                      const uint8_t* weight_mask, int64_t weight_mask_bs,
                      const uint8_t* chan_mask_a, int64_t chan_mask_a_bs,
                      const uint8_t* chan_mask_b, int64_t chan_mask_b_bs,
                      int32_t with_mask_chan, int32_t occlude,
                      float* accum,
                      int32_t n, int32_t c, int32_t h, int32_t w, void* stream);

/*
 * Forward splat, pass 2: normalise, masks, un-occlude fill.
 *
 *   den        = accum[n,0];  dcl = max(den, 1e-3f)
 *   dst[n,c]   = accum[n,1+c] / dcl ;  mch = (den - accum[n,1+C]) / dcl
 *   where (weight_mask & zero & den == 0) [occlude only]:  dst[n,c] = data_sign*data[n,c], mch = chan masks
 *   density[n] = den                      (optional)
 *   warped[n]  = den > 0                  (optional; apply_s_flow's returned mask)
 *   valid[n]   = mch > 0.99999f           (optional; requires with_mask_chan)
 *   mask_chan[n] = mch                    (optional; requires with_mask_chan; valid_target's `== 1` test)
 *   then `round_mode` on dst.
 */
int ofl_splat_finalize_f32(const float* accum,
                           const float* flow, int64_t flow_bs,
                           const float* data, int64_t data_bs, float data_sign,
                           const uint8_t* weight_mask, int64_t weight_mask_bs,
                           const uint8_t* chan_mask_a, int64_t chan_mask_a_bs,
                           const uint8_t* chan_mask_b, int64_t chan_mask_b_bs,
                           int32_t with_mask_chan, int32_t occlude,
                           float* dst, float* density, uint8_t* warped, uint8_t* valid, float* mask_chan,
                           int32_t n, int32_t c, int32_t h, int32_t w,
                           int32_t round_mode, void* stream);

/*
 * Forward splat, single fused call (the fast path of the two passes above, same arguments) -- an in-order GATHER:
 * a bin kernel appends the id of every 16 x 2 source subtile to the list of each destination tile (64 x 16: ofl_splat_tile_geometry) its end points
 * touch; a gather kernel (one block per destination tile) re-reads the listed source pixels, keeps those that land in
 * the tile as LDS records per unit cell, puts every cell in raster order of its source pixels and sums each destination
 * pixel's contributions in registers, per corner class in that order and ((c0 + c1) + c2) + c3 across the classes -- the
 * order of the reference's four scatter_add_ passes and corner sum (utils.py:1133-1143): results are BIT-IDENTICAL to the
 * reference's (and from run to run), not just within a tolerance.  Normalise / masks / un-occlude fill happen in the
 * same kernel; no float atomics, no accumulator, no per-pixel records in HBM.
 * Needs 4 <= W < 32768, H < 32768 (any width: 16-byte accesses at 4-byte alignment; more than 3 channels are
 * processed in groups of 3), else it returns OFL_E_UNSUPPORTED and the caller
 * uses ofl_splat_fwd_f32 + ofl_splat_finalize_f32.
 *   workspace      int32[ofl_splat_tiled_workspace_ints(n, h, w)]: 8 statistics words | one flag per image | list
 *                  lengths | 256 list entries per destination tile | the redo list (up to 16 bands of 2 words per tile),
 *                  sized for ONE pass of the batch (fixed addresses; ~2 B/px).  Contents irrelevant on entry: the first
 *                  pass zeroes statistics, flags and lengths in-stream, a later pass the redo counters, flags and lengths
 *                  (the statistics accumulate over the call), every further channel group the redo counters; list
 *                  entries are read only below the length their pass wrote.  Afterwards workspace[0] = 1
 *                  if some IMAGE took the two-pass path, workspace[1] = number of tiles that left the exact path,
 *                  workspace[2] = number of such images
 *   data_b         optional [*,C,H,W] fp32 (C <= 2, else OFL_E_ARG): the data splatted is data - data_b (ONE fp32 subtraction per value, the
 *                  reference's `flow - self` in combine_with modes 1-2, flow_class.py:1763,1768), then x data_sign
 *   dst_flags      optional int32[N] (C == 2 only, else OFL_E_ARG; zeroed in-stream): the flag word (see
 *                  ofl_flow_flags_f32) of the OUTPUT read as a flow under its `valid` mask -- a by-product that spares
 *                  the caller the validation pass (utils.py:98, flow_class.py:1226-1244) over an intermediate flow
 *   accum_fallback fp32[ofl_splat_tiled_fallback_images(n, planes, h, w) * planes * H * W] with planes = 1 + min(C, 3) +
 *                  with_mask_chan (at most one pass of the batch, capped at 1 GiB: flagged images beyond that are served
 *                  in rounds).  Contents irrelevant on entry:
 *                  used (and zeroed in-stream, per image and round, by the kernel that then adds into it) only for an image in which a destination tile is touched by
 *                  more than 256 source subtiles (16 x 2 pixels each) or a subtile spreads over more than 256 destination tiles: the two-pass
 *                  global-atomics path then runs for THAT image inside the same call, decided on the device (no host
 *                  sync; tolerance instead of bit-exactness).  A heavy fold of the flow (> 64 source pixels ending in
 *                  one unit cell, or more records for one tile than four bands of its rows can hold) makes only ITS
 *                  tile fall back to (LDS) float atomics.  The limits are on lengths, never on timing: the choice of
 *                  path, and with it every bit of the result, is the same in every run.
 */
int64_t ofl_splat_tiled_workspace_ints(int32_t n, int32_t h, int32_t w);
int64_t ofl_splat_tiled_pass_images(int32_t n, int32_t h, int32_t w);   /* images handled per pass (<= n) */
/* images `accum_fallback` must hold, for `planes` = 1 + min(C, 3) + (with_mask_chan ? 1 : 0) planes per image: the pass, capped
 * at 1 GiB (>= 1) -- accum_fallback is fp32 [that many, planes, H, W] */
int64_t ofl_splat_tiled_fallback_images(int32_t n, int32_t planes, int32_t h, int32_t w);
/* the geometry this build of the gather splat works with (what the stats words of a call count in, and what a caller that wants
 * to provoke / predict the fallbacks has to know): destination tile width and height in pixels, and the number of 16 x 2 source
 * subtiles one destination tile can list before its IMAGE takes the two-pass path.  Any pointer may be NULL; returns OFL_OK. */
int ofl_splat_tile_geometry(int32_t* tile_w, int32_t* tile_h, int32_t* list_capacity);
/* resources of the gather kernel the given kind of call runs on (round 6: the evidence behind "three blocks per CU"), as the HIP
 * runtime reports them for the loaded code object: info4[0] = 512-thread blocks resident per CU (with `extra_lds` bytes of dynamic
 * LDS added, see OFL_OPT_SPLAT_EXTRA_LDS), [1] = static LDS bytes per block, [2] = VGPRs, [3] = scratch bytes per thread.
 * channels 1..3; elem 0 = fp32, 1 = fp16 in / fp32 out, 2 = fp16 in and out (2 channels), 3 / 4 = an fp32 flow with fp16 / bf16 data
 * and dst (ofl_splat_sum_x16; no mask channel); lean: the common-case instantiation
 * (a flow, no window, W % 4 == 0, no rounding; 2 and 3 channels).  Needs a HIP device. */
int ofl_splat_gather_info(int32_t channels, int32_t with_mask_chan, int32_t elem, int32_t lean, int32_t extra_lds, int32_t* info4);
int ofl_splat_tiled_f32(const float* flow, int64_t flow_bs, float flow_sign,
                        const float* xs, const float* ys, int64_t xy_bs,
                        const float* data, int64_t data_bs, float data_sign,
                        const float* data_b, int64_t data_b_bs,
                        const uint8_t* weight_mask, int64_t weight_mask_bs,
                        const uint8_t* chan_mask_a, int64_t chan_mask_a_bs,
                        const uint8_t* chan_mask_b, int64_t chan_mask_b_bs,
                        int32_t with_mask_chan, int32_t occlude,
                        float* dst, float* density, uint8_t* warped, uint8_t* valid, float* mask_chan,
                        int32_t* dst_flags,
                        int32_t* workspace, int64_t workspace_ints, float* accum_fallback,
                        int32_t n, int32_t c, int32_t h, int32_t w,
                        int32_t round_mode, void* stream);

/*
 * ofl_splat_tiled_f32 with a flow that covers a WINDOW of the frame -- Flow.apply(target, padding=...) with an 's' flow
 * (flow_class.py:880-895, 906-913): the reference pads the flow with mode 'replicate' and its mask with False.  Here flow
 * [*,2,fh,fw], weight_mask and chan_mask_b [*,fh,fw] are read through replicate addressing (flow) / False outside the
 * window (masks; a NULL chan_mask_b is "all True INSIDE the window"; a NULL weight_mask still means every pixel of the frame
 * contributes: consider_mask=False); data, chan_mask_a and every output have the h x w geometry of the frame.
 * Same kernels as ofl_splat_tiled_f32 (bit-identical sums), per-pixel loads for the windowed operands.
 */
int ofl_splat_tiled_win_f32(const float* flow, int64_t flow_bs, float flow_sign,
                            int32_t fh, int32_t fw, int32_t foy, int32_t fox,
                            const float* data, int64_t data_bs, float data_sign,
                            const uint8_t* weight_mask, int64_t weight_mask_bs,
                            const uint8_t* chan_mask_a, int64_t chan_mask_a_bs,
                            const uint8_t* chan_mask_b, int64_t chan_mask_b_bs,
                            int32_t with_mask_chan, int32_t occlude,
                            float* dst, float* density, uint8_t* warped, uint8_t* valid, float* mask_chan,
                            int32_t* workspace, int64_t workspace_ints, float* accum_fallback,
                            int32_t n, int32_t c, int32_t h, int32_t w,
                            int32_t round_mode, void* stream);

/*
 * The weighted sums of a forward splat WITHOUT the division by the density:
 *   dst[n,c,q] = sum over source pixels i and corners k that land on q of  w_ik * data_sign * data[n,c,i]
 * with the weights of ofl_splat_tiled_f32 (every pixel contributes: no weight mask, no occlusion rule) at the end points
 * unnormalise(grid + flow_sign * flow) -- the float32 sample positions of ofl_warp_bwd_f32, through normalise_coords and the
 * grid sampler's un-normalise on every axis longer than 1, so that the weights are the forward warp's bit for bit.
 * This is the transpose of the backward warp: with data = the upstream gradient and flow_sign = MINUS the warp's
 * flow_sign it is the gradient of ofl_warp_bwd_f32 with respect to its source (ATen: the grad_input scatter of
 * grid_sampler_2d_backward) -- one gather launch instead of twelve global float atomics per pixel (B=16 1080p C=3:
 * 1.0 ms instead of 7.1 ms).  Same workspace, fallback accumulator ((1 + C) planes per image of a pass) and limits as
 * ofl_splat_tiled_f32; OFL_E_UNSUPPORTED for shapes that one does not take (the caller then uses the atomics of
 * ofl_warp_bwd_grad_f32).
 */
int ofl_splat_sum_f32(const float* flow, int64_t flow_bs, float flow_sign,
                      const float* data, int64_t data_bs, float data_sign, float* dst,
                      int32_t* workspace, int64_t workspace_ints, float* accum_fallback,
                      int32_t n, int32_t c, int32_t h, int32_t w, void* stream);

/*
 * Per-batch-element flag word of a flow field (OR-ed into flags[n]; caller zeroes):
 *   bit 0 (1)  some component is NaN / +-Inf
 *   bit 1 (2)  some component != 0
 *   bit 2 (4)  some component outside (-thr, thr)
 *   bit 3 (8)  some component != 0 where mask is True
 *   bit 4 (16) some component outside (-thr, thr) where mask is True
 * mask [*,H,W] u8 or NULL (all True).
 */
#define OFL_FLAG_NONFINITE 1
#define OFL_FLAG_NZ 2
#define OFL_FLAG_NZ_THR 4
#define OFL_FLAG_NZ_MASKED 8
#define OFL_FLAG_NZ_THR_MASKED 16

int ofl_flow_flags_f32(const float* flow, int64_t flow_bs,
                       const uint8_t* mask, int64_t mask_bs, float thr,
                       int32_t* flags, int32_t n, int32_t h, int32_t w, void* stream);

/*
 * The same reduction with the read-back built in (the reference's constructor raises on non-finite vectors, utils.py:98, so
 * `Flow(...)` has to WAIT for the words: this entry point makes that wait one kernel and one polled host word instead of a
 * memset, the kernel, a copy and an event).
 *   flow        [*,2,H,W] fp32, or fp16 when flow_is_f16 (then H*W % 4 == 0 and 8 / 4-byte aligned planes, else
 *               OFL_E_UNSUPPORTED);
 *   work        DEVICE int32[n + OFL_FLAGS_HOST_WORK_EXTRA], all zero before the first call; the kernel leaves it all zero again
 *               (flag words + arrival counters: one buffer can serve every later call on the same stream, ONE call in flight
 *               at a time);
 *   host_words  HOST-VISIBLE int32[2 * n], 8-byte aligned (hipHostMalloc, coherent + mapped: ofl_host_words_alloc): the block
 *               that finishes last stores, for every batch element i, the pair {host_words[2 i] = serial, host_words[2 i + 1] =
 *               flag word} with ONE 8-byte store.  The caller polls until every host_words[2 i] == serial (a value it has not
 *               used before) and reads the words beside them.
 * Contract of the shared buffers (what the binder must enforce; oflibpytorch_amd/_native.py does it with a pool of slots):
 *   * ONE call in flight per (work, host_words) pair -- a second launch on the same pair before the first one's words have
 *     been seen corrupts both.  Two threads (or two streams) that validate at once need two pairs; nothing in the library
 *     serialises them.  The last block zeroes the arrival counters with returning atomics BEFORE it publishes the first pair,
 *     so a pair may be handed to the next call (on any stream) the moment every host_words[2 i] == serial has been read.
 *   * The wait is a HOST poll of memory the kernel writes: it cannot be part of a stream capture / hipGraph, and the calling
 *     thread spins (then sleeps) until the device has run the kernel.  A caller that builds graphs validates outside them
 *     (ofl_flow_flags_f32 writes device words and captures fine).
 *   * If the caller abandons a wait (exception, interrupt) it must synchronise the stream before it re-uses or frees the pair.
 */
#define OFL_FLAGS_HOST_WORK_EXTRA 33
int ofl_flow_flags_host(const void* flow, int32_t flow_is_f16, int64_t flow_bs,
                        const uint8_t* mask, int64_t mask_bs, float thr,
                        int32_t* work, int32_t* host_words, int32_t serial,
                        int32_t n, int32_t h, int32_t w, void* stream);
/* pinned, coherent, device-mapped host words for ofl_flow_flags_host (zeroed); *out is usable as host AND device pointer */
int ofl_host_words_alloc(int64_t ints, void** out);
int ofl_host_words_free(void* ptr);

/*
 * fp16-STORED FLOWS (BASELINE config 5; SURVEY.md section 8b "fp16-I/O variants").  The reference up-casts every flow to
 * fp32 on entry (utils.py:95, 118) and computes in fp32; so do these entry points -- the up-conversion is exact and happens
 * in registers, the arithmetic is the fp32 arithmetic of the plain entry points, and the results are bit-identical to
 * feeding them the up-cast tensors -- but the fp16 planes are read as they are (half the operand bytes, no conversion pass).
 *
 *   ofl_flow_from_f16     validation of an fp16-stored flow: flags[n] |= flag word under `mask` (caller zeroes flags) and,
 *                         when dst != NULL, dst[N,2,H,W] fp32 = (float) src in the same pass (12 instead of 12 + 9 B/px).
 *                         dst == NULL: flags only (5 B/px) -- the flow stays in fp16.  src [*,2,H,W] fp16, H*W % 4 == 0,
 *                         8-byte aligned planes (dst 16-byte, mask 4-byte aligned); otherwise OFL_E_UNSUPPORTED.
 *   ofl_splat_tiled_f16   ofl_splat_tiled_f32 for a flow splatted by a flow (switch_ref, invert, Flow.apply(Flow) with 's'
 *                         flows): warper flow_f16 [*,2,H,W] and data data_f16 [*,2,H,W] both fp16; dst [N,2,H,W] fp32, or
 *                         fp16 when dst_is_f16 (an OPTION for fp16 pipelines: one round-to-nearest-even at the store, and
 *                         dst_flags then describe the stored values; never the default -- the reference returns fp32).
 *                         Same gather kernels, same bit-exact sums, same workspace / fallback contract.
 *   ofl_warp_bwd_h_f32    ofl_warp_bwd_f32 with a 2-channel SOURCE stored in fp16 (the `flow` operand of combine_with mode
 *                         1 't', flow_class.py:1763), optionally minus an fp32 src_b; fp32 warper, fp32 dst, valid mask.
 *                         Staged kernel only (W >= 4, H >= 2, H*W < 2^24), else OFL_E_UNSUPPORTED.
 */
int ofl_flow_from_f16(const void* src_f16, int64_t src_bs,
                      const uint8_t* mask, int64_t mask_bs,
                      float* dst, int32_t* flags,
                      int32_t n, int32_t h, int32_t w, void* stream);
int ofl_splat_tiled_f16(const void* flow_f16, int64_t flow_bs, float flow_sign,
                        const void* data_f16, int64_t data_bs, float data_sign,
                        const uint8_t* weight_mask, int64_t weight_mask_bs,
                        const uint8_t* chan_mask_a, int64_t chan_mask_a_bs,
                        const uint8_t* chan_mask_b, int64_t chan_mask_b_bs,
                        int32_t with_mask_chan, int32_t occlude,
                        void* dst, int32_t dst_is_f16, uint8_t* valid, int32_t* dst_flags,
                        int32_t* workspace, int64_t workspace_ints, float* accum_fallback,
                        int32_t n, int32_t h, int32_t w, void* stream);
int ofl_warp_bwd_h_f32(const float* flow, int64_t flow_bs, float flow_sign,
                       const void* src_f16, int64_t src_bs,
                       const float* src_b, int64_t src_b_bs,
                       const uint8_t* src_mask, int64_t src_mask_bs,
                       const uint8_t* flow_mask, int64_t flow_mask_bs,
                       float* dst, uint8_t* valid,
                       int32_t n, int32_t h, int32_t w, void* stream);

/*
 * FEATURE TENSORS STORED IN fp16 / bf16 (Flow.apply / apply_flow 't' of an N-C-H-W tensor held in half precision, as flow
 * networks under autocast hold them).  The reference converts the target to fp32, samples in fp32 and converts the result
 * back (utils.py:512-618: `target.float()` -> grid_sample -> `result.to(target_dtype)`); so does this entry point, inside
 * the kernel: the 16-bit planes are up-converted at the load (exact), the fp32 arithmetic is that of ofl_warp_bwd_f32 in
 * the same order, and the result is rounded ONCE, to nearest even, at the store (NaN -> a NaN, +-inf and overflow -> +-inf,
 * as `Tensor.to`).  Bit-identical to converting, calling ofl_warp_bwd_f32 and converting back, without the two fp32 copies
 * (2 + 2 instead of ~20 bytes per element through HBM).
 *
 *   ofl_warp_bwd_x16      the arguments of ofl_warp_bwd_f32, with src [*,C,H,W] and dst [N,C,H,W] planes of `dtype`
 *                         (OFL_X16_HALF: IEEE binary16, OFL_X16_BFLOAT: bfloat16) at 2-byte alignment, any W; `flow` fp32.
 *                         src_mask / flow_mask / valid as there; batch strides of 0 broadcast.  The PLAIN warp only: with
 *                         src_b, addend, flow_flags / src_flags / dst_flags or a rounding mode, off the automatic
 *                         OFL_OPT_WARP_PATH, or beyond the staged kernels (W < 4, H < 2, H*W >= 2^24) it returns
 *                         OFL_E_UNSUPPORTED and launches nothing: convert and call ofl_warp_bwd_f32 (a flow window:
 *                         ofl_warp_bwd_win_f32).  OFL_E_ARG for another dtype.  ofl_last_kernel_name() then names an
 *                         instantiation on `half_t` / `bf16_t`.
 */
#define OFL_X16_HALF 0
#define OFL_X16_BFLOAT 1
int ofl_warp_bwd_x16(const float* flow, int64_t flow_bs, float flow_sign,
                     const void* src, int64_t src_bs,
                     const void* src_b, int64_t src_b_bs,
                     const uint8_t* src_mask, int64_t src_mask_bs,
                     const uint8_t* flow_mask, int64_t flow_mask_bs,
                     const void* addend, int64_t addend_bs, float a_sign, float g_sign,
                     void* dst, uint8_t* valid,
                     int32_t* flow_flags, int32_t* src_flags, int32_t* dst_flags,
                     int32_t n, int32_t c, int32_t h, int32_t w,
                     int32_t round_mode, int32_t dtype, void* stream);

/*
 * The BACKWARD pass of ofl_warp_bwd_x16, from and to the 16-bit planes: no fp32 copy of the source, of the upstream gradient or of
 * the source gradient.  Both are gathers without float atomics and compute what their fp32 siblings compute on the up-converted
 * inputs, bit for bit: the 16-bit values are up-converted at the load (exact), the fp32 arithmetic and its order are the siblings',
 * and a 16-bit output is rounded ONCE, to nearest even, at the store.  `dtype` as above (OFL_E_ARG for another); 16-bit planes at
 * 2-byte alignment, any W; negative batch strides are OFL_E_ARG.
 *
 *   ofl_warp_bwd_grad_x16   the gradient with respect to the FLOW: the arguments of ofl_warp_bwd_grad_f32 without grad_src /
 *                           grad_src_bs (that gradient is ofl_splat_sum_x16), src [*,C,H,W] and grad_out [N,C,H,W] (contiguous)
 *                           planes of `dtype`; grad_flow fp32 [N,2,H,W], written, not accumulated.  Up to 3 planes run the GRAD
 *                           instantiations of the staged kernels on `half_t` / `bf16_t`; more planes one pixel per lane, as the
 *                           fp32 entry point does (the sums chain over all planes).  A frame the staged kernels do not take
 *                           (W < 4, H < 2, H*W >= 2^24), or a call off the automatic OFL_OPT_WARP_PATH, returns
 *                           OFL_E_UNSUPPORTED and launches nothing: convert and call ofl_warp_bwd_grad_f32.
 *   ofl_splat_sum_x16       the gradient with respect to the SOURCE: ofl_splat_sum_f32 (raw weighted sums) with an fp32 flow,
 *                           `data` (the upstream gradient) and `dst` planes of `dtype`.  The gather kernel up-converts the data
 *                           at its record loads and sums in fp32 in its own order; the band launch and the fallback accumulator
 *                           stay fp32; only the store that produces dst converts.  Workspace, fallback accumulator, limits and
 *                           OFL_E_UNSUPPORTED cases of ofl_splat_sum_f32.
 */
int ofl_warp_bwd_grad_x16(const float* flow, int64_t flow_bs, float flow_sign,
                          const void* src, int64_t src_bs,
                          const void* grad_out, float g_scale, float* grad_flow,
                          int32_t n, int32_t c, int32_t h, int32_t w, int32_t dtype, void* stream);
int ofl_splat_sum_x16(const float* flow, int64_t flow_bs, float flow_sign,
                      const void* data, int64_t data_bs, float data_sign, void* dst,
                      int32_t* workspace, int64_t workspace_ints, float* accum_fallback,
                      int32_t n, int32_t c, int32_t h, int32_t w, int32_t dtype, void* stream);

/*
 * FEATURE TENSORS STORED N-H-W-C (Flow.apply / apply_flow 't' of a tensor in torch.channels_last, the memory format convolution
 * networks are trained in on this hardware).  The plain backward warp of ofl_warp_bwd_f32 / ofl_warp_bwd_x16 on that storage: the
 * four taps of a destination pixel are four runs of C contiguous elements, the destination is one streaming store, nothing is
 * transposed before or after.  The arithmetic and its order are those of ofl_warp_bwd_f32 (taps outside the frame are not loaded and
 * count as 0, in-bounds tests on floats); 16-bit elements are up-converted at the load (exact) and rounded ONCE, to nearest even, at
 * the store, as in ofl_warp_bwd_x16.  Bit-identical to transposing, calling the planar entry point and transposing back.  No atomics.
 *
 *   ofl_warp_bwd_nhwc     flow fp32 planes [*,2,H,W] as everywhere else; src [*,H,W,C] and dst [N,H,W,C] (contiguous in that order)
 *                         elements of `dtype` (OFL_NHWC_F32, OFL_X16_HALF, OFL_X16_BFLOAT); src_mask / flow_mask [*,H,W] and valid
 *                         [N,H,W] (optional, layout-free) as in ofl_warp_bwd_f32; batch strides in elements, 0 broadcasts one flow /
 *                         source / mask.  A lane owns 16 bytes of consecutive channels (4 with 16-bit elements when C % 8 != 0):
 *                         with C < 4 or C % 4 != 0, H < 2 or W < 2, src or dst not aligned to 16 bytes (fp32) / 8 bytes (16-bit),
 *                         N > 65535 or 2^32 lanes and more per image it returns OFL_E_UNSUPPORTED and launches nothing: take the
 *                         planar entry point.  OFL_E_ARG for another dtype, negative strides or sizes, a flow_sign other than +-1;
 *                         OFL_E_SHAPE for a zero size or H*W >= 2^31.  64-bit element offsets throughout (N*C*H*W may pass 2^31).
 *                         ofl_last_kernel_name() then names `warp_bwd_nhwc_kernel<float | half_t | bf16_t, channels per lane, valid>`.
 */
#define OFL_NHWC_F32 2
int ofl_warp_bwd_nhwc(const float* flow, int64_t flow_bs, float flow_sign,
                      const void* src, int64_t src_bs,
                      const uint8_t* src_mask, int64_t src_mask_bs,
                      const uint8_t* flow_mask, int64_t flow_mask_bs,
                      void* dst, uint8_t* valid,
                      int32_t n, int32_t c, int32_t h, int32_t w, int32_t dtype, void* stream);

/*
 * The BACKWARD pass of ofl_warp_bwd_nhwc without a transposed copy of the saved source or of the upstream gradient.
 *
 *   ofl_warp_bwd_grad_nhwc  the gradient with respect to the FLOW: the arguments of ofl_warp_bwd_grad_x16 with src [*,H,W,C] and
 *                           grad_out [N,H,W,C] elements of `dtype` (OFL_NHWC_F32, OFL_X16_HALF, OFL_X16_BFLOAT), read as they are
 *                           stored; grad_flow fp32 planes [N,2,H,W], written, not accumulated.  flow_bs 0: one flow for all images.
 *                           One pixel per lane and ONE chain per pixel over the channels 0 .. C-1 -- the arithmetic, order and
 *                           association of ofl_warp_bwd_grad_f32's one-pixel-per-lane kernel (g = g_scale * grad_out, eight updates
 *                           per channel, a tap outside the frame counts as 0 and is not loaded, in-bounds tests on floats, then
 *                           -flow_sign * (((gix * half_wm1) / wm1) * 2)), 16-bit elements up-converted exactly at the load: the
 *                           result equals the planar entry points' on the transposed operands bit for bit.  No LDS, no atomics,
 *                           64-bit element offsets.  OFL_E_UNSUPPORTED (nothing launched) with C < 4 or C % 4 != 0, H < 2 or W < 2,
 *                           src or grad_out not aligned to 16 bytes (fp32) / 8 bytes (16-bit), N > 65535; OFL_E_ARG, OFL_E_SHAPE and
 *                           OFL_E_NULL as ofl_warp_bwd_nhwc.  ofl_last_kernel_name() then names
 *                           `warp_grad_flow_nhwc_kernel<float | half_t | bf16_t, channels per chunk>`.
 *   ofl_nhwc_to_planes      bit copy of `elem_bytes`-sized elements (2 or 4, else OFL_E_ARG) from src [N,H,W,C] to dst [N,C,H,W];
 *   ofl_planes_to_nhwc      the same from src [N,C,H,W] to dst [N,H,W,C].  A tile of pixels x channels (64 x 32 4-byte, 128 x 64
 *                           2-byte elements) goes through LDS: 16-byte accesses on the N-H-W-C side (8 bytes with 2-byte elements
 *                           and C % 8 != 0), element-sized accesses coalesced along the pixels on the plane side (H*W may be odd).
 *                           The gradient with respect to the SOURCE uses them either side of ofl_splat_sum_f32 / _x16.  C any
 *                           multiple of 4, else OFL_E_UNSUPPORTED, as with the N-H-W-C operand not aligned to 16 bytes (4-byte
 *                           elements) / 8 bytes (2-byte), N > 65535 or C > 2 097 120.  The operands must not overlap (OFL_E_ARG, as
 *                           for a plane operand not aligned to its element, negative sizes); OFL_E_SHAPE for a zero size or
 *                           H*W >= 2^31.  64-bit offsets.  ofl_last_kernel_name() then names
 *                           `nhwc_transpose_kernel<unsigned int | unsigned short, elements per access, to planes>`.
 */
int ofl_warp_bwd_grad_nhwc(const float* flow, int64_t flow_bs, float flow_sign,
                           const void* src, int64_t src_bs,
                           const void* grad_out, float g_scale, float* grad_flow,
                           int32_t n, int32_t c, int32_t h, int32_t w, int32_t dtype, void* stream);
int ofl_nhwc_to_planes(const void* src, void* dst, int32_t n, int32_t c, int32_t h, int32_t w, int32_t elem_bytes, void* stream);
int ofl_planes_to_nhwc(const void* src, void* dst, int32_t n, int32_t c, int32_t h, int32_t w, int32_t elem_bytes, void* stream);


/* ------------------------------------------------------------------------------------------------
 * Either side of the path: backward passes, point tracking, padding extents.
 * ---------------------------------------------------------------------------------------------- */

/*
 * Backward pass of ofl_warp_bwd_f32 (the reference relies on autograd through F.grid_sample, utils.py:555, and through
 * normalise_coords / `grid - flow`, utils.py:462-465, 549; differentiability is asserted by its tests, e.g.
 * test_utils.py:500):
 *   grad_src[n,c,tap] += g_scale * w_tap * grad_out[n,c]       float atomics; grad_src is ZEROED BY THE CALLER; its batch
 *                                                               stride may be 0 when the forward source was broadcast
 *   grad_flow[n,:]     = -flow_sign * d(sample)/d(position)     [N,2,H,W], written (not accumulated); a broadcast flow's
 *                                                               gradient is the caller's sum over n
 * flow / src as in the forward call (src = the field that was gathered, i.e. src - src_b where that was used); grad_out
 * [N,C,H,W] contiguous; g_scale = the forward g_sign.  Either output may be NULL (not both).  Sums are not in ATen's CPU
 * order: results agree with the reference's autograd within fp32 rounding (tests: rtol 1e-4 of the gradient scale).
 */
int ofl_warp_bwd_grad_f32(const float* flow, int64_t flow_bs, float flow_sign,
                          const float* src, int64_t src_bs,
                          const float* grad_out, float g_scale,
                          float* grad_src, int64_t grad_src_bs, float* grad_flow,
                          int32_t n, int32_t c, int32_t h, int32_t w, void* stream);

/*
 * Backward pass of the forward splat (autograd through utils.py:1098-1144 and :1185-1203 in the reference; claims at
 * utils.py:1079-1080, 1167; asserted at test_utils.py:1113-1114).  A gather per source pixel, no atomics:
 *   grad_data[n,c,i] = sum_k w_ik * grad_out[n,c,p_ik] / max(D[p_ik], 1e-3)        (+ grad_out[n,c,i] where i was un-occlude-filled)
 *   grad_xy[n,0|1,i] = d/dx, d/dy of the same sums through the corner weights (and through D where D >= 1e-3)
 * flow|xs,ys / data (the data actually splatted: data_sign * (data - data_b)) / weight_mask / occlude as in the forward
 * call; out [N,C,H,W] and density [N,H,W] are the forward results (out before any rounding); grad_out [N,C,H,W];
 * grad_density optional [N,H,W] (upstream gradient of the density output).  grad_data [N,C,H,W], grad_xy [N,2,H,W]
 * (x then y; for a flow operand grad_flow = flow_sign * grad_xy) -- either may be NULL.  C <= 3 per call, else
 * OFL_E_UNSUPPORTED (split the channels; grad_density with the first group only; the grad_xy of the groups add up).
 * scratch: fp32[N * 4 * H * W], contents irrelevant on entry (a first pass leaves g_c / max(D, 1e-3) and the density term of every destination pixel in
 * one 16-byte slot: the divisions are done once, and the gather loads one slot per corner instead of 2 C + 1 scalars).
 */
int ofl_splat_grad_f32(const float* flow, int64_t flow_bs, float flow_sign,
                       const float* xs, const float* ys, int64_t xy_bs,
                       const float* data, int64_t data_bs,
                       const uint8_t* weight_mask, int64_t weight_mask_bs, int32_t occlude,
                       const float* out, const float* density,
                       const float* grad_out, const float* grad_density, float* scratch,
                       float* grad_data, float* grad_xy,
                       int32_t n, int32_t c, int32_t h, int32_t w, void* stream);

/*
 * Sparse point sampler of track_pts (utils.py:1004-1014, 1033-1035): pts [*,M,2] fp32 as (y, x); out[n,m] = pts + the
 * flow bilinearly sampled there (flip -> normalise_coords -> grid_sample(align_corners=True) -> flip: same fp32 operation
 * order and FMA chain as the dense warp), rows with a NaN set to 0.  pts_bs = 0 broadcasts one point list.
 * ..._grad: grad_flow [N,2,H,W] (float atomics; zeroed by the caller) and / or grad_pts [N,M,2].
 */
int ofl_sample_pts_f32(const float* flow, int64_t flow_bs, const float* pts, int64_t pts_bs, float* out,
                       int32_t n, int32_t m, int32_t h, int32_t w, void* stream);
int ofl_sample_pts_grad_f32(const float* flow, int64_t flow_bs, const float* pts, int64_t pts_bs,
                            const float* grad_out, float* grad_flow, float* grad_pts,
                            int32_t n, int32_t m, int32_t h, int32_t w, void* stream);

/*
 * Extents of the positions a flow reaches, under its mask -- the reduction of Flow.get_padding (flow_class.py:1196-1219):
 *   pos = -(sign * thr(v) - grid) per component (thr: threshold_vectors, |v| < 1e-3 -> 0); sign = +1 for 't', -1 for 's'
 *   extents[n] = { min y, max y, min x, max x, any valid pixel (0 / 1) }   fp32[N][5]
 * workspace int32[5 N] (scratch; contents irrelevant on entry: flow_extents_init_kernel writes all 5 N words first).  extents: written,
 * every one of the 5 N floats (an image without a valid pixel: the decoded start values and 0).  min / max are exact in any order.
 */
int ofl_flow_extents_f32(const float* flow, int64_t flow_bs, const uint8_t* mask, int64_t mask_bs, float sign,
                         int32_t* workspace, float* extents, int32_t n, int32_t h, int32_t w, void* stream);

/*
 * Valid area of a backward warp -- Flow.valid_target of a 't' flow (flow_class.py:1119-1122) and Flow.valid_source of an 's' flow
 * (:1151-1157; flow_sign = -1 restates its `-self._vecs`):
 *   valid[n] = (grid_sample(ones, normalise_coords(grid - flow_sign * flow[n]), align_corners=True) > thr) & mask[n]
 * replaces torch.ones + F.grid_sample (utils.py:555) + gt + and.  The all-ones image is never made: its taps are the in-frame
 * indicators of the four neighbours, blended by the same FMA chain -- bit-identical to warping a ones image.  mask may be NULL
 * (all True); valid uint8 [N,H,W]; thr = 0.9999f in both callers.  9 B/px read, 1 B/px written.
 */
int ofl_warp_valid_f32(const float* flow, int64_t flow_bs, float flow_sign, const uint8_t* mask, int64_t mask_bs, float thr,
                       uint8_t* valid, int32_t n, int32_t h, int32_t w, void* stream);

/*
 * Bilinear resize -- the `F.interpolate(x, scale_factor=[sh, sw], mode='bilinear')` (align_corners=False) of resize_flow
 * (utils.py:908) and Flow.resize (flow_class.py:710), computed as ATen's CPU kernels compute it, so that a resize on a HIP device
 * returns the reference's PyTorch-CPU values BIT FOR BIT (ATen's own GPU kernel differs in the last bits):
 *   source index fmaf(rcp_scale, dst + 0.5, -0.5) clamped at 0; a dimension that keeps its size is copied; ATen's two kernels
 *   (chosen by oh + ow <= 128) both restated -- see ofl_aux_kernels.hip / oracle/ofl_oracle.c.
 * src [planes, h, w] fp32 contiguous -> dst [planes, oh, ow]; the caller passes oh = floor(h * sh), ow = floor(w * sw) (doubles, as
 * torch computes the output size) and rcp_scale_* = (float)(1.0 / s*).  The components of a flow are scaled by the caller
 * afterwards (utils.py:913-914: two exact multiplications).  planes <= 65535.
 */
int ofl_resize_bilinear_f32(const float* src, float* dst, int32_t planes, int32_t h, int32_t w, int32_t oh, int32_t ow,
                            float rcp_scale_h, float rcp_scale_w, void* stream);

/*
 * Flow field of a 3 x 3 transformation matrix (flow_from_matrix, utils.py:339-376; the O(HW) half of from_matrix :646-705 and
 * from_transforms :729-807, whose 3 x 3 algebra stays on the host):
 *   hom      = M [x, y, 1]^T    accumulated as ATen's CPU batched matmul does for 3 x 3 operands (acc = 0; acc += m_ik * v_k)
 *   dst[n,0] = sign * (hom.x / hom.z - x),  dst[n,1] = sign * (hom.y / hom.z - y)
 * matrices [*,3,3] fp32 DEVICE memory (matrix_bs = 9, or 0 to broadcast one matrix), sign = +1 ('s') / -1 (the reference's
 * negation of its 't' branch, exact), dst [N,2,H,W] fp32.  Bit-identical to the reference's PyTorch-CPU result.
 */
int ofl_flow_from_matrix_f32(const float* matrices, int64_t matrix_bs, float sign, float* dst,
                             int32_t n, int32_t h, int32_t w, void* stream);

/*
 * The flag words of a batch (ofl_flow_flags_f32, or the by-product words of the warp / splat kernels), copied, followed by
 * their OR over the batch as FIVE 0 / 1 integers, one per bit -- the form an all-reduce (MAX; NCCL / RCCL has no bitwise
 * OR) over the ranks of a batch-sharded job needs, so that the reference's batch-global tests (isfinite().all(),
 * utils.py:98; all(is_zero), utils.py:497, flow_class.py:1046, 1729, 1738) stay exact under sharding with one launch, one
 * collective and one read-back per tensor.   words int32[N] -> out int32[N + 5]
 */
int ofl_flag_words_or_i32(const int32_t* words, int32_t n, int32_t* out, void* stream);

/*
 * Flow.visualise (flow_class.py:1246-1356) and visualise_flow (flow_operations.py:339-367): the HSV colour coding of a flow.
 * ofl_visualise.hip; bit-exact with the reference's NumPy / OpenCV host code (cv2.cartToPolar restated from OpenCV 4.x, its FMA form).
 *
 * ofl_visualise_workspace_ints(n): int32 words of the workspace ofl_visualise_range_f32 needs for n images (OFL_E_SHAPE if n is
 *   out of [1, 65535]).  The workspace is cleared inside the call (one hipMemsetAsync on `stream`).
 *
 * ofl_visualise_range_f32 <- the `range_max is None` branch (flow_class.py:1300-1309): per image, np.percentile(m, 99) (numpy 2.2.6,
 *   'linear', computed in fp32 as numpy computes it for fp32 input), else np.max(m) if that is > 0, else 1, over the magnitudes m of
 *   the thresholded flow (utils.py:623-643, strict fp32 test against 1e-3) -- all pixels, or the pixels where mask != 0 when `mask`
 *   is given (show_mask).  An exact order statistic (radix select on the fp32 bit patterns, integer histograms): bitwise
 *   reproducible.  flow [N,2,H,W] fp32 (flow_half = 0) or fp16 (flow_half = 1) with batch stride flow_bs (elements), mask
 *   [N,H,W] bytes or NULL, workspace int32[ofl_visualise_workspace_ints(n)], range_max float64[N] out, counts int32[N] out (the
 *   number of values per image; optional).  An image with no counted pixel gets range_max 1 and count 0: the caller raises numpy's
 *   IndexError for it.
 *
 * ofl_visualise_u8 <- flow_class.py:1287-1349: threshold, cartToPolar, hue = mod(angle, 360) / 2, value 255 (180 where show_mask
 *   and the mask is False), saturation clip(float64(mag * 255) / range_max, 0, 255) stored as fp32, mask borders
 *   (show_mask_borders: findContours + drawContours of :1323-1327 = the True pixels with a False 4-neighbour or on the image edge)
 *   set to 0, then mode 0 = 'hsv' (np.round of the planes), 1 = 'rgb', 2 = 'bgr' (the float64 HSV -> RGB of :1333-1349, rounded half
 *   to even).  mask NULL = all True.  range_max float64[N] DEVICE memory (ofl_visualise_range_f32's output, or the caller's values).
 *   out uint8: layout 0 = [N,3,H,W] planes (the tensor the reference returns), 1 = [N,H,W,3] (its NumPy array), contiguous.
 */
int64_t ofl_visualise_workspace_ints(int32_t n);
int ofl_visualise_range_f32(const void* flow, int64_t flow_bs, int32_t flow_half, const uint8_t* mask, int64_t mask_bs,
                            int32_t* workspace, double* range_max, int32_t* counts, int32_t n, int32_t h, int32_t w, void* stream);
int ofl_visualise_u8(const void* flow, int64_t flow_bs, int32_t flow_half, const uint8_t* mask, int64_t mask_bs, int32_t show_mask,
                     int32_t show_mask_borders, const double* range_max, int32_t mode, int32_t layout, uint8_t* out, int32_t n,
                     int32_t h, int32_t w, void* stream);

/*
 * Flow.matrix (flow_class.py:1566-1646) and get_flow_matrix (flow_operations.py:306-336): the similarity (dof 4), affine map
 * (dof 6) or homography (dof 8) of the point pairs of a flow field.  ofl_matrix.hip; the numerics are DEFINED in DESIGN.md 3.10
 * (the reference calls OpenCV's estimators; restated, not checked against OpenCV; no Levenberg-Marquardt polish).
 *
 * ofl_matrix_workspace_bytes(n, h, w, dof, method): bytes of the workspace ofl_matrix_fit_f64 needs (8-byte aligned; cleared
 *   inside the call by one hipMemsetAsync on `stream`), or OFL_E_SHAPE / OFL_E_ARG.
 *
 * ofl_matrix_fit_f64 <- the loop of flow_class.py:1632-1646: per image, the point pairs of :1600-1610 in float64 (ref 0 = 't':
 *   dst = grid, src = grid - vecs; 1 = 's': src = grid, dst = grid + vecs), of the pixels where mask != 0 (mask NULL = all; the
 *   `masked` argument), fitted by method 0 = 'lms' (float64 least squares: closed form / 3 x 3 normal equations / normalised DLT
 *   with cyclic Jacobi), 1 = 'ransac' (256 hypotheses, inliers within 3 px, most inliers wins) or 2 = 'lmeds' (128 hypotheses,
 *   smallest exact median of the squared residuals wins), the robust methods followed by ONE least-squares fit of the winner's
 *   inliers.  dof 4 / 6 / 8; any method with any dof (the 'lms' -> 'ransac' switch of :1612-1615 is the caller's).
 *   flow [N,2,H,W] fp32 (flow_half = 0) or fp16 (1), batch stride flow_bs (elements); mask [N,H,W] bytes, stride mask_bs.
 *   out_matrix float64[N * 9] (row-major 3 x 3; zeros where status != 0), out_info int32[N * 4] = {n_valid, the winner's k (-1 for
 *   'lms'), inlier count, status}; status 0 ok, 1 fewer valid pixels than the model needs (2 / 3 / 4), 2 no non-degenerate
 *   hypothesis, 3 singular fit of the inliers.  Integer atomics only and fixed summation order: bitwise reproducible, and image
 *   i's result does not depend on the batch.  h * w < 2^31, n <= 65535.
 */
int64_t ofl_matrix_workspace_bytes(int32_t n, int32_t h, int32_t w, int32_t dof, int32_t method);
int ofl_matrix_fit_f64(const void* flow, int64_t flow_bs, int32_t flow_half, int32_t ref, const uint8_t* mask, int64_t mask_bs,
                       int32_t n, int32_t h, int32_t w, int32_t dof, int32_t method, void* workspace, double* out_matrix,
                       int32_t* out_info, void* stream);

/*
 * Flow.visualise_arrows (flow_class.py:1358-1496) and visualise_flow_arrows (flow_operations.py:370-409): the flow as arrows on a
 * grid of points.  ofl_arrows.hip.  The reference's NumPy steps are kept bit for bit; the anti-aliased arrow itself is DEFINED in
 * DESIGN.md 3.11 (three capsules, float64, no fused multiply-add), not OpenCV's LINE_AA.  Grid points: rows
 * arange(grid_dist / 2, h - 1, grid_dist), columns likewise with w, P per image, row-major.  1 <= grid_dist <= min(h, w) / 2
 * (so h, w >= 2), else OFL_E_ARG; n <= 65535, n * P < 2^31.  Three calls on one stream, one workspace:
 *
 * ofl_arrows_workspace_ints(n, h, w, grid_dist): int32 words of the workspace (header | per-image sums | magnitudes | records | tile counts,
 *   offsets and cursors), or an OFL_E_* code.  Contents irrelevant on entry of each of the three calls below, as are those of `list`:
 *   the magnitudes are written by ofl_arrows_scale_f32 before its select reads them; ofl_arrows_plan zeroes the tile counts in-stream
 *   and writes every word of every record, every offset, every per-image sum and the header; ofl_arrows_u8 zeroes the cursors
 *   in-stream and reads only the list entries it has just filled.
 *
 * ofl_arrows_scale_f32 <- `scaling is None` (flow_class.py:1456-1458): the magnitudes of the thresholded flow at the grid points
 *   (cartToPolar, FMA form), np.percentile(., 99) over all n * P of them (numpy 2.2.6 'linear' in fp32; exact order statistics
 *   by one block's radix select), *scaling = fp32(grid_dist) / percentile (inf for a percentile of 0).  scaling: DEVICE float[1].
 *
 * ofl_arrows_plan <- flow_class.py:1459-1480 up to the drawing: per (image, grid point) the scaled magnitude and vector (fp32),
 *   drawn iff 0.5 < magnitude <= 2^20, the end point np.round(point +- vector) (float64, half to even; ref_s = 1: 's', arrow
 *   from the point, thickness 1 whatever `thickness`; 0: 't', arrow to the point), tip length fp32(tip_size) / magnitude, the
 *   barbs, the colour (`colour` = b | g << 8 | r << 16, or -1: the 'bgr' colour of Flow.visualise for the hue
 *   uint8(round(mod(angle, 360) / 2)) at full saturation), boxes clipped to the frame; then the number of arrows per 64 x 16
 *   output tile and the exclusive scan of those counts.  Afterwards workspace[0..1] (int64) = the list entries of all tiles: the
 *   caller reads it back and sizes `list` from it.  scaling: DEVICE float[1] (ofl_arrows_scale_f32's, or the caller's value);
 *   1 <= thickness <= 32767; tip_size = fp32(sqrt(thickness) * 3.5).
 *
 * ofl_arrows_u8 <- the drawing (flow_class.py:1468-1492): fills the tile lists, then one block per tile paints its pixels in
 *   registers: background (img uint8, img_layout 0 = [*,3,H,W] planes, 1 = [*,H,W,3], batch stride img_bs in BYTES, 0 broadcasts;
 *   NULL = white), the tile's arrows in the reference's order (image by image, point by point), each point's pixel set to
 *   (0, 0, 255) after its arrow, np.round(0.5 * pixel) outside the mask (show_mask), the mask borders black
 *   (show_mask_borders; the rule of ofl_visualise_u8), one store per pixel.  mask NULL = all True.  list int32[list_ints] with
 *   list_ints >= workspace[0..1] (a shorter list drops arrows, never writes past it).  out uint8, layout 0 = [N,3,H,W],
 *   1 = [N,H,W,3], BGR.  `img` is only read.  Bitwise reproducible: integer atomics only, order restored per tile.
 */
int64_t ofl_arrows_workspace_ints(int32_t n, int32_t h, int32_t w, int32_t grid_dist);
int ofl_arrows_scale_f32(const void* flow, int64_t flow_bs, int32_t flow_half, int32_t grid_dist, int32_t* workspace,
                         float* scaling, int32_t n, int32_t h, int32_t w, void* stream);
int ofl_arrows_plan(const void* flow, int64_t flow_bs, int32_t flow_half, int32_t ref_s, int32_t grid_dist, const float* scaling,
                    int32_t colour, int32_t thickness, float tip_size, int32_t* workspace, int32_t n, int32_t h, int32_t w,
                    void* stream);
int ofl_arrows_u8(const uint8_t* img, int64_t img_bs, int32_t img_layout, const uint8_t* mask, int64_t mask_bs, int32_t show_mask,
                  int32_t show_mask_borders, int32_t grid_dist, int32_t* workspace, int32_t* list, int64_t list_ints,
                  int32_t layout, uint8_t* out, int32_t n, int32_t h, int32_t w, void* stream);

/*
 * The triangle-mesh interpolator (ofl_mesh.hip): apply_flow(ref='s') and track_pts(ref='t') with PURE_PYTORCH unset
 * and set_mesh_interpolation() on -- where the reference calls scipy.interpolate.griddata (utils.py:577-600, :1020-1032).  Vertices:
 * pixel (i, j) of flow image b at (j + flow_sign * u, i + flow_sign * v) in float64; usable iff mask (NULL = all True) is set there and
 * both coordinates are finite.  Quad q = i * (w - 1) + j with four usable vertices gives triangles 2 q and 2 q + 1, split along the
 * diagonal the in-circle test keeps (a tie keeps (i, j)-(i + 1, j + 1)); zero-area triangles are dropped.  A query takes the barycentric
 * interpolation of the lowest-numbered triangle that contains it (edges included, exact signs of the float64 edge functions) or 0.
 * h, w >= 2, h * w < 2^30, nf <= 65535.  flow fp32 [nf,2,h,w] (flow_bs elements between images), mask uint8 [nf,h,w].
 *
 * ofl_mesh_workspace_ints(nf, h, w, points): int32 words of the workspace (header | tile offsets, counts, cursors), or an OFL_E_* code;
 *   points = 0: pixel queries over 64 x 16 tiles (ofl_mesh_apply), 1: point queries over 8 x 8 tiles (ofl_mesh_points).  Contents
 *   irrelevant on entry, as are those of `list`: ofl_mesh_plan zeroes the counts in-stream and writes every offset and the header,
 *   ofl_mesh_apply / ofl_mesh_points zero the cursors in-stream and read only the list entries they have just filled.
 *
 * ofl_mesh_plan: the number of quads whose box touches each tile and the exclusive scan of those counts.  Afterwards workspace[0..1]
 *   (int64) = the list entries of all tiles: the caller reads it back and sizes `list` from it.  Nothing is capped: a quad is listed in
 *   every tile its box touches.
 *
 * ofl_mesh_apply: fills the tile lists, then one block per tile: every pixel keeps the lowest triangle that contains its centre and
 *   interpolates the c channels of src ([*,c,h,w] fp32, or uint8 with src_u8 = 1; src_bs elements between images, 0 broadcasts; nf is
 *   1 or n) from that triangle's three source pixels; the float64 value is rounded to fp32, then by round_mode (OFL_ROUND_*; uint8 needs
 *   OFL_ROUND_U8).  dst [n,c,h,w] of src's type; inside (optional) uint8 [n,h,w] 1 where a triangle was found; owner (optional) int32
 *   [n,h,w] its number or -1.  list int32[list_ints] with list_ints >= workspace[0..1] (a shorter list drops quads, never writes past
 *   it).  Bitwise reproducible: the only atomics are integer minima and list cursors, and no result depends on the list's order.
 *
 * ofl_mesh_points: fills the lists of a points = 1 plan, then one thread per point: pts float64 [*,m,2] (y, x; pts_bs doubles between
 *   images, 0 broadcasts) -> vecs float64 [nf,m,2] (y, x) the interpolated flow vector (0 outside every triangle and outside
 *   [0, w - 1] x [0, h - 1]) and inside uint8 [nf,m].
 */
int64_t ofl_mesh_workspace_ints(int32_t nf, int32_t h, int32_t w, int32_t points);
int ofl_mesh_plan(const float* flow, int64_t flow_bs, float flow_sign, const uint8_t* mask, int64_t mask_bs, int32_t points,
                  int32_t* workspace, int32_t nf, int32_t h, int32_t w, void* stream);
int ofl_mesh_apply(const float* flow, int64_t flow_bs, float flow_sign, const uint8_t* mask, int64_t mask_bs, const void* src,
                   int64_t src_bs, int32_t src_u8, int32_t round_mode, int32_t* workspace, int32_t* list, int64_t list_ints, void* dst,
                   uint8_t* inside, int32_t* owner, int32_t nf, int32_t n, int32_t c, int32_t h, int32_t w, void* stream);
int ofl_mesh_points(const float* flow, int64_t flow_bs, float flow_sign, const uint8_t* mask, int64_t mask_bs, const double* pts,
                    int64_t pts_bs, int32_t* workspace, int32_t* list, int64_t list_ints, double* vecs, uint8_t* inside, int32_t nf,
                    int32_t m, int32_t h, int32_t w, void* stream);

/*
 * The dataset loaders: Flow.from_kitti / from_sintel, load_kitti / load_sintel / load_sintel_mask (reference
 * flow_class.py:330-374, utils.py:810-875).
 *
 * HOST side (ofl_png_host.cpp: plain C++, HOST pointers, no HIP call -- the one exception to "every pointer is a device pointer").  The
 * binding parses the PNG chunks and inflates the IDAT stream; these two undo what is sequential per byte lane.  Every length comes from
 * the caller and nothing is read or written beyond it, whatever the bytes say.
 *
 * ofl_png_unfilter: `inflated` = height scanlines of one filter byte (0 None, 1 Sub, 2 Up, 3 Average, 4 Paeth) + row_bytes samples, with
 *   row_bytes = ceil(width * channels * bit_depth / 8) and channels 1 / 3 / 1 / 2 / 4 for colour type 0 / 2 / 3 / 4 / 6; `out` = the
 *   height * row_bytes unfiltered bytes (samples as the file stores them: 16-bit ones big-endian).  Non-interlaced images only.
 *   OFL_E_SHAPE: width or height outside 1 .. 2^24, inflated_len != height * (row_bytes + 1), out_len != height * row_bytes;
 *   OFL_E_ARG: a colour type / bit depth pair PNG does not define, a filter byte above 4 (nothing of `out` is meaningful then).
 * ofl_png_grey8: the 8-bit grey value cv2.imread(path, 0) gives for every pixel of an unfiltered image: grey 8 bits as stored, 1 / 2 / 4
 *   bits scaled by 255 / 85 / 17, 16 bits the high byte; 8-bit R G B (colour type 2, 6: alpha ignored; 3: the palette entry, `palette`
 *   = palette_entries * 3 bytes) as (4899 R + 9617 G + 1868 B + 8192) >> 14.  (cvtColor's weights; not verified against cv2.imread for
 *   colour / palette images)  grey = height * width bytes.  OFL_E_UNSUPPORTED: grey with
 *   alpha, 16-bit colour; OFL_E_ARG: a palette index beyond palette_entries, an undefined pair; OFL_E_SHAPE: lengths as above.
 *
 * DEVICE side (ofl_loaders.hip; device pointers as everywhere else).  One lane decodes 4 consecutive pixels of the dense image; both
 * kernels also form the image's flag word (OFL_FLAG_*; flags int32[n], zeroed in-stream) exactly as ofl_flow_flags_f32 would for the
 * vectors and mask they write, so that nothing has to read them again.  n <= 65535, h * w < 2^31.
 *
 * ofl_decode_kitti: raw = n images of h * w * 3 big-endian 16-bit samples R G B (raw_bs BYTES between images, >= 6 h w), any alignment
 *   (16-byte / 8-byte loads where an image's first byte is 8-byte aligned).  vecs fp32 [n,2,h,w]: u = (R - 32768) / 64,
 *   v = (G - 32768) / 64 (exact in fp32); mask (optional) uint8 [n,h,w] = B > 0.  Without `mask` the flags are those of an all-True mask.
 * ofl_decode_flo: raw = n images of h * w interleaved (u, v) fp32 pairs (raw_bs FLOATS between images, >= 2 h w; 4-byte aligned, else
 *   OFL_E_ARG), copied to the planes of vecs bit for bit; grey (optional) uint8 [n,h,w] (grey_bs bytes between images) and mask uint8
 *   [n,h,w] = grey == 0 -- both or neither, else OFL_E_ARG.
 */
int ofl_png_unfilter(const uint8_t* inflated, int64_t inflated_len, int32_t width, int32_t height, int32_t bit_depth,
                     int32_t colour_type, uint8_t* out, int64_t out_len);
int ofl_png_grey8(const uint8_t* raw, int64_t raw_len, int32_t width, int32_t height, int32_t bit_depth, int32_t colour_type,
                  const uint8_t* palette, int32_t palette_entries, uint8_t* grey, int64_t grey_len);
int ofl_decode_kitti(const uint8_t* raw, int64_t raw_bs, float* vecs, uint8_t* mask, int32_t* flags, int32_t n, int32_t h, int32_t w,
                     void* stream);
int ofl_decode_flo(const float* raw, int64_t raw_bs, const uint8_t* grey, int64_t grey_bs, float* vecs, uint8_t* mask, int32_t* flags,
                   int32_t n, int32_t h, int32_t w, void* stream);

/*
 * Scoring an estimated flow against a ground truth (ofl_metrics.hip): Flow.error_stats / epe_map / epe.  An extension: the
 * reference has no such function.  Per pixel, every step fp32 with one rounding per operation: du = u - ug, dv = v - vg,
 * e = sqrt(du du + dv dv), g = sqrt(ug ug + vg vg), both roots correctly rounded; a pixel counts where both masks are True (a NULL mask
 * is all True).  est / gt [*,2,H,W] fp32 (half = 0) or fp16 (1: up-converted in registers, exact), batch strides in elements; masks
 * [*,H,W] bytes.  n <= 65535, h * w < 2^31.
 *
 * ofl_flow_error_workspace_bytes(n, h, w): bytes of the workspace of ofl_flow_error_f64 (8-byte aligned; every word the second launch
 *   reads is written by the first: nothing to clear), or OFL_E_SHAPE.
 *
 * ofl_flow_error_f64: records float64 [n, OFL_FLOW_ERROR_RECORD], per image over its valid pixels
 *     [0] count   [1] sum e   [2] max e (0 without a valid pixel)   [3 .. 6] pixels with e > t_k, k < n_thresholds (strict; 0 <=
 *     n_thresholds <= 4, t_k finite and >= 0, else OFL_E_ARG)   [7] pixels with e > 3 and e > 0.05f * g (KITTI's Fl outliers, the product
 *     in fp32)   [8 .. 10] pixels with g in [0, 10), [10, 40), [40, inf)   [11 .. 13] sum e of those   [14], [15] 0.
 *   Counts are exact (integers up to the record).  Sums are float64 sums of the fp32 e in a fixed order -- a lane's pixels ascending,
 *   the lanes of a wave by a butterfly, the waves and then the blocks of an image in index order -- and the number of blocks depends on
 *   h * w only: no float atomics, an image's record has the same bits in any batch and on any run.  epe_map (optional) fp32 [n,h,w]: e,
 *   0 where not valid.  Two launches: ofl_last_kernel_name() then names flow_error_finish_kernel.
 *
 * ofl_flow_epe_grad_f32: the backward of the per-image mean of e.  scale fp32 [n] DEVICE memory (the upstream gradient / count);
 *   grad_est and / or grad_gt fp32 [n,2,h,w] (one may be NULL, not both): grad_est = the float64 quotient (scale du) / sqrt(du du + dv dv)
 *   of the fp32 differences, rounded once to fp32, where the pixel is valid and the fp32 e is > 0; 0 elsewhere (the subgradient torch's
 *   norm takes at 0); grad_gt = -grad_est.  A scale that is not finite (count 0) meets no valid pixel: that image's gradient is 0.
 */
#define OFL_FLOW_ERROR_RECORD 16
int64_t ofl_flow_error_workspace_bytes(int32_t n, int32_t h, int32_t w);
int ofl_flow_error_f64(const void* est, int64_t est_bs, int32_t est_half, const void* gt, int64_t gt_bs, int32_t gt_half,
                       const uint8_t* est_mask, int64_t est_mask_bs, const uint8_t* gt_mask, int64_t gt_mask_bs, int32_t n_thresholds,
                       float t0, float t1, float t2, float t3, void* workspace, float* epe_map, double* records,
                       int32_t n, int32_t h, int32_t w, void* stream);
int ofl_flow_epe_grad_f32(const void* est, int64_t est_bs, int32_t est_half, const void* gt, int64_t gt_bs, int32_t gt_half,
                          const uint8_t* est_mask, int64_t est_mask_bs, const uint8_t* gt_mask, int64_t gt_mask_bs, const float* scale,
                          float* grad_est, float* grad_gt, int32_t n, int32_t h, int32_t w, void* stream);

/*
 * The forward-backward consistency check of two flows (ofl_consistency.hip): Flow.consistency / consistency_mask /
 * filter_consistent.  An extension: the reference has no such function.  `a` is a flow from frame 1 to frame 2, `back` a flow from frame 2
 * to frame 1, both of one reference: flow_sign -1 for 's' flows (the partner of pixel p is `back` at p + a(p)), +1 for 't' flows (at
 * x - a(x)).  Per pixel, every step fp32 with one rounding per operation (the fused multiply-adds are those of the backward warp):
 *   (bu, bv), mr   the two planes of `back` and the validity of its taps sampled bilinearly at unnormalise(grid - flow_sign a), in the
 *                  expressions of ofl_warp_bwd_f32: a tap outside the frame contributes 0, a tap where back_mask is 0 contributes 0 to mr
 *   known          (mr > 0.99999f) and a_mask (a NULL mask is all True); a non-finite vector of `a` fails the comparisons: not known
 *   e              sqrt(du du + dv dv) with du = u + bu, dv = v + bv, the root correctly rounded
 *   consistent     known and du du + dv dv <= alpha ((u u + v v) + (bu bu + bv bv)) + beta        (inclusive)
 * du, dv and known carry the bits of the vectors and the mask that mode 3 of combine_with gives (ofl_warp_bwd_f32 with the addend).
 *
 * ofl_flow_consistency_workspace_bytes(n, h, w): bytes of the workspace of ofl_flow_consistency_f32, or OFL_E_ARG for sizes that call
 *   rejects.
 *
 * ofl_flow_consistency_f32:
 *   a, back            [*,2,H,W] fp32 (half = 0) or fp16 (1: up-converted in registers, exact), a_bs / back_bs elements between images
 *                      (0 broadcasts one image); aligned to their element.  Never written.
 *   a_mask, back_mask  optional [*,H,W] bytes (any non-zero byte is True), batch strides in bytes.  Never written.
 *   flow_sign          +-1 (above); alpha, beta: finite and >= 0
 *   workspace          device memory of ofl_flow_consistency_workspace_bytes(n, h, w) bytes, 8-byte aligned; needed (and touched) only
 *                      when `record` is given.  Its contents are irrelevant on entry: every word the second launch reads is written by
 *                      the first.
 *   error              optional fp32 [n,h,w]: e, 0 where the pixel is not known
 *   consistent, known  optional uint8 [n,h,w]: bytes 0 / 1
 *   record             optional float64 [n, OFL_CONSISTENCY_RECORD], 8-byte aligned, per image: [0] known pixels  [1] consistent pixels
 *                      [2] sum e over the known pixels  [3] max e over the known pixels (0 without one)  [4] sum e over the consistent
 *                      pixels  [5 .. 7] 0.  Counts are exact; sums are float64 sums of the fp32 e in the fixed order of
 *                      ofl_flow_error_f64 (lane, butterfly, waves, blocks ascending; the number of blocks depends on h * w only): no
 *                      float atomics, an image's record has the same bits in any batch and on any run.
 *   Every element of every output given is WRITTEN (not accumulated into; nothing to clear beforehand); an output that is NULL is not
 *   written; at least one must be given.  OFL_E_ARG, before any launch, for: n outside 1 .. 65535, h or w < 2, h * w >= 2^31, a flow_sign
 *   other than +-1, alpha or beta negative or not finite, a NULL flow pointer, all four outputs NULL, a record without a workspace, a
 *   negative stride, a misaligned pointer.  One launch, two with a record: ofl_last_kernel_name() then names
 *   flow_consistency_finish_kernel.
 */
#define OFL_CONSISTENCY_RECORD 8
int64_t ofl_flow_consistency_workspace_bytes(int32_t n, int32_t h, int32_t w);
int ofl_flow_consistency_f32(const void* a, int64_t a_bs, int32_t a_half, const void* back, int64_t back_bs, int32_t back_half,
                             const uint8_t* a_mask, int64_t a_mask_bs, const uint8_t* back_mask, int64_t back_mask_bs, float flow_sign,
                             float alpha, float beta, void* workspace, float* error, uint8_t* consistent, uint8_t* known, double* record,
                             int32_t n, int32_t h, int32_t w, void* stream);

/*
 * The edge-aware smoothness penalty of a flow (which defines the numbers; ofl_smoothness.hip): Flow.smoothness /
 * smoothness_map / smoothness_stats.  An extension: the reference has no such function.  Per pixel p = (i, j), every step fp32 with one
 * rounding per operation; direction x is written out, direction y is the same along rows.
 *   order 1   the term exists iff j + 1 < w:  d = f(i,j+1) - f(i,j) per component,  g = (sum_c |I_c(i,j+1) - I_c(i,j)|) / float(C)
 *   order 2   the term exists iff 1 <= j and j + 1 < w:  d = (f(i,j-1) - (f(i,j) + f(i,j))) + f(i,j+1),
 *             g = ((sum_c |I_c(i,j+1) - I_c(i,j-1)|) / float(C)) * 0.5f          (channels added in ascending order)
 *   r = sqrt(du du + eps eps) + sqrt(dv dv + eps eps), both roots correctly rounded;  w = 1.0f without an image, else
 *   w = float(exp(double(-(alpha g)))): the float64 exp of the fp32 argument, rounded once;  t_x(p) = w r.
 * A term is valid iff it exists and every pixel it reads (2 / 3) is True in the mask (a NULL mask is all True); an invalid term is +0.0f.
 * flow [*,2,H,W] fp32 (half = 0) or fp16 (1: up-converted in registers, exact), flow_bs elements between images (0 broadcasts one
 * image); mask optional [*,H,W] bytes (any non-zero byte is True), mask_bs bytes between images; img optional [*,C,H,W], 1 <= C <= 4,
 * fp32 (img_u8 = 0) or uint8 (1: a sample s is float(s) / 255.0f), img_bs elements between images (0 broadcasts one image).  Without
 * an image, img_bs, img_channels and img_u8 are ignored and no image pointer is touched.  Inputs are never written.
 *
 * ofl_flow_smoothness_workspace_bytes(n, h, w): bytes of the workspace of ofl_flow_smoothness_f64 (8-byte aligned; every word the second
 *   launch reads is written by the first: nothing to clear), or OFL_E_ARG for sizes that call rejects.
 *
 * ofl_flow_smoothness_f64: records float64 [n, OFL_SMOOTHNESS_RECORD], per image over its valid terms
 *     [0] count_x   [1] count_y   [2] sum t_x   [3] sum t_y   [4] max over all valid terms (0 without one)   [5 .. 7] 0.
 *   Counts are exact (integers up to the record).  Sums are float64 sums of the fp32 terms in a fixed order -- a lane's pixels
 *   ascending, the lanes of a wave by a butterfly, the waves and then the blocks of an image in index order -- and the number of blocks
 *   depends on (h, w) only: no float atomics, an image's record has the same bits in any batch and on any run.  smoothness_map
 *   (optional) fp32 [n,h,w]: t_x(p) + t_y(p), one fp32 addition; the term is attributed to the left / upper pixel (order 1) or to the
 *   centre pixel (order 2).  Every element of every output is WRITTEN.  Two launches: ofl_last_kernel_name() then names
 *   flow_smoothness_finish_kernel.
 *
 * ofl_flow_smoothness_grad_f32: the backward of the per-image mean (sum_x + sum_y) / (count_x + count_y) with respect to the flow.  scale
 *   fp32 [n] DEVICE memory (the upstream gradient / total count); grad fp32 [n,2,h,w], every element written.  For a valid term T and
 *   each component, in float64: q_T = (double(w) double(d)) / sqrt(double(d) double(d) + double(eps) double(eps)), 0 where the root is
 *   0.  grad(s) = float(double(scale) * sum_k coef_k q_Tk) over the valid terms that read s -- order 1: +1 from the term at s - 1, -1 from
 *   the term at s; order 2: +1, -2, +1 from the terms at s - 1, s, s + 1 -- added x before y and lower term index first in float64,
 *   rounded once; exactly 0 where no valid term reads s (so an image without a valid term, whose scale is not finite, has gradient 0).
 *   The kernel gathers: every output pixel recomputes its 4 / 6 terms from the inputs; no scatter, no atomics.  The image carries no
 *   gradient.
 *
 * OFL_E_ARG, before any launch, for: n outside 1 .. 65535, h or w < 1, h * w >= 2^31, an order other than 1 or 2, C outside 1 .. 4 (with
 * an image), alpha or eps negative or not finite, a NULL flow, workspace, records, scale or grad pointer, a negative stride, a flag that
 * is neither 0 nor 1, a pointer not aligned to its element (workspace, records: 8 bytes).
 */
#define OFL_SMOOTHNESS_RECORD 8
int64_t ofl_flow_smoothness_workspace_bytes(int32_t n, int32_t h, int32_t w);
int ofl_flow_smoothness_f64(const void* flow, int64_t flow_bs, int32_t flow_half, const uint8_t* mask, int64_t mask_bs, const void* img,
                            int64_t img_bs, int32_t img_channels, int32_t img_u8, int32_t order, float alpha, float eps, void* workspace,
                            float* smoothness_map, double* records, int32_t n, int32_t h, int32_t w, void* stream);
int ofl_flow_smoothness_grad_f32(const void* flow, int64_t flow_bs, int32_t flow_half, const uint8_t* mask, int64_t mask_bs,
                                 const void* img, int64_t img_bs, int32_t img_channels, int32_t img_u8, int32_t order, float alpha,
                                 float eps, const float* scale, float* grad, int32_t n, int32_t h, int32_t w, void* stream);

/*
 * The photometric term of an unsupervised flow loss, warp and comparison in one pass (which defines the numbers;
 * ofl_photometric.hip): Flow.photometric / photometric_map / photometric_stats.  An extension: the reference has no such function.
 * `img` is the frame on the flow's own grid, `other` the frame the flow points into; flow_sign -1 for 's' flows (the sample of pixel p
 * lies at p + a(p)), +1 for 't' flows (at p - a(p)).  Per pixel p, every step fp32 with one rounding per operation (the fused
 * multiply-adds are those of the backward warp):
 *   Iw_c, mr   plane c of `other` and the insideness of its taps sampled bilinearly at unnormalise(grid - flow_sign a), in the
 *              expressions of ofl_warp_bwd_f32: a tap outside the frame reads as 0
 *   known      (mr > 0.99999f) and mask (a NULL mask is all True); a non-finite vector fails the comparisons: not known
 *   d_c        Iw_c - I_c(p);  r_c = sqrt(d_c d_c + eps eps), the root correctly rounded
 *   rho        (((r_0 + r_1) + ...)) / float(C): channels added in ascending order, one division; +0.0f where the pixel is not known
 * flow [*,2,H,W] fp32 (half = 0) or fp16 (1: up-converted in registers, exact), flow_bs elements between images (0 broadcasts one
 * image); mask optional [*,H,W] bytes (any non-zero byte is True), mask_bs bytes between images; img, other [*,C,H,W], 1 <= C <= 4, both
 * fp32 (img_u8 = 0) or both uint8 (1: a sample s is float(s) / 255.0f), img_bs / other_bs elements between images (0 broadcasts one
 * image).  Inputs are never written.  The warped image is never written.
 *
 * ofl_flow_photometric_workspace_bytes(n, h, w): bytes of the workspace of ofl_flow_photometric_f64 (8-byte aligned; every word the
 *   second launch reads is written by the first: nothing to clear), or OFL_E_ARG for sizes that call rejects.
 *
 * ofl_flow_photometric_f64: records (optional) float64 [n, OFL_PHOTOMETRIC_RECORD], per image over its known pixels
 *     [0] count   [1] sum rho   [2] max rho (0 without a known pixel)   [3 .. 7] 0.
 *   The count is exact.  The sum is the float64 sum of the fp32 rho in a fixed order -- a lane's pixels ascending, the lanes of a wave
 *   by a butterfly, the waves and then the blocks of an image in index order -- and the number of blocks depends on (h, w) only: no
 *   float atomics, an image's record has the same bits in any batch and on any run.  photometric_map (optional) fp32 [n,h,w]: rho.  At
 *   least one of the two must be given; the workspace is needed (and touched) only with records.  Every element of every output given
 *   is WRITTEN.  One launch, two with records: ofl_last_kernel_name() then names flow_photometric_finish_kernel.
 *
 * ofl_flow_photometric_grad_f32: the backward of the per-image mean sum / count with respect to the flow vectors.  scale fp32 [n] DEVICE
 *   memory (the upstream gradient / count); grad fp32 [n,2,h,w], every element written.  A known pixel recomputes the fp32 d_c of the
 *   forward; then, in float64: q_c = double(d_c) / sqrt(double(d_c)^2 + double(eps)^2), 0 where the root is 0;
 *   gx_c = sum_j sgn_j fr_j double(v_j,c) over the taps nw, ne, sw, se inside the frame, sgn -1 for west and +1 for east taps, fr the other
 *   axis's weight, from the fractions double(sx) - double(floorf(sx)) and their complements to 1; gy_c likewise (north -1, south +1).
 *   grad_u(p) = float(double(scale) * (-flow_sign) * (((q_0 gx_0 + q_1 gx_1) + ...) / double(C))), grad_v with gy; exactly 0 where the
 *   pixel is not known (so an image without a known pixel, whose scale is not finite, has gradient 0).  The kernel gathers: no scatter,
 *   no atomics.  The images carry no gradient.
 *
 * OFL_E_ARG, before any launch, for: n outside 1 .. 65535, h or w < 2, h * w >= 2^31, a flow_sign other than +-1, C outside 1 .. 4, eps
 * negative or not finite, a NULL flow, img, other, scale or grad pointer, map and records both NULL, records without a workspace, a
 * negative stride, a flag that is neither 0 nor 1, a pointer not aligned to its element (workspace, records: 8 bytes).
 */
#define OFL_PHOTOMETRIC_RECORD 8
int64_t ofl_flow_photometric_workspace_bytes(int32_t n, int32_t h, int32_t w);
int ofl_flow_photometric_f64(const void* flow, int64_t flow_bs, int32_t flow_half, const uint8_t* mask, int64_t mask_bs, const void* img,
                             int64_t img_bs, const void* other, int64_t other_bs, int32_t channels, int32_t img_u8, float flow_sign,
                             float eps, void* workspace, float* photometric_map, double* records, int32_t n, int32_t h, int32_t w,
                             void* stream);
int ofl_flow_photometric_grad_f32(const void* flow, int64_t flow_bs, int32_t flow_half, const uint8_t* mask, int64_t mask_bs,
                                  const void* img, int64_t img_bs, const void* other, int64_t other_bs, int32_t channels, int32_t img_u8,
                                  float flow_sign, float eps, const float* scale, float* grad, int32_t n, int32_t h, int32_t w,
                                  void* stream);

/*
 * The census data term of an unsupervised flow loss, warp and comparison of soft ternary census signatures in one pass (DESIGN.md
 * 3.21, which defines the numbers; ofl_census.hip): Flow.census / census_map / census_stats.  An extension: the reference has no such
 * function.  `img`, `other` and flow_sign as for ofl_flow_photometric_f64.  patch is 3, 5 or 7, R = patch / 2.  Every step fp32 with one
 * rounding per operation unless it says float64:
 *   Iw_c, mr   as in ofl_flow_photometric_f64, except that a uint8 sample s is read as float(s), on the scale 0 .. 255
 *   grey       g = v_0 for C = 1, (0.299f v_0 + 0.587f v_1) + 0.114f v_2 for C = 3;  G = 255.0f g for fp32 images, G = g for uint8.
 *              Gw(p) is the grey of Iw (the channels are warped, then combined), Gi(p) the grey of img
 *   usable(p)  p in the frame, mask(p) (a NULL mask is all True), mr(p) > 0.99999f
 *   U(p), n    the offsets o != 0 of the patch around p with usable(p + o), and their number;  known(p) = usable(p) and n >= 1.  There
 *              is no border rule: a neighbour that is not usable is no term
 *   per term   o in U(p), dy ascending and dx ascending within it:  dW = Gw(p+o) - Gw(p), tw = dW / sqrtf(0.81f + dW dW), ti likewise
 *              from Gi, e = ti - tw, s = e e, f = s / (thresh + s)
 *   per pixel  hd = (sum of f in that order) / float(n), b = hd + eps, rho = float(pow(double(b), double(q))): the float64 pow rounded
 *              once; +0.0f where the pixel is not known
 * flow, mask, img, other, their strides and flags as for ofl_flow_photometric_f64, with C = 1 or 3.  Inputs are never written; neither
 * the warped image nor any tensor of patch^2 - 1 channels is.
 *
 * ofl_flow_census_workspace_bytes(n, h, w, patch): bytes of the workspace of ofl_flow_census_f64 (8-byte aligned; every word the
 *   second launch reads is written by the first: nothing to clear), or OFL_E_ARG for sizes that call rejects.
 *
 * ofl_flow_census_f64: records (optional) float64 [n, OFL_CENSUS_RECORD], per image over its known pixels
 *     [0] count   [1] sum rho   [2] max rho (0 without a known pixel)   [3] sum n(p)   [4 .. 7] 0.
 *   [0] and [3] are exact.  The sum is the float64 sum of the fp32 rho in a fixed order -- a lane's pixels ascending, the lanes of a
 *   wave by a butterfly, the waves and then the blocks of an image in index order -- and the number of blocks depends on (h, w) only:
 *   no float atomics, an image's record has the same bits in any batch and on any run.  census_map (optional) fp32 [n,h,w]: rho.  At
 *   least one of the two must be given; the workspace is needed (and touched) only with records.  Every element of every output given
 *   is WRITTEN.  One launch, two with records: ofl_last_kernel_name() then names flow_census_finish_kernel.
 *
 * ofl_flow_census_grad_f32: the backward of the per-image mean sum / count with respect to the flow vectors.  scale fp32 [n] DEVICE
 *   memory (the upstream gradient / count); grad fp32 [n,2,h,w], every element written.  In float64 on the fp32 Gw, Gi and b of the
 *   forward: kappa(p) = q b(p)^(q-1) / n(p) where p is known, k_o(p) = thresh / (thresh + s)^2 (-2 e) 0.81 / (0.81 + dW^2)^(3/2),
 *     dL/dGw(x) = scale ( sum over known p with x - p in U(p) of kappa(p) k_{x-p}(p)  -  [x known] kappa(x) sum over o in U(x) of k_o(x) ),
 *   grad_u(x) = float(dL/dGw(x) (-flow_sign) S sum_c g_c gx_c(x)) with S = 255 for fp32 images and 1 for uint8, g_c the grey weight
 *   (1 for C = 1) and gx_c, gy_c as in ofl_flow_photometric_grad_f32; exactly 0 where the pixel is not known.  One launch that
 *   recomputes kappa over a halo: no workspace, no scatter, no atomics.  The images carry no gradient.
 *
 * OFL_E_ARG, before any launch, for: n outside 1 .. 65535, h or w < 2, h * w >= 2^31, a flow_sign other than +-1, C other than 1 or 3,
 * a patch other than 3, 5 or 7, thresh or eps not positive or not finite, q outside (0, 1], a NULL flow, img, other, scale or grad
 * pointer, map and records both NULL, records without a workspace, a negative stride, a flag that is neither 0 nor 1, a pointer not
 * aligned to its element (workspace, records: 8 bytes).
 */
#define OFL_CENSUS_RECORD 8
int64_t ofl_flow_census_workspace_bytes(int32_t n, int32_t h, int32_t w, int32_t patch);
int ofl_flow_census_f64(const void* flow, int64_t flow_bs, int32_t flow_half, const uint8_t* mask, int64_t mask_bs, const void* img,
                        int64_t img_bs, const void* other, int64_t other_bs, int32_t channels, int32_t img_u8, float flow_sign,
                        int32_t patch, float thresh, float eps, float q, void* workspace, float* census_map, double* records, int32_t n,
                        int32_t h, int32_t w, void* stream);
int ofl_flow_census_grad_f32(const void* flow, int64_t flow_bs, int32_t flow_half, const uint8_t* mask, int64_t mask_bs, const void* img,
                             int64_t img_bs, const void* other, int64_t other_bs, int32_t channels, int32_t img_u8, float flow_sign,
                             int32_t patch, float thresh, float eps, float q, const float* scale, float* grad, int32_t n, int32_t h,
                             int32_t w, void* stream);

/*
 * The structural-similarity data term of an unsupervised flow loss, warp and windowed comparison in one pass (which
 * defines the numbers; ofl_ssim.hip): Flow.ssim / ssim_map / ssim_stats.  An extension: the reference has no such function.  `img`,
 * `other`, flow_sign and the reading of a uint8 sample (float(s) / 255.0f) as for ofl_flow_photometric_f64, C = 1 or 3.  window is 3, 5
 * or 7, R = window / 2.  Every step fp32 with one rounding per operation unless it says float64:
 *   X_c = Iw_c, mr  as in ofl_flow_photometric_f64;  Y_c = img_c
 *   usable(p)   p in the frame, valid in the mask, mr(p) > 0.99999f; a pixel that is not usable loads no image sample
 *   W(p)        the usable pixels p + o with |dy|, |dx| <= R, the centre included; n(p) their number; known(p) = usable(p)
 *   per channel, two walks of W(p), dy ascending, dx ascending within it:
 *     mux = (sum X) / float(n), muy likewise;  sxx = (sum (X - mux) (X - mux)) / float(n), syy and sxy likewise (each product rounded,
 *     then added)
 *     l1 = (2 mux) muy + c1   l2 = (mux mux + muy muy) + c1   s1 = 2 sxy + c2   s2 = (sxx + syy) + c2
 *     d_c = (1 - (l1 s1) / (l2 s2)) 0.5, then d_c < 0 ? 0 : (d_c > 1 ? 1 : d_c)  (a NaN passes)
 *   rho(p) = ((d_0 + d_1) + d_2) / float(C)
 * Inputs are never written; neither the warped image nor a pooled tensor is.
 *
 * ofl_flow_ssim_workspace_bytes(n, h, w, window): bytes of the workspace of ofl_flow_ssim_f64 (8-byte aligned; every word the second
 *   launch reads is written by the first: nothing to clear), or OFL_E_ARG for sizes that call rejects.
 *
 * ofl_flow_ssim_f64: records (optional) float64 [n, OFL_SSIM_RECORD], per image over its known pixels
 *     [0] count   [1] sum rho   [2] max rho (0 without a known pixel; a NaN is never the max)   [3] sum n(p)   [4 .. 7] 0.
 *   [0] and [3] are exact.  The sum is the float64 sum of the fp32 rho in a fixed order -- a lane's pixels ascending, the lanes of a
 *   wave by a butterfly, the waves and then the blocks of an image in index order -- and the number of blocks depends on (h, w) only:
 *   no float atomics, an image's record has the same bits in any batch and on any run.  ssim_map (optional) fp32 [n,h,w]: rho, +0 where
 *   the pixel is not known.  At least one of the two must be given; the workspace is needed (and touched) only with records.  Every
 *   element of every output given is WRITTEN.  One launch, two with records: ofl_last_kernel_name() then names flow_ssim_finish_kernel.
 *
 * ofl_flow_ssim_grad_f32: the backward of the per-image mean sum / count with respect to the flow vectors; the clamp is taken as the
 *   identity.  scale fp32 [n] DEVICE memory (the upstream gradient / count); grad fp32 [n,2,h,w], every element written.  In float64 on
 *   the fp32 X, Y of the forward, mu, sigma, A = l1, D = l2, B = s1, E = s2 re-formed in float64 by the same two walks; per known centre
 *   p and channel
 *     a0 = (2/n) (B muy / (D E) - A B mux / (D^2 E) - A muy / (D E) + A B mux / (D E^2))   a1 = (2/n) A / (D E)   a2 = -(2/n) A B / (D E^2)
 *     dL/dX_c(x) = -scale / (2 C) (S0(x) + S1(x) Y_c(x) + S2(x) X_c(x)),  S_k(x) the sum of a_k(p) over the known p within R of x
 *   grad_u(x) = float(sum_c dL/dX_c(x) (-flow_sign) gx_c(x)) with gx_c, gy_c as in ofl_flow_photometric_grad_f32; exactly 0 where the
 *   pixel is not known.  One launch that runs the channels one after the other through the same LDS: no workspace, no scatter, no
 *   atomics.  The images carry no gradient.
 *
 * OFL_E_ARG, before any launch, for: n outside 1 .. 65535, h or w < 2, h * w >= 2^31, a flow_sign other than +-1, C other than 1 or 3,
 * a window other than 3, 5 or 7, c1 or c2 not positive or not finite, a NULL flow, img, other, scale or grad pointer, map and records
 * both NULL, records without a workspace, a negative stride, a flag that is neither 0 nor 1, a pointer not aligned to its element
 * (workspace, records: 8 bytes).
 */
#define OFL_SSIM_RECORD 8
int64_t ofl_flow_ssim_workspace_bytes(int32_t n, int32_t h, int32_t w, int32_t window);
int ofl_flow_ssim_f64(const void* flow, int64_t flow_bs, int32_t flow_half, const uint8_t* mask, int64_t mask_bs, const void* img,
                      int64_t img_bs, const void* other, int64_t other_bs, int32_t channels, int32_t img_u8, float flow_sign,
                      int32_t window, float c1, float c2, void* workspace, float* ssim_map, double* records, int32_t n, int32_t h,
                      int32_t w, void* stream);
int ofl_flow_ssim_grad_f32(const void* flow, int64_t flow_bs, int32_t flow_half, const uint8_t* mask, int64_t mask_bs, const void* img,
                           int64_t img_bs, const void* other, int64_t other_bs, int32_t channels, int32_t img_u8, float flow_sign,
                           int32_t window, float c1, float c2, const float* scale, float* grad, int32_t n, int32_t h, int32_t w,
                           void* stream);

/*
 * The local cost volume of a flow network (PWC-Net, LiteFlowNet, ARFlow, UFlow), warp and correlation in one pass (which
 * defines the numbers; ofl_cost_volume.hip): Flow.cost_volume.  An extension: the reference has no such function.  `feat`: the features
 * on the flow's own grid, `other`: those of the frame the flow points into, fp32 [*,C,h,w] with a batch stride in elements (0: one
 * image for the whole batch), C >= 1; flow, flow_half, mask, flow_sign as for ofl_flow_photometric_f64.  radius R is 1 .. 4,
 * D = (2 R + 1)^2.  Every step fp32 with one rounding per operation:
 *   W_c(q), mr(q)  the sample of other_c where the flow points from q and the weight sum of its taps inside the frame, as in
 *               ofl_flow_photometric_f64
 *   usable(q)   q in the frame, valid in the mask, mr(q) > 0.99999f
 *   W'_c(q)     usable(q) ? W_c(q) : +0  (selected: a pixel that is not usable loads no sample)
 *   V[o](p)     = (sum over c ascending, from +0, of feat_c(p) * W'_c(p + o)) / float(C),  o = (dy + R) (2 R + 1) + dx + R, each product
 *               rounded, then each sum: no fused multiply-add.  All C products are formed, against +0 too.
 * Inputs are never written; the warped tensor is not written either.  No workspace.
 *
 * ofl_flow_cost_volume_f32: volume fp32 [n,D,h,w], every element WRITTEN.  One launch.
 *
 * ofl_flow_cost_volume_grad_f32: with the upstream gradient grad_volume fp32 [n,D,h,w] and gs = grad_volume / float(C),
 *     grad_feat_c(p)   = sum over o ascending, from +0, of gs[o](p) * W'_c(p + o)                                      [n,C,h,w]
 *     grad_warped_c(q) = usable(q) ? sum over o ascending, from +0, of gs[o](q - o) * feat_c(q - o), q - o in the frame : +0   [n,C,h,w]
 *   both gathers: no scatter, no atomics, the same bits on any run.  Either output may be NULL, not both; every element of an output
 *   given is written (a batch-broadcast feat still gets n gradient images: the caller adds them).  One launch per output.
 *   grad_warped is the upstream gradient of the warp: ofl_warp_bwd_grad_f32 turns it into the gradients of `other` and of the flow.
 *
 * OFL_E_ARG, before any launch, for: n outside 1 .. 65535, h or w < 2, h * w >= 2^31, a flow_sign other than +-1, C < 1, a radius
 * outside 1 .. 4, a NULL flow, feat, other, volume or grad_volume pointer, grad_feat and grad_warped both NULL, a negative stride, a
 * flow_half that is neither 0 nor 1, a pointer not aligned to its element.
 */
int ofl_flow_cost_volume_f32(const void* flow, int64_t flow_bs, int32_t flow_half, const uint8_t* mask, int64_t mask_bs, const float* feat,
                             int64_t feat_bs, const float* other, int64_t other_bs, int32_t channels, float flow_sign, int32_t radius,
                             float* volume, int32_t n, int32_t h, int32_t w, void* stream);
int ofl_flow_cost_volume_grad_f32(const void* flow, int64_t flow_bs, int32_t flow_half, const uint8_t* mask, int64_t mask_bs,
                                  const float* feat, int64_t feat_bs, const float* other, int64_t other_bs, int32_t channels,
                                  float flow_sign, int32_t radius, const float* grad_volume, float* grad_feat, float* grad_warped,
                                  int32_t n, int32_t h, int32_t w, void* stream);
/*
 * The two per-pixel launches around ofl_warp_bwd_grad_f32 in the backward of the cost volume.  The rule: the gradient of the flow is +0
 * wherever the pixel is not usable, and a value of `other` that no usable pixel samples reaches no gradient -- selected, not
 * multiplied, as in the forward.
 *
 * ofl_flow_cost_volume_chain_f32: chain fp32 [n,2,h,w], every element WRITTEN: the flow's vectors as fp32, and (flow_sign * 2^31, 0)
 *   where a component is not finite (that pixel is not usable and its grad_warped is +0; the vector puts its sample left of every
 *   frame, so that no tap of it is read or written).  The backward of the warp is run on `chain`, not on the flow.
 * ofl_flow_cost_volume_gate_f32: grad_flow fp32 [n,2,h,w], IN PLACE: +0 where usable(q) is false, untouched elsewhere.
 *
 * OFL_E_ARG, before any launch, for the frame, flow, flow_half, stride and flow_sign conditions above and a NULL or misaligned chain or
 * grad_flow.
 */
int ofl_flow_cost_volume_chain_f32(const void* flow, int64_t flow_bs, int32_t flow_half, float flow_sign, float* chain, int32_t n,
                                   int32_t h, int32_t w, void* stream);
int ofl_flow_cost_volume_gate_f32(const void* flow, int64_t flow_bs, int32_t flow_half, const uint8_t* mask, int64_t mask_bs,
                                  float flow_sign, float* grad_flow, int32_t n, int32_t h, int32_t w, void* stream);

/*
 * The correlation lookup of RAFT-style networks (RAFT, GMA, SEA-RAFT, CRAFT), computed on the fly at the looked-up positions without
 * the all-pairs volume (which defines the numbers; ofl_corr_lookup.hip): Flow.corr_lookup.  An extension: the reference
 * has no such function.  One call serves ONE pyramid level l = `level`, 0 .. 5: `other` is that level, fp32 [*,C,level_h,level_w] with a
 * batch stride in elements (0: one image for the whole batch), level_h and level_w 1 .. 2^24 with level_h * level_w < 2^31; `feat`: the
 * features on the flow's own grid, fp32 [*,C,h,w]; flow, flow_half, mask, flow_sign as for ofl_flow_photometric_f64, but h and w may
 * be 1.  radius R is 1 .. 4, D = (2 R + 1)^2.  Every step fp32 with one rounding per operation:
 *   usable(p)   valid in the mask and both vector components finite
 *   position    px = float(x) - flow_sign * u, sx = px * 2^-l, x_w = floorf(sx), ww = sx - x_w, e = 1 - ww; py, sy, y_n, nn, s alike;
 *               nw = s * e, ne = s * ww, sw = nn * e, se = nn * ww
 *   node (j,i)  j, i = 0 .. 2 R + 1: column cx = x_w + float(i - R), row cy = y_n + float(j - R) of the level; inside where
 *               cx > -1 && cx < level_w && cy > -1 && cy < level_h (float compares)
 *   K[j,i]      = sum over c ascending, from +0, of feat_c(p) * other[c, cy, cx], each product rounded, then each sum; +0 (selected)
 *               for a node outside
 *   entry (dx + R) (2 R + 1) + dy + R, dx, dy = -R .. R  (the x offset is the outer index: RAFT's order)
 *               = (K[dy+R, dx+R] * nw, then fmaf of K[dy+R, dx+R+1] with ne, K[dy+R+1, dx+R] with sw, K[dy+R+1, dx+R+1] with se)
 *                 / sqrtf(float(C)); +0 (selected) for all D entries where usable(p) is false.
 * Inputs are never written.
 *
 * ofl_flow_corr_lookup_f32: the D planes of the level into `out`, fp32 [n][D][h w] with `out_bs` >= D h w elements between images (the
 *   level's channel slice of a result [n, L D, h, w]); every element of the D planes WRITTEN.  One launch.
 *
 * The backward of a level, with the level's slice `grad_out` of the upstream gradient (laid out as `out`, stride grad_bs) and
 * gs = grad_out / sqrtf(float(C)):
 * ofl_flow_corr_lookup_nodes_f32: nodes fp32 [n][(2 R + 2)^2][h w], every element WRITTEN:
 *     Gn[j,i](p) = from +0, the terms that exist in this order, each product rounded, then added: gs[(i-R, j-R)] * nw  (j, i <= 2 R),
 *                  gs[(i-1-R, j-R)] * ne  (j <= 2 R, i >= 1),  gs[(i-R, j-1-R)] * sw  (j >= 1, i <= 2 R),  gs[(i-1-R, j-1-R)] * se
 *                  (j, i >= 1); +0 where usable(p) is false.
 *   keys (NULL: not made) int64 [n][h w], every element WRITTEN: (image * cells + cell(p)) * h w + p, where cells =
 *   ofl_flow_corr_lookup_cells(level_h, level_w, R) = (level_h + 2 R + 1) (level_w + 2 R + 1) + 1 and cell(p) =
 *   (y_n - R + 2 R + 1) (level_w + 2 R + 1) + (x_w - R + 2 R + 1), the window's first node on the level's grid padded to the north and
 *   west; the sentinel cells - 1 where usable(p) is false or no node of the window is inside.  The keys are unique.
 * ofl_flow_corr_lookup_grad_feat_f32: grad_feat fp32 [n,C,h,w], every element WRITTEN:
 *     grad_feat_c(p) = (accumulate ? the stored value : +0) + sum over j, then i ascending of Gn[j,i](p) * other[c, node], nodes outside
 *     skipped; +0 where usable(p) is false.  Levels run as ascending calls, accumulate 0 for the first: one running sum.
 * ofl_flow_corr_lookup_grad_other_f32: grad_other fp32 [n,C,level_h,level_w], every element WRITTEN, a gather without atomics:
 *     grad_other[c,q] = from +0, over j, then i, then the pixels p of cell q - (j, i) in ascending order: + Gn[j,i](p) * feat_c(p)
 *   `order` int64 [n h w]: the pixel index image * h w + p of every key in ascending key order; `starts` int64 [n cells + 1]: the
 *   number of keys below k h w, k = 0 .. n cells.  Entries of `order` outside the image and runs outside [0, n h w] are skipped.
 *
 * OFL_E_ARG, before any launch, for: n outside 1 .. 65535, h or w < 1, h * w >= 2^31, C < 1 (the gather: C > 524280), a radius outside
 * 1 .. 4, a level outside 0 .. 5, a level_h or level_w outside 1 .. 2^24 or level_h * level_w >= 2^31, n * cells * h * w >= 4e18, a
 * flow_sign other than +-1, a NULL required pointer, a negative stride, out_bs or grad_bs < D h w, a flow_half or accumulate that is
 * neither 0 nor 1, a pointer not aligned to its element.  ofl_flow_corr_lookup_cells returns OFL_E_ARG for a level or radius so refused.
 */
int64_t ofl_flow_corr_lookup_cells(int32_t level_h, int32_t level_w, int32_t radius);
int ofl_flow_corr_lookup_f32(const void* flow, int64_t flow_bs, int32_t flow_half, const uint8_t* mask, int64_t mask_bs, const float* feat,
                             int64_t feat_bs, const float* other, int64_t other_bs, int32_t channels, float flow_sign, int32_t radius,
                             int32_t level, int32_t level_h, int32_t level_w, float* out, int64_t out_bs, int32_t n, int32_t h, int32_t w,
                             void* stream);
int ofl_flow_corr_lookup_nodes_f32(const void* flow, int64_t flow_bs, int32_t flow_half, const uint8_t* mask, int64_t mask_bs,
                                   int32_t channels, float flow_sign, int32_t radius, int32_t level, int32_t level_h, int32_t level_w,
                                   const float* grad_out, int64_t grad_bs, float* nodes, int64_t* keys, int32_t n, int32_t h, int32_t w,
                                   void* stream);
int ofl_flow_corr_lookup_grad_feat_f32(const void* flow, int64_t flow_bs, int32_t flow_half, const uint8_t* mask, int64_t mask_bs,
                                       const float* other, int64_t other_bs, int32_t channels, float flow_sign, int32_t radius,
                                       int32_t level, int32_t level_h, int32_t level_w, const float* nodes, float* grad_feat,
                                       int32_t accumulate, int32_t n, int32_t h, int32_t w, void* stream);
int ofl_flow_corr_lookup_grad_other_f32(const float* feat, int64_t feat_bs, int32_t channels, int32_t radius, int32_t level_h,
                                        int32_t level_w, const float* nodes, const int64_t* order, const int64_t* starts,
                                        float* grad_other, int32_t n, int32_t h, int32_t w, void* stream);

/*
 * The convex upsampling of RAFT-style networks (RAFT, GMA, CRAFT, SEA-RAFT, FlowFormer, RAFT-Stereo), one streaming pass (DESIGN.md 3.26,
 * which defines the numbers; ofl_upsample.hip): Flow.upsample_convex.  An extension: the reference has no such function.  flow, flow_bs
 * and flow_half as for ofl_flow_photometric_f64, but h and w may be 1; `logits` fp32 [n][9 K^2][h w], contiguous, K = `factor`, 2, 4 or 8:
 * channel t K^2 + i K + j belongs to tap t = 3 (dy + 1) + (dx + 1), dy, dx = -1 .. 1, sub-row i and sub-column j (RAFT's order).  For the
 * fine pixel (K y + i, K x + j), every step float64 with one rounding per operation unless said otherwise:
 *   m        the maximum of the nine logits by a running float32 compare: m = l_0; m = (l_t > m) ? l_t : m
 *   e_t      = exp((double)l_t - (double)m);  s = (((e_0 + e_1) + ...) + e_8);  w_t = e_t / s
 *   F_{c,t}  = K * (double)f_c(y + dy, x + dx), exact; +0, selected and not loaded, where the neighbour lies outside the coarse frame
 *   o_c      = sum over t ascending, from +0, of w_t * F_{c,t}: each product rounded, then the sum (no fused multiply-add)
 * The mask does not enter the arithmetic.  Inputs are never written.
 *
 * ofl_flow_upsample_convex_f32: out fp32 [n][2][K h][K w] = (float)o_c, every element WRITTEN; with a mask ([*,h,w] bytes, stride mask_bs)
 *   out_mask bytes [n][K h][K w], every element WRITTEN: (mask(y, x) != 0) over the K x K block of the coarse pixel.  mask and out_mask
 *   are both given or both NULL.  One launch.
 * ofl_flow_upsample_convex_grad_f32: with the upstream gradient grad_out fp32 [n][2][K h][K w] and G_c = (double)grad_out_c:
 *   grad_logits (NULL: not made) fp32 [n][9 K^2][h w], every element WRITTEN:
 *     (float)( w_t * ((G_0 * F_{0,t} + G_1 * F_{1,t}) - (G_0 * o_0 + G_1 * o_1)) ), w and o as in the forward
 *   grad_flow (NULL: not made) fp32 [n][2][h w], every element WRITTEN, a gather without atomics:
 *     grad_flow_c(q) = (float)( K * sum over t, then i, then j ascending, from +0, of w_t(i, j; q - delta_t) * G_c(q - delta_t; i, j) ),
 *     over the taps whose coarse pixel q - delta_t lies in the frame, delta_t = (dy, dx) of tap t
 *   workspace: float64 [n][2][K h][K w], required exactly when grad_flow is given; the first launch WRITES m and s of every fine pixel
 *   to it and the second reads them (w_t = exp((double)l_t - m) / s).  Two launches, or one without grad_flow.
 *
 * OFL_E_ARG, before any launch, for: a factor other than 2, 4, 8, n outside 1 .. 65535, h or w < 1, (K h) * (K w) >= 2^31, a NULL
 * required pointer, mask without out_mask or the reverse, grad_flow without workspace or the reverse, neither gradient, a negative
 * stride, a flow_half that is neither 0 nor 1, a pointer not aligned to its element (out and grad_out: to 16 bytes, out_mask: to 8).
 */
int ofl_flow_upsample_convex_f32(const void* flow, int64_t flow_bs, int32_t flow_half, const uint8_t* mask, int64_t mask_bs,
                                 const float* logits, int32_t factor, float* out, uint8_t* out_mask, int32_t n, int32_t h, int32_t w,
                                 void* stream);
int ofl_flow_upsample_convex_grad_f32(const void* flow, int64_t flow_bs, int32_t flow_half, const float* logits, int32_t factor,
                                      const float* grad_out, float* grad_logits, float* grad_flow, double* workspace, int32_t n, int32_t h,
                                      int32_t w, void* stream);

/*
 * The global matching of GMFlow-style networks (GMFlow, UniMatch, matching heads of tracking and stereo networks), streamed without the
 * (h w)^2 volume (which defines the numbers; ofl_matching.hip): Flow.from_matching.  An extension: the reference has no
 * such function.  `feat` and `other` fp32 [*,C,h,w], planes contiguous, feat_bs / other_bs elements between images (0: one image for the
 * whole batch), C = `channels` >= 1, h, w >= 1; flow_sign -1 for an 's' flow, +1 for a 't' flow.  For pixel p = (y, x) and every position
 * q = (qy, qx) of `other` in ascending raster order:
 *   s_q      = (sum over c ascending, from +0, of feat_c(p) * other_c(q)) / sqrtf((float)C): float32, each product rounded, then the sum
 *   chain    m float32; S, X, Y float64, one rounding per operation.  At q = 0: m = s_0, S = X = Y = +0.  For every q: if s_q > m then
 *            r = exp((double)m - (double)s_q), S = S r, X = X r, Y = Y r, m = s_q; then e = exp((double)s_q - (double)m), S = S + e,
 *            X = X + e (double)qx, Y = Y + e (double)qy
 *   result   ox = X / S, oy = Y / S; u = (float)((ox - (double)x) * -flow_sign), v = (float)((oy - (double)y) * -flow_sign);
 *            prob = (float)(1.0 / S)
 * Inputs are never written.
 *
 * ofl_flow_global_match_f32: out fp32 [n][2][h w] = (u, v), every element WRITTEN; prob (NULL: not made) fp32 [n][h w], every element
 *   WRITTEN; workspace (NULL: no backward will follow) 28 n h w bytes, 8-byte aligned, every byte WRITTEN: float64 [3][n][h w] = S, ox, oy,
 *   then float32 [n][h w] = m.  One launch.
 * ofl_flow_global_match_grad_f32: with the workspace of the forward of the same operands, the upstream gradient grad_out fp32 [n][2][h w]
 *   and G = -flow_sign * (double)grad_out of p, per pair:  w = exp((double)s_q - (double)m) / S,
 *   ds = (float)(w * ((G_x * ((double)qx - ox)) + (G_y * ((double)qy - oy)))),  dss = ds / sqrtf((float)C), and
 *     grad_feat  (NULL: not made) fp32 [n][C][h w], every element WRITTEN: sum over q ascending, from +0, of dss(p, q) * other_c(q)
 *     grad_other (NULL: not made) fp32 [n][C][h w], every element WRITTEN: sum over p ascending, from +0, of dss(p, q) * feat_c(p)
 *   float32 products and one float32 sum per element, no atomics.  One launch per gradient; any C (a launch walks the frame once per 128
 *   channels).
 *
 * OFL_E_ARG, before any launch, for: n outside 1 .. 65535, h or w outside 1 .. 2^24, h * w >= 2^31, C < 1, a flow_sign other than +-1, a
 * NULL required pointer, neither gradient, a negative stride, a pointer not aligned to its element (the workspace: to 8 bytes).
 */
int ofl_flow_global_match_f32(const float* feat, int64_t feat_bs, const float* other, int64_t other_bs, int32_t channels, float flow_sign,
                              float* out, float* prob, void* workspace, int32_t n, int32_t h, int32_t w, void* stream);
int ofl_flow_global_match_grad_f32(const float* feat, int64_t feat_bs, const float* other, int64_t other_bs, int32_t channels,
                                   float flow_sign, const void* workspace, const float* grad_out, float* grad_feat, float* grad_other,
                                   int32_t n, int32_t h, int32_t w, void* stream);

/*
 * The global matching of fp16 / bf16 features on the matrix cores (which defines the numbers; ofl_matching_x16.hip):
 * Flow.from_matching of two tensors of one 16-bit dtype.  `feat` and `other` [*,C,h,w] elements of `elem` (OFL_X16_HALF, OFL_X16_BFLOAT,
 * the convention of ofl_warp_bwd_x16), planes contiguous, feat_bs / other_bs elements between images (0: one image for the whole batch),
 * C >= 1 without an upper limit (padded with zeros on both sides to a multiple of 16), h, w >= 1.  For pixel p and every position q:
 *   s_q      = (sum over c of feat_c(p) * other_c(q)) * kInvRoot: the products exact in float32, summed in float32 by
 *            v_mfma_f32_32x32x16_{f16,bf16} in its own order, then ONE float32 product with kInvRoot = (float)(1.0 / sqrt((double)C))
 *   softmax  a float32 running maximum; weights exp(s_q - m) by v_exp_f32 of the float32 product with log2(e) (exactly 1 at 0, +0 below
 *            -128); float32 sums over the 16 positions a lane holds of a chunk of 32; float64 sums across chunks with the float64 rescale
 *            of ofl_flow_global_match_f32; a position beyond h w takes no part
 *   result   ox = X / S, oy = Y / S; u = (float)((ox - (double)x) * -flow_sign), v alike; prob = (float)(1.0 / S), as there
 * out fp32 [n][2][h w], every element WRITTEN; prob (NULL: not made) fp32 [n][h w], every element WRITTEN; stats (NULL: no backward will
 * follow) 28 n h w bytes, 8-byte aligned, every byte WRITTEN, the layout and meaning of ofl_flow_global_match_f32's workspace (m the FINAL
 * maximum): ofl_flow_global_match_grad_f32 reads it, given the exact float32 up-conversions of the features.  `workspace`:
 * ofl_flow_global_match_x16_pack_bytes(C, n, h, w) bytes, 16-byte aligned, every byte WRITTEN by the first launch and read by the second
 * (both tensors pixel-major, padded with zeros); its contents mean nothing afterwards.  Inputs are never written.  Two launches:
 * ofl_last_kernel_name() then names flow_global_match_x16_kernel<half_t | bf16_t, channels stay in registers>.
 *
 * OFL_E_ARG, before any launch, for: n outside 1 .. 65535, h or w outside 1 .. 2^24, h * w >= 2^31, C < 1, another `elem`, a flow_sign
 * other than +-1, a NULL feat, other, out or workspace, a negative stride, a pointer not aligned to what is loaded through it (the
 * features: 2 bytes, out and prob: 4, stats: 8, workspace: 16).  ofl_flow_global_match_x16_pack_bytes returns OFL_E_ARG (negative) for
 * a frame so refused.
 */
int64_t ofl_flow_global_match_x16_pack_bytes(int32_t channels, int32_t n, int32_t h, int32_t w);
int ofl_flow_global_match_x16(const void* feat, int64_t feat_bs, const void* other, int64_t other_bs, int32_t channels, int32_t elem,
                              float flow_sign, float* out, float* prob, void* stats, void* workspace, int32_t n, int32_t h, int32_t w,
                              void* stream);

/* ---- flow propagation by attention -----------------------------------------------------------------------------------------------
 * flow'(p) = sum_q softmax_q(query(p) . key(q) / sqrt(C)) flow(q), GMFlow's and UniMatch's propagation of matched vectors by
 * self-attention, over ALL positions q (global) or over the (2 radius + 1)^2 window of p with zero padding (local), without the (h w)^2
 * volume and without an unfold (which defines the numbers; ofl_propagate.hip): Flow.propagate.  An extension: the
 * reference has no such function.  `query` and `key` fp32 [*,C,h,w], `flow` fp32 [*,2,h,w] = (u, v), `mask` (NULL: nothing is excluded)
 * bytes [*,h,w], planes contiguous, *_bs elements between images (0: one image for the whole batch), C = `channels` >= 1, h, w >= 1.
 * A position q inside the frame is EXCLUDED where its mask byte is 0.
 *   s(p, q)  = (sum over c ascending, from +0, of query_c(p) * key_c(q)) / sqrtf((float)C): float32, each product rounded, then the sum
 *   global   the chain of ofl_flow_global_match_f32 over the positions that are not excluded, in ascending raster order: m float32; S, X,
 *            Y float64.  The first participating position sets m = s, S = X = Y = +0; every step: if s > m then r = exp((double)m -
 *            (double)s), S = S r, X = X r, Y = Y r, m = s; then e = exp((double)s - (double)m), S = S + e, X = X + e (double)u(q),
 *            Y = Y + e (double)v(q).  An excluded position contributes no step
 *   local    the offsets (dy, dx), dy outermost, both ascending from -radius.  A position outside the frame takes part with the logit +0
 *            and the vector (0, 0), whatever the mask.  Two passes: m = the first participating logit, replaced by every later one with
 *            s > m; then S, X, Y as above in offset order on that final m, without a rescale
 *   result   ox = X / S, oy = Y / S; out = ((float)ox, (float)oy).  A pixel is EMPTY when no position inside the frame takes part: its
 *            result is (+0, +0), its byte of `valid` 0 (every other pixel: 1), its statistics S = 0, m = ox = oy = +0
 * Inputs are never written.
 *
 * ofl_flow_propagate_global_f32 / ofl_flow_propagate_local_f32: out fp32 [n][2][h w], every element WRITTEN; valid (NULL: not made) bytes
 *   [n][h w], every element WRITTEN; workspace (NULL: no backward will follow) 28 n h w bytes, 8-byte aligned, every byte WRITTEN: float64
 *   [3][n][h w] = S, ox, oy, then float32 [n][h w] = m.  One launch.
 * ofl_flow_propagate_global_grad_f32 / ofl_flow_propagate_local_grad_f32: with the workspace of the forward of the same operands and the
 *   upstream gradient grad_out fp32 [n][2][h w] = (g_x, g_y), per pair:  w = exp((double)s - (double)m) / S,
 *   ds = (float)(w * (((double)g_x * ((double)u(q) - ox)) + ((double)g_y * ((double)v(q) - oy)))),  dss = ds / sqrtf((float)C),
 *   tx = (float)(w * (double)g_x), ty = (float)(w * (double)g_y); dss, tx and ty are exactly +0 where q is excluded or p is empty, and
 *     grad_query (NULL: not made) fp32 [n][C][h w], every element WRITTEN: sum over q in forward order, from +0, of dss(p, q) * key_c(q)
 *     grad_key   (NULL: not made) fp32 [n][C][h w], every element WRITTEN: sum over p ascending, from +0, of dss(p, q) * query_c(p)
 *     grad_flow  (NULL: not made) fp32 [n][2][h w], every element WRITTEN: sum over p ascending, from +0, of tx(p, q); of ty(p, q)
 *   float32 products and one float32 sum per element, no atomics; a position outside the frame has no gradient.  Global: one launch
 *   for grad_query and one for grad_key and grad_flow together, each recomputing the logits.  Local: `scratch` fp32 [n][k][(2 radius +
 *   1)^2][h w], k = 3 with grad_flow and 1 without, every element WRITTEN by a first launch (dss, tx, ty per offset), from which the
 *   gradients are gathered by one launch for grad_query and one for grad_key and grad_flow.
 *
 * OFL_E_ARG, before any launch, for: n outside 1 .. 65535, h or w outside 1 .. 2^24, h * w >= 2^31, C < 1, a radius outside 1 .. 4, a
 * NULL required pointer, no gradient at all, a negative stride, a pointer not aligned to its element (the workspace: to 8 bytes).
 */
int ofl_flow_propagate_global_f32(const float* query, int64_t query_bs, const float* key, int64_t key_bs, int32_t channels,
                                  const float* flow, int64_t flow_bs, const uint8_t* mask, int64_t mask_bs, float* out, uint8_t* valid,
                                  void* workspace, int32_t n, int32_t h, int32_t w, void* stream);
int ofl_flow_propagate_global_grad_f32(const float* query, int64_t query_bs, const float* key, int64_t key_bs, int32_t channels,
                                       const float* flow, int64_t flow_bs, const uint8_t* mask, int64_t mask_bs, const void* workspace,
                                       const float* grad_out, float* grad_query, float* grad_key, float* grad_flow, int32_t n, int32_t h,
                                       int32_t w, void* stream);
int ofl_flow_propagate_local_f32(const float* query, int64_t query_bs, const float* key, int64_t key_bs, int32_t channels,
                                 const float* flow, int64_t flow_bs, const uint8_t* mask, int64_t mask_bs, int32_t radius, float* out,
                                 uint8_t* valid, void* workspace, int32_t n, int32_t h, int32_t w, void* stream);
int ofl_flow_propagate_local_grad_f32(const float* query, int64_t query_bs, const float* key, int64_t key_bs, int32_t channels,
                                      const float* flow, int64_t flow_bs, const uint8_t* mask, int64_t mask_bs, int32_t radius,
                                      const void* workspace, const float* grad_out, float* scratch, float* grad_query, float* grad_key,
                                      float* grad_flow, int32_t n, int32_t h, int32_t w, void* stream);

/* ---- local matching ----------------------------------------------------------------------------------------------------------------
 * flow'(p) = flow(p) - flow_sign * E[o], E the expectation of the offsets o of the (2 radius + 1)^2 window of p under
 * softmax_o(feat(p) . W'(p + o) / sqrt(C)), W' being `other` sampled where the flow points: the local matching of GMFlow's and UniMatch's
 * refinement stage, without the warped tensor, the volume or the unfold (which defines the numbers;
 * ofl_local_match.hip): Flow.match_local.  An extension: the reference has no such function.  Operands as for ofl_flow_cost_volume_f32:
 * `flow` fp32 or fp16 [*,2,h,w], `mask` (NULL: all True) bytes [*,h,w], `feat` and `other` fp32 [*,C,h,w], *_bs elements between images
 * (0: one image for the whole batch), flow_sign -1 ('s') or +1 ('t'), h, w >= 2.  W'_c(q) and usable(q) are those of the cost volume, bit
 * for bit: the sample where the mask is True and the weight sum of the taps inside the frame exceeds 0.99999, +0 elsewhere (selected).
 *   offsets  o = (dy, dx), dy outermost, both ascending from -radius.  A position p + o OUTSIDE the frame takes NO part: no step, no
 *            gradient.  A position inside always takes part, usable or not (through W' = +0).  The centre is inside: no pixel is empty
 *   s(p, o)  = (sum over c ascending, from +0, of feat_c(p) * W'_c(p + o)) / sqrtf((float)C): float32, each product rounded, then the sum
 *   softmax  two passes: m = the first participating logit, replaced by every later one with s > m; then in offset order on that final m
 *            e = exp((double)s - (double)m), S = S + e, X = X + e (double)dx, Y = Y + e (double)dy, float64 from +0
 *   result   ox = X / S, oy = Y / S; u' = (float)((double)u + (-flow_sign) ox), v' = (float)((double)v + (-flow_sign) oy), one
 *            rounding each; prob = (float)(1.0 / S)
 * Inputs are never written.
 *
 * ofl_flow_local_match_f32: out fp32 [n][2][h w], every element WRITTEN; prob (NULL: not made) fp32 [n][h w], every element WRITTEN;
 *   workspace (NULL: no backward will follow) 28 n h w bytes, 8-byte aligned, every byte WRITTEN: float64 [3][n][h w] = S, ox, oy, then
 *   float32 [n][h w] = m.  One launch.
 * ofl_flow_local_match_grad_f32: with the workspace of the forward of the same operands and the upstream gradient grad_out fp32
 *   [n][2][h w] = (g_x, g_y), G = -flow_sign (double)g:  w = exp((double)s - (double)m) / S,
 *   ds = (float)(w * ((G_x * ((double)dx - ox)) + (G_y * ((double)dy - oy)))),  dss = ds / sqrtf((float)C), exactly +0 (selected) at a
 *   position outside the frame.  `scratch` fp32 [n][(2 radius + 1)^2][h w], every element WRITTEN by a first launch (dss per offset);
 *     grad_feat   (NULL: not made) fp32 [n][C][h w], every element WRITTEN: sum over o ascending, from +0, of dss(p, o) * W'_c(p + o)
 *     grad_warped (NULL: not made) fp32 [n][C][h w], every element WRITTEN: usable(q) ? sum over o ascending, from +0, of
 *                 dss(q - o, o) * feat_c(q - o), q - o inside the frame : +0 -- the gradient with respect to the sample W, which the
 *                 backward of the warp (ofl_flow_cost_volume_chain_f32, ofl_warp_bwd_grad_f32, ofl_flow_cost_volume_gate_f32) turns into
 *                 those of `other` and of the warp's part of the flow; the flow's own term is grad_out itself
 *   float32 products and one float32 sum per element, no atomics; one launch per gradient after the first.
 *
 * OFL_E_ARG, before any launch, for: n outside 1 .. 65535, h or w < 2, h * w >= 2^31, C < 1, a radius outside 1 .. 4, a flow_sign other
 * than +-1, a NULL required pointer, neither gradient, a negative stride, a pointer not aligned to its element (the workspace: to 8).
 */
int ofl_flow_local_match_f32(const void* flow, int64_t flow_bs, int32_t flow_half, const uint8_t* mask, int64_t mask_bs, const float* feat,
                             int64_t feat_bs, const float* other, int64_t other_bs, int32_t channels, float flow_sign, int32_t radius,
                             float* out, float* prob, void* workspace, int32_t n, int32_t h, int32_t w, void* stream);
int ofl_flow_local_match_grad_f32(const void* flow, int64_t flow_bs, int32_t flow_half, const uint8_t* mask, int64_t mask_bs,
                                  const float* feat, int64_t feat_bs, const float* other, int64_t other_bs, int32_t channels,
                                  float flow_sign, int32_t radius, const void* workspace, const float* grad_out, float* scratch,
                                  float* grad_feat, float* grad_warped, int32_t n, int32_t h, int32_t w, void* stream);

/*
 * The sequence loss of RAFT, GMA, CRAFT, GMFlow, UniMatch and FlowFormer: the T refinement outputs of a network scored against ONE ground
 * truth in one pass (which defines the numbers; ofl_sequence_loss.hip): Flow.sequence_loss / sequence_stats.  An
 * extension: the reference has no such function.  preds / pred_bs / pred_half: HOST arrays of t entries, 1 <= t <= OFL_SEQUENCE_LOSS_MAX_T
 * -- the device pointer of prediction i, [*,2,h,w] fp32 (half 0) or fp16 (1: up-converted in registers, exact), and the elements between
 * its images; they are copied into the kernel arguments, nothing is uploaded.  gt likewise one flow, gt_mask (NULL: all True) bytes
 * [*,h,w].  Per pixel, every step fp32 with one rounding per operation, both roots correctly rounded:
 *   valid  = gt_mask and sqrt(ug ug + vg vg) < max_flow: a float compare, which a NaN or infinite magnitude (a square that overflows
 *            included) fails; max_flow > 0, +inf allowed.  The predictions carry no mask
 *   e_i    = sqrt(du du + dv dv), du = u_i - ug, dv = v_i - vg
 *   t_i    = fabsf(du) + fabsf(dv) (penalty OFL_SEQUENCE_LOSS_L1) or e_i (OFL_SEQUENCE_LOSS_L2)
 *
 * ofl_flow_sequence_loss_workspace_bytes(t, n, h, w): bytes of the workspace of ofl_flow_sequence_loss_f64 (8-byte aligned; every word
 *   the second launch reads is written by the first: nothing to clear), or OFL_E_SHAPE.
 *
 * ofl_flow_sequence_loss_f64: records float64 [n, 2 t + 4], per image over its valid pixels
 *     [0] count   [1 + i] sum t_i   [1 + t + i] sum e_i   [1 + 2 t + k] pixels with e_{t-1} < 1, 3, 5 px (k = 0, 1, 2; an fp32 compare and
 *     STRICTLY below, as RAFT's 1px / 3px / 5px metrics: the opposite sense to the `>` of ofl_flow_error_f64's thresholds)
 *   Counts are exact.  Sums are float64 sums of the fp32 terms in a fixed order -- a lane's pixels ascending, the lanes of a wave by a
 *   butterfly, the waves and then the blocks of an image in index order; a block owns OFL_SEQUENCE_LOSS_CHUNK consecutive pixels, so the
 *   order depends on h * w and t only: no float atomics, an image's record has the same bits in any batch and on any run.  A valid
 *   pixel's NaN term makes that sum NaN; a pixel that is not valid contributes nothing whatever it holds.  Two launches:
 *   ofl_last_kernel_name() then names flow_sequence_loss_finish_kernel.
 *
 * ofl_flow_sequence_loss_grad_f32: scale fp32 [n, t] DEVICE memory (upstream gradient * weight_i / divisor); grads: a HOST array of t
 *   device pointers fp32 [n,2,h,w], NULL for a prediction that wants none (at least one must be given).  Every element of every
 *   gradient given is WRITTEN; +0 where the pixel is not valid.  L1: +scale where d > 0, -scale where d < 0, +0 where d is 0 or NaN, d
 *   being du or dv.  L2: the float64 quotient (scale d) / sqrt(du du + dv dv) of the fp32 differences rounded once, +0 where the fp32
 *   du du + dv dv is not > 0.  One launch: flow_sequence_loss_grad_kernel.
 *
 * `normalise` (OFL_SEQUENCE_LOSS_ALL / _VALID) names the divisor the caller forms the loss and `scale` with -- 2 h w or 2 count (L1), h w
 * or count (L2); the kernels do not divide, the code is only checked.  Before any launch: OFL_E_NULL for a NULL required pointer (an
 * entry of preds included; grads all NULL), OFL_E_SHAPE for t outside 1 .. 32, n outside 1 .. 65535, h or w < 1, h * w >= 2^31, OFL_E_ARG
 * for another penalty or normalise code, a max_flow that is NaN or <= 0, a storage kind other than 0 or 1, a negative stride, a pointer
 * not aligned to its element.  64-bit element offsets throughout.
 */
#define OFL_SEQUENCE_LOSS_MAX_T 32
#define OFL_SEQUENCE_LOSS_CHUNK 2048
#define OFL_SEQUENCE_LOSS_L1 0
#define OFL_SEQUENCE_LOSS_L2 1
#define OFL_SEQUENCE_LOSS_ALL 0
#define OFL_SEQUENCE_LOSS_VALID 1
int64_t ofl_flow_sequence_loss_workspace_bytes(int32_t t, int32_t n, int32_t h, int32_t w);
int ofl_flow_sequence_loss_f64(const void* const* preds, const int64_t* pred_bs, const int32_t* pred_half, int32_t t, const void* gt,
                               int64_t gt_bs, int32_t gt_half, const uint8_t* gt_mask, int64_t gt_mask_bs, float max_flow, int32_t penalty,
                               int32_t normalise, void* workspace, double* records, int32_t n, int32_t h, int32_t w, void* stream);
int ofl_flow_sequence_loss_grad_f32(const void* const* preds, const int64_t* pred_bs, const int32_t* pred_half, int32_t t, const void* gt,
                                    int64_t gt_bs, int32_t gt_half, const uint8_t* gt_mask, int64_t gt_mask_bs, float max_flow,
                                    int32_t penalty, int32_t normalise, const float* scale, float* const* grads, int32_t n, int32_t h,
                                    int32_t w, void* stream);

/*
 * The composition of a clip's frame-to-frame flows f_1 .. f_t into the flow from the first frame to the last, in one launch (DESIGN.md
 * 3.31, which defines the numbers; ofl_chain.hip): Flow.chain / chain_flows.  An extension: the reference composes two flows at a time
 * (combine_with mode 3), of which this is the fold without the intermediate flows.  flows / flow_bs / flow_half / masks / mask_bs: HOST
 * arrays of t entries in the order of TIME, 2 <= t <= OFL_CHAIN_MAX_T -- the device pointer of flow k, [*,2,h,w] fp32 (half 0) or fp16
 * (1: up-converted in registers, exact), the elements between its images (0 broadcasts one image), its mask [*,h,w] bytes (any non-zero
 * byte is True; a NULL entry, or masks == NULL for all of them, is all True and no byte is read for it) and the bytes between the
 * mask's images; they are copied into the kernel arguments, nothing is uploaded.  Inputs are never written.
 *
 * Per pixel p, an independent walk, every step fp32 with one rounding per operation:
 *   flow_sign -1 ('s' flows, result on the first frame's grid): acc = f_1(p), m = mask_1(p); for k = 2 .. t the position is p + acc
 *   flow_sign +1 ('t' flows, result on the last frame's grid):  acc = f_t(p), m = mask_t(p); for k = t - 1 .. 1 the position is p - acc
 *   step k: the four taps and weights of the backward warp at that position (ofl_warp_bwd_f32); (bu, bv) the sample of f_k, a tap outside
 *   the frame reading 0, `v_nw * nw` then three fmaf in the order ne, sw, se; mr the same chain over the taps' validity (inside the
 *   frame and True in mask_k); then acc = acc + (bu, bv), two plain adds, and m = m and (mr > 0.99999f).
 * The vectors are accumulated whatever m says, positions outside the frame included; a non-finite position fails every comparison, its
 * taps read 0 and m turns false.  These are the bits of the fold of combine_with mode 3 (ofl_warp_bwd_f32 with the addend) where that
 * fold takes none of its early exits.
 *
 *   out, out_mask   want_all == 0: fp32 [n,2,h,w] and uint8 [n,h,w], the whole chain.  want_all == 1: fp32 [t-1,n,2,h,w] and uint8
 *                   [t-1,n,h,w], every partial chain of two flows and more as the walk passes it: flow_sign -1, slot j holds the chain
 *                   of f_1 .. f_{j+2}; flow_sign +1, slot j holds the chain of f_{j+1} .. f_t (the whole chain: slot t - 2 and slot 0).
 *   Every element of both outputs is WRITTEN (vectors under a false mask included; nothing to clear beforehand); mask bytes are 0 / 1.
 * OFL_E_ARG, before any launch, for: t outside 2 .. 32, n outside 1 .. 65535, h or w < 2, h * w >= 2^31, a flow_sign other than +-1, a
 * want_all or storage kind other than 0 or 1, a NULL flows, flow_bs or flow_half array (mask_bs with masks given), a NULL flow or output,
 * a negative stride, a pointer not aligned to its element.  One launch: flow_chain_kernel.  64-bit element offsets throughout.
 */
#define OFL_CHAIN_MAX_T 32
int ofl_flow_chain_f32(const void* const* flows, const int64_t* flow_bs, const int32_t* flow_half, const uint8_t* const* masks,
                       const int64_t* mask_bs, int32_t t, float flow_sign, float* out, uint8_t* out_mask, int32_t want_all, int32_t n,
                       int32_t h, int32_t w, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OFLIB_HIP_H */
