// ofl_loss_common.hpp -- what the fused metric and loss sources share (ofl_metrics.hip, ofl_consistency.hip, ofl_smoothness.hip,
// ofl_photometric.hip, ofl_census.hip, ofl_ssim.hip, ofl_cost_volume.hip, ofl_corr_lookup.hip, ofl_upsample.hip, ofl_sequence_loss.hip, ofl_chain.hip): the launch recorder, the bilinear sample of the backward warp
// and its derivative, the per-block record sums and their finish, the host checks.  Internal: not part of the C ABI
// (include/oflib_hip.h).  Every geometry constant (kThreads, kRec, tile and block limits) stays in the including source and comes in as a
// template argument; a source pulls `ofl_loss` into its anonymous namespace.
//
// THE SAMPLE.  unnormalise(), taps_of() and sample_of() RESTATE unnormalise() and the body of warp_bwd_kernel of ofl_kernels.hip: position
// unnormalise(grid - flow_sign * a), floorf, nw / ne / sw / se, `v_nw * nw` then three fmaf in the order ne, sw, se, the same chain over
// the taps' insideness for mr; a tap outside the frame reads as 0.  A change there is made HERE and in partner() of ofl_consistency.hip, which
// writes the same geometry out (its vector kernels grow from 102 to 111-122 VGPRs through Taps: tools/isa_stats.py shows it when
// partner() is put on taps_of()); the GPU tiers of the including sources compare the two on the device.
//
// THE SUMS.  The number of blocks of an image depends on its shape only, a lane adds its pixels in ascending order, reduce_record() adds
// the lanes by a butterfly and the waves in index order, finish_records() the blocks in index order: no float atomics, the record of an
// image carries the same bits in any batch and on any run.
#ifndef OFL_LOSS_COMMON_HPP
#define OFL_LOSS_COMMON_HPP

#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "oflib_hip.h"

#pragma clang fp contract(off)

// the launch recorder of ofl_kernels.hip (ofl_last_kernel_name)
extern const void* g_ofl_last_kernel;
#define OFL_KLAUNCH(K, ...) do { g_ofl_last_kernel = (const void*)(K); hipLaunchKernelGGL(K, __VA_ARGS__); } while (0)

namespace ofl_loss {

constexpr float kValidThr = 0.99999f;              // ofl_kernels.hip (flow_class.py:922)

// unnormalise() of ofl_kernels.hip: normalise_coords (utils.py:462-465) followed by the grid sampler's align_corners un-normalise
__device__ __forceinline__ float unnormalise(float p, float size_m1, float half_size_m1) {
    float g = p * 2.0f;
    g = g / size_m1;  // IEEE correctly-rounded divide (no fast-math)
    g = g - 1.0f;
    return (g + 1.0f) * half_size_m1;
}

template <bool HALF>
__device__ __forceinline__ float ld_flow(const void* base, int64_t i) {
    return HALF ? __half2float(reinterpret_cast<const __half*>(base)[i]) : reinterpret_cast<const float*>(base)[i];
}

// one sample of an image plane on the scale 0 .. 1: a uint8 sample s is float(s) / 255.0f
template <bool U8>
__device__ __forceinline__ float ld_img_unit(const void* base, int64_t i) {
    return U8 ? (float)reinterpret_cast<const uint8_t*>(base)[i] / 255.0f : reinterpret_cast<const float*>(base)[i];
}

// one sample of an image plane as it is stored: a uint8 sample s is float(s), on the scale 0 .. 255
template <bool U8>
__device__ __forceinline__ float ld_img_raw(const void* base, int64_t i) {
    return U8 ? (float)reinterpret_cast<const uint8_t*>(base)[i] : reinterpret_cast<const float*>(base)[i];
}

// correctly rounded fp32 square root: what hipcc makes of sqrtf by default (no fast-math, correctly rounded divide / sqrt left on).  The
// float64 root rounded once is the same value by construction (53 >= 2 * 24 + 2 bits) and measured 15 % slower on the whole pass
// (DESIGN.md 3.16); tests/test_gpu_flow_error.py holds this one to np.sqrt bit for bit, denormal sums of squares included
__device__ __forceinline__ float sqrt_rn(float s) { return __builtin_sqrtf(s); }

// the four taps of the sample of pixel (x, y) whose vector is (u, v): the head of warp_bwd_kernel (ofl_kernels.hip)
struct Taps {
    float sx, sy, x_w, y_n;                        // the position and its floors
    float nw, ne, sw, se;                          // fp32 weights
    int64_t o_nw, o_ne, o_sw, o_se;                // offsets in a plane, clamped into it: always addressable
    bool k_nw, k_ne, k_sw, k_se;                   // inside the frame
    float mr;                                      // weight sum of the taps inside
};

// P: a parameter struct with w, h, flow_sign, wm1, hm1, half_wm1, half_hm1
template <class P>
__device__ __forceinline__ Taps taps_of(const P& p, int x, int y, float u, float v) {
    Taps t;
    const int w = p.w, h = p.h;
    const float px = (float)x - p.flow_sign * u;
    const float py = (float)y - p.flow_sign * v;
    t.sx = unnormalise(px, p.wm1, p.half_wm1);
    t.sy = unnormalise(py, p.hm1, p.half_hm1);
    t.x_w = floorf(t.sx); t.y_n = floorf(t.sy);
    const float ww = t.sx - t.x_w, e = 1.0f - ww;
    const float nn = t.sy - t.y_n, s = 1.0f - nn;
    t.nw = s * e; t.ne = s * ww; t.sw = nn * e; t.se = nn * ww;
    const float x_e = t.x_w + 1.0f, y_s = t.y_n + 1.0f;
    const bool x0ok = (t.x_w > -1.0f) && (t.x_w < (float)w);
    const bool x1ok = (x_e > -1.0f) && (x_e < (float)w);
    const bool y0ok = (t.y_n > -1.0f) && (t.y_n < (float)h);
    const bool y1ok = (y_s > -1.0f) && (y_s < (float)h);
    const int ix0 = x0ok ? (int)t.x_w : 0, ix1 = x1ok ? (int)x_e : 0;
    const int iy0 = y0ok ? (int)t.y_n : 0, iy1 = y1ok ? (int)y_s : 0;
    t.o_nw = (int64_t)iy0 * w + ix0; t.o_ne = (int64_t)iy0 * w + ix1;
    t.o_sw = (int64_t)iy1 * w + ix0; t.o_se = (int64_t)iy1 * w + ix1;
    t.k_nw = x0ok && y0ok; t.k_ne = x1ok && y0ok; t.k_sw = x0ok && y1ok; t.k_se = x1ok && y1ok;
    float mr = (t.k_nw ? 1.0f : 0.0f) * t.nw;
    mr = __builtin_fmaf(t.k_ne ? 1.0f : 0.0f, t.ne, mr);
    mr = __builtin_fmaf(t.k_sw ? 1.0f : 0.0f, t.sw, mr);
    mr = __builtin_fmaf(t.k_se ? 1.0f : 0.0f, t.se, mr);
    t.mr = mr;
    return t;
}

// the sample of four tap values (a tap outside the frame: 0)
__device__ __forceinline__ float sample_of(const Taps& t, float v_nw, float v_ne, float v_sw, float v_se) {
    float r = v_nw * t.nw;
    r = __builtin_fmaf(v_ne, t.ne, r);
    r = __builtin_fmaf(v_sw, t.sw, r);
    r = __builtin_fmaf(v_se, t.se, r);
    return r;
}

// the derivative of that sample with respect to its position, in float64 on the float64 fractions of the float32 position
// (tests/grad_oracle64.py, Taps.dx / Taps.dy): west taps -1, east taps +1 (north -1, south +1), each times the other axis's weight
__device__ __forceinline__ void sample_grad(const Taps& t, double v_nw, double v_ne, double v_sw, double v_se, double& gx, double& gy) {
    const double ww = (double)t.sx - (double)t.x_w, e = 1.0 - ww;
    const double nn = (double)t.sy - (double)t.y_n, s = 1.0 - nn;
    gx = (((-s) * v_nw + s * v_ne) - nn * v_sw) + nn * v_se;
    gy = (((-e) * v_nw - ww * v_ne) + e * v_sw) + ww * v_se;
}

// The record of a block from the records of its lanes: slots 0 .. kUsed - 1 of `rec` by a butterfly (every lane ends with the wave's
// value), the kWaves waves in index order out of `s_red` [kWaves * kRec] by the first kRec threads, which store the record of block
// blockIdx.x of image `img` to `partial` [n][nblk][kRec].  Slot kMax is a maximum, every other slot a sum.  Called by every thread of
// the block.  (The address is formed at the store, where the kernels formed it before they shared this function: handed in as a
// pointer, the address arithmetic comes ahead of the butterfly and the compiler interleaves the bpermutes and adds in another order --
// 43 instead of 4 changed lines in flow_photometric_kernel's tail, 112 instead of 72 in flow_smoothness_kernel's)
template <int kRec, int kUsed, int kMax, int kWaves>
__device__ __forceinline__ void reduce_record(double (&rec)[kRec], double* s_red, double* partial, int64_t img, int nblk) {
#pragma unroll
    for (int i = 0; i < kUsed; ++i) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double o = __shfl_xor(rec[i], off);
            rec[i] = (i == kMax) ? fmax(rec[i], o) : rec[i] + o;
        }
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int i = 0; i < kRec; ++i) s_red[wave * kRec + i] = rec[i];
    }
    __syncthreads();
    if (threadIdx.x < kRec) {
        double s = s_red[threadIdx.x];
        for (int wv = 1; wv < kWaves; ++wv) {
            const double o = s_red[wv * kRec + threadIdx.x];
            s = (threadIdx.x == kMax) ? fmax(s, o) : s + o;
        }
        partial[(img * nblk + blockIdx.x) * kRec + threadIdx.x] = s;
    }
}

// The body of a finish kernel, one block of kThreads per image (blockIdx.x): the `nblk` block records of the image out of `partial`
// [n][nblk][kRec] staged in LDS by all threads, kChunk at a time (independent loads: summing straight from memory serialises a load
// latency per record and slot), then slot i added in ascending block order by thread i into `out` [n][kRec]
template <int kRec, int kMax, int kChunk, int kThreads>
__device__ __forceinline__ void finish_records(const double* partial, int nblk, double* out) {
    __shared__ double s_part[kChunk * kRec];
    const int64_t n_img = blockIdx.x;
    const double* part = partial + n_img * nblk * kRec;
    double s = 0.0;
    for (int base = 0; base < nblk; base += kChunk) {
        const int cnt = nblk - base < kChunk ? nblk - base : kChunk;
        for (int i = threadIdx.x; i < cnt * kRec; i += kThreads) s_part[i] = part[(int64_t)base * kRec + i];
        __syncthreads();
        if ((int)threadIdx.x < kRec) {
            for (int b = 0; b < cnt; ++b) {
                const double o = s_part[b * kRec + threadIdx.x];
                s = (threadIdx.x == kMax) ? fmax(s, o) : s + o;
            }
        }
        __syncthreads();
    }
    if ((int)threadIdx.x < kRec) out[n_img * kRec + threadIdx.x] = s;
}

inline bool aligned(const void* ptr, int a) { return ((uintptr_t)ptr % (uintptr_t)a) == 0; }

// a batch the grids can index: n in blockIdx.y, a pixel index in 31 bits; `min_extent`: the smallest height and width the term accepts
inline bool dims_ok(int32_t n, int32_t h, int32_t w, int32_t min_extent) {
    return n >= 1 && n <= 65535 && h >= min_extent && w >= min_extent && (int64_t)h * w < (1ll << 31);
}

// The operands the image-pair losses share (photometric, census, SSIM): the checks of the flow, its mask and the two frames, and the
// fields of P they fill -- the operands, the shape, the sample's constants, every output pointer cleared
template <class P>
int fill_pair_operands(P* p, const void* flow, int64_t flow_bs, int32_t flow_half, const uint8_t* mask, int64_t mask_bs, const void* img,
                       int64_t img_bs, const void* other, int64_t other_bs, int32_t channels, int32_t img_u8, float flow_sign, int32_t n,
                       int32_t h, int32_t w) {
    if (!dims_ok(n, h, w, 2)) return OFL_E_ARG;
    if (flow_sign != 1.0f && flow_sign != -1.0f) return OFL_E_ARG;
    if (flow == nullptr || img == nullptr || other == nullptr) return OFL_E_ARG;
    if ((flow_half != 0 && flow_half != 1) || (img_u8 != 0 && img_u8 != 1)) return OFL_E_ARG;
    if (flow_bs < 0 || mask_bs < 0 || img_bs < 0 || other_bs < 0) return OFL_E_ARG;
    if (!aligned(flow, flow_half ? 2 : 4) || !aligned(img, img_u8 ? 1 : 4) || !aligned(other, img_u8 ? 1 : 4)) return OFL_E_ARG;
    p->flow = flow; p->flow_bs = flow_bs;
    p->mask = mask; p->mask_bs = mask_bs;
    p->img = img; p->other = other; p->img_bs = img_bs; p->other_bs = other_bs;
    p->hw = (int64_t)h * w;
    p->chan = channels; p->h = h; p->w = w; p->nblk = 0;
    p->flow_sign = flow_sign;
    p->wm1 = (float)(w - 1); p->hm1 = (float)(h - 1);
    p->half_wm1 = p->wm1 / 2.0f; p->half_hm1 = p->hm1 / 2.0f;
    p->partial = nullptr; p->map = nullptr; p->out = nullptr; p->scale = nullptr; p->grad = nullptr;
    return OFL_OK;
}

// two run-time flags to the <A, B> instantiation: f(std::bool_constant<A>, std::bool_constant<B>)
template <class F>
void dispatch_flags(bool a, bool b, F&& f) {
    if (a) {
        if (b) f(std::true_type{}, std::true_type{});
        else f(std::true_type{}, std::false_type{});
    } else {
        if (b) f(std::false_type{}, std::true_type{});
        else f(std::false_type{}, std::false_type{});
    }
}

}  // namespace ofl_loss

#endif  // OFL_LOSS_COMMON_HPP
