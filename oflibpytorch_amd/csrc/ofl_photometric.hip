// ofl_photometric.hip -- Flow.photometric / photometric_map / photometric_stats on gfx950: the photometric term of an unsupervised flow
// loss, warp and comparison in one pass (which DEFINES the numbers; tests/photometric_oracle.py is the same definition in
// NumPy).  An extension: the reference has no such function.
//
//   flow_photometric_kernel<HALF, U8, false>   per pixel: the C planes of `other` sampled bilinearly where the flow points and the weight
//                                              sum mr of the taps inside the frame, known = (mr > kValidThr) and the flow's mask, per
//                                              channel d = Iw - I and r = sqrt(d d + eps eps), rho = (sum r) / C.  Writes rho (0 where not
//                                              known) if a map is wanted and, per block, ONE record of 8 float64 values if records are
//   flow_photometric_finish_kernel             one block per image: the block records added in ascending block order, from LDS
//   flow_photometric_kernel<HALF, U8, true>    the backward of the per-image mean with respect to the flow vectors: every pixel recomputes
//                                              its own taps and d and writes its own two gradient elements; no scatter, no atomics
//
// The warped image is never written.  The sample position, the tap weights and the four-term sums RESTATE unnormalise() and the body of
// warp_bwd_kernel of ofl_kernels.hip as ofl_consistency.hip does (position unnormalise(grid - flow_sign * a), floorf, nw / ne / sw / se,
// `v_nw * nw` then three fmaf in the order ne, sw, se, the same chain over the taps' insideness for mr; a tap outside the frame reads as
// 0) -- a change there is made here too; tests/test_gpu_photometric.py compares the two on the device.
//
// One lane takes ONE pixel per round and the lanes of a wave take consecutive pixels of the image (of a row, up to where a row ends),
// the rounds a grid stride apart: on a smooth flow a wave's load of one tap of one plane is one contiguous run of 256 bytes (64 of a uint8
// image), which the four-pixels-per-lane form of ofl_consistency.hip spreads over 1 KiB.  Taps are single loads
// straight from global memory at offsets clamped into the plane: always addressable.  Sums as in ofl_metrics.hip: the number of blocks
// depends on (h, w) only, a lane adds its pixels in ascending order, lanes by a butterfly, waves and then blocks in index order: no float
// atomics, the record of an image carries the same bits in any batch and on any run.  C ABI: include/oflib_hip.h.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <math.h>
#include <stdint.h>

#include "oflib_hip.h"

#pragma clang fp contract(off)

// the launch recorder of ofl_kernels.hip (ofl_last_kernel_name)
extern const void* g_ofl_last_kernel;
#define OFL_KLAUNCH(K, ...) do { g_ofl_last_kernel = (const void*)(K); hipLaunchKernelGGL(K, __VA_ARGS__); } while (0)

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxBlocks = 256;                    // forward: blocks per image at most (one per CU); 1080p: each walks 31 or 32 rounds
constexpr int kMaxGradBlocks = 2048;               // backward: nothing to reduce
constexpr int kRec = OFL_PHOTOMETRIC_RECORD;       // doubles per record
constexpr int kMaxChan = 4;
constexpr float kValidThr = 0.99999f;              // ofl_kernels.hip (flow_class.py:922)
enum { R_COUNT = 0, R_SUM = 1, R_MAX = 2, R_USED = 3 };

struct PhotoParams {
    const void* flow;                              // [*,2,H,W] fp32 or fp16
    int64_t flow_bs;                               // elements between images
    const uint8_t* mask;                           // [*,H,W] bytes or nullptr (all True)
    int64_t mask_bs;
    const void* img; const void* other;            // [*,C,H,W] fp32 or uint8: the frame on the flow's grid, the frame it points into
    int64_t img_bs, other_bs;
    int64_t hw;
    int32_t chan, h, w, nblk;
    float flow_sign, eps;
    float wm1, hm1, half_wm1, half_hm1;
    double* partial;                               // [n][nblk][kRec] or nullptr (no record wanted)
    float* map;                                    // [n][H*W] or nullptr
    double* out;                                   // [n][kRec]
    const float* scale;                            // backward: [n]
    float* grad;                                   // backward: [n][2][H*W]
};

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

// one sample of an image plane: a uint8 sample s is float(s) / 255.0f
template <bool U8>
__device__ __forceinline__ float ld_img(const void* base, int64_t i) {
    return U8 ? (float)reinterpret_cast<const uint8_t*>(base)[i] / 255.0f : reinterpret_cast<const float*>(base)[i];
}

// correctly rounded fp32 square root (ofl_metrics.hip)
__device__ __forceinline__ float sqrt_rn(float s) { return __builtin_sqrtf(s); }

// the four taps of the sample of pixel (x, y) whose vector is (u, v): the head of warp_bwd_kernel (ofl_kernels.hip)
struct Taps {
    float sx, sy, x_w, y_n;                        // the position and its floors
    float nw, ne, sw, se;                          // fp32 weights
    int64_t o_nw, o_ne, o_sw, o_se;                // offsets in a plane, clamped into it
    bool k_nw, k_ne, k_sw, k_se;                   // inside the frame
    float mr;                                      // weight sum of the taps inside
};

__device__ __forceinline__ Taps taps_of(const PhotoParams& p, int x, int y, float u, float v) {
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

template <bool HALF, bool U8, bool BWD>
__global__ void __launch_bounds__(kThreads) flow_photometric_kernel(PhotoParams p) {
    const int64_t n_img = blockIdx.y;
    const int64_t fo = n_img * p.flow_bs;
    const uint8_t* mk = p.mask ? p.mask + n_img * p.mask_bs : nullptr;
    const int64_t io = n_img * p.img_bs, oo = n_img * p.other_bs;
    const float ee = p.eps * p.eps;
    const float fc = (float)p.chan;
    // the pixel of this lane and the step to its next round, kept as (x, y) so that no round divides
    const uint32_t stride = gridDim.x * (uint32_t)kThreads;
    const int step_y = (int)(stride / (uint32_t)p.w), step_x = (int)(stride % (uint32_t)p.w);
    int64_t pix = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    int y = (int)((uint32_t)pix / (uint32_t)p.w), x = (int)((uint32_t)pix - (uint32_t)y * (uint32_t)p.w);      // (h * w < 2^31)
    uint32_t count = 0u;
    double sum = 0.0;
    float mx = 0.0f;
    double sc = 0.0, ee64 = 0.0;
    if constexpr (BWD) {
        sc = (double)p.scale[n_img] * (double)(-p.flow_sign);
        ee64 = (double)p.eps * (double)p.eps;
    }
    for (; pix < p.hw; pix += stride) {
        const float u = ld_flow<HALF>(p.flow, fo + pix), v = ld_flow<HALF>(p.flow, fo + p.hw + pix);
        const bool valid = mk == nullptr || mk[pix] != 0;
        const Taps t = taps_of(p, x, y, u, v);
        const bool known = (t.mr > kValidThr) && valid;
        if constexpr (!BWD) {
            float s = 0.0f;
            for (int c = 0; c < p.chan; ++c) {
                const int64_t pl = oo + (int64_t)c * p.hw;
                const float v_nw = t.k_nw ? ld_img<U8>(p.other, pl + t.o_nw) : 0.0f;
                const float v_ne = t.k_ne ? ld_img<U8>(p.other, pl + t.o_ne) : 0.0f;
                const float v_sw = t.k_sw ? ld_img<U8>(p.other, pl + t.o_sw) : 0.0f;
                const float v_se = t.k_se ? ld_img<U8>(p.other, pl + t.o_se) : 0.0f;
                float iw = v_nw * t.nw;
                iw = __builtin_fmaf(v_ne, t.ne, iw);
                iw = __builtin_fmaf(v_sw, t.sw, iw);
                iw = __builtin_fmaf(v_se, t.se, iw);
                const float d = iw - ld_img<U8>(p.img, io + (int64_t)c * p.hw + pix);
                s = s + sqrt_rn(d * d + ee);
            }
            const float rho = known ? s / fc : 0.0f;
            if (p.map != nullptr) p.map[n_img * p.hw + pix] = rho;
            count += known ? 1u : 0u;
            sum += (double)rho;
            mx = (known && rho > mx) ? rho : mx;
        } else {
            // float64 fractions of the float32 position (tests/grad_oracle64.py, Taps.dx / Taps.dy)
            const double ww = (double)t.sx - (double)t.x_w, e = 1.0 - ww;
            const double nn = (double)t.sy - (double)t.y_n, s = 1.0 - nn;
            double ax = 0.0, ay = 0.0;
            for (int c = 0; c < p.chan; ++c) {
                const int64_t pl = oo + (int64_t)c * p.hw;
                const float v_nw = t.k_nw ? ld_img<U8>(p.other, pl + t.o_nw) : 0.0f;
                const float v_ne = t.k_ne ? ld_img<U8>(p.other, pl + t.o_ne) : 0.0f;
                const float v_sw = t.k_sw ? ld_img<U8>(p.other, pl + t.o_sw) : 0.0f;
                const float v_se = t.k_se ? ld_img<U8>(p.other, pl + t.o_se) : 0.0f;
                float iw = v_nw * t.nw;
                iw = __builtin_fmaf(v_ne, t.ne, iw);
                iw = __builtin_fmaf(v_sw, t.sw, iw);
                iw = __builtin_fmaf(v_se, t.se, iw);
                const float d = iw - ld_img<U8>(p.img, io + (int64_t)c * p.hw + pix);
                const double dd = (double)d;
                const double den = sqrt(dd * dd + ee64);
                const double q = den != 0.0 ? dd / den : 0.0;
                // west taps -1, east taps +1 (north -1, south +1), each times the other axis's weight; a tap outside the frame is 0
                const double gx = (((-s) * (double)v_nw + s * (double)v_ne) - nn * (double)v_sw) + nn * (double)v_se;
                const double gy = (((-e) * (double)v_nw - ww * (double)v_ne) + e * (double)v_sw) + ww * (double)v_se;
                ax = c == 0 ? q * gx : ax + q * gx;
                ay = c == 0 ? q * gy : ay + q * gy;
            }
            float* go = p.grad + n_img * 2 * p.hw + pix;
            go[0] = known ? (float)(sc * (ax / (double)fc)) : 0.0f;
            go[p.hw] = known ? (float)(sc * (ay / (double)fc)) : 0.0f;
        }
        x += step_x; y += step_y;
        if (x >= p.w) { x -= p.w; ++y; }
    }
    if constexpr (!BWD) {
        if (p.partial == nullptr) return;          // (the same for every thread of the launch)
        // lanes: butterfly (every lane ends with the wave's value); waves: added in index order by the first threads
        __shared__ double s_red[kWaves * kRec];
        double rec[kRec];
#pragma unroll
        for (int i = 0; i < kRec; ++i) rec[i] = 0.0;
        rec[R_COUNT] = (double)count; rec[R_SUM] = sum; rec[R_MAX] = (double)mx;
#pragma unroll
        for (int i = 0; i < R_USED; ++i) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const double o = __shfl_xor(rec[i], off);
                rec[i] = (i == R_MAX) ? fmax(rec[i], o) : rec[i] + o;
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
                s = (threadIdx.x == R_MAX) ? fmax(s, o) : s + o;
            }
            p.partial[(n_img * p.nblk + blockIdx.x) * kRec + threadIdx.x] = s;
        }
    }
}

// one block per image: the block records staged in LDS by all threads (independent loads), then slot i added in
// ascending block order by thread i
__global__ void __launch_bounds__(kThreads) flow_photometric_finish_kernel(PhotoParams p) {
    __shared__ double s_part[kMaxBlocks * kRec];
    const int64_t n_img = blockIdx.x;
    const double* part = p.partial + n_img * p.nblk * kRec;
    for (int i = threadIdx.x; i < p.nblk * kRec; i += kThreads) s_part[i] = part[i];
    __syncthreads();
    if (threadIdx.x >= kRec) return;
    double s = 0.0;
    for (int b = 0; b < p.nblk; ++b) {
        const double o = s_part[b * kRec + threadIdx.x];
        s = (threadIdx.x == R_MAX) ? fmax(s, o) : s + o;
    }
    p.out[n_img * kRec + threadIdx.x] = s;
}

bool dims_ok(int32_t n, int32_t h, int32_t w) {
    return n >= 1 && n <= 65535 && h >= 2 && w >= 2 && (int64_t)h * w < (1ll << 31);
}

bool aligned(const void* ptr, int a) { return ((uintptr_t)ptr % (uintptr_t)a) == 0; }

int64_t blocks_of(int64_t hw, int cap) {
    const int64_t b = (hw + kThreads - 1) / kThreads;
    return b < cap ? b : cap;
}

// the operands and the checks both entry points share
int fill_operands(PhotoParams* p, const void* flow, int64_t flow_bs, int32_t flow_half, const uint8_t* mask, int64_t mask_bs,
                  const void* img, int64_t img_bs, const void* other, int64_t other_bs, int32_t channels, int32_t img_u8, float flow_sign,
                  float eps, int32_t n, int32_t h, int32_t w) {
    if (!dims_ok(n, h, w)) return OFL_E_ARG;
    if (flow_sign != 1.0f && flow_sign != -1.0f) return OFL_E_ARG;
    if (channels < 1 || channels > kMaxChan) return OFL_E_ARG;
    if (!(eps >= 0.0f) || isinf(eps)) return OFL_E_ARG;                                            // (NaN fails the first test)
    if (flow == nullptr || img == nullptr || other == nullptr) return OFL_E_ARG;
    if ((flow_half != 0 && flow_half != 1) || (img_u8 != 0 && img_u8 != 1)) return OFL_E_ARG;
    if (flow_bs < 0 || mask_bs < 0 || img_bs < 0 || other_bs < 0) return OFL_E_ARG;
    if (!aligned(flow, flow_half ? 2 : 4) || !aligned(img, img_u8 ? 1 : 4) || !aligned(other, img_u8 ? 1 : 4)) return OFL_E_ARG;
    p->flow = flow; p->flow_bs = flow_bs;
    p->mask = mask; p->mask_bs = mask_bs;
    p->img = img; p->other = other; p->img_bs = img_bs; p->other_bs = other_bs;
    p->hw = (int64_t)h * w;
    p->chan = channels; p->h = h; p->w = w; p->nblk = 0;
    p->flow_sign = flow_sign; p->eps = eps;
    p->wm1 = (float)(w - 1); p->hm1 = (float)(h - 1);
    p->half_wm1 = p->wm1 / 2.0f; p->half_hm1 = p->hm1 / 2.0f;
    p->partial = nullptr; p->map = nullptr; p->out = nullptr; p->scale = nullptr; p->grad = nullptr;
    return OFL_OK;
}

template <bool BWD>
void launch(const PhotoParams& p, bool half, bool u8, dim3 grid, hipStream_t s) {
    if (half) {
        if (u8) OFL_KLAUNCH((flow_photometric_kernel<true, true, BWD>), grid, dim3(kThreads), 0, s, p);
        else OFL_KLAUNCH((flow_photometric_kernel<true, false, BWD>), grid, dim3(kThreads), 0, s, p);
    } else {
        if (u8) OFL_KLAUNCH((flow_photometric_kernel<false, true, BWD>), grid, dim3(kThreads), 0, s, p);
        else OFL_KLAUNCH((flow_photometric_kernel<false, false, BWD>), grid, dim3(kThreads), 0, s, p);
    }
}

}  // namespace

extern "C" {

__attribute__((visibility("default"))) int64_t ofl_flow_photometric_workspace_bytes(int32_t n, int32_t h, int32_t w) {
    if (!dims_ok(n, h, w)) return OFL_E_ARG;
    return (int64_t)n * blocks_of((int64_t)h * w, kMaxBlocks) * kRec * (int64_t)sizeof(double);
}

__attribute__((visibility("default"))) int ofl_flow_photometric_f64(const void* flow, int64_t flow_bs, int32_t flow_half, const uint8_t* mask,
                                                                    int64_t mask_bs, const void* img, int64_t img_bs, const void* other,
                                                                    int64_t other_bs, int32_t channels, int32_t img_u8, float flow_sign,
                                                                    float eps, void* workspace, float* photometric_map, double* records,
                                                                    int32_t n, int32_t h, int32_t w, void* stream) {
    PhotoParams p;
    const int rc = fill_operands(&p, flow, flow_bs, flow_half, mask, mask_bs, img, img_bs, other, other_bs, channels, img_u8, flow_sign, eps,
                                 n, h, w);
    if (rc) return rc;
    if (!photometric_map && !records) return OFL_E_ARG;
    if (records && !workspace) return OFL_E_ARG;
    if (!aligned(workspace, 8) || !aligned(records, 8) || !aligned(photometric_map, 4)) return OFL_E_ARG;
    p.nblk = (int32_t)blocks_of(p.hw, kMaxBlocks);
    p.partial = records ? reinterpret_cast<double*>(workspace) : nullptr;
    p.map = photometric_map;
    p.out = records;
    hipStream_t s = (hipStream_t)stream;
    launch<false>(p, flow_half != 0, img_u8 != 0, dim3((unsigned)p.nblk, (unsigned)n), s);
    if (records) OFL_KLAUNCH(flow_photometric_finish_kernel, dim3((unsigned)n), dim3(kThreads), 0, s, p);
    return (int)hipGetLastError();
}

__attribute__((visibility("default"))) int ofl_flow_photometric_grad_f32(const void* flow, int64_t flow_bs, int32_t flow_half,
                                                                         const uint8_t* mask, int64_t mask_bs, const void* img,
                                                                         int64_t img_bs, const void* other, int64_t other_bs,
                                                                         int32_t channels, int32_t img_u8, float flow_sign, float eps,
                                                                         const float* scale, float* grad, int32_t n, int32_t h, int32_t w,
                                                                         void* stream) {
    PhotoParams p;
    const int rc = fill_operands(&p, flow, flow_bs, flow_half, mask, mask_bs, img, img_bs, other, other_bs, channels, img_u8, flow_sign, eps,
                                 n, h, w);
    if (rc) return rc;
    if (!scale || !grad || !aligned(scale, 4) || !aligned(grad, 4)) return OFL_E_ARG;
    p.scale = scale; p.grad = grad;
    hipStream_t s = (hipStream_t)stream;
    launch<true>(p, flow_half != 0, img_u8 != 0, dim3((unsigned)blocks_of(p.hw, kMaxGradBlocks), (unsigned)n), s);
    return (int)hipGetLastError();
}

}  // extern "C"
