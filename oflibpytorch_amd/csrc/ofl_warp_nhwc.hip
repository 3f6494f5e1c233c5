// ofl_warp_nhwc.hip -- the backward bilinear warp of a feature tensor stored N-H-W-C (torch.channels_last), for Flow.apply / apply_flow 't'
// (ofl_warp_bwd_nhwc).  In this layout the four taps of a destination pixel are four runs of C contiguous elements and
// the destination is one streaming store, so nothing is staged in LDS: the work is flattened to items (pixel, chunk) of one image, a lane
// owns one item = 16 bytes of consecutive channels (4 fp32, 8 or 4 16-bit elements), and item i of image n is stored at byte 16 * i of
// that image (8 * i with 4 16-bit elements) -- a wave's store is one contiguous run, its tap loads are contiguous across the lanes that
// share a pixel.  Those lanes read the same flow vector and recompute the same weights; the lane of chunk 0 writes the `valid` byte.
// Re-use of a source pixel by neighbouring destination pixels is left to the caches (blocks of one label b % 8 -- one XCD, one L2 --
// walk one contiguous band of the image's rows).
//
// Arithmetic: that of ofl_warp_bwd_f32 (warp_bwd_kernel of ofl_kernels.hip, oracle/ofl_oracle.c orc_warp_bwd_f32) in the same order --
// p = g - sign * flow, normalise / un-normalise, floor, four weights, one product and three explicit FMAs; in-bounds tests on floats
// before any integer cast; a tap outside the frame is not loaded and counts as 0.  16-bit elements are up-converted at the load (exact)
// and rounded once, to nearest even, at the store, as ofl_warp_bwd_x16 does.  No atomics: every output is bitwise reproducible.
// C ABI: include/oflib_hip.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "oflib_hip.h"

#pragma clang fp contract(off)

// the launch recorder of ofl_kernels.hip (ofl_last_kernel_name)
extern const void* g_ofl_last_kernel;
#define OFL_KLAUNCH(K, ...) do { g_ofl_last_kernel = (const void*)(K); hipLaunchKernelGGL(K, __VA_ARGS__); } while (0)

namespace {

constexpr int kThreads = 256;
constexpr float kValidThr = 0.99999f;  // flow_class.py:922

struct NhwcParams {
    const float* flow; int64_t flow_bs;                  // [*, 2, H, W] fp32 planes
    const void* src; int64_t src_bs;                     // [*, H, W, C] elements of the kernel's type; batch strides in elements
    const uint8_t* src_mask; int64_t src_mask_bs;        // [*, H, W] or nullptr
    const uint8_t* flow_mask; int64_t flow_mask_bs;
    void* dst; uint8_t* valid;                           // [N, H, W, C]; [N, H, W] or nullptr
    int32_t c, h, w, cq;                                 // cq: chunks (lanes) per pixel
    uint32_t items, blocks, per_label;                   // items = H * W * cq of ONE image, in blocks of kThreads; blocks per label b % 8
    uint32_t cq_m, cq_s, w_m, w_s;                       // magic divisors by cq and by w
    float flow_sign, wm1, hm1, half_wm1, half_hm1;
};

// storage types of the 16-bit instantiations, under names every demangler prints (as in ofl_kernels.hip)
struct half_t { _Float16 v; };
struct bf16_t { uint16_t bits; };

// exact u32 division by an invariant divisor: q = (((n - t) >> s1) + t) >> s2 with t = umulhi(m, n); s = (s1 << 16) | s2
__device__ __forceinline__ uint32_t fastdiv(uint32_t n, uint32_t m, uint32_t s) {
    const uint32_t t = __umulhi(m, n);
    return (((n - t) >> (s >> 16)) + t) >> (s & 0xffffu);
}

__device__ __forceinline__ float unnormalise(float p, float size_m1, float half_size_m1) {
    // normalise_coords (utils.py:462-465) followed by the grid sampler's align_corners un-normalise
    float g = p * 2.0f;
    g = g / size_m1;  // IEEE correctly-rounded divide (no fast-math)
    g = g - 1.0f;
    return (g + 1.0f) * half_size_m1;
}

// one lane's V consecutive channels <-> floats: one access of V * sizeof(T) bytes, aligned as the entry point checked (16 bytes for
// fp32, 8 bytes for 16-bit elements: a lane of 8 such elements makes a 16-byte access at 8-byte alignment, which gfx950 serves as one)
template <typename T, int V> struct Lane;
template <> struct Lane<float, 4> {
    typedef float vec __attribute__((ext_vector_type(4), aligned(16)));
    static __device__ __forceinline__ void load(const float* p, float (&o)[4]) {
        const vec v = *reinterpret_cast<const vec*>(p);
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = v[k];
    }
    static __device__ __forceinline__ void store(float* p, const float (&o)[4]) {
        const vec v = {o[0], o[1], o[2], o[3]};
        __builtin_nontemporal_store(v, reinterpret_cast<vec*>(p));   // written once, never read here: streams past the taps' lines
    }
};
template <int V> struct Lane<half_t, V> {
    typedef _Float16 vec __attribute__((ext_vector_type(V), aligned(8)));
    static __device__ __forceinline__ void load(const half_t* p, float (&o)[V]) {
        const vec v = *reinterpret_cast<const vec*>(p);
#pragma unroll
        for (int k = 0; k < V; ++k) o[k] = (float)v[k];
    }
    static __device__ __forceinline__ void store(half_t* p, const float (&o)[V]) {
        vec v;
#pragma unroll
        for (int k = 0; k < V; ++k) v[k] = (_Float16)o[k];
        __builtin_nontemporal_store(v, reinterpret_cast<vec*>(p));
    }
};
// a bf16 value is the upper half of the fp32 with the same value; the store is the compiler's float -> __bf16 conversion (to nearest
// even, NaN to a quiet NaN: what `Tensor.to(torch.bfloat16)` gives, and what ofl_warp_bwd_x16 stores)
template <int V> struct Lane<bf16_t, V> {
    typedef uint16_t vec __attribute__((ext_vector_type(V), aligned(8)));
    static __device__ __forceinline__ void load(const bf16_t* p, float (&o)[V]) {
        const vec v = *reinterpret_cast<const vec*>(p);
#pragma unroll
        for (int k = 0; k < V; ++k) o[k] = __builtin_bit_cast(float, (uint32_t)v[k] << 16);
    }
    static __device__ __forceinline__ void store(bf16_t* p, const float (&o)[V]) {
        vec v;
#pragma unroll
        for (int k = 0; k < V; ++k) v[k] = __builtin_bit_cast(uint16_t, (__bf16)o[k]);
        __builtin_nontemporal_store(v, reinterpret_cast<vec*>(p));
    }
};

// T: storage type; V: channels per lane; VALID: the valid mask is wanted.  grid (blocks of one image, N)
template <typename T, int V, bool VALID>
__global__ __launch_bounds__(kThreads) void warp_bwd_nhwc_kernel(const NhwcParams p) {
    // hardware deals blocks round-robin over the 8 XCDs: blocks of one label b % 8 take one contiguous range of the image's items (speed only)
    const uint32_t b = blockIdx.x;
    const uint32_t lb = (b & 7u) * p.per_label + (b >> 3);
    if (lb >= p.blocks) return;
    const uint32_t item = lb * (uint32_t)kThreads + threadIdx.x;     // (items <= 2^32 - kThreads: no wrap)
    if (item >= p.items) return;
    const uint32_t pix = fastdiv(item, p.cq_m, p.cq_s);              // < H * W < 2^31
    const uint32_t chunk = item - pix * (uint32_t)p.cq;
    const uint32_t yy = fastdiv(pix, p.w_m, p.w_s);
    const int x = (int)(pix - yy * (uint32_t)p.w), y = (int)yy;
    const int w = p.w, h = p.h;
    const int64_t n = blockIdx.y;
    const int64_t hw = (int64_t)h * w;

    const float* __restrict__ fu = p.flow + n * p.flow_bs;
    const T* __restrict__ sb = static_cast<const T*>(p.src) + n * p.src_bs + (int64_t)chunk * V;
    const float u = fu[pix], v = fu[hw + pix];

    // sample position: grid - flow (utils.py:549), flow_sign = -1 restates Flow(-vecs)
    const float px = (float)x - p.flow_sign * u;
    const float py = (float)y - p.flow_sign * v;
    const float sx = unnormalise(px, p.wm1, p.half_wm1);
    const float sy = unnormalise(py, p.hm1, p.half_hm1);
    const float x_w = floorf(sx), y_n = floorf(sy);
    const float ww = sx - x_w, e = 1.0f - ww;
    const float nn = sy - y_n, s = 1.0f - nn;
    const float nw = s * e, ne = s * ww, sw = nn * e, se = nn * ww;
    const float x_e = x_w + 1.0f, y_s = y_n + 1.0f;
    // in-bounds tests in float: huge coordinates never reach an integer cast
    const bool x0ok = (x_w > -1.0f) && (x_w < (float)w);
    const bool x1ok = (x_e > -1.0f) && (x_e < (float)w);
    const bool y0ok = (y_n > -1.0f) && (y_n < (float)h);
    const bool y1ok = (y_s > -1.0f) && (y_s < (float)h);
    const int ix0 = x0ok ? (int)x_w : 0, ix1 = x1ok ? (int)x_e : 0;
    const int iy0 = y0ok ? (int)y_n : 0, iy1 = y1ok ? (int)y_s : 0;
    const int64_t o_nw = (int64_t)iy0 * w + ix0, o_ne = (int64_t)iy0 * w + ix1;     // pixel offsets, always inside the frame
    const int64_t o_sw = (int64_t)iy1 * w + ix0, o_se = (int64_t)iy1 * w + ix1;
    const bool k_nw = x0ok && y0ok, k_ne = x1ok && y0ok, k_sw = x0ok && y1ok, k_se = x1ok && y1ok;

    float v_nw[V], v_ne[V], v_sw[V], v_se[V];
#pragma unroll
    for (int k = 0; k < V; ++k) v_nw[k] = v_ne[k] = v_sw[k] = v_se[k] = 0.0f;
    if (k_nw) Lane<T, V>::load(sb + o_nw * p.c, v_nw);
    if (k_ne) Lane<T, V>::load(sb + o_ne * p.c, v_ne);
    if (k_sw) Lane<T, V>::load(sb + o_sw * p.c, v_sw);
    if (k_se) Lane<T, V>::load(sb + o_se * p.c, v_se);

    if (VALID) {
        if (chunk == 0) {
            const uint8_t* __restrict__ sm = p.src_mask ? p.src_mask + n * p.src_mask_bs : nullptr;
            const bool fmv = p.flow_mask ? (p.flow_mask[n * p.flow_mask_bs + pix] != 0) : true;
            float m_nw, m_ne, m_sw, m_se;
            if (sm) {
                m_nw = k_nw ? (float)(sm[o_nw] != 0) : 0.0f;
                m_ne = k_ne ? (float)(sm[o_ne] != 0) : 0.0f;
                m_sw = k_sw ? (float)(sm[o_sw] != 0) : 0.0f;
                m_se = k_se ? (float)(sm[o_se] != 0) : 0.0f;
            } else {
                m_nw = k_nw ? 1.0f : 0.0f; m_ne = k_ne ? 1.0f : 0.0f;
                m_sw = k_sw ? 1.0f : 0.0f; m_se = k_se ? 1.0f : 0.0f;
            }
            float mr = m_nw * nw;
            mr = __builtin_fmaf(m_ne, ne, mr);
            mr = __builtin_fmaf(m_sw, sw, mr);
            mr = __builtin_fmaf(m_se, se, mr);
            p.valid[n * hw + pix] = (uint8_t)((mr > kValidThr) && fmv);
        }
    }

    float out[V];
#pragma unroll
    for (int k = 0; k < V; ++k) {
        float rr = v_nw[k] * nw;
        rr = __builtin_fmaf(v_ne[k], ne, rr);
        rr = __builtin_fmaf(v_sw[k], sw, rr);
        rr = __builtin_fmaf(v_se[k], se, rr);
        out[k] = rr;
    }
    // item i of image n is elements [V * i, V * i + V) of that image
    Lane<T, V>::store(static_cast<T*>(p.dst) + (n * (int64_t)p.items + item) * V, out);
}

inline void magic_u32(uint32_t d, uint32_t& m, uint32_t& s) {   // d >= 1; see fastdiv()
    uint32_t l = 0;
    while ((1ull << l) < d) ++l;
    m = (uint32_t)(((1ull << 32) * ((1ull << l) - d)) / d + 1);
    s = ((l ? 1u : 0u) << 16) | (l ? l - 1 : 0);
}

template <typename T, int V>
int nhwc_launch(NhwcParams& p, int32_t n, hipStream_t st) {
    p.cq = p.c / V;
    p.items = (uint32_t)((int64_t)p.h * p.w * p.cq);
    p.blocks = (p.items + kThreads - 1) / kThreads;
    p.per_label = (p.blocks + 7) / 8;
    magic_u32((uint32_t)p.cq, p.cq_m, p.cq_s);
    magic_u32((uint32_t)p.w, p.w_m, p.w_s);
    const dim3 grid(p.per_label * 8, (unsigned)n);
    if (p.valid) OFL_KLAUNCH((warp_bwd_nhwc_kernel<T, V, true>), grid, dim3(kThreads), 0, st, p);
    else OFL_KLAUNCH((warp_bwd_nhwc_kernel<T, V, false>), grid, dim3(kThreads), 0, st, p);
    return (int)hipGetLastError();
}

// ---- ofl_warp_bwd_grad_nhwc: the gradient of that warp with respect to its FLOW, from the saved source and the upstream gradient as stored ----
// One pixel per lane; the channels of the pixel and of each of its four taps are contiguous runs, walked in chunks of V (one 16-byte load of
// the upstream gradient and up to four of the taps per chunk).  The sums are warp_grad_kernel's (ofl_aux_kernels.hip): ONE chain per pixel
// over the channels 0 .. C-1, the eight updates per channel in that kernel's order and association, then the same chain rule -- so the
// result is bit-identical to the planar routes' (warp_grad_kernel, warp_grad_flow_x16_kernel, the staged GRAD kernels).  No LDS, no atomics.
struct NhwcGradParams {
    const float* flow; int64_t flow_bs;                  // [*, 2, H, W] fp32 planes
    const void* src; int64_t src_bs;                     // [*, H, W, C]
    const void* gout;                                    // [N, H, W, C]
    float* gflow;                                        // [N, 2, H, W] fp32 planes
    int32_t c, h, w;
    float flow_sign, g_scale, wm1, hm1, half_wm1, half_hm1;
};

template <typename T, int V>
__global__ __launch_bounds__(kThreads) void warp_grad_flow_nhwc_kernel(const NhwcGradParams p) {
    const int w = p.w, h = p.h;
    const int64_t hw = (int64_t)h * w;
    const int64_t pix = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (pix >= hw) return;
    const int64_t n = blockIdx.y;
    const int y = (int)(pix / w), x = (int)(pix - (int64_t)y * w);
    const float* __restrict__ fu = p.flow + n * p.flow_bs;
    const T* __restrict__ sb = static_cast<const T*>(p.src) + n * p.src_bs;
    const T* __restrict__ gp = static_cast<const T*>(p.gout) + (n * hw + pix) * p.c;

    const float sx = unnormalise((float)x - p.flow_sign * fu[pix], p.wm1, p.half_wm1);
    const float sy = unnormalise((float)y - p.flow_sign * fu[hw + pix], p.hm1, p.half_hm1);
    // the four taps: fractions, validity, offsets clamped into the frame (make_taps of ofl_aux_kernels.hip)
    const float x_w = floorf(sx), y_n = floorf(sy), x_e = x_w + 1.0f, y_s = y_n + 1.0f;
    const float ww = sx - x_w, e = 1.0f - ww, nn = sy - y_n, s = 1.0f - nn;
    const bool x0ok = (x_w > -1.0f) && (x_w < (float)w), x1ok = (x_e > -1.0f) && (x_e < (float)w);
    const bool y0ok = (y_n > -1.0f) && (y_n < (float)h), y1ok = (y_s > -1.0f) && (y_s < (float)h);
    const int ix0 = x0ok ? (int)x_w : 0, ix1 = x1ok ? (int)x_e : 0, iy0 = y0ok ? (int)y_n : 0, iy1 = y1ok ? (int)y_s : 0;
    const T* __restrict__ t_nw = sb + ((int64_t)iy0 * w + ix0) * p.c;
    const T* __restrict__ t_ne = sb + ((int64_t)iy0 * w + ix1) * p.c;
    const T* __restrict__ t_sw = sb + ((int64_t)iy1 * w + ix0) * p.c;
    const T* __restrict__ t_se = sb + ((int64_t)iy1 * w + ix1) * p.c;
    const bool k_nw = x0ok && y0ok, k_ne = x1ok && y0ok, k_sw = x0ok && y1ok, k_se = x1ok && y1ok;

    float gix = 0.0f, giy = 0.0f;
    for (int c0 = 0; c0 < p.c; c0 += V) {
        float gv[V], v_nw[V], v_ne[V], v_sw[V], v_se[V];
#pragma unroll
        for (int k = 0; k < V; ++k) v_nw[k] = v_ne[k] = v_sw[k] = v_se[k] = 0.0f;
        Lane<T, V>::load(gp + c0, gv);
        if (k_nw) Lane<T, V>::load(t_nw + c0, v_nw);
        if (k_ne) Lane<T, V>::load(t_ne + c0, v_ne);
        if (k_sw) Lane<T, V>::load(t_sw + c0, v_sw);
        if (k_se) Lane<T, V>::load(t_se + c0, v_se);
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const float g = p.g_scale * gv[k];
            gix -= v_nw[k] * s * g; gix += v_ne[k] * s * g; gix -= v_sw[k] * nn * g; gix += v_se[k] * nn * g;
            giy -= v_nw[k] * e * g; giy -= v_ne[k] * ww * g; giy += v_sw[k] * e * g; giy += v_se[k] * ww * g;
        }
    }
    float* __restrict__ gf = p.gflow + n * 2 * hw;
    // grad of the grid (x half_size), of normalise_coords (/ size_m1, * 2), of `grid - flow` (negation)
    gf[pix] = -p.flow_sign * (((gix * p.half_wm1) / p.wm1) * 2.0f);
    gf[hw + pix] = -p.flow_sign * (((giy * p.half_hm1) / p.hm1) * 2.0f);
}

template <typename T, int V>
int nhwc_grad_launch(const NhwcGradParams& p, int32_t n, hipStream_t st) {
    const int64_t hw = (int64_t)p.h * p.w;
    const dim3 grid((unsigned)((hw + kThreads - 1) / kThreads), (unsigned)n);
    OFL_KLAUNCH((warp_grad_flow_nhwc_kernel<T, V>), grid, dim3(kThreads), 0, st, p);
    return (int)hipGetLastError();
}

// ---- ofl_nhwc_to_planes / ofl_planes_to_nhwc: bit copies between [N, H, W, C] and [N, C, H, W] through an LDS tile ----
// A block moves a tile of TP pixels x TC channels of one image (TC elements = 128 bytes of a pixel: whole cache lines on the N-H-W-C
// side).  LDS holds it channel-major, tile[ch][px] with a pitch of TP + 1 elements.  N-H-W-C side: item i of the tile is V consecutive
// channels (one 16-byte access, 8 bytes with 4 16-bit elements) of pixel i / (TC / V), so the lanes of a pixel cover its 128 bytes and
// consecutive pixels follow; its V elements go to / come from V rows of the tile at one column -- with the odd pitch the 32 lanes of an
// LDS group (TC / V chunks x a few pixels) fall on distinct banks with 4-byte elements and at worst two to a bank with 2-byte ones.
// Plane side: consecutive lanes take consecutive pixels of one channel (coalesced; element-sized accesses, as a plane's base is only
// element-aligned when H * W is odd), consecutive columns of one tile row in LDS.  Tiles at the end of the pixels or of the channels
// are cut by the bounds tests; C is a multiple of V, so a chunk is inside or outside as a whole.
template <typename E> struct TileShape;
template <> struct TileShape<uint32_t> { static constexpr int TP = 64, TC = 32; };
template <> struct TileShape<uint16_t> { static constexpr int TP = 128, TC = 64; };

template <typename E, int V> struct EVec {
    typedef E vec __attribute__((ext_vector_type(V), aligned(sizeof(E) == 4 ? 16 : 8)));
};

struct TransposeParams {
    const void* src; void* dst;
    int64_t hw; int32_t c;
};

// TO_PLANES: src [N, H*W, C] -> dst [N, C, H*W]; else src [N, C, H*W] -> dst [N, H*W, C].  grid (pixel tiles, channel tiles, N)
template <typename E, int V, bool TO_PLANES>
__global__ __launch_bounds__(kThreads) void nhwc_transpose_kernel(const TransposeParams p) {
    constexpr int TP = TileShape<E>::TP, TC = TileShape<E>::TC, PITCH = TP + 1, CPT = TC / V;
    typedef typename EVec<E, V>::vec vec;
    __shared__ E tile[TC * PITCH];
    const int64_t hw = p.hw, C = p.c;
    const int64_t p0 = (int64_t)blockIdx.x * TP;
    const int c0 = (int)blockIdx.y * TC;
    const int64_t img = (int64_t)blockIdx.z * hw * C;
    const E* __restrict__ src = static_cast<const E*>(p.src) + img;
    E* __restrict__ dst = static_cast<E*>(p.dst) + img;
    const int np = (int)(hw - p0 < TP ? hw - p0 : TP);       // pixels and channels of this tile
    const int nc = (int)(C - c0 < TC ? C - c0 : TC);
    if (TO_PLANES) {
#pragma unroll
        for (int i = threadIdx.x; i < TP * CPT; i += kThreads) {
            const int px = i / CPT, ch = (i % CPT) * V;
            if (px < np && ch < nc) {
                const vec v = *reinterpret_cast<const vec*>(src + (p0 + px) * C + c0 + ch);
#pragma unroll
                for (int k = 0; k < V; ++k) tile[(ch + k) * PITCH + px] = v[k];
            }
        }
        __syncthreads();
#pragma unroll 4
        for (int j = threadIdx.x; j < TP * TC; j += kThreads) {
            const int ch = j / TP, px = j % TP;
            if (px < np && ch < nc) dst[(int64_t)(c0 + ch) * hw + p0 + px] = tile[ch * PITCH + px];
        }
    } else {
#pragma unroll 4
        for (int j = threadIdx.x; j < TP * TC; j += kThreads) {
            const int ch = j / TP, px = j % TP;
            if (px < np && ch < nc) tile[ch * PITCH + px] = src[(int64_t)(c0 + ch) * hw + p0 + px];
        }
        __syncthreads();
#pragma unroll
        for (int i = threadIdx.x; i < TP * CPT; i += kThreads) {
            const int px = i / CPT, ch = (i % CPT) * V;
            if (px < np && ch < nc) {
                vec v;
#pragma unroll
                for (int k = 0; k < V; ++k) v[k] = tile[(ch + k) * PITCH + px];
                *reinterpret_cast<vec*>(dst + (p0 + px) * C + c0 + ch) = v;
            }
        }
    }
}

template <typename E, int V, bool TO_PLANES>
int transpose_launch(const TransposeParams& p, int32_t n, hipStream_t st) {
    constexpr int TP = TileShape<E>::TP, TC = TileShape<E>::TC;
    const dim3 grid((unsigned)((p.hw + TP - 1) / TP), (unsigned)((p.c + TC - 1) / TC), (unsigned)n);
    OFL_KLAUNCH((nhwc_transpose_kernel<E, V, TO_PLANES>), grid, dim3(kThreads), 0, st, p);
    return (int)hipGetLastError();
}

// `nhwc` is the operand stored [N, H, W, C] (the source of ofl_nhwc_to_planes, the destination of ofl_planes_to_nhwc)
template <bool TO_PLANES>
int transpose_entry(const void* src, void* dst, const void* nhwc, const void* planes, int32_t n, int32_t c, int32_t h, int32_t w,
                    int32_t elem_bytes, void* stream) {
    if (!src || !dst) return OFL_E_NULL;
    if (elem_bytes != 2 && elem_bytes != 4) return OFL_E_ARG;
    if (n < 0 || c < 0 || h < 0 || w < 0) return OFL_E_ARG;
    if (n < 1 || c < 1 || h < 1 || w < 1 || (int64_t)h * w >= (1ll << 31)) return OFL_E_SHAPE;
    if ((uintptr_t)planes & (uintptr_t)(elem_bytes - 1)) return OFL_E_ARG;
    if ((c & 3) != 0) return OFL_E_UNSUPPORTED;
    if ((uintptr_t)nhwc & (uintptr_t)(elem_bytes == 4 ? 15 : 7)) return OFL_E_UNSUPPORTED;
    if (n > 65535 || c > 65535 * 32) return OFL_E_UNSUPPORTED;                   // images and channel tiles on the grid's y and z axes
    const double bytes = (double)n * c * h * w * elem_bytes;                   // the two operands must not overlap
    const uintptr_t a = (uintptr_t)src, b = (uintptr_t)dst;
    if ((a <= b && (double)(b - a) < bytes) || (b < a && (double)(a - b) < bytes)) return OFL_E_ARG;
    TransposeParams p;
    p.src = src; p.dst = dst; p.hw = (int64_t)h * w; p.c = c;
    hipStream_t st = (hipStream_t)stream;
    if (elem_bytes == 4) return transpose_launch<uint32_t, 4, TO_PLANES>(p, n, st);
    return (c & 7) == 0 ? transpose_launch<uint16_t, 8, TO_PLANES>(p, n, st) : transpose_launch<uint16_t, 4, TO_PLANES>(p, n, st);
}

}  // namespace

extern "C" __attribute__((visibility("default"))) int ofl_warp_bwd_grad_nhwc(
    const float* flow, int64_t flow_bs, float flow_sign, const void* src, int64_t src_bs, const void* grad_out, float g_scale,
    float* grad_flow, int32_t n, int32_t c, int32_t h, int32_t w, int32_t dtype, void* stream) {
    if (!flow || !src || !grad_out || !grad_flow) return OFL_E_NULL;
    if (dtype != OFL_X16_HALF && dtype != OFL_X16_BFLOAT && dtype != OFL_NHWC_F32) return OFL_E_ARG;
    if (n < 0 || c < 0 || h < 0 || w < 0 || flow_bs < 0 || src_bs < 0) return OFL_E_ARG;
    if (!(flow_sign == 1.0f || flow_sign == -1.0f)) return OFL_E_ARG;
    if (n < 1 || c < 1 || h < 1 || w < 1 || (int64_t)h * w >= (1ll << 31)) return OFL_E_SHAPE;
    // whole chunks of 4 channels, a frame the normalisation is defined on (the divide by size - 1), operands aligned to the chunk's vector
    if (c < 4 || (c & 3) != 0 || h < 2 || w < 2) return OFL_E_UNSUPPORTED;
    const uintptr_t align = dtype == OFL_NHWC_F32 ? 16 : 8;
    if (((uintptr_t)src | (uintptr_t)grad_out) & (align - 1)) return OFL_E_UNSUPPORTED;
    if (n > 65535) return OFL_E_UNSUPPORTED;                                     // images on the grid's second axis
    NhwcGradParams p = {};
    p.flow = flow; p.flow_bs = flow_bs; p.src = src; p.src_bs = src_bs; p.gout = grad_out; p.gflow = grad_flow;
    p.c = c; p.h = h; p.w = w;
    p.flow_sign = flow_sign; p.g_scale = g_scale;
    p.wm1 = (float)(w - 1); p.hm1 = (float)(h - 1);
    p.half_wm1 = p.wm1 / 2.0f; p.half_hm1 = p.hm1 / 2.0f;
    hipStream_t st = (hipStream_t)stream;
    const bool v8 = dtype != OFL_NHWC_F32 && (c & 7) == 0;
    if (dtype == OFL_NHWC_F32) return nhwc_grad_launch<float, 4>(p, n, st);
    if (dtype == OFL_X16_HALF) return v8 ? nhwc_grad_launch<half_t, 8>(p, n, st) : nhwc_grad_launch<half_t, 4>(p, n, st);
    return v8 ? nhwc_grad_launch<bf16_t, 8>(p, n, st) : nhwc_grad_launch<bf16_t, 4>(p, n, st);
}

extern "C" __attribute__((visibility("default"))) int ofl_nhwc_to_planes(
    const void* src, void* dst, int32_t n, int32_t c, int32_t h, int32_t w, int32_t elem_bytes, void* stream) {
    return transpose_entry<true>(src, dst, src, dst, n, c, h, w, elem_bytes, stream);
}

extern "C" __attribute__((visibility("default"))) int ofl_planes_to_nhwc(
    const void* src, void* dst, int32_t n, int32_t c, int32_t h, int32_t w, int32_t elem_bytes, void* stream) {
    return transpose_entry<false>(src, dst, dst, src, n, c, h, w, elem_bytes, stream);
}

extern "C" __attribute__((visibility("default"))) int ofl_warp_bwd_nhwc(
    const float* flow, int64_t flow_bs, float flow_sign, const void* src, int64_t src_bs,
    const uint8_t* src_mask, int64_t src_mask_bs, const uint8_t* flow_mask, int64_t flow_mask_bs,
    void* dst, uint8_t* valid, int32_t n, int32_t c, int32_t h, int32_t w, int32_t dtype, void* stream) {
    if (!flow || !src || !dst) return OFL_E_NULL;
    if (dtype != OFL_X16_HALF && dtype != OFL_X16_BFLOAT && dtype != OFL_NHWC_F32) return OFL_E_ARG;
    if (n < 0 || c < 0 || h < 0 || w < 0 || flow_bs < 0 || src_bs < 0 || src_mask_bs < 0 || flow_mask_bs < 0) return OFL_E_ARG;
    if (!(flow_sign == 1.0f || flow_sign == -1.0f)) return OFL_E_ARG;
    if (n < 1 || c < 1 || h < 1 || w < 1 || (int64_t)h * w >= (1ll << 31)) return OFL_E_SHAPE;
    // whole lanes of 4 channels, a frame the normalisation is defined on (the divide by size - 1), operands aligned to the lane's vector
    if (c < 4 || (c & 3) != 0 || h < 2 || w < 2) return OFL_E_UNSUPPORTED;
    const uintptr_t align = dtype == OFL_NHWC_F32 ? 16 : 8;
    if (((uintptr_t)src | (uintptr_t)dst) & (align - 1)) return OFL_E_UNSUPPORTED;
    // 32-bit item numbers inside one image (64-bit element offsets everywhere), images on the grid's second axis
    const int v = (dtype != OFL_NHWC_F32 && (c & 7) == 0) ? 8 : 4;
    if ((int64_t)h * w * (c / v) > (int64_t)0xffffffffu - kThreads || n > 65535) return OFL_E_UNSUPPORTED;
    NhwcParams p = {};
    p.flow = flow; p.flow_bs = flow_bs; p.src = src; p.src_bs = src_bs;
    p.src_mask = src_mask; p.src_mask_bs = src_mask_bs; p.flow_mask = flow_mask; p.flow_mask_bs = flow_mask_bs;
    p.dst = dst; p.valid = valid;
    p.c = c; p.h = h; p.w = w;
    p.flow_sign = flow_sign;
    p.wm1 = (float)(w - 1); p.hm1 = (float)(h - 1);
    p.half_wm1 = p.wm1 / 2.0f; p.half_hm1 = p.hm1 / 2.0f;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == OFL_NHWC_F32) return nhwc_launch<float, 4>(p, n, st);
    if (dtype == OFL_X16_HALF) return v == 8 ? nhwc_launch<half_t, 8>(p, n, st) : nhwc_launch<half_t, 4>(p, n, st);
    return v == 8 ? nhwc_launch<bf16_t, 8>(p, n, st) : nhwc_launch<bf16_t, 4>(p, n, st);
}
