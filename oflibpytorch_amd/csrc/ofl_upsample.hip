// ofl_upsample.hip -- Flow.upsample_convex on gfx950: the learned convex upsampling that ends every refinement iteration of RAFT, GMA,
// CRAFT, SEA-RAFT, FlowFormer and RAFT-Stereo (which DEFINES the numbers; tests/upsample_convex_oracle.py is the same
// definition in NumPy).  An extension: the reference has no such function.
//
//   flow_upsample_convex_kernel<K, HALF>              one launch.  A wave owns 64 coarse pixels along x and ONE fine row K y + i of them,
//                                                     a block four fine rows: a wave's load of a logit plane is 256 contiguous bytes, and
//                                                     a lane holds the K results of its fine row in registers, so that the wave's store of
//                                                     a channel is 256 K contiguous bytes.  The 3 x 3 flow neighbourhood is read directly
//                                                     (18 loads a lane next to 9 K of logits; its neighbours' lanes share the lines).  The
//                                                     mask block is written by the same launch
//   flow_upsample_convex_grad_logits_kernel<K, HALF>  the backward's per-fine-pixel pass with the forward's layout: d logits (9 K planes a
//                                                     lane, each contiguous across the wave) and, for d flow, the maximum m and the sum s
//                                                     of the softmax of every fine pixel into a workspace [n][2][K H][K W] of float64
//   flow_upsample_convex_grad_flow_kernel<K>          d flow, a gather: one lane per coarse pixel q walks the taps t, the sub-rows i and
//                                                     the sub-columns j in ascending order with one float64 sum per channel; the weight
//                                                     of tap t at the neighbour q - delta_t is exp(l_t - m) / s from the workspace -- one
//                                                     exp per term instead of nine, and every logit is read once
//
// No float atomics and no scatter anywhere: every sum has one owner and a fixed order, the same bits on any run and in any batch.  The
// position arithmetic (taps_of) and the softmax (e_of, softmax_of) are shared by all kernels, so that they agree on every weight: the
// gather's exp(l_t - m) / s is the forward's expression on the forward's m and s.
//
// Every product is rounded, then every sum: fp contraction is off (ofl_loss_common.hpp).  C ABI: include/oflib_hip.h.
#include "ofl_loss_common.hpp"

namespace {

using namespace ofl_loss;

constexpr int kThreads = 256;
constexpr int kTileW = 64;                         // coarse pixels of a block along x: one per lane of a wave
constexpr int kTileH = 4;                          // FINE rows of a block: one per wave
constexpr int kTaps = 9;                           // tap t = 3 (dy + 1) + (dx + 1)

static_assert(kThreads == kTileW * kTileH && kTileW == 64, "a wave owns one fine row of 64 coarse pixels");

struct UpParams {
    const void* flow;                              // [*,2,H,W] fp32 or fp16
    int64_t flow_bs;                               // elements between images
    const uint8_t* mask;                           // [*,H,W] bytes or nullptr
    int64_t mask_bs;
    const float* logits;                           // [n][9 K^2][H W]
    float* out;                                    // forward: [n][2][K H][K W]
    uint8_t* out_mask;                             // forward: [n][K H][K W] or nullptr
    const float* g;                                // backward: the upstream gradient, laid out as `out`
    float* d_logits;                               // [n][9 K^2][H W] or nullptr
    double* ws;                                    // [n][2][K H][K W]: m, then s, of every fine pixel; or nullptr
    float* d_flow;                                 // [n][2][H W]
    int64_t hw;                                    // H W
    int32_t h, w, tiles_x;
};

// The 3 x 3 neighbourhood of coarse pixel (x, y): F[c][t] = K * (double)f_c(y + dy, x + dx), exact (K is a power of two); +0, selected and
// not loaded, where the neighbour lies outside the coarse frame
template <int K, bool HALF>
__device__ __forceinline__ void taps_of(const UpParams& p, int64_t n_img, int x, int y, double (&F)[2][kTaps]) {
    const int64_t fo = n_img * p.flow_bs;
#pragma unroll
    for (int t = 0; t < kTaps; ++t) {
        const int ny = y + t / 3 - 1, nx = x + t % 3 - 1;
        F[0][t] = 0.0; F[1][t] = 0.0;
        if (ny >= 0 && ny < p.h && nx >= 0 && nx < p.w) {
            const int64_t at = (int64_t)ny * p.w + nx;
            F[0][t] = (double)K * (double)ld_flow<HALF>(p.flow, fo + at);
            F[1][t] = (double)K * (double)ld_flow<HALF>(p.flow, fo + p.hw + at);
        }
    }
}

// e_t = exp((double)l_t - m) in float64
__device__ __forceinline__ double e_of(float l, double m) { return exp((double)l - m); }

// The softmax over the nine taps of one fine pixel: m by a running float32 compare, e_t, s = (((e_0 + e_1) + ...) + e_8), w_t = e_t / s
__device__ __forceinline__ void softmax_of(const float (&l)[kTaps], double (&wt)[kTaps], double& m_out, double& s_out) {
    float m = l[0];
#pragma unroll
    for (int t = 1; t < kTaps; ++t) m = (l[t] > m) ? l[t] : m;
    const double md = (double)m;
    double e[kTaps];
#pragma unroll
    for (int t = 0; t < kTaps; ++t) e[t] = e_of(l[t], md);
    double s = e[0] + e[1];
#pragma unroll
    for (int t = 2; t < kTaps; ++t) s = s + e[t];
#pragma unroll
    for (int t = 0; t < kTaps; ++t) wt[t] = e[t] / s;
    m_out = md; s_out = s;
}

// o_c = sum_t w_t * F_{c,t} from +0, t ascending, each product rounded, then the sum
__device__ __forceinline__ void mix_of(const double (&wt)[kTaps], const double (&F)[2][kTaps], double& o0, double& o1) {
    o0 = 0.0; o1 = 0.0;
#pragma unroll
    for (int t = 0; t < kTaps; ++t) {
        const double q0 = wt[t] * F[0][t], q1 = wt[t] * F[1][t];
        o0 = o0 + q0; o1 = o1 + q1;
    }
}

// the K floats of a lane's fine row: K * 4 bytes, aligned to as many (the row starts at a multiple of K floats of a 16-byte aligned base)
template <int K>
__device__ __forceinline__ void store_row(float* dst, const float (&v)[K]) {
    if constexpr (K == 2) {
        *reinterpret_cast<float2*>(dst) = make_float2(v[0], v[1]);
    } else {
#pragma unroll
        for (int q = 0; q < K; q += 4) *reinterpret_cast<float4*>(dst + q) = make_float4(v[q], v[q + 1], v[q + 2], v[q + 3]);
    }
}

template <int K>
__device__ __forceinline__ void load_row(const float* src, float (&v)[K]) {
    if constexpr (K == 2) {
        const float2 a = *reinterpret_cast<const float2*>(src);
        v[0] = a.x; v[1] = a.y;
    } else {
#pragma unroll
        for (int q = 0; q < K; q += 4) {
            const float4 a = *reinterpret_cast<const float4*>(src + q);
            v[q] = a.x; v[q + 1] = a.y; v[q + 2] = a.z; v[q + 3] = a.w;
        }
    }
}

// the lane's coarse pixel (x, y) and sub-row i; false where the lane has none (no barrier in these kernels)
template <int K>
__device__ __forceinline__ bool lane_of(const UpParams& p, int& x, int& y, int& i, int& r) {
    const int by = (int)(blockIdx.x / (uint32_t)p.tiles_x), tx = (int)(blockIdx.x - (uint32_t)by * (uint32_t)p.tiles_x);
    x = tx * kTileW + (int)(threadIdx.x % kTileW);
    r = by * kTileH + (int)(threadIdx.x / kTileW);             // the fine row
    y = r / K; i = r % K;
    return x < p.w && y < p.h;
}

template <int K, bool HALF>
__global__ void __launch_bounds__(kThreads) flow_upsample_convex_kernel(UpParams p) {
    const int64_t n_img = blockIdx.y;
    int x, y, i, r;
    if (!lane_of<K>(p, x, y, i, r)) return;
    double F[2][kTaps];
    taps_of<K, HALF>(p, n_img, x, y, F);
    const int64_t pix = (int64_t)y * p.w + x;
    const float* lg = p.logits + n_img * (kTaps * K * K) * p.hw + pix;
    float o0[K], o1[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
        float l[kTaps];
#pragma unroll
        for (int t = 0; t < kTaps; ++t) l[t] = lg[(int64_t)(t * K * K + i * K + j) * p.hw];
        double wt[kTaps], m, s, a0, a1;
        softmax_of(l, wt, m, s);
        mix_of(wt, F, a0, a1);
        o0[j] = (float)a0; o1[j] = (float)a1;
    }
    const int64_t fw = (int64_t)K * p.w, fhw = (int64_t)K * K * p.hw;
    const int64_t fine = (int64_t)r * fw + (int64_t)K * x;
    float* o = p.out + n_img * 2 * fhw + fine;
    store_row<K>(o, o0);
    store_row<K>(o + fhw, o1);
    if (p.out_mask != nullptr) {
        const uint8_t bit = p.mask[n_img * p.mask_bs + pix] != 0 ? 1 : 0;
        uint8_t* om = p.out_mask + n_img * fhw + fine;         // K bytes at a multiple of K of an 8-byte aligned base
        if constexpr (K == 2) *reinterpret_cast<uint16_t*>(om) = (uint16_t)(bit * 0x0101u);
        else if constexpr (K == 4) *reinterpret_cast<uint32_t*>(om) = (uint32_t)bit * 0x01010101u;
        else *reinterpret_cast<uint64_t*>(om) = (uint64_t)bit * 0x0101010101010101ull;
    }
}

template <int K, bool HALF>
__global__ void __launch_bounds__(kThreads) flow_upsample_convex_grad_logits_kernel(UpParams p) {
    const int64_t n_img = blockIdx.y;
    int x, y, i, r;
    if (!lane_of<K>(p, x, y, i, r)) return;
    double F[2][kTaps];
    taps_of<K, HALF>(p, n_img, x, y, F);
    const int64_t pix = (int64_t)y * p.w + x;
    const int64_t img = n_img * (kTaps * K * K) * p.hw + pix;
    const float* lg = p.logits + img;
    const int64_t fw = (int64_t)K * p.w, fhw = (int64_t)K * K * p.hw;
    const int64_t fine = (int64_t)r * fw + (int64_t)K * x;
    float g0[K], g1[K];
    load_row<K>(p.g + n_img * 2 * fhw + fine, g0);
    load_row<K>(p.g + n_img * 2 * fhw + fhw + fine, g1);
#pragma unroll
    for (int j = 0; j < K; ++j) {
        float l[kTaps];
#pragma unroll
        for (int t = 0; t < kTaps; ++t) l[t] = lg[(int64_t)(t * K * K + i * K + j) * p.hw];
        double wt[kTaps], m, s, a0, a1;
        softmax_of(l, wt, m, s);
        if (p.ws != nullptr) {
            double* ws = p.ws + n_img * 2 * fhw + fine + j;
            ws[0] = m; ws[fhw] = s;
        }
        if (p.d_logits != nullptr) {
            mix_of(wt, F, a0, a1);
            const double G0 = (double)g0[j], G1 = (double)g1[j];
            const double b0 = G0 * a0, b1 = G1 * a1;
            const double go = b0 + b1;
            float* dl = p.d_logits + img;
#pragma unroll
            for (int t = 0; t < kTaps; ++t) {
                const double c0 = G0 * F[0][t], c1 = G1 * F[1][t];
                const double gf = c0 + c1;
                const double diff = gf - go;
                dl[(int64_t)(t * K * K + i * K + j) * p.hw] = (float)(wt[t] * diff);
            }
        }
    }
}

template <int K>
__global__ void __launch_bounds__(kThreads) flow_upsample_convex_grad_flow_kernel(UpParams p) {
    const int64_t n_img = blockIdx.y;
    const int64_t fw = (int64_t)K * p.w, fhw = (int64_t)K * K * p.hw;
    const float* lg_img = p.logits + n_img * (kTaps * K * K) * p.hw;
    const double* ws = p.ws + n_img * 2 * fhw;
    const float* g = p.g + n_img * 2 * fhw;
    for (int64_t pix = (int64_t)blockIdx.x * kThreads + threadIdx.x; pix < p.hw; pix += (int64_t)gridDim.x * kThreads) {
        const int y = (int)(pix / p.w), x = (int)(pix - (int64_t)y * p.w);
        double a0 = 0.0, a1 = 0.0;
#pragma unroll 1
        for (int t = 0; t < kTaps; ++t) {
            const int py = y - (t / 3 - 1), px = x - (t % 3 - 1);          // the coarse pixel whose tap t is (x, y)
            if (py < 0 || py >= p.h || px < 0 || px >= p.w) continue;
            const float* lg = lg_img + (int64_t)t * (K * K) * p.hw + (int64_t)py * p.w + px;
#pragma unroll 1
            for (int i = 0; i < K; ++i) {
                const int64_t fine = ((int64_t)K * py + i) * fw + (int64_t)K * px;
                float l[K], g0[K], g1[K];
                double m[K], s[K];
#pragma unroll
                for (int j = 0; j < K; ++j) {
                    l[j] = lg[(int64_t)(i * K + j) * p.hw];
                    m[j] = ws[fine + j]; s[j] = ws[fhw + fine + j];
                }
                load_row<K>(g + fine, g0);
                load_row<K>(g + fhw + fine, g1);
#pragma unroll
                for (int j = 0; j < K; ++j) {
                    const double wt = e_of(l[j], m[j]) / s[j];
                    const double q0 = wt * (double)g0[j], q1 = wt * (double)g1[j];
                    a0 = a0 + q0; a1 = a1 + q1;
                }
            }
        }
        float* d = p.d_flow + n_img * 2 * p.hw + pix;
        d[0] = (float)((double)K * a0);
        d[p.hw] = (float)((double)K * a1);
    }
}

int64_t tiles_of(int64_t extent, int tile) { return (extent + tile - 1) / tile; }

// the frame and the flow: the fields and the checks both entry points share
int fill_frame(UpParams* p, const void* flow, int64_t flow_bs, int32_t flow_half, const float* logits, int32_t factor, int32_t n, int32_t h,
               int32_t w) {
    if (factor != 2 && factor != 4 && factor != 8) return OFL_E_ARG;
    if (!dims_ok(n, h, w, 1)) return OFL_E_ARG;
    if ((int64_t)factor * h >= (1ll << 31) || (int64_t)factor * w >= (1ll << 31)) return OFL_E_ARG;
    if (!dims_ok(n, (int32_t)(factor * h), (int32_t)(factor * w), 1)) return OFL_E_ARG;        // the fine grid's own bounds
    if (flow == nullptr || logits == nullptr) return OFL_E_ARG;
    if (flow_half != 0 && flow_half != 1) return OFL_E_ARG;
    if (flow_bs < 0) return OFL_E_ARG;
    if (!aligned(flow, flow_half ? 2 : 4) || !aligned(logits, 4)) return OFL_E_ARG;
    p->flow = flow; p->flow_bs = flow_bs; p->mask = nullptr; p->mask_bs = 0;
    p->logits = logits;
    p->out = nullptr; p->out_mask = nullptr; p->g = nullptr; p->d_logits = nullptr; p->ws = nullptr; p->d_flow = nullptr;
    p->hw = (int64_t)h * w; p->h = h; p->w = w;
    p->tiles_x = (int32_t)tiles_of(w, kTileW);
    return OFL_OK;
}

// the grid of the per-fine-pixel kernels (K H * K W < 2^31: under 2^30 blocks)
dim3 grid_of(int32_t factor, int32_t n, int32_t h, int32_t w) {
    return dim3((unsigned)(tiles_of(w, kTileW) * tiles_of((int64_t)factor * h, kTileH)), (unsigned)n);
}

// the factor and the flow's storage to the <K, HALF> instantiation: f(std::integral_constant<int, K>, std::bool_constant<HALF>)
template <class F>
void dispatch(int factor, bool half, F&& f) {
    auto with_k = [&](auto KK) {
        if (half) f(KK, std::true_type{});
        else f(KK, std::false_type{});
    };
    if (factor == 2) with_k(std::integral_constant<int, 2>{});
    else if (factor == 4) with_k(std::integral_constant<int, 4>{});
    else with_k(std::integral_constant<int, 8>{});
}

}  // namespace

extern "C" {

__attribute__((visibility("default"))) int ofl_flow_upsample_convex_f32(const void* flow, int64_t flow_bs, int32_t flow_half,
                                                                        const uint8_t* mask, int64_t mask_bs, const float* logits,
                                                                        int32_t factor, float* out, uint8_t* out_mask, int32_t n, int32_t h,
                                                                        int32_t w, void* stream) {
    UpParams p;
    const int rc = fill_frame(&p, flow, flow_bs, flow_half, logits, factor, n, h, w);
    if (rc) return rc;
    if (out == nullptr || mask_bs < 0) return OFL_E_ARG;
    if ((mask == nullptr) != (out_mask == nullptr)) return OFL_E_ARG;
    if (!aligned(out, 16) || !aligned(out_mask, 8)) return OFL_E_ARG;
    p.mask = mask; p.mask_bs = mask_bs; p.out = out; p.out_mask = out_mask;
    hipStream_t s = (hipStream_t)stream;
    dispatch(factor, flow_half != 0, [&](auto KK, auto HALF) {
        OFL_KLAUNCH((flow_upsample_convex_kernel<decltype(KK)::value, decltype(HALF)::value>), grid_of(factor, n, h, w), dim3(kThreads), 0, s,
                    p);
    });
    return (int)hipGetLastError();
}

__attribute__((visibility("default"))) int ofl_flow_upsample_convex_grad_f32(const void* flow, int64_t flow_bs, int32_t flow_half,
                                                                             const float* logits, int32_t factor, const float* grad_out,
                                                                             float* grad_logits, float* grad_flow, double* workspace,
                                                                             int32_t n, int32_t h, int32_t w, void* stream) {
    UpParams p;
    const int rc = fill_frame(&p, flow, flow_bs, flow_half, logits, factor, n, h, w);
    if (rc) return rc;
    if (grad_out == nullptr || (grad_logits == nullptr && grad_flow == nullptr)) return OFL_E_ARG;
    if ((grad_flow == nullptr) != (workspace == nullptr)) return OFL_E_ARG;
    if (!aligned(grad_out, 16) || !aligned(grad_logits, 4) || !aligned(grad_flow, 4) || !aligned(workspace, 8)) return OFL_E_ARG;
    p.g = grad_out; p.d_logits = grad_logits; p.d_flow = grad_flow; p.ws = workspace;
    hipStream_t s = (hipStream_t)stream;
    dispatch(factor, flow_half != 0, [&](auto KK, auto HALF) {
        OFL_KLAUNCH((flow_upsample_convex_grad_logits_kernel<decltype(KK)::value, decltype(HALF)::value>), grid_of(factor, n, h, w),
                    dim3(kThreads), 0, s, p);
    });
    if (grad_flow != nullptr) {
        const int64_t blocks = (p.hw + kThreads - 1) / kThreads;
        const dim3 grid((unsigned)(blocks < 65536 ? blocks : 65536), (unsigned)n);
        dispatch(factor, false, [&](auto KK, auto) {
            OFL_KLAUNCH((flow_upsample_convex_grad_flow_kernel<decltype(KK)::value>), grid, dim3(kThreads), 0, s, p);
        });
    }
    return (int)hipGetLastError();
}

}  // extern "C"
