// ofl_matching.hip -- Flow.from_matching on gfx950: the global matching of GMFlow, UniMatch and the matching heads of tracking and stereo
// networks -- for every pixel p of one frame the softmax, over ALL positions q of the other, of feat(p) . other(q) / sqrt(C), and the
// expected position minus p as the flow -- without the (H W)^2 volume (which DEFINES the numbers;
// tests/matching_oracle.py is the same definition in NumPy).  An extension: the reference has no such function.
//
//   flow_global_match_kernel              one launch.  A block is ONE wave and owns kTileP = 64 pixels p, one per lane.  It walks the other
//                                         frame in chunks of kChunkQ = 32 positions: a lane holds the 32 dot products of its pixel in
//                                         registers and walks the channels once, kChanChunk = 2 at a time (its own feature of the two
//                                         channels goes out as two loads, coalesced across the wave; the 32 values of the walked frame
//                                         are the same for every lane and come through the scalar cache).  The lane's softmax chain
//                                         (m, S, X, Y) then takes the chunk's logits in q order out of a lane-private LDS column
//   flow_global_match_grad_kernel<OTHER>  both gradients, the forward's walk with the roles named by OTHER: d feat (false) owns a tile of p
//                                         and walks q, d other (true) owns a tile of q and walks p.  A block is kGradWaves = 4 waves on
//                                         the SAME 64 pixels and walks four chunks at a time: wave k recomputes the logits of chunk k as
//                                         the forward does, then the chunk's dss(p, q) from the saved FINAL m and S, into slot k of an LDS
//                                         tile; after a barrier wave k owns kGradChan = 32 channels, one float32 sum each in a register
//                                         per lane, and takes the four chunks' 128 products of every one of them in ascending order.
//                                         More than 128 channels: another walk per group of 128
//
// No float atomics and no scatter: every sum has one owner -- one lane of one wave -- and a fixed order that no tile size enters (a chunk
// only groups consecutive steps of one chain), the same bits on any run and in any batch.  The forward has no barrier: every LDS column
// has one lane.  The dot product (dots_of), the
// softmax step (chain_step) and the gradient of a logit (dss_of) are one set of device functions for all three kernels.
//
// Every product is rounded, then every sum: fp contraction is off (ofl_loss_common.hpp); there is no fused multiply-add in this file.
// C ABI: include/oflib_hip.h.
#include "ofl_loss_common.hpp"

namespace {

using namespace ofl_loss;

constexpr int kTileP = 64;                         // pixels a block owns: one per lane of its single wave
constexpr int kChunkQ = 32;                        // positions of the walked frame whose dot products a lane holds at a time
constexpr int kChanChunk = 2;                      // channels whose lane-side loads go out together
constexpr int kThreads = kTileP;
constexpr int kGradWaves = 4;                      // waves of a gradient block: each recomputes one chunk, then sums its share of the channels
constexpr int kGradChan = 32;                      // channels whose sums a wave of a gradient block keeps in registers
constexpr int kGradThreads = kGradWaves * kTileP;
constexpr int kGradWavesPerSimd = 3;               // the gradient kernels are compiled for three waves per SIMD (168 VGPRs; left alone: 196)
constexpr int kMaxExtent = 1 << 24;

static_assert(kThreads == 64, "a wave owns the tile: one pixel per lane, the forward's LDS columns are lane-private and need no barrier");
static_assert(kGradWaves * kChunkQ * kTileP * 4 <= 64 * 1024, "the LDS of a gradient block");

struct GmParams {
    const float* feat; const float* other;         // [*,C,H,W]
    int64_t feat_bs, other_bs;                     // elements between images
    int64_t hw, nhw;                               // H W; n H W
    int32_t chan, h, w;
    float flow_sign;
    float* out;                                    // forward: [n][2][H W]
    float* prob;                                   // forward: [n][H W] or nullptr
    double* ws_d;                                  // the workspace's float64 part [3][n][H W]: S, ox, oy; or nullptr
    float* ws_m;                                   // its float32 part [n][H W]: m
    const float* g;                                // backward: the upstream gradient [n][2][H W]
    float* grad;                                   // backward: d feat or d other [n][C][H W]
};

// The walked operand is read at addresses that are the same in every lane of a wave and is never written by these kernels: a pointer into
// the constant address space makes each such read a scalar load whatever stores the kernel has around it (the d feat / d other kernel
// stores between two walks, which otherwise turns every one of them into a vector load and its 32 x 32 values into registers)
typedef const __attribute__((address_space(4))) float* Walked;
__device__ __forceinline__ Walked walked_of(const float* ptr) { return (Walked)(uintptr_t)ptr; }

// acc[j] = sum_c own_c * walked_c(j), from +0, c ascending, each product rounded, then the sum.  `own`: the lane's element of channel 0;
// `walked`: the chunk's first element of channel 0 of the walked operand, the same address in every lane; FULL: the chunk has kChunkQ
// positions, else `cnt`, and the sums beyond them are those of position cnt - 1 (never used)
template <bool FULL>
__device__ __forceinline__ void dots_step(float f, Walked wk, int cnt, float (&acc)[kChunkQ]) {
#pragma unroll
    for (int j = 0; j < kChunkQ; ++j) {
        const float v = wk[FULL ? j : (j < cnt ? j : cnt - 1)];
        const float prod = f * v;
        acc[j] = acc[j] + prod;
    }
}

template <bool FULL>
__device__ __forceinline__ void dots_of(const float* own, Walked walked, int64_t hw, int chan, int cnt, float (&acc)[kChunkQ]) {
#pragma unroll
    for (int j = 0; j < kChunkQ; ++j) acc[j] = 0.0f;
    int c = 0;
#pragma unroll 1
    for (; c + kChanChunk <= chan; c += kChanChunk) {
        float f[kChanChunk];
#pragma unroll
        for (int k = 0; k < kChanChunk; ++k) f[k] = own[(int64_t)(c + k) * hw];
#pragma unroll
        for (int k = 0; k < kChanChunk; ++k) dots_step<FULL>(f[k], walked + (int64_t)(c + k) * hw, cnt, acc);
    }
#pragma unroll 1
    for (; c < chan; ++c) dots_step<FULL>(own[(int64_t)c * hw], walked + (int64_t)c * hw, cnt, acc);
}

// e = exp((double)s - (double)m) in float64
__device__ __forceinline__ double e_of(float s, float m) { return exp((double)s - (double)m); }

// the running softmax of one pixel: the maximum so far and the sums of e, e qx, e qy on it
struct Chain {
    float m;
    double S, X, Y;
};

// one position (qx, qy) with the logit s: the rescale where the maximum rises, then the three sums
__device__ __forceinline__ void chain_step(Chain& k, float s, double qx, double qy) {
    if (s > k.m) {
        const double r = exp((double)k.m - (double)s);
        k.S = k.S * r; k.X = k.X * r; k.Y = k.Y * r;
        k.m = s;
    }
    const double e = e_of(s, k.m);
    const double ex = e * qx, ey = e * qy;
    k.S = k.S + e; k.X = k.X + ex; k.Y = k.Y + ey;
}

// dss(p, q) from the dot product of the pair, the saved m, S, ox, oy of p, G = -flow_sign (double)g of p and the position of q
__device__ __forceinline__ float dss_of(float dot, float root, float m, double S, double ox, double oy, double Gx, double Gy, double qx,
                                        double qy) {
    const float s = dot / root;
    const double wt = e_of(s, m) / S;
    const double dx = qx - ox, dy = qy - oy;
    const double ax = Gx * dx, ay = Gy * dy;
    const double t = ax + ay;
    const float ds = (float)(wt * t);
    return ds / root;
}

__global__ void __launch_bounds__(kThreads) flow_global_match_kernel(GmParams p) {
    __shared__ float s_dot[kChunkQ * kTileP];      // column `lane`: the chunk's dot products of the lane's pixel
    const int64_t n_img = blockIdx.y;
    const int lane = (int)threadIdx.x;
    const int64_t mine = (int64_t)blockIdx.x * kTileP + lane;
    const bool live = mine < p.hw;
    const int64_t pix = live ? mine : p.hw - 1;    // (a lane beyond the frame walks with the last pixel and stores nothing)
    const float* own = p.feat + n_img * p.feat_bs + pix;
    const Walked walked = walked_of(p.other + n_img * p.other_bs);
    const float root = sqrt_rn((float)p.chan);
    Chain k;
    k.m = 0.0f; k.S = 0.0; k.X = 0.0; k.Y = 0.0;
#pragma unroll 1
    for (int64_t q0 = 0; q0 < p.hw; q0 += kChunkQ) {
        const int64_t left = p.hw - q0;
        const int cnt = left < kChunkQ ? (int)left : kChunkQ;
        float acc[kChunkQ];
        if (cnt == kChunkQ) dots_of<true>(own, walked + q0, p.hw, p.chan, cnt, acc);
        else dots_of<false>(own, walked + q0, p.hw, p.chan, cnt, acc);
#pragma unroll
        for (int j = 0; j < kChunkQ; ++j) s_dot[j * kTileP + lane] = acc[j];
        int qy = (int)(q0 / p.w), qx = (int)(q0 - (int64_t)qy * p.w);
#pragma unroll 1
        for (int j = 0; j < cnt; ++j) {
            const float s = s_dot[j * kTileP + lane] / root;
            if (q0 + j == 0) k.m = s;
            chain_step(k, s, (double)qx, (double)qy);
            if (++qx == p.w) { qx = 0; ++qy; }
        }
    }
    if (!live) return;
    const int y = (int)(pix / p.w), x = (int)(pix - (int64_t)y * p.w);
    const double ox = k.X / k.S, oy = k.Y / k.S;
    const double sg = (double)(-p.flow_sign);
    float* o = p.out + n_img * 2 * p.hw + pix;
    o[0] = (float)((ox - (double)x) * sg);
    o[p.hw] = (float)((oy - (double)y) * sg);
    if (p.prob != nullptr) p.prob[n_img * p.hw + pix] = (float)(1.0 / k.S);
    if (p.ws_d != nullptr) {
        double* wd = p.ws_d + n_img * p.hw + pix;
        wd[0] = k.S; wd[p.nhw] = ox; wd[2 * p.nhw] = oy;
        p.ws_m[n_img * p.hw + pix] = k.m;
    }
}

// the saved statistics and the upstream gradient of pixel `at` of image n_img
struct Saved {
    float m;
    double S, ox, oy, Gx, Gy;
};

__device__ __forceinline__ Saved saved_of(const GmParams& p, int64_t n_img, int64_t at) {
    Saved v;
    const double* wd = p.ws_d + n_img * p.hw + at;
    v.m = p.ws_m[n_img * p.hw + at];
    v.S = wd[0]; v.ox = wd[p.nhw]; v.oy = wd[2 * p.nhw];
    const double sg = (double)(-p.flow_sign);
    const float* g = p.g + n_img * 2 * p.hw + at;
    v.Gx = sg * (double)g[0]; v.Gy = sg * (double)g[p.hw];
    return v;
}

// sum[c] += d[j] * walked_{c0 + c}(j) over the positions j ascending of a whole chunk, for the kGradChan channels of a wave: one float32
// sum per channel in a register, each product rounded, then the sum.  `walked`: the chunk's first element of channel 0; a channel at or
// beyond `chan` sums the last channel's products and is never stored
__device__ __forceinline__ void sums_of(const float (&d)[kChunkQ], Walked walked, int64_t hw, int c0, int chan,
                                        float (&sum)[kGradChan]) {
#pragma unroll
    for (int c = 0; c < kGradChan; ++c) {
        const int ch = c0 + c < chan ? c0 + c : chan - 1;
        const Walked wk = walked + (int64_t)ch * hw;
        float a = sum[c];
#pragma unroll
        for (int j = 0; j < kChunkQ; ++j) {
            const float prod = d[j] * wk[j];
            a = a + prod;
        }
        sum[c] = a;
        // (nothing is scheduled across two channels: left alone, the scalar loads of all kGradChan channels are hoisted to the top and
        // their 32 x 32 values spilled through VGPR lanes, over a thousand lane moves a chunk)
        if (c % 2 == 1) __builtin_amdgcn_sched_barrier(0);
    }
}

// the same over the `cnt` positions of the frame's last, partial chunk, one position at a time out of the chunk's LDS column
__device__ __forceinline__ void sums_tail(const float* slot, Walked walked, int64_t hw, int c0, int chan, int cnt,
                                          float (&sum)[kGradChan]) {
#pragma unroll 1
    for (int j = 0; j < cnt; ++j) {
        const float d = slot[j * kTileP];
#pragma unroll
        for (int c = 0; c < kGradChan; ++c) {
            const int ch = c0 + c < chan ? c0 + c : chan - 1;
            const float prod = d * walked[(int64_t)ch * hw + j];
            sum[c] = sum[c] + prod;
        }
    }
}

template <bool OTHER>
__global__ void __launch_bounds__(kGradThreads) __attribute__((amdgpu_waves_per_eu(kGradWavesPerSimd))) flow_global_match_grad_kernel(GmParams p) {
    __shared__ float s_dss[kGradWaves * kChunkQ * kTileP];     // slot `wave`, column `lane`: a chunk's dot products, then its dss
    const int64_t n_img = blockIdx.y;
    const int lane = (int)(threadIdx.x % kTileP);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kTileP));         // (the same in every lane, and known to be)
    const int64_t mine = (int64_t)blockIdx.x * kTileP + lane;
    const bool live = mine < p.hw;
    const int64_t pix = live ? mine : p.hw - 1;    // (a lane beyond the frame walks with the last pixel and stores nothing)
    const float* own = (OTHER ? p.other + n_img * p.other_bs : p.feat + n_img * p.feat_bs) + pix;
    const Walked walked = walked_of(OTHER ? p.feat + n_img * p.feat_bs : p.other + n_img * p.other_bs);
    const float root = sqrt_rn((float)p.chan);
    const int my = (int)(pix / p.w), mx = (int)(pix - (int64_t)my * p.w);
    Saved sv = {};
    if (!OTHER) sv = saved_of(p, n_img, pix);
    float* col = s_dss + wave * kChunkQ * kTileP + lane;
    float* go = p.grad + n_img * p.chan * p.hw + pix;
    // (every loop bound below is the same for all threads of the block: each of them meets every barrier)
#pragma unroll 1
    for (int cg = 0; cg < p.chan; cg += kGradWaves * kGradChan) {
        const int c0 = cg + wave * kGradChan;      // the wave's channels of this group
        float sum[kGradChan];
#pragma unroll
        for (int c = 0; c < kGradChan; ++c) sum[c] = 0.0f;
#pragma unroll 1
        for (int64_t t0 = 0; t0 < p.hw; t0 += kGradWaves * kChunkQ) {
            // the wave's chunk of these kGradWaves: the dot products, then dss, into its slot
            const int64_t tw = t0 + (int64_t)wave * kChunkQ;
            const int64_t left = p.hw - tw;
            const int cnt = left < kChunkQ ? (left > 0 ? (int)left : 0) : kChunkQ;
            if (cnt > 0) {
                float acc[kChunkQ];
                if (cnt == kChunkQ) dots_of<true>(own, walked + tw, p.hw, p.chan, cnt, acc);
                else dots_of<false>(own, walked + tw, p.hw, p.chan, cnt, acc);
#pragma unroll
                for (int j = 0; j < kChunkQ; ++j) col[j * kTileP] = acc[j];
                int ty = (int)(tw / p.w), tx = (int)(tw - (int64_t)ty * p.w);
#pragma unroll 1
                for (int j = 0; j < cnt; ++j) {
                    const float dot = col[j * kTileP];
                    float d;
                    if (OTHER) {                   // the walked position is p, the lane's own is q
                        const Saved wv = saved_of(p, n_img, tw + j);
                        d = dss_of(dot, root, wv.m, wv.S, wv.ox, wv.oy, wv.Gx, wv.Gy, (double)mx, (double)my);
                    } else {
                        d = dss_of(dot, root, sv.m, sv.S, sv.ox, sv.oy, sv.Gx, sv.Gy, (double)tx, (double)ty);
                    }
                    col[j * kTileP] = d;
                    if (++tx == p.w) { tx = 0; ++ty; }
                }
            }
            __syncthreads();
            // the wave's channels take the kGradWaves chunks in ascending order
            if (c0 < p.chan) {
#pragma unroll 1
                for (int k = 0; k < kGradWaves; ++k) {
                    const int64_t tk = t0 + (int64_t)k * kChunkQ;
                    const int64_t lk = p.hw - tk;
                    if (lk <= 0) break;
                    const int ck = lk < kChunkQ ? (int)lk : kChunkQ;
                    const float* slot = s_dss + k * kChunkQ * kTileP + lane;
                    if (ck == kChunkQ) {
                        float d[kChunkQ];
#pragma unroll
                        for (int j = 0; j < kChunkQ; ++j) d[j] = slot[j * kTileP];
                        sums_of(d, walked + tk, p.hw, c0, p.chan, sum);
                    } else {
                        sums_tail(slot, walked + tk, p.hw, c0, p.chan, ck, sum);
                    }
                }
            }
            __syncthreads();
        }
        if (live) {
#pragma unroll
            for (int c = 0; c < kGradChan; ++c) {
                if (c0 + c < p.chan) go[(int64_t)(c0 + c) * p.hw] = sum[c];
            }
        }
    }
}

// the frame and the two feature tensors: the fields and the checks both entry points share
int fill_frame(GmParams* p, const float* feat, int64_t feat_bs, const float* other, int64_t other_bs, int32_t channels, float flow_sign,
               int32_t n, int32_t h, int32_t w) {
    if (!dims_ok(n, h, w, 1)) return OFL_E_ARG;
    if (h > kMaxExtent || w > kMaxExtent) return OFL_E_ARG;
    if (channels < 1) return OFL_E_ARG;
    if (flow_sign != 1.0f && flow_sign != -1.0f) return OFL_E_ARG;
    if (feat == nullptr || other == nullptr) return OFL_E_ARG;
    if (feat_bs < 0 || other_bs < 0) return OFL_E_ARG;
    if (!aligned(feat, 4) || !aligned(other, 4)) return OFL_E_ARG;
    p->feat = feat; p->other = other; p->feat_bs = feat_bs; p->other_bs = other_bs;
    p->hw = (int64_t)h * w; p->nhw = (int64_t)n * p->hw;
    p->chan = channels; p->h = h; p->w = w;
    p->flow_sign = flow_sign;
    p->out = nullptr; p->prob = nullptr; p->ws_d = nullptr; p->ws_m = nullptr; p->g = nullptr; p->grad = nullptr;
    return OFL_OK;
}

// the workspace [3][n][H W] float64, then [n][H W] float32
void fill_workspace(GmParams* p, void* workspace) {
    p->ws_d = reinterpret_cast<double*>(workspace);
    p->ws_m = workspace == nullptr ? nullptr : reinterpret_cast<float*>(p->ws_d + 3 * p->nhw);
}

dim3 grid_of(const GmParams& p, int32_t n) {
    return dim3((unsigned)((p.hw + kTileP - 1) / kTileP), (unsigned)n);                  // (H W < 2^31: under 2^25 blocks)
}

}  // namespace

extern "C" {

__attribute__((visibility("default"))) int ofl_flow_global_match_f32(const float* feat, int64_t feat_bs, const float* other,
                                                                     int64_t other_bs, int32_t channels, float flow_sign, float* out,
                                                                     float* prob, void* workspace, int32_t n, int32_t h, int32_t w,
                                                                     void* stream) {
    GmParams p;
    const int rc = fill_frame(&p, feat, feat_bs, other, other_bs, channels, flow_sign, n, h, w);
    if (rc) return rc;
    if (out == nullptr) return OFL_E_ARG;
    if (!aligned(out, 4) || !aligned(prob, 4) || !aligned(workspace, 8)) return OFL_E_ARG;
    p.out = out; p.prob = prob;
    fill_workspace(&p, workspace);
    OFL_KLAUNCH(flow_global_match_kernel, grid_of(p, n), dim3(kThreads), 0, (hipStream_t)stream, p);
    return (int)hipGetLastError();
}

__attribute__((visibility("default"))) int ofl_flow_global_match_grad_f32(const float* feat, int64_t feat_bs, const float* other,
                                                                          int64_t other_bs, int32_t channels, float flow_sign,
                                                                          const void* workspace, const float* grad_out, float* grad_feat,
                                                                          float* grad_other, int32_t n, int32_t h, int32_t w,
                                                                          void* stream) {
    GmParams p;
    const int rc = fill_frame(&p, feat, feat_bs, other, other_bs, channels, flow_sign, n, h, w);
    if (rc) return rc;
    if (workspace == nullptr || grad_out == nullptr || (grad_feat == nullptr && grad_other == nullptr)) return OFL_E_ARG;
    if (!aligned(workspace, 8) || !aligned(grad_out, 4) || !aligned(grad_feat, 4) || !aligned(grad_other, 4)) return OFL_E_ARG;
    fill_workspace(&p, const_cast<void*>(workspace));
    p.g = grad_out;
    hipStream_t s = (hipStream_t)stream;
    if (grad_feat != nullptr) {
        p.grad = grad_feat;
        OFL_KLAUNCH(flow_global_match_grad_kernel<false>, grid_of(p, n), dim3(kGradThreads), 0, s, p);
    }
    if (grad_other != nullptr) {
        p.grad = grad_other;
        OFL_KLAUNCH(flow_global_match_grad_kernel<true>, grid_of(p, n), dim3(kGradThreads), 0, s, p);
    }
    return (int)hipGetLastError();
}

}  // extern "C"
