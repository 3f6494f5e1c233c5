// ofl_propagate.hip -- Flow.propagate on gfx950: the flow propagation by self-attention of GMFlow, UniMatch and their stereo and depth
// siblings -- flow'(p) = sum_q softmax_q(query(p) . key(q) / sqrt(C)) flow(q), over ALL positions q (the global form, without the
// (H W)^2 volume) or over a (2 r + 1)^2 window with zero padding (the local form, without the unfold) -- with the positions that the
// flow's mask excludes left out of the softmax (which DEFINES the numbers; tests/propagate_oracle.py is the same
// definition in NumPy).  An extension: the reference has no such function.
//
//   flow_propagate_global_kernel               the walk of flow_global_match_kernel (ofl_matching.hip): a block is ONE wave and owns
//                                              kTileP = 64 pixels p, one per lane; it walks the key in chunks of kChunkQ = 32 positions,
//                                              whose key values, vectors and mask bytes are the same for every lane and come through the
//                                              scalar cache.  The chain (m, S, X, Y) mixes the two components of flow(q); an excluded
//                                              position is a wave-uniform branch around its step
//   flow_propagate_global_grad_kernel<OTHER,   the gradients, the forward's walk with the roles named by OTHER: d query (false) owns a tile
//                                     VALUE>   of p and walks q; d key (true) owns a tile of q and walks p, and with VALUE the last wave of
//                                              the block also owns the two float32 sums d u(q), d v(q), whose terms the four waves leave
//                                              in LDS next to dss.  kGradWaves = 4 waves on the SAME 64 pixels, as in ofl_matching.hip
//   flow_propagate_local_kernel<R, GRAD>       a tile of kLTileW x kLTileH pixels, one per lane: the tile and its halo of the key go into
//                                              LDS kLChan channels at a time, the (2 R + 1)^2 dot products of a lane's pixel stay in
//                                              registers; the logits then go into a lane-private LDS column and the softmax (two passes)
//                                              or, with GRAD, dss and the value terms of every offset walk them in a rolled loop
//   flow_propagate_local_gather_kernel<R,      the three gradients of the local form as gathers from that workspace, one pixel per
//                                      OTHER>  thread: d query(p) over the offsets ascending; d key(q), d u(q), d v(q) over p ascending
//
// No float atomics and no scatter: every sum has one owner and a fixed order that no tile size enters, the same bits on any run and in
// any batch.  dots_step / dots_of / e_of / chain_step / sums_of / sums_tail are those of ofl_matching.hip, copied: that file's code
// is left as it was compiled.
//
// Every product is rounded, then every sum: fp contraction is off (ofl_loss_common.hpp); there is no fused multiply-add in this file.
// C ABI: include/oflib_hip.h.
#include "ofl_loss_common.hpp"

namespace {

using namespace ofl_loss;

constexpr int kTileP = 64;                         // pixels a block of the global kernels owns: one per lane of a wave
constexpr int kChunkQ = 32;                        // positions of the walked operand whose dot products a lane holds at a time
constexpr int kChanChunk = 2;                      // channels whose lane-side loads go out together
constexpr int kThreads = kTileP;
constexpr int kGradWaves = 4;                      // waves of a gradient block: each recomputes one chunk, then sums its share of the channels
constexpr int kGradChan = 32;                      // channels whose sums a wave of a gradient block keeps in registers
constexpr int kGradThreads = kGradWaves * kTileP;
constexpr int kLTileW = 32;                        // the local form's tile: one pixel per thread
constexpr int kLTileH = 4;
constexpr int kLThreads = kLTileW * kLTileH;
constexpr int kLChan = 8;                          // channels of the key's tile and halo that are in LDS at a time
constexpr int kGatherThreads = 256;
constexpr int kMaxRadius = 4;
constexpr int kMaxExtent = 1 << 24;

static_assert(kThreads == 64, "a wave owns the tile: one pixel per lane, the forward's LDS columns are lane-private and need no barrier");
static_assert(3 * kGradWaves * kChunkQ * kTileP * 4 <= 160 * 1024, "the LDS of a gradient block that also sums d u and d v");

struct PpParams {
    const float* query; const float* key;          // [*,C,H,W]
    int64_t query_bs, key_bs;                      // elements between images
    const float* flow; int64_t flow_bs;            // [*,2,H,W]
    const uint8_t* mask; int64_t mask_bs;          // [*,H,W] or nullptr: nothing is excluded
    int64_t hw, nhw;                               // H W; n H W
    int32_t chan, h, w;
    int32_t tiles_x;                               // local form: tiles in a row of tiles
    int32_t planes;                                // local backward: 1 (dss) or 3 (dss, tx, ty) planes of the scratch
    float* out;                                    // forward: [n][2][H W]
    uint8_t* valid;                                // forward: [n][H W], 0 for an empty pixel; or nullptr
    double* ws_d;                                  // the workspace's float64 part [3][n][H W]: S, ox, oy; or nullptr
    float* ws_m;                                   // its float32 part [n][H W]: m
    const float* g;                                // backward: the upstream gradient [n][2][H W]
    float* grad;                                   // backward: d query or d key [n][C][H W]; or nullptr
    float* grad_flow;                              // backward: d flow [n][2][H W]; or nullptr
    float* scratch;                                // local backward: [n][planes][D][H W]
};

// The walked operands are read at addresses that are the same in every lane of a wave and are never written by these kernels: a pointer
// into the constant address space makes each such read a scalar load whatever stores the kernel has around it (ofl_matching.hip)
typedef const __attribute__((address_space(4))) float* Walked;
typedef const __attribute__((address_space(4))) uint8_t* WalkedMask;
__device__ __forceinline__ Walked walked_of(const float* ptr) { return (Walked)(uintptr_t)ptr; }
__device__ __forceinline__ WalkedMask walked_of(const uint8_t* ptr) { return (WalkedMask)(uintptr_t)ptr; }

// acc[j] = sum_c own_c * walked_c(j), from +0, c ascending, each product rounded, then the sum (ofl_matching.hip)
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

// the running softmax of one pixel: the maximum so far and the sums of e, e u, e v on it
struct Chain {
    float m;
    double S, X, Y;
};

// one participating position with the logit s and the vector (u, v): the rescale where the maximum rises, then the three sums
__device__ __forceinline__ void chain_step(Chain& k, float s, double u, double v) {
    if (s > k.m) {
        const double r = exp((double)k.m - (double)s);
        k.S = k.S * r; k.X = k.X * r; k.Y = k.Y * r;
        k.m = s;
    }
    const double e = e_of(s, k.m);
    const double ex = e * u, ey = e * v;
    k.S = k.S + e; k.X = k.X + ex; k.Y = k.Y + ey;
}

// What a pair (p, q) gives the backward: dss, and the terms (float)(w g_x(p)), (float)(w g_y(p)) of d u(q), d v(q) -- from the logit of
// the pair, the saved m, S, ox, oy and the upstream gradient (Gx, Gy) of p and the vector (u, v) of q.  `zero`: q is excluded or p is
// empty, all three are exactly +0
struct Pair {
    float dss, tx, ty;
};

__device__ __forceinline__ Pair pair_of(float s, float root, float m, double S, double ox, double oy, double Gx, double Gy, double u,
                                        double v, bool zero) {
    const double wt = e_of(s, m) / S;
    const double dx = u - ox, dy = v - oy;
    const double ax = Gx * dx, ay = Gy * dy;
    const double t = ax + ay;
    const float ds = (float)(wt * t);
    Pair r;
    r.dss = zero ? 0.0f : ds / root;
    r.tx = zero ? 0.0f : (float)(wt * Gx);
    r.ty = zero ? 0.0f : (float)(wt * Gy);
    return r;
}

// the statistics of a pixel as the forwards leave them: an empty pixel has S = 0, m = ox = oy = +0
__device__ __forceinline__ void save_stats(const PpParams& p, int64_t n_img, int64_t pix, float m, double S, double ox, double oy) {
    double* wd = p.ws_d + n_img * p.hw + pix;
    wd[0] = S; wd[p.nhw] = ox; wd[2 * p.nhw] = oy;
    p.ws_m[n_img * p.hw + pix] = m;
}

__global__ void __launch_bounds__(kThreads) flow_propagate_global_kernel(PpParams p) {
    __shared__ float s_dot[kChunkQ * kTileP];      // column `lane`: the chunk's dot products of the lane's pixel
    const int64_t n_img = blockIdx.y;
    const int lane = (int)threadIdx.x;
    const int64_t mine = (int64_t)blockIdx.x * kTileP + lane;
    const bool live = mine < p.hw;
    const int64_t pix = live ? mine : p.hw - 1;    // (a lane beyond the frame walks with the last pixel and stores nothing)
    const float* own = p.query + n_img * p.query_bs + pix;
    const Walked walked = walked_of(p.key + n_img * p.key_bs);
    const Walked wu = walked_of(p.flow + n_img * p.flow_bs);
    const Walked wv = wu + p.hw;
    const bool masked = p.mask != nullptr;
    const WalkedMask wm = walked_of(masked ? p.mask + n_img * p.mask_bs : nullptr);
    const float root = sqrt_rn((float)p.chan);
    Chain k;
    k.m = 0.0f; k.S = 0.0; k.X = 0.0; k.Y = 0.0;
    bool started = false;                          // (wave-uniform: the mask is the same for every pixel)
#pragma unroll 1
    for (int64_t q0 = 0; q0 < p.hw; q0 += kChunkQ) {
        const int64_t left = p.hw - q0;
        const int cnt = left < kChunkQ ? (int)left : kChunkQ;
        float acc[kChunkQ];
        if (cnt == kChunkQ) dots_of<true>(own, walked + q0, p.hw, p.chan, cnt, acc);
        else dots_of<false>(own, walked + q0, p.hw, p.chan, cnt, acc);
#pragma unroll
        for (int j = 0; j < kChunkQ; ++j) s_dot[j * kTileP + lane] = acc[j];
#pragma unroll 1
        for (int j = 0; j < cnt; ++j) {
            if (masked && wm[q0 + j] == 0) continue;                   // excluded: no step at all
            const float s = s_dot[j * kTileP + lane] / root;
            if (!started) { k.m = s; started = true; }
            chain_step(k, s, (double)wu[q0 + j], (double)wv[q0 + j]);
        }
    }
    if (!live) return;
    const double ox = started ? k.X / k.S : 0.0, oy = started ? k.Y / k.S : 0.0;
    float* o = p.out + n_img * 2 * p.hw + pix;
    o[0] = (float)ox;
    o[p.hw] = (float)oy;
    if (p.valid != nullptr) p.valid[n_img * p.hw + pix] = started ? 1 : 0;
    if (p.ws_d != nullptr) save_stats(p, n_img, pix, started ? k.m : 0.0f, started ? k.S : 0.0, ox, oy);
}

// the saved statistics and the upstream gradient of pixel `at` of image n_img
struct Saved {
    float m;
    double S, ox, oy, Gx, Gy;
};

__device__ __forceinline__ Saved saved_of(const PpParams& p, int64_t n_img, int64_t at) {
    Saved v;
    const double* wd = p.ws_d + n_img * p.hw + at;
    v.m = p.ws_m[n_img * p.hw + at];
    v.S = wd[0]; v.ox = wd[p.nhw]; v.oy = wd[2 * p.nhw];
    const float* g = p.g + n_img * 2 * p.hw + at;
    v.Gx = (double)g[0]; v.Gy = (double)g[p.hw];
    return v;
}

// sum[c] += d[j] * walked_{c0 + c}(j) over the positions j ascending of a whole chunk, for the kGradChan channels of a wave
// (ofl_matching.hip)
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
        // (nothing is scheduled across two channels: see ofl_matching.hip)
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

template <bool OTHER, bool VALUE>
__global__ void __launch_bounds__(kGradThreads) flow_propagate_global_grad_kernel(PpParams p) {
    constexpr int kSlot = kChunkQ * kTileP;
    __shared__ float s_dss[kGradWaves * kSlot];                // slot `wave`, column `lane`: a chunk's dot products, then its dss
    __shared__ float s_val[VALUE ? 2 * kGradWaves * kSlot : 1];          // the terms of d u, then of d v, laid out alike
    static_assert(OTHER || !VALUE, "d u and d v are owned by the kernel that owns q");
    const int64_t n_img = blockIdx.y;
    const int lane = (int)(threadIdx.x % kTileP);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kTileP));         // (the same in every lane, and known to be)
    const int64_t mine = (int64_t)blockIdx.x * kTileP + lane;
    const bool live = mine < p.hw;
    const int64_t pix = live ? mine : p.hw - 1;    // (a lane beyond the frame walks with the last pixel and stores nothing)
    const float* own = (OTHER ? p.key + n_img * p.key_bs : p.query + n_img * p.query_bs) + pix;
    const Walked walked = walked_of(OTHER ? p.query + n_img * p.query_bs : p.key + n_img * p.key_bs);
    const float* flow = p.flow + n_img * p.flow_bs;
    const Walked wu = walked_of(flow);
    const Walked wv = wu + p.hw;
    const bool masked = p.mask != nullptr;
    const uint8_t* mask = masked ? p.mask + n_img * p.mask_bs : nullptr;
    const WalkedMask wm = walked_of(mask);
    const float root = sqrt_rn((float)p.chan);
    Saved sv = {};
    double mu = 0.0, mv = 0.0;                     // OTHER: the vector of the lane's own q
    bool mzero = false;                            // the lane's own side makes the pair +0: its q is excluded, or its p is empty
    if (OTHER) {
        mu = (double)flow[pix]; mv = (double)flow[p.hw + pix];
        mzero = masked && mask[pix] == 0;
    } else {
        sv = saved_of(p, n_img, pix);
        mzero = sv.S == 0.0;
    }
    float* col = s_dss + wave * kSlot + lane;
    const bool sums = p.grad != nullptr;
    float* go = sums ? p.grad + n_img * p.chan * p.hw + pix : nullptr;
    const int cend = sums ? p.chan : 1;            // (d flow alone: one walk, no channel sums)
    // (every loop bound below is the same for all threads of the block: each of them meets every barrier)
#pragma unroll 1
    for (int cg = 0; cg < cend; cg += kGradWaves * kGradChan) {
        const int c0 = cg + wave * kGradChan;      // the wave's channels of this group
        const bool values = VALUE && cg == 0 && p.grad_flow != nullptr;
        float sum[kGradChan];
#pragma unroll
        for (int c = 0; c < kGradChan; ++c) sum[c] = 0.0f;
        float du = 0.0f, dv = 0.0f;
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
#pragma unroll 1
                for (int j = 0; j < cnt; ++j) {
                    const float s = col[j * kTileP] / root;
                    Pair r;
                    if (OTHER) {                   // the walked position is p, the lane's own is q
                        const Saved wsv = saved_of(p, n_img, tw + j);
                        r = pair_of(s, root, wsv.m, wsv.S, wsv.ox, wsv.oy, wsv.Gx, wsv.Gy, mu, mv, mzero || wsv.S == 0.0);
                    } else {
                        const bool out = masked && wm[tw + j] == 0;
                        r = pair_of(s, root, sv.m, sv.S, sv.ox, sv.oy, sv.Gx, sv.Gy, (double)wu[tw + j], (double)wv[tw + j], mzero || out);
                    }
                    col[j * kTileP] = r.dss;
                    if (VALUE) {
                        if (values) {
                            s_val[wave * kSlot + j * kTileP + lane] = r.tx;
                            s_val[(kGradWaves + wave) * kSlot + j * kTileP + lane] = r.ty;
                        }
                    }
                }
            }
            __syncthreads();
            // the wave's channels take the kGradWaves chunks in ascending order
            if (sums && c0 < p.chan) {
#pragma unroll 1
                for (int k = 0; k < kGradWaves; ++k) {
                    const int64_t tk = t0 + (int64_t)k * kChunkQ;
                    const int64_t lk = p.hw - tk;
                    if (lk <= 0) break;
                    const int ck = lk < kChunkQ ? (int)lk : kChunkQ;
                    const float* slot = s_dss + k * kSlot + lane;
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
            // and the last wave the terms of d u and d v, p ascending
            if (VALUE) {
                if (values && wave == kGradWaves - 1) {
#pragma unroll 1
                    for (int k = 0; k < kGradWaves; ++k) {
                        const int64_t lk = p.hw - (t0 + (int64_t)k * kChunkQ);
                        if (lk <= 0) break;
                        const int ck = lk < kChunkQ ? (int)lk : kChunkQ;
                        const float* sx = s_val + k * kSlot + lane;
                        const float* sy = s_val + (kGradWaves + k) * kSlot + lane;
#pragma unroll 4
                        for (int j = 0; j < ck; ++j) {
                            du = du + sx[j * kTileP];
                            dv = dv + sy[j * kTileP];
                        }
                    }
                }
            }
            __syncthreads();
        }
        if (live) {
            if (sums) {
#pragma unroll
                for (int c = 0; c < kGradChan; ++c) {
                    if (c0 + c < p.chan) go[(int64_t)(c0 + c) * p.hw] = sum[c];
                }
            }
            if (VALUE) {
                if (values && wave == kGradWaves - 1) {
                    float* gf = p.grad_flow + n_img * 2 * p.hw + pix;
                    gf[0] = du; gf[p.hw] = dv;
                }
            }
        }
    }
}

// ---- the local form ------------------------------------------------------------------------------------------------------------------
template <int R>
struct Local {
    static constexpr int kSide = 2 * R + 1;
    static constexpr int kD = kSide * kSide;
    static constexpr int kHaloW = kLTileW + 2 * R;
    static constexpr int kHaloH = kLTileH + 2 * R;
    static constexpr int kHalo = kHaloW * kHaloH;
    static constexpr int kLds = kLChan * kHalo > kD * kLThreads ? kLChan * kHalo : kD * kLThreads;    // floats: the staged key, then the logits
};

template <int R, bool GRAD>
__global__ void __launch_bounds__(kLThreads) flow_propagate_local_kernel(PpParams p) {
    using L = Local<R>;
    __shared__ float s_buf[L::kLds];
    const int64_t n_img = blockIdx.y;
    const int tid = (int)threadIdx.x;
    const int lx = tid % kLTileW, ly = tid / kLTileW;
    const int tile_y = (int)(blockIdx.x / (unsigned)p.tiles_x), tile_x = (int)(blockIdx.x - (unsigned)tile_y * (unsigned)p.tiles_x);
    const int x0 = tile_x * kLTileW, y0 = tile_y * kLTileH;
    const int x = x0 + lx, y = y0 + ly;
    const bool live = x < p.w && y < p.h;
    // (a lane beyond the frame computes on the nearest pixel's query and stores nothing; its window is taken at (x, y) all the same,
    // and a position outside the frame is never loaded)
    const int64_t pix = (int64_t)(y < p.h ? y : p.h - 1) * p.w + (x < p.w ? x : p.w - 1);
    const float* own = p.query + n_img * p.query_bs + pix;
    const float* key = p.key + n_img * p.key_bs;
    const float root = sqrt_rn((float)p.chan);
    float acc[L::kD];
#pragma unroll
    for (int o = 0; o < L::kD; ++o) acc[o] = 0.0f;
#pragma unroll 1
    for (int c0 = 0; c0 < p.chan; c0 += kLChan) {
        const int cc = p.chan - c0 < kLChan ? p.chan - c0 : kLChan;
        __syncthreads();                           // (the chunk before has been read)
        for (int i = tid; i < cc * L::kHalo; i += kLThreads) {
            const int c = i / L::kHalo, r = i - c * L::kHalo;
            const int hy = r / L::kHaloW, hx = r - hy * L::kHaloW;
            const int gy = y0 - R + hy, gx = x0 - R + hx;
            const bool in = gy >= 0 && gy < p.h && gx >= 0 && gx < p.w;
            s_buf[i] = in ? key[(int64_t)(c0 + c) * p.hw + (int64_t)gy * p.w + gx] : 0.0f;
        }
        __syncthreads();
#pragma unroll 1
        for (int c = 0; c < cc; ++c) {
            const float qv = own[(int64_t)(c0 + c) * p.hw];
            const float* base = s_buf + c * L::kHalo + ly * L::kHaloW + lx;
#pragma unroll
            for (int o = 0; o < L::kD; ++o) {
                const float prod = qv * base[(o / L::kSide) * L::kHaloW + o % L::kSide];
                acc[o] = acc[o] + prod;
            }
        }
    }
    __syncthreads();                               // (the last chunk has been read: the buffer becomes the logits' columns)
    float* col = s_buf + tid;
#pragma unroll
    for (int o = 0; o < L::kD; ++o) {
        const int qy = y + o / L::kSide - R, qx = x + o % L::kSide - R;
        const bool in = qy >= 0 && qy < p.h && qx >= 0 && qx < p.w;
        col[o * kLThreads] = in ? acc[o] / root : 0.0f;                // a padded position: the logit is exactly +0
    }
    // (from here on a lane reads its own column only: no barrier)
    const float* flow = p.flow + n_img * p.flow_bs;
    const bool masked = p.mask != nullptr;
    const uint8_t* mask = masked ? p.mask + n_img * p.mask_bs : nullptr;
    if (!GRAD) {
        float m = 0.0f;
        bool started = false, any_in = false;
        {
            int dy = -R, dx = -R;
#pragma unroll 1
            for (int o = 0; o < L::kD; ++o) {
                const int qy = y + dy, qx = x + dx;
                const bool in = qy >= 0 && qy < p.h && qx >= 0 && qx < p.w;
                const bool part = !in || !masked || mask[(int64_t)qy * p.w + qx] != 0;
                if (part) {
                    const float s = col[o * kLThreads];
                    if (!started) { m = s; started = true; }
                    else if (s > m) m = s;
                    any_in = any_in || in;
                }
                if (++dx > R) { dx = -R; ++dy; }
            }
        }
        double S = 0.0, X = 0.0, Y = 0.0;
        {
            int dy = -R, dx = -R;
#pragma unroll 1
            for (int o = 0; o < L::kD; ++o) {
                const int qy = y + dy, qx = x + dx;
                const bool in = qy >= 0 && qy < p.h && qx >= 0 && qx < p.w;
                const int64_t q = in ? (int64_t)qy * p.w + qx : 0;
                const bool part = !in || !masked || mask[q] != 0;
                if (part) {
                    const double e = e_of(col[o * kLThreads], m);
                    const double u = in ? (double)flow[q] : 0.0, v = in ? (double)flow[p.hw + q] : 0.0;
                    const double ex = e * u, ey = e * v;
                    S = S + e; X = X + ex; Y = Y + ey;
                }
                if (++dx > R) { dx = -R; ++dy; }
            }
        }
        if (!live) return;
        const double ox = any_in ? X / S : 0.0, oy = any_in ? Y / S : 0.0;
        float* out = p.out + n_img * 2 * p.hw + pix;
        out[0] = (float)ox;
        out[p.hw] = (float)oy;
        if (p.valid != nullptr) p.valid[n_img * p.hw + pix] = any_in ? 1 : 0;
        if (p.ws_d != nullptr) save_stats(p, n_img, pix, any_in ? m : 0.0f, any_in ? S : 0.0, ox, oy);
    } else {
        const Saved sv = saved_of(p, n_img, pix);
        const bool empty = sv.S == 0.0;
        float* sc = p.scratch + n_img * p.planes * L::kD * p.hw + pix;
        int dy = -R, dx = -R;
#pragma unroll 1
        for (int o = 0; o < L::kD; ++o) {
            const int qy = y + dy, qx = x + dx;
            const bool in = qy >= 0 && qy < p.h && qx >= 0 && qx < p.w;
            const int64_t q = in ? (int64_t)qy * p.w + qx : 0;
            const bool zero = !in || empty || (masked && mask[q] == 0);                  // (a padded position has no gradient)
            const double u = in ? (double)flow[q] : 0.0, v = in ? (double)flow[p.hw + q] : 0.0;
            const Pair r = pair_of(col[o * kLThreads], root, sv.m, sv.S, sv.ox, sv.oy, sv.Gx, sv.Gy, u, v, zero);
            if (live) {
                sc[(int64_t)o * p.hw] = r.dss;
                if (p.planes == 3) {
                    sc[(int64_t)(L::kD + o) * p.hw] = r.tx;
                    sc[(int64_t)(2 * L::kD + o) * p.hw] = r.ty;
                }
            }
            if (++dx > R) { dx = -R; ++dy; }
        }
    }
}

// d query (OTHER false): sum over the offsets o ascending of dss(p, o) * key_c(p + o); d key, d u, d v (OTHER true): sum over the pixels
// p = q - o ascending -- the offsets DEscending -- of dss(p, o) * query_c(p), of tx(p, o), of ty(p, o).  Positions inside the frame only
template <int R, bool OTHER>
__global__ void __launch_bounds__(kGatherThreads) flow_propagate_local_gather_kernel(PpParams p) {
    using L = Local<R>;
    const int64_t n_img = blockIdx.y;
    const int64_t pix = (int64_t)blockIdx.x * kGatherThreads + threadIdx.x;
    if (pix >= p.hw) return;
    const int y = (int)(pix / p.w), x = (int)(pix - (int64_t)y * p.w);
    const float* sc = p.scratch + n_img * p.planes * L::kD * p.hw;
    const float* walked = OTHER ? p.query + n_img * p.query_bs : p.key + n_img * p.key_bs;
    // step i of the sum: offset o = i (d query) or kD - 1 - i (the others); the other end of the pair is pix + sign * (dy w + dx)
    float d[L::kD];
    float du = 0.0f, dv = 0.0f;
    const bool values = OTHER && p.grad_flow != nullptr;
#pragma unroll
    for (int i = 0; i < L::kD; ++i) {
        const int o = OTHER ? L::kD - 1 - i : i;
        const int dy = o / L::kSide - R, dx = o % L::kSide - R;
        const int ty = OTHER ? y - dy : y + dy, tx = OTHER ? x - dx : x + dx;
        const bool in = ty >= 0 && ty < p.h && tx >= 0 && tx < p.w;
        const int64_t at = OTHER ? (int64_t)ty * p.w + tx : pix;       // the pixel p of the pair, whose workspace entry this is
        d[i] = in ? sc[(int64_t)o * p.hw + at] : 0.0f;
        if (OTHER) {
            if (values && in) {
                du = du + sc[(int64_t)(L::kD + o) * p.hw + at];
                dv = dv + sc[(int64_t)(2 * L::kD + o) * p.hw + at];
            }
        }
    }
    if (values) {
        float* gf = p.grad_flow + n_img * 2 * p.hw + pix;
        gf[0] = du; gf[p.hw] = dv;
    }
    if (p.grad == nullptr) return;
    float* go = p.grad + n_img * p.chan * p.hw + pix;
#pragma unroll 1
    for (int c = 0; c < p.chan; ++c) {
        const float* plane = walked + (int64_t)c * p.hw;
        float sum = 0.0f;
#pragma unroll
        for (int i = 0; i < L::kD; ++i) {
            const int o = OTHER ? L::kD - 1 - i : i;
            const int dy = o / L::kSide - R, dx = o % L::kSide - R;
            const int ty = OTHER ? y - dy : y + dy, tx = OTHER ? x - dx : x + dx;
            if (ty >= 0 && ty < p.h && tx >= 0 && tx < p.w) {
                const float prod = d[i] * plane[(int64_t)ty * p.w + tx];
                sum = sum + prod;
            }
        }
        go[(int64_t)c * p.hw] = sum;
    }
}

// the frame and the operands: the fields and the checks all four entry points share
int fill_frame(PpParams* p, const float* query, int64_t query_bs, const float* key, int64_t key_bs, int32_t channels, const float* flow,
               int64_t flow_bs, const uint8_t* mask, int64_t mask_bs, int32_t n, int32_t h, int32_t w) {
    if (!dims_ok(n, h, w, 1)) return OFL_E_ARG;
    if (h > kMaxExtent || w > kMaxExtent) return OFL_E_ARG;
    if (channels < 1) return OFL_E_ARG;
    if (query == nullptr || key == nullptr || flow == nullptr) return OFL_E_ARG;
    if (query_bs < 0 || key_bs < 0 || flow_bs < 0 || mask_bs < 0) return OFL_E_ARG;
    if (!aligned(query, 4) || !aligned(key, 4) || !aligned(flow, 4)) return OFL_E_ARG;
    p->query = query; p->key = key; p->query_bs = query_bs; p->key_bs = key_bs;
    p->flow = flow; p->flow_bs = flow_bs; p->mask = mask; p->mask_bs = mask_bs;
    p->hw = (int64_t)h * w; p->nhw = (int64_t)n * p->hw;
    p->chan = channels; p->h = h; p->w = w;
    p->tiles_x = (w + kLTileW - 1) / kLTileW; p->planes = 0;
    p->out = nullptr; p->valid = nullptr; p->ws_d = nullptr; p->ws_m = nullptr; p->g = nullptr; p->grad = nullptr;
    p->grad_flow = nullptr; p->scratch = nullptr;
    return OFL_OK;
}

// the workspace [3][n][H W] float64, then [n][H W] float32
void fill_workspace(PpParams* p, void* workspace) {
    p->ws_d = reinterpret_cast<double*>(workspace);
    p->ws_m = workspace == nullptr ? nullptr : reinterpret_cast<float*>(p->ws_d + 3 * p->nhw);
}

dim3 grid_of(const PpParams& p, int32_t n) {
    return dim3((unsigned)((p.hw + kTileP - 1) / kTileP), (unsigned)n);                  // (H W < 2^31: under 2^25 blocks)
}

dim3 tiles_of(const PpParams& p, int32_t n) {
    const int64_t tiles_y = (p.h + kLTileH - 1) / kLTileH;                              // (H W < 2^31: under 2^29 tiles)
    return dim3((unsigned)(tiles_y * p.tiles_x), (unsigned)n);
}

dim3 gather_of(const PpParams& p, int32_t n) {
    return dim3((unsigned)((p.hw + kGatherThreads - 1) / kGatherThreads), (unsigned)n);
}

template <int R>
void launch_local(const PpParams& p, int32_t n, hipStream_t s) {
    OFL_KLAUNCH((flow_propagate_local_kernel<R, false>), tiles_of(p, n), dim3(kLThreads), 0, s, p);
}

template <int R>
void launch_local_grad(PpParams p, float* grad_query, float* grad_key, float* grad_flow, int32_t n, hipStream_t s) {
    OFL_KLAUNCH((flow_propagate_local_kernel<R, true>), tiles_of(p, n), dim3(kLThreads), 0, s, p);
    if (grad_query != nullptr) {
        p.grad = grad_query; p.grad_flow = nullptr;
        OFL_KLAUNCH((flow_propagate_local_gather_kernel<R, false>), gather_of(p, n), dim3(kGatherThreads), 0, s, p);
    }
    if (grad_key != nullptr || grad_flow != nullptr) {
        p.grad = grad_key; p.grad_flow = grad_flow;
        OFL_KLAUNCH((flow_propagate_local_gather_kernel<R, true>), gather_of(p, n), dim3(kGatherThreads), 0, s, p);
    }
}

}  // namespace

extern "C" {

__attribute__((visibility("default"))) int ofl_flow_propagate_global_f32(const float* query, int64_t query_bs, const float* key,
                                                                         int64_t key_bs, int32_t channels, const float* flow,
                                                                         int64_t flow_bs, const uint8_t* mask, int64_t mask_bs, float* out,
                                                                         uint8_t* valid, void* workspace, int32_t n, int32_t h, int32_t w,
                                                                         void* stream) {
    PpParams p;
    const int rc = fill_frame(&p, query, query_bs, key, key_bs, channels, flow, flow_bs, mask, mask_bs, n, h, w);
    if (rc) return rc;
    if (out == nullptr) return OFL_E_ARG;
    if (!aligned(out, 4) || !aligned(workspace, 8)) return OFL_E_ARG;
    p.out = out; p.valid = valid;
    fill_workspace(&p, workspace);
    OFL_KLAUNCH(flow_propagate_global_kernel, grid_of(p, n), dim3(kThreads), 0, (hipStream_t)stream, p);
    return (int)hipGetLastError();
}

__attribute__((visibility("default"))) int ofl_flow_propagate_global_grad_f32(const float* query, int64_t query_bs, const float* key,
                                                                              int64_t key_bs, int32_t channels, const float* flow,
                                                                              int64_t flow_bs, const uint8_t* mask, int64_t mask_bs,
                                                                              const void* workspace, const float* grad_out,
                                                                              float* grad_query, float* grad_key, float* grad_flow,
                                                                              int32_t n, int32_t h, int32_t w, void* stream) {
    PpParams p;
    const int rc = fill_frame(&p, query, query_bs, key, key_bs, channels, flow, flow_bs, mask, mask_bs, n, h, w);
    if (rc) return rc;
    if (workspace == nullptr || grad_out == nullptr || (grad_query == nullptr && grad_key == nullptr && grad_flow == nullptr)) return OFL_E_ARG;
    if (!aligned(workspace, 8) || !aligned(grad_out, 4) || !aligned(grad_query, 4) || !aligned(grad_key, 4) || !aligned(grad_flow, 4)) {
        return OFL_E_ARG;
    }
    fill_workspace(&p, const_cast<void*>(workspace));
    p.g = grad_out;
    hipStream_t s = (hipStream_t)stream;
    if (grad_query != nullptr) {
        p.grad = grad_query;
        OFL_KLAUNCH((flow_propagate_global_grad_kernel<false, false>), grid_of(p, n), dim3(kGradThreads), 0, s, p);
    }
    if (grad_flow != nullptr) {
        p.grad = grad_key; p.grad_flow = grad_flow;
        OFL_KLAUNCH((flow_propagate_global_grad_kernel<true, true>), grid_of(p, n), dim3(kGradThreads), 0, s, p);
    } else if (grad_key != nullptr) {
        p.grad = grad_key;
        OFL_KLAUNCH((flow_propagate_global_grad_kernel<true, false>), grid_of(p, n), dim3(kGradThreads), 0, s, p);
    }
    return (int)hipGetLastError();
}

__attribute__((visibility("default"))) int ofl_flow_propagate_local_f32(const float* query, int64_t query_bs, const float* key,
                                                                        int64_t key_bs, int32_t channels, const float* flow,
                                                                        int64_t flow_bs, const uint8_t* mask, int64_t mask_bs, int32_t radius,
                                                                        float* out, uint8_t* valid, void* workspace, int32_t n, int32_t h,
                                                                        int32_t w, void* stream) {
    PpParams p;
    const int rc = fill_frame(&p, query, query_bs, key, key_bs, channels, flow, flow_bs, mask, mask_bs, n, h, w);
    if (rc) return rc;
    if (radius < 1 || radius > kMaxRadius) return OFL_E_ARG;
    if (out == nullptr) return OFL_E_ARG;
    if (!aligned(out, 4) || !aligned(workspace, 8)) return OFL_E_ARG;
    p.out = out; p.valid = valid;
    fill_workspace(&p, workspace);
    hipStream_t s = (hipStream_t)stream;
    switch (radius) {
        case 1: launch_local<1>(p, n, s); break;
        case 2: launch_local<2>(p, n, s); break;
        case 3: launch_local<3>(p, n, s); break;
        default: launch_local<4>(p, n, s); break;
    }
    return (int)hipGetLastError();
}

__attribute__((visibility("default"))) int ofl_flow_propagate_local_grad_f32(const float* query, int64_t query_bs, const float* key,
                                                                             int64_t key_bs, int32_t channels, const float* flow,
                                                                             int64_t flow_bs, const uint8_t* mask, int64_t mask_bs,
                                                                             int32_t radius, const void* workspace, const float* grad_out,
                                                                             float* scratch, float* grad_query, float* grad_key,
                                                                             float* grad_flow, int32_t n, int32_t h, int32_t w,
                                                                             void* stream) {
    PpParams p;
    const int rc = fill_frame(&p, query, query_bs, key, key_bs, channels, flow, flow_bs, mask, mask_bs, n, h, w);
    if (rc) return rc;
    if (radius < 1 || radius > kMaxRadius) return OFL_E_ARG;
    if (workspace == nullptr || grad_out == nullptr || scratch == nullptr) return OFL_E_ARG;
    if (grad_query == nullptr && grad_key == nullptr && grad_flow == nullptr) return OFL_E_ARG;
    if (!aligned(workspace, 8) || !aligned(grad_out, 4) || !aligned(scratch, 4) || !aligned(grad_query, 4) || !aligned(grad_key, 4) ||
        !aligned(grad_flow, 4)) {
        return OFL_E_ARG;
    }
    fill_workspace(&p, const_cast<void*>(workspace));
    p.g = grad_out; p.scratch = scratch;
    p.planes = grad_flow != nullptr ? 3 : 1;
    hipStream_t s = (hipStream_t)stream;
    switch (radius) {
        case 1: launch_local_grad<1>(p, grad_query, grad_key, grad_flow, n, s); break;
        case 2: launch_local_grad<2>(p, grad_query, grad_key, grad_flow, n, s); break;
        case 3: launch_local_grad<3>(p, grad_query, grad_key, grad_flow, n, s); break;
        default: launch_local_grad<4>(p, grad_query, grad_key, grad_flow, n, s); break;
    }
    return (int)hipGetLastError();
}

}  // extern "C"
