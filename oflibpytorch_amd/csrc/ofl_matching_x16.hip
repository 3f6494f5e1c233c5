// ofl_matching_x16.hip -- Flow.from_matching of fp16 / bf16 features on the matrix cores of gfx950 (which DEFINES the
// numbers; tests/matching_x16_oracle.py holds them to the float64 evaluation of tests/matching_oracle.py).  The float32 route and its
// bits are ofl_matching.hip and stay as they are; the backward of this route is that file's gradient kernels on the statistics saved here.
//
//   match_x16_pack_kernel                 a pre-pass: both tensors [*,C,h,w] to pixel-major rows [n][kQPad rows][kKStep channels padded],
//                                         16-bit, every padded channel and every padded row ZERO, so that an operand fragment of the
//                                         MFMA is one 16-byte load and padding multiplies zero with zero
//   flow_global_match_x16_kernel<T, HOIST>  one launch, the structure of fused attention with a two-column value matrix.  A block is ONE
//                                         wave and owns kTileP = 64 pixels, two sub-tiles of kSubP = 32.  It walks `other` in chunks
//                                         of kChunkQ = 32 positions: the logits of a chunk are TRANSPOSED, `other` the A operand and
//                                         `feat` the B operand of v_mfma_f32_32x32x16_{f16,bf16}, so that a lane's 16 accumulator
//                                         registers hold kLaneQ = 16 walked positions of ONE pixel (column = lane & 31) and the online
//                                         softmax needs no cross-lane step inside the walk: a lane keeps (m, S, X, Y) of its half of
//                                         the positions and the two halves of a pixel (lanes l and l + 32) are merged once at the end.
//                                         HOIST: at most kRegSteps K steps -- the pixels' fragments stay in registers for the whole
//                                         walk and the next chunk's are loaded while the softmax of this one runs
//
// No logit is written to memory.  The sums inside a chunk are float32 (16 terms a lane), the sums across chunks float64 with the float64
// rescale of 3.27.  No atomics: the same bits on any run and in any batch.
// C ABI: include/oflib_hip.h.
#include "ofl_loss_common.hpp"

namespace {

using namespace ofl_loss;

constexpr int kTileP = 64;                         // pixels a block owns: two sub-tiles of its single wave
constexpr int kSubP = 32;                          // pixels of one MFMA tile: its columns
constexpr int kChunkQ = 32;                        // walked positions of one MFMA tile: its rows
constexpr int kLaneQ = 16;                         // of them in one lane's accumulator registers: a float32 chunk sum has this many terms
constexpr int kKStep = 16;                         // channels of one MFMA: C is padded to a multiple with zeros
constexpr int kRegSteps = 8;                       // K steps whose pixel fragments stay in registers (C <= 128)
constexpr int kQPad = 64;                          // the packed rows are padded to a multiple: whole pixel tiles, whole chunks
constexpr int kThreads = 64;
constexpr int kWavesPerSimd = 2;                   // compiled for two waves per SIMD: one softmax runs beside the other's MFMAs
constexpr int kPackThreads = 256;
constexpr int kMaxExtent = 1 << 24;
constexpr float kLog2e = 1.44269504088896340736f;  // the float32 nearest to log2(e): exp(x) is v_exp_f32 of the float32 product x * kLog2e

static_assert(kTileP == 2 * kSubP && kThreads == 64 && kChunkQ == 32 && kLaneQ == kChunkQ / 2, "the 32x32x16 tile on one wave");
static_assert(kQPad % kTileP == 0 && kQPad % kChunkQ == 0, "padded rows hold whole tiles and whole chunks");

struct half_t {};
struct bf16_t {};

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ f32x16 mfma_of(half_t, uint4 a, uint4 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}
__device__ __forceinline__ f32x16 mfma_of(bf16_t, uint4 a, uint4 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

struct GxParams {
    const uint16_t* feat; const uint16_t* other;   // [*,C,H,W], the 16-bit patterns
    int64_t feat_bs, other_bs;                     // elements between images
    int64_t hw, nhw, rows;                         // H W; n H W; H W rounded up to kQPad
    int32_t chan, cpad, h, w;                      // C; C rounded up to kKStep
    float flow_sign, inv_root;                     // kInvRoot: the float32 nearest to 1 / sqrt(C), computed in float64 on the host
    uint4* pack_feat; uint4* pack_other;           // [n][rows][cpad] 16-bit each, as 16-byte groups of 8 channels
    float* out; float* prob;
    double* ws_d; float* ws_m;
};

// [*,C,H W] planes to [n][rows][cpad] rows: a thread owns 8 consecutive channels of one row (pixels along the lanes: the loads coalesce)
__global__ void __launch_bounds__(kPackThreads) match_x16_pack_kernel(GxParams p) {
    const int64_t n_img = blockIdx.y;
    const bool second = blockIdx.z != 0;
    const uint16_t* src = second ? p.other + n_img * p.other_bs : p.feat + n_img * p.feat_bs;
    const int groups = p.cpad / 8;
    uint4* dst = (second ? p.pack_other : p.pack_feat) + n_img * p.rows * groups;
    const int64_t total = p.rows * groups;
    for (int64_t i = (int64_t)blockIdx.x * kPackThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kPackThreads) {
        const int64_t row = i % p.rows;
        const int g = (int)(i / p.rows);
        uint32_t v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int c = g * 8 + k;
            v[k] = (row < p.hw && c < p.chan) ? (uint32_t)src[(int64_t)c * p.hw + row] : 0u;
        }
        uint4 o;
        o.x = v[0] | (v[1] << 16); o.y = v[2] | (v[3] << 16); o.z = v[4] | (v[5] << 16); o.w = v[6] | (v[7] << 16);
        dst[row * groups + g] = o;
    }
}

// the running softmax of a lane's half of the positions of one pixel
struct Chain {
    float m;
    double S, X, Y;
};

// exp(x) for x <= 0 (and NaN): v_exp_f32 of the float32 product x * kLog2e.  Exactly 1 at 0, exactly +0 below -128
__device__ __forceinline__ float exp_of(float x) { return __builtin_amdgcn_exp2f(x * kLog2e); }

// One chunk into the chain of a lane: the lane's kLaneQ logits are acc[r] * inv_root, register r being row (r & 3) + 8 (r >> 2) + 4 half
// of the chunk; FULL: every row is a position of the frame, else rows at or beyond `cnt` take no part, neither weight nor maximum
template <bool FULL>
__device__ __forceinline__ void chain_chunk(Chain& k, const f32x16& acc, float inv_root, const float (&qx)[kLaneQ],
                                            const float (&qy)[kLaneQ], int half, int cnt) {
    float s[kLaneQ];
    float mc = -INFINITY;
#pragma unroll
    for (int r = 0; r < kLaneQ; ++r) {
        s[r] = acc[r] * inv_root;
        const bool in = FULL || ((r & 3) + 8 * (r >> 2) + 4 * half) < cnt;
        mc = in ? fmaxf(mc, s[r]) : mc;
    }
    if (mc > k.m) {                                // the rescale of 3.27, float64 (from -inf: exp(-inf) = +0 on sums of +0)
        const double rs = exp((double)k.m - (double)mc);
        k.S = k.S * rs; k.X = k.X * rs; k.Y = k.Y * rs;
        k.m = mc;
    }
    const float mm = k.m == -INFINITY ? 0.0f : k.m; // (nothing finite seen yet: a logit of -inf has the weight exp(-inf) = +0)
    float se = 0.0f, sx = 0.0f, sy = 0.0f;
#pragma unroll
    for (int r = 0; r < kLaneQ; ++r) {
        const bool in = FULL || ((r & 3) + 8 * (r >> 2) + 4 * half) < cnt;
        const float d = s[r] - mm;
        const float e = in ? exp_of(d) : 0.0f;
        const float ex = e * qx[r], ey = e * qy[r];
        se = se + e; sx = sx + ex; sy = sy + ey;
    }
    k.S = k.S + (double)se; k.X = k.X + (double)sx; k.Y = k.Y + (double)sy;
}

// the chains of the two halves of a pixel into one, lower half first: both lanes get the same bits
__device__ __forceinline__ Chain merged(const Chain& k, int half) {
    Chain o;
    o.m = __shfl_xor(k.m, 32); o.S = __shfl_xor(k.S, 32); o.X = __shfl_xor(k.X, 32); o.Y = __shfl_xor(k.Y, 32);
    const Chain& lo = half ? o : k;
    const Chain& hi = half ? k : o;
    Chain t;
    t.m = fmaxf(lo.m, hi.m);
    const double rl = exp((double)lo.m - (double)t.m), rh = exp((double)hi.m - (double)t.m);
    const double sl = lo.S * rl, sh = hi.S * rh, xl = lo.X * rl, xh = hi.X * rh, yl = lo.Y * rl, yh = hi.Y * rh;
    t.S = sl + sh; t.X = xl + xh; t.Y = yl + yh;
    return t;
}

template <typename T, bool HOIST>
__global__ void __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(kWavesPerSimd))) flow_global_match_x16_kernel(GxParams p) {
    __shared__ __attribute__((aligned(16))) float s_qx[2][kChunkQ];       // the positions of the chunk, by chunk parity
    __shared__ __attribute__((aligned(16))) float s_qy[2][kChunkQ];
    const int64_t n_img = blockIdx.y;
    const int lane = (int)threadIdx.x;
    const int col = lane & 31, half = lane >> 5;
    const int groups = p.cpad / 8, ksteps = p.cpad / kKStep;
    const int64_t p0 = (int64_t)blockIdx.x * kTileP;                      // p0 + kTileP <= rows: the packed rows are padded
    // fragment of K step k of a row: the 16-byte groups 2 k + half of that row
    const uint4* frow0 = p.pack_feat + (n_img * p.rows + p0 + col) * groups + half;
    const uint4* frow1 = frow0 + (int64_t)kSubP * groups;
    const uint4* orow = p.pack_other + (n_img * p.rows + col) * groups + half;
    uint4 b0[HOIST ? kRegSteps : 1], b1[HOIST ? kRegSteps : 1], a[HOIST ? kRegSteps : 1];
    if (HOIST) {
#pragma unroll
        for (int k = 0; k < kRegSteps; ++k) {
            if (k < ksteps) { b0[k] = frow0[2 * k]; b1[k] = frow1[2 * k]; a[k] = orow[2 * k]; }
            else { b0[k] = make_uint4(0, 0, 0, 0); b1[k] = b0[k]; a[k] = b0[k]; }
        }
    }
    Chain k0, k1;
    k0.m = -INFINITY; k0.S = 0.0; k0.X = 0.0; k0.Y = 0.0;
    k1 = k0;
    int par = 0;
#pragma unroll 1
    for (int64_t q0 = 0; q0 < p.hw; q0 += kChunkQ, par ^= 1) {
        if (lane < kChunkQ) {                      // (q0 + lane < 2^31 + 32: fits 32 bits unsigned)
            const uint32_t q = (uint32_t)(q0 + lane);
            const uint32_t y = q / (uint32_t)p.w;
            s_qx[par][lane] = (float)(q - y * (uint32_t)p.w);
            s_qy[par][lane] = (float)y;
        }
        f32x16 acc0, acc1;
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc0[r] = 0.0f; acc1[r] = 0.0f; }
        if (HOIST) {
#pragma unroll
            for (int k = 0; k < kRegSteps; ++k) {
                if (k < ksteps) { acc0 = mfma_of(T{}, a[k], b0[k], acc0); acc1 = mfma_of(T{}, a[k], b1[k], acc1); }
            }
            // the next chunk's rows while this chunk's softmax runs (past the last chunk: this one's again, rows that exist)
            const int64_t qn = q0 + kChunkQ < p.hw ? q0 + kChunkQ : q0;
            const uint4* nrow = orow + qn * groups;
#pragma unroll
            for (int k = 0; k < kRegSteps; ++k) {
                if (k < ksteps) a[k] = nrow[2 * k];
            }
        } else {
            const uint4* arow = orow + q0 * groups;
#pragma unroll 1
            for (int k = 0; k < ksteps; ++k) {
                const uint4 av = arow[2 * k], bv0 = frow0[2 * k], bv1 = frow1[2 * k];
                acc0 = mfma_of(T{}, av, bv0, acc0);
                acc1 = mfma_of(T{}, av, bv1, acc1);
            }
        }
        __syncthreads();                           // (one wave: the table of this parity is written; the other parity's readers are done)
        float qx[kLaneQ], qy[kLaneQ];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 vx = *reinterpret_cast<const float4*>(&s_qx[par][8 * g + 4 * half]);
            const float4 vy = *reinterpret_cast<const float4*>(&s_qy[par][8 * g + 4 * half]);
            qx[4 * g] = vx.x; qx[4 * g + 1] = vx.y; qx[4 * g + 2] = vx.z; qx[4 * g + 3] = vx.w;
            qy[4 * g] = vy.x; qy[4 * g + 1] = vy.y; qy[4 * g + 2] = vy.z; qy[4 * g + 3] = vy.w;
        }
        const int64_t left = p.hw - q0;
        if (left >= kChunkQ) {
            chain_chunk<true>(k0, acc0, p.inv_root, qx, qy, half, kChunkQ);
            chain_chunk<true>(k1, acc1, p.inv_root, qx, qy, half, kChunkQ);
        } else {
            chain_chunk<false>(k0, acc0, p.inv_root, qx, qy, half, (int)left);
            chain_chunk<false>(k1, acc1, p.inv_root, qx, qy, half, (int)left);
        }
    }
    const Chain t0 = merged(k0, half), t1 = merged(k1, half);
    const Chain& k = half ? t1 : t0;               // lane l stores pixel p0 + l
    const int64_t pix = p0 + lane;
    if (pix >= p.hw) return;
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

int64_t rows_of(int32_t h, int32_t w) { return ((int64_t)h * w + kQPad - 1) / kQPad * kQPad; }
int32_t cpad_of(int32_t channels) { return (int32_t)(((int64_t)channels + kKStep - 1) / kKStep * kKStep); }

bool frame_ok(int32_t channels, int32_t n, int32_t h, int32_t w) {
    return dims_ok(n, h, w, 1) && h <= kMaxExtent && w <= kMaxExtent && channels >= 1 && channels <= INT32_MAX - kKStep;
}

template <typename T>
void launch(const GxParams& p, int32_t n, hipStream_t s) {
    const int64_t total = p.rows * (p.cpad / 8);
    const int64_t want = (total + kPackThreads - 1) / kPackThreads;
    OFL_KLAUNCH(match_x16_pack_kernel, dim3((unsigned)(want < 65536 ? want : 65536), (unsigned)n, 2), dim3(kPackThreads), 0, s, p);
    const dim3 grid((unsigned)(p.rows / kTileP), (unsigned)n);           // (H W < 2^31: under 2^25 blocks)
    if (p.cpad / kKStep <= kRegSteps) OFL_KLAUNCH((flow_global_match_x16_kernel<T, true>), grid, dim3(kThreads), 0, s, p);
    else OFL_KLAUNCH((flow_global_match_x16_kernel<T, false>), grid, dim3(kThreads), 0, s, p);
}

}  // namespace

extern "C" {

__attribute__((visibility("default"))) int64_t ofl_flow_global_match_x16_pack_bytes(int32_t channels, int32_t n, int32_t h, int32_t w) {
    if (!frame_ok(channels, n, h, w)) return OFL_E_ARG;
    return 2 * (int64_t)n * rows_of(h, w) * cpad_of(channels) * 2;
}

__attribute__((visibility("default"))) int ofl_flow_global_match_x16(const void* feat, int64_t feat_bs, const void* other, int64_t other_bs,
                                                                     int32_t channels, int32_t elem, float flow_sign, float* out,
                                                                     float* prob, void* stats, void* workspace, int32_t n, int32_t h,
                                                                     int32_t w, void* stream) {
    if (!frame_ok(channels, n, h, w)) return OFL_E_ARG;
    if (elem != OFL_X16_HALF && elem != OFL_X16_BFLOAT) return OFL_E_ARG;
    if (flow_sign != 1.0f && flow_sign != -1.0f) return OFL_E_ARG;
    if (feat == nullptr || other == nullptr || out == nullptr || workspace == nullptr) return OFL_E_ARG;
    if (feat_bs < 0 || other_bs < 0) return OFL_E_ARG;
    if (!aligned(feat, 2) || !aligned(other, 2) || !aligned(out, 4) || !aligned(prob, 4) || !aligned(stats, 8) || !aligned(workspace, 16))
        return OFL_E_ARG;
    GxParams p;
    p.feat = reinterpret_cast<const uint16_t*>(feat); p.other = reinterpret_cast<const uint16_t*>(other);
    p.feat_bs = feat_bs; p.other_bs = other_bs;
    p.hw = (int64_t)h * w; p.nhw = (int64_t)n * p.hw; p.rows = rows_of(h, w);
    p.chan = channels; p.cpad = cpad_of(channels); p.h = h; p.w = w;
    p.flow_sign = flow_sign;
    p.inv_root = (float)(1.0 / sqrt((double)channels));                  // kInvRoot of DESIGN.md 3.32: the float32 nearest to 1 / sqrt(C)
    p.pack_feat = reinterpret_cast<uint4*>(workspace);
    p.pack_other = p.pack_feat + (int64_t)n * p.rows * (p.cpad / 8);
    p.out = out; p.prob = prob;
    p.ws_d = reinterpret_cast<double*>(stats);
    p.ws_m = stats == nullptr ? nullptr : reinterpret_cast<float*>(p.ws_d + 3 * p.nhw);
    if (elem == OFL_X16_HALF) launch<half_t>(p, n, (hipStream_t)stream);
    else launch<bf16_t>(p, n, (hipStream_t)stream);
    return (int)hipGetLastError();
}

}  // extern "C"
