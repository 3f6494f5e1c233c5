// ofl_sequence_loss.hip -- Flow.sequence_loss / sequence_stats on gfx950: the T refinement outputs of a flow network scored against one
// ground truth, RAFT's gamma-weighted sequence loss (which DEFINES the numbers; tests/sequence_loss_oracle.py is the same
// definition in NumPy).  An extension: the reference has no such function.
//
//   flow_sequence_loss_kernel          one pass over the ground truth, its mask and all T predictions ((8 T + 9) B/px in fp32): per block ONE
//                                      record of 2 T + 4 float64 values -- count, T sums of the penalty, T sums of the end-point error, the
//                                      pixels of the last prediction under 1, 3 and 5 px
//   flow_sequence_loss_finish_kernel   one block per image: the block records added in ascending block order
//   flow_sequence_loss_grad_kernel     the backward with respect to every prediction that wants one, from one read of the ground truth
//
// A block owns kChunk consecutive pixels of one image; a lane takes kQuads groups of 4 consecutive pixels, kThreads groups apart.  It
// reads the ground truth and the mask of its pixels ONCE, keeps the vectors and the valid bits in registers and walks the predictions past
// them, so only the two float64 sums of one prediction are live at a time.  16-byte loads of the vector planes (8 bytes of an fp16-stored
// flow), 4-byte loads of the mask and 16-byte stores of the gradients where H*W, the batch strides and the pointers allow (chosen per
// launch), else one element at a time with bounds checks: both forms give a lane the same pixels, so the choice changes no bit.  The
// predictions' base pointers, batch strides and storage kinds travel by value in the kernel arguments.  The sums follow
// ofl_loss_common.hpp: a lane's pixels ascending, the lanes by a butterfly, the waves and then the blocks in index order; no float
// atomics.  C ABI: include/oflib_hip.h.
#include "ofl_loss_common.hpp"

namespace {

using namespace ofl_loss;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kQuads = 2;                                   // groups of 4 pixels per lane
constexpr int kChunk = OFL_SEQUENCE_LOSS_CHUNK;             // pixels per block
static_assert(kChunk == kThreads * 4 * kQuads, "the chunk is what a block's lanes hold in registers");
constexpr int kMaxT = OFL_SEQUENCE_LOSS_MAX_T;
constexpr int kMaxRec = 2 * kMaxT + 4;                      // doubles of the longest record
constexpr int kFinishDoubles = 32 * kMaxRec;                // LDS of the finish kernel: at least 32 block records at a time
constexpr float kWithin[3] = {1.0f, 3.0f, 5.0f};

struct Pred {
    const void* base;                                       // [*,2,H,W] fp32 or fp16
    int64_t bs_kind;                                        // (elements between images) << 1 | (1: fp16)
};

struct SeqParams {
    Pred pred[kMaxT];
    const void* gt; int64_t gt_bs;                          // [*,2,H,W] fp32 or fp16
    const uint8_t* mask; int64_t mask_bs;                   // [*,H,W] bytes or nullptr (all True)
    int64_t hw;
    int32_t t, gt_half, l2, nblk;
    float max_flow;
    double* partial;                                        // [n][nblk][2 t + 4]
    double* out;                                            // [n][2 t + 4]
    const float* scale;                                     // backward: [n][t]
};

struct GradPtrs { float* g[kMaxT]; };                       // backward: [n][2][H*W] each, or nullptr (not wanted)

// four consecutive elements p0 .. p0 + 3 of one plane (`base` + o: its first element), 0 for those past the image; VEC: H*W is a
// multiple of 4 and the access is aligned
template <bool VEC>
__device__ __forceinline__ void ld4(const void* base, bool half, int64_t o, int64_t p0, int64_t hw, float v[4]) {
    if (VEC) {
        v[0] = v[1] = v[2] = v[3] = 0.0f;
        if (p0 < hw) {
            if (half) {
                const uint2 u = *reinterpret_cast<const uint2*>(reinterpret_cast<const __half*>(base) + o + p0);
                const __half2 a = *reinterpret_cast<const __half2*>(&u.x), b = *reinterpret_cast<const __half2*>(&u.y);
                v[0] = __low2float(a); v[1] = __high2float(a); v[2] = __low2float(b); v[3] = __high2float(b);
            } else {
                const float4 f = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(base) + o + p0);
                v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            v[k] = 0.0f;
            if (p0 + k < hw) v[k] = half ? ld_flow<true>(base, o + p0 + k) : ld_flow<false>(base, o + p0 + k);
        }
    }
}

// bit k: pixel p0 + k exists and is True in `mask` (nullptr: all True)
template <bool VEC>
__device__ __forceinline__ uint32_t mask4(const uint8_t* mask, int64_t o, int64_t p0, int64_t hw) {
    uint32_t bits = 0u;
    if (VEC) {
        if (p0 >= hw) return 0u;
        if (mask == nullptr) return 15u;
        const uint32_t m = *reinterpret_cast<const uint32_t*>(mask + o + p0);
#pragma unroll
        for (int k = 0; k < 4; ++k) bits |= ((m >> (8 * k)) & 0xffu) ? (1u << k) : 0u;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (p0 + k < hw && (mask == nullptr || mask[o + p0 + k] != 0)) bits |= 1u << k;
    }
    return bits;
}

// first pixel of group s of this lane
__device__ __forceinline__ int64_t group_pixel(int s) {
    return (int64_t)blockIdx.x * kChunk + 4 * (int64_t)(s * kThreads + (int)threadIdx.x);
}

// the ground truth of this lane's pixels and their valid bits (bit 4 s + k: pixel k of group s): in the mask and mag < max_flow, a float
// compare that a NaN or infinite magnitude fails
template <bool VEC>
__device__ __forceinline__ uint32_t load_truth(const SeqParams& p, int64_t img, float ug[kQuads][4], float vg[kQuads][4]) {
    uint32_t valid = 0u;
#pragma unroll
    for (int s = 0; s < kQuads; ++s) {
        const int64_t p0 = group_pixel(s);
        ld4<VEC>(p.gt, p.gt_half != 0, img * p.gt_bs, p0, p.hw, ug[s]);
        ld4<VEC>(p.gt, p.gt_half != 0, img * p.gt_bs + p.hw, p0, p.hw, vg[s]);
        uint32_t bits = mask4<VEC>(p.mask, img * p.mask_bs, p0, p.hw);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float mag = sqrt_rn(ug[s][k] * ug[s][k] + vg[s][k] * vg[s][k]);
            bits &= (mag < p.max_flow) ? ~0u : ~(1u << k);
        }
        valid |= bits << (4 * s);
    }
    return valid;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

template <bool VEC>
__global__ void __launch_bounds__(kThreads) flow_sequence_loss_kernel(SeqParams p) {
    __shared__ double s_red[kWaves * kMaxRec];
    const int64_t img = blockIdx.y;
    const int wave = threadIdx.x >> 6;
    const bool first = (threadIdx.x & 63) == 0;
    const int t = p.t;
    float ug[kQuads][4], vg[kQuads][4];
    const uint32_t valid = load_truth<VEC>(p, img, ug, vg);
    uint32_t within[3] = {0u, 0u, 0u};
    for (int i = 0; i < t; ++i) {
        const bool half = (p.pred[i].bs_kind & 1) != 0;
        const int64_t o = img * (p.pred[i].bs_kind >> 1);
        const void* base = p.pred[i].base;
        float u[kQuads][4], v[kQuads][4];
#pragma unroll
        for (int s = 0; s < kQuads; ++s) {
            ld4<VEC>(base, half, o, group_pixel(s), p.hw, u[s]);
            ld4<VEC>(base, half, o + p.hw, group_pixel(s), p.hw, v[s]);
        }
        double st = 0.0, se = 0.0;
#pragma unroll
        for (int s = 0; s < kQuads; ++s) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool on = (valid >> (4 * s + k)) & 1u;
                const float du = u[s][k] - ug[s][k], dv = v[s][k] - vg[s][k];
                const float e = sqrt_rn(du * du + dv * dv);
                const float term = p.l2 ? e : fabsf(du) + fabsf(dv);
                st += on ? (double)term : 0.0;
                se += on ? (double)e : 0.0;
                if (i == t - 1) {
#pragma unroll
                    for (int j = 0; j < 3; ++j) within[j] += (on && e < kWithin[j]) ? 1u : 0u;
                }
            }
        }
        st = wave_sum(st);
        se = wave_sum(se);
        if (first) { s_red[wave * kMaxRec + 1 + i] = st; s_red[wave * kMaxRec + 1 + t + i] = se; }
    }
    const double cnt = wave_sum((double)__popc(valid));
    double win[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) win[j] = wave_sum((double)within[j]);
    if (first) {
        s_red[wave * kMaxRec] = cnt;
#pragma unroll
        for (int j = 0; j < 3; ++j) s_red[wave * kMaxRec + 1 + 2 * t + j] = win[j];
    }
    __syncthreads();
    const int rec = 2 * t + 4;
    if ((int)threadIdx.x < rec) {
        double s = s_red[threadIdx.x];
        for (int wv = 1; wv < kWaves; ++wv) s += s_red[wv * kMaxRec + threadIdx.x];
        p.partial[(img * p.nblk + blockIdx.x) * rec + threadIdx.x] = s;
    }
}

// one block per image: finish_records() of ofl_loss_common.hpp with the record's length at run time -- the block records staged in LDS by
// all threads, as many at a time as fit, then slot i added in ascending block order by thread i
__global__ void __launch_bounds__(kThreads) flow_sequence_loss_finish_kernel(const double* partial, int nblk, int rec, double* out) {
    __shared__ double s_part[kFinishDoubles];
    const int64_t n_img = blockIdx.x;
    const double* part = partial + n_img * nblk * rec;
    const int chunk = kFinishDoubles / rec;
    double s = 0.0;
    for (int base = 0; base < nblk; base += chunk) {
        const int cnt = nblk - base < chunk ? nblk - base : chunk;
        for (int i = threadIdx.x; i < cnt * rec; i += kThreads) s_part[i] = part[(int64_t)base * rec + i];
        __syncthreads();
        if ((int)threadIdx.x < rec) {
            for (int b = 0; b < cnt; ++b) s += s_part[b * rec + threadIdx.x];
        }
        __syncthreads();
    }
    if ((int)threadIdx.x < rec) out[n_img * rec + threadIdx.x] = s;
}

// 'l1': scale * sign(d), +0 where d is 0 or NaN (torch's abs).  'l2': (scale d) / sqrt(du du + dv dv), the float64 quotient of the fp32
// differences rounded once, +0 where the fp32 sum of squares is not > 0 (ofl_metrics.hip).  +0 at every pixel that is not valid.
template <bool VEC>
__global__ void __launch_bounds__(kThreads) flow_sequence_loss_grad_kernel(SeqParams p, GradPtrs gp) {
    const int64_t img = blockIdx.y;
    const int t = p.t;
    float ug[kQuads][4], vg[kQuads][4];
    const uint32_t valid = load_truth<VEC>(p, img, ug, vg);
    for (int i = 0; i < t; ++i) {
        float* go = gp.g[i];
        if (go == nullptr) continue;
        const bool half = (p.pred[i].bs_kind & 1) != 0;
        const int64_t o = img * (p.pred[i].bs_kind >> 1);
        const void* base = p.pred[i].base;
        const float sc = p.scale[img * t + i];
        float u[kQuads][4], v[kQuads][4];
#pragma unroll
        for (int s = 0; s < kQuads; ++s) {
            ld4<VEC>(base, half, o, group_pixel(s), p.hw, u[s]);
            ld4<VEC>(base, half, o + p.hw, group_pixel(s), p.hw, v[s]);
        }
#pragma unroll
        for (int s = 0; s < kQuads; ++s) {
            float gu[4], gv[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool on = (valid >> (4 * s + k)) & 1u;
                const float du = u[s][k] - ug[s][k], dv = v[s][k] - vg[s][k];
                if (p.l2) {
                    const bool pos = on && (du * du + dv * dv > 0.0f);
                    const double dx = (double)du, dy = (double)dv;
                    const double e = sqrt(dx * dx + dy * dy);
                    gu[k] = pos ? (float)(((double)sc * dx) / e) : 0.0f;
                    gv[k] = pos ? (float)(((double)sc * dy) / e) : 0.0f;
                } else {
                    gu[k] = (on && du > 0.0f) ? sc : ((on && du < 0.0f) ? -sc : 0.0f);
                    gv[k] = (on && dv > 0.0f) ? sc : ((on && dv < 0.0f) ? -sc : 0.0f);
                }
            }
            const int64_t p0 = group_pixel(s);
            float* gq = go + img * 2 * p.hw + p0;
            if (VEC) {
                if (p0 < p.hw) {
                    *reinterpret_cast<float4*>(gq) = make_float4(gu[0], gu[1], gu[2], gu[3]);
                    *reinterpret_cast<float4*>(gq + p.hw) = make_float4(gv[0], gv[1], gv[2], gv[3]);
                }
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (p0 + k < p.hw) { gq[k] = gu[k]; gq[p.hw + k] = gv[k]; }
                }
            }
        }
    }
}

int64_t blocks_of(int64_t hw) { return (hw + kChunk - 1) / kChunk; }

// the checks both launches share, all before any launch, and the operands they fill
int fill_operands(SeqParams* p, const void* const* preds, const int64_t* pred_bs, const int32_t* pred_half, int32_t t, const void* gt,
                  int64_t gt_bs, int32_t gt_half, const uint8_t* gt_mask, int64_t gt_mask_bs, float max_flow, int32_t penalty,
                  int32_t normalise, int32_t n, int32_t h, int32_t w) {
    if (!preds || !pred_bs || !pred_half || !gt) return OFL_E_NULL;
    if (!dims_ok(n, h, w, 1) || t < 1 || t > kMaxT) return OFL_E_SHAPE;
    for (int i = 0; i < t; ++i)
        if (!preds[i]) return OFL_E_NULL;
    if (penalty != OFL_SEQUENCE_LOSS_L1 && penalty != OFL_SEQUENCE_LOSS_L2) return OFL_E_ARG;
    if (normalise != OFL_SEQUENCE_LOSS_ALL && normalise != OFL_SEQUENCE_LOSS_VALID) return OFL_E_ARG;
    if (!(max_flow > 0.0f)) return OFL_E_ARG;                                   // (NaN fails the test; +inf passes)
    if ((gt_half != 0 && gt_half != 1) || gt_bs < 0 || gt_mask_bs < 0 || !aligned(gt, gt_half ? 2 : 4)) return OFL_E_ARG;
    for (int i = 0; i < kMaxT; ++i) { p->pred[i].base = nullptr; p->pred[i].bs_kind = 0; }
    for (int i = 0; i < t; ++i) {
        if ((pred_half[i] != 0 && pred_half[i] != 1) || pred_bs[i] < 0 || pred_bs[i] >= (1ll << 62)) return OFL_E_ARG;
        if (!aligned(preds[i], pred_half[i] ? 2 : 4)) return OFL_E_ARG;
        p->pred[i].base = preds[i];
        p->pred[i].bs_kind = (int64_t)((uint64_t)pred_bs[i] << 1) | pred_half[i];
    }
    p->gt = gt; p->gt_bs = gt_bs; p->gt_half = gt_half;
    p->mask = gt_mask; p->mask_bs = gt_mask_bs;
    p->hw = (int64_t)h * w;
    p->t = t; p->l2 = penalty == OFL_SEQUENCE_LOSS_L2 ? 1 : 0;
    p->nblk = (int32_t)blocks_of(p->hw);
    p->max_flow = max_flow;
    p->partial = nullptr; p->out = nullptr; p->scale = nullptr;
    return OFL_OK;
}

// 16-byte (fp16: 8-byte) accesses of the vector planes and 4-byte accesses of the mask are aligned for every lane of every image
bool inputs_vectorise(const SeqParams& p) {
    if (p.hw % 4 != 0 || p.gt_bs % 4 != 0 || p.mask_bs % 4 != 0) return false;
    if (!aligned(p.gt, p.gt_half ? 8 : 16) || !aligned(p.mask, 4)) return false;
    for (int i = 0; i < p.t; ++i) {
        const bool half = (p.pred[i].bs_kind & 1) != 0;
        if ((p.pred[i].bs_kind >> 1) % 4 != 0 || !aligned(p.pred[i].base, half ? 8 : 16)) return false;
    }
    return true;
}

}  // namespace

extern "C" {

__attribute__((visibility("default"))) int64_t ofl_flow_sequence_loss_workspace_bytes(int32_t t, int32_t n, int32_t h, int32_t w) {
    if (!dims_ok(n, h, w, 1) || t < 1 || t > kMaxT) return OFL_E_SHAPE;
    return (int64_t)n * blocks_of((int64_t)h * w) * (2 * t + 4) * (int64_t)sizeof(double);
}

__attribute__((visibility("default"))) int ofl_flow_sequence_loss_f64(const void* const* preds, const int64_t* pred_bs,
                                                                      const int32_t* pred_half, int32_t t, const void* gt, int64_t gt_bs,
                                                                      int32_t gt_half, const uint8_t* gt_mask, int64_t gt_mask_bs,
                                                                      float max_flow, int32_t penalty, int32_t normalise, void* workspace,
                                                                      double* records, int32_t n, int32_t h, int32_t w, void* stream) {
    if (!workspace || !records) return OFL_E_NULL;
    SeqParams p;
    const int rc = fill_operands(&p, preds, pred_bs, pred_half, t, gt, gt_bs, gt_half, gt_mask, gt_mask_bs, max_flow, penalty, normalise,
                                 n, h, w);
    if (rc) return rc;
    if (!aligned(workspace, 8) || !aligned(records, 8)) return OFL_E_ARG;
    p.partial = reinterpret_cast<double*>(workspace);
    p.out = records;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)p.nblk, (unsigned)n);
    if (inputs_vectorise(p)) OFL_KLAUNCH(flow_sequence_loss_kernel<true>, grid, dim3(kThreads), 0, s, p);
    else OFL_KLAUNCH(flow_sequence_loss_kernel<false>, grid, dim3(kThreads), 0, s, p);
    OFL_KLAUNCH(flow_sequence_loss_finish_kernel, dim3((unsigned)n), dim3(kThreads), 0, s, (const double*)p.partial, (int)p.nblk, 2 * t + 4,
                p.out);
    return (int)hipGetLastError();
}

__attribute__((visibility("default"))) int ofl_flow_sequence_loss_grad_f32(const void* const* preds, const int64_t* pred_bs,
                                                                           const int32_t* pred_half, int32_t t, const void* gt,
                                                                           int64_t gt_bs, int32_t gt_half, const uint8_t* gt_mask,
                                                                           int64_t gt_mask_bs, float max_flow, int32_t penalty,
                                                                           int32_t normalise, const float* scale, float* const* grads,
                                                                           int32_t n, int32_t h, int32_t w, void* stream) {
    if (!scale || !grads) return OFL_E_NULL;
    SeqParams p;
    const int rc = fill_operands(&p, preds, pred_bs, pred_half, t, gt, gt_bs, gt_half, gt_mask, gt_mask_bs, max_flow, penalty, normalise,
                                 n, h, w);
    if (rc) return rc;
    if (!aligned(scale, 4)) return OFL_E_ARG;
    GradPtrs gp;
    bool any = false, vec = inputs_vectorise(p);
    for (int i = 0; i < kMaxT; ++i) gp.g[i] = nullptr;
    for (int i = 0; i < t; ++i) {
        if (!aligned(grads[i], 4)) return OFL_E_ARG;
        gp.g[i] = grads[i];
        any = any || grads[i] != nullptr;
        vec = vec && aligned(grads[i], 16);
    }
    if (!any) return OFL_E_NULL;
    p.scale = scale;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)p.nblk, (unsigned)n);
    if (vec) OFL_KLAUNCH(flow_sequence_loss_grad_kernel<true>, grid, dim3(kThreads), 0, s, p, gp);
    else OFL_KLAUNCH(flow_sequence_loss_grad_kernel<false>, grid, dim3(kThreads), 0, s, p, gp);
    return (int)hipGetLastError();
}

}  // extern "C"
