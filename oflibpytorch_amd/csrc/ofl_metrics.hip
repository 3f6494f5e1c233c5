// ofl_metrics.hip -- Flow.error_stats / epe_map / epe on gfx950: an estimated flow scored against a ground truth (which
// DEFINES the numbers; tests/flow_error_oracle.py is the same definition in NumPy).  An extension: the reference has no such function.
//
//   flow_error_kernel          one pass over both flows and both masks (18 B/px in fp32): the end-point error e of every pixel in fp32
//                              (optionally stored as a map, 0 where not valid) and, per block, ONE record of 16 float64 values: count,
//                              sum e, max e, the pixels over each threshold, KITTI's Fl outliers, count and sum e of three speed bins
//   flow_error_finish_kernel   one block per image: the block records added in ascending block order
//   flow_epe_grad_kernel       the backward of the per-image mean of e: scale[n] * (du, dv) / e where valid and e > 0, else 0
//
// One lane takes the 4 pixels 4 q .. 4 q + 3 of an image: 16-byte loads of the four vector planes (8 bytes of an fp16-stored flow) and
// 4-byte loads of the masks where H*W, the batch strides and the pointers allow (chosen per launch), else one element at a time with
// bounds checks.  Blocks walk an image with a grid stride; their number depends on H*W only.  The sums are those of
// ofl_loss_common.hpp; counts are integers until the record, where they are exact doubles.  C ABI: include/oflib_hip.h.
#include "ofl_loss_common.hpp"

namespace {

using namespace ofl_loss;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxBlocks = 256;                    // forward: blocks per image at most (one per CU); 1080p: each walks 7 or 8 steps of 1024 px
constexpr int kMaxGradBlocks = 2048;               // backward: elementwise, nothing to reduce
constexpr int kRec = OFL_FLOW_ERROR_RECORD;        // doubles per record
constexpr int kMaxThr = 4;
// slots of a record (include/oflib_hip.h)
enum { R_COUNT = 0, R_SUM = 1, R_MAX = 2, R_OVER = 3, R_FL = 7, R_SPEED_COUNT = 8, R_SPEED_SUM = 11 };
constexpr float kFlAbs = 3.0f, kFlRel = 0.05f;     // KITTI: an outlier is off by more than 3 px AND more than 5 % of the true speed
constexpr float kSpeed0 = 10.0f, kSpeed1 = 40.0f;  // speed bins [0, 10), [10, 40), [40, inf)

struct ErrParams {
    const void* est; const void* gt;               // [*,2,H,W] fp32 or fp16
    int64_t est_bs, gt_bs;                         // elements between images
    int32_t est_half, gt_half;
    const uint8_t* est_mask; const uint8_t* gt_mask;   // [*,H,W] bytes or nullptr (all True)
    int64_t est_mask_bs, gt_mask_bs;
    int64_t hw;
    int32_t nblk, nthr;
    float thr[kMaxThr];
    double* partial;                               // [n][nblk][kRec]
    float* map;                                    // [n][H*W] or nullptr
    double* out;                                   // [n][kRec]
    const float* scale;                            // backward: [n]
    float* grad_est; float* grad_gt;               // backward: [n][2][H*W] or nullptr
};

// four consecutive elements p0 .. p0 + 3 of one plane (`base` + o: its first element); VEC: all four exist and the access is aligned
template <bool VEC>
__device__ __forceinline__ void ld4(const void* base, bool half, int64_t o, int64_t p0, int64_t hw, float v[4]) {
    if (VEC) {
        if (half) {
            const uint2 u = *reinterpret_cast<const uint2*>(reinterpret_cast<const __half*>(base) + o + p0);
            const __half2 a = *reinterpret_cast<const __half2*>(&u.x), b = *reinterpret_cast<const __half2*>(&u.y);
            v[0] = __low2float(a); v[1] = __high2float(a); v[2] = __low2float(b); v[3] = __high2float(b);
        } else {
            const float4 f = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(base) + o + p0);
            v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            v[k] = 0.0f;
            if (p0 + k < hw) {
                v[k] = half ? __half2float(reinterpret_cast<const __half*>(base)[o + p0 + k])
                            : reinterpret_cast<const float*>(base)[o + p0 + k];
            }
        }
    }
}

// bit k: pixel p0 + k exists and is True in `mask` (nullptr: all True)
template <bool VEC>
__device__ __forceinline__ uint32_t mask4(const uint8_t* mask, int64_t o, int64_t p0, int64_t hw) {
    uint32_t bits = 0u;
    if (VEC) {
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

// the 4 pixels of lane `q`: the fp32 differences, the valid bits
template <bool VEC>
__device__ __forceinline__ uint32_t load_quad(const ErrParams& p, int64_t img, int64_t q, float du[4], float dv[4], float ug[4], float vg[4]) {
    const int64_t p0 = 4 * q;
    float u[4], v[4];
    ld4<VEC>(p.est, p.est_half, img * p.est_bs, p0, p.hw, u);
    ld4<VEC>(p.est, p.est_half, img * p.est_bs + p.hw, p0, p.hw, v);
    ld4<VEC>(p.gt, p.gt_half, img * p.gt_bs, p0, p.hw, ug);
    ld4<VEC>(p.gt, p.gt_half, img * p.gt_bs + p.hw, p0, p.hw, vg);
    const uint32_t bits = mask4<VEC>(p.est_mask, img * p.est_mask_bs, p0, p.hw) & mask4<VEC>(p.gt_mask, img * p.gt_mask_bs, p0, p.hw);
#pragma unroll
    for (int k = 0; k < 4; ++k) { du[k] = u[k] - ug[k]; dv[k] = v[k] - vg[k]; }
    return bits;
}

template <bool VEC>
__global__ void __launch_bounds__(kThreads) flow_error_kernel(ErrParams p) {
    __shared__ double s_red[kWaves * kRec];
    const int64_t img = blockIdx.y;
    const int64_t quads = (p.hw + 3) >> 2, stride = (int64_t)gridDim.x * kThreads;
    uint32_t cnt = 0u, over[kMaxThr] = {0u, 0u, 0u, 0u}, fl = 0u, scnt[3] = {0u, 0u, 0u};
    double sum = 0.0, ssum[3] = {0.0, 0.0, 0.0};
    float mx = 0.0f;
    for (int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x; q < quads; q += stride) {
        float du[4], dv[4], ug[4], vg[4], e[4];
        const uint32_t bits = load_quad<VEC>(p, img, q, du, dv, ug, vg);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool valid = (bits >> k) & 1u;
            const float ek = sqrt_rn(du[k] * du[k] + dv[k] * dv[k]);
            const float g = sqrt_rn(ug[k] * ug[k] + vg[k] * vg[k]);
            e[k] = valid ? ek : 0.0f;
            const double ed = valid ? (double)ek : 0.0;
            cnt += valid ? 1u : 0u;
            sum += ed;
            mx = (valid && ek > mx) ? ek : mx;
#pragma unroll
            for (int t = 0; t < kMaxThr; ++t) over[t] += (valid && t < p.nthr && ek > p.thr[t]) ? 1u : 0u;
            fl += (valid && ek > kFlAbs && ek > kFlRel * g) ? 1u : 0u;
            const int bin = (g < kSpeed0) ? 0 : ((g < kSpeed1) ? 1 : 2);
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                scnt[b] += (valid && bin == b) ? 1u : 0u;
                ssum[b] += (bin == b) ? ed : 0.0;
            }
        }
        if (p.map != nullptr) {
            float* mo = p.map + img * p.hw + 4 * q;
            if (VEC) {
                *reinterpret_cast<float4*>(mo) = make_float4(e[0], e[1], e[2], e[3]);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (4 * q + k < p.hw) mo[k] = e[k];
            }
        }
    }
    double rec[kRec];
#pragma unroll
    for (int i = 0; i < kRec; ++i) rec[i] = 0.0;
    rec[R_COUNT] = (double)cnt; rec[R_SUM] = sum; rec[R_MAX] = (double)mx; rec[R_FL] = (double)fl;
#pragma unroll
    for (int t = 0; t < kMaxThr; ++t) rec[R_OVER + t] = (double)over[t];
#pragma unroll
    for (int b = 0; b < 3; ++b) { rec[R_SPEED_COUNT + b] = (double)scnt[b]; rec[R_SPEED_SUM + b] = ssum[b]; }
    reduce_record<kRec, R_SPEED_SUM + 3, R_MAX, kWaves>(rec, s_red, p.partial, img, p.nblk);
}

// one block per image: the block records added in ascending block order (all of them fit one chunk)
__global__ void __launch_bounds__(kThreads) flow_error_finish_kernel(ErrParams p) {
    finish_records<kRec, R_MAX, kMaxBlocks, kThreads>(p.partial, p.nblk, p.out);
}

// d mean(e) / d est = scale * (du, dv) / e: the float64 quotient of the fp32 differences, rounded once; 0 where not valid or e == 0
// (the fp32 e of the forward pass is 0 exactly when the fp32 sum of squares is)
template <bool VEC>
__global__ void __launch_bounds__(kThreads) flow_epe_grad_kernel(ErrParams p) {
    const int64_t img = blockIdx.y;
    const int64_t quads = (p.hw + 3) >> 2, stride = (int64_t)gridDim.x * kThreads;
    const double sc = (double)p.scale[img];
    for (int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x; q < quads; q += stride) {
        float du[4], dv[4], ug[4], vg[4], gu[4], gv[4];
        const uint32_t bits = load_quad<VEC>(p, img, q, du, dv, ug, vg);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool on = ((bits >> k) & 1u) && (du[k] * du[k] + dv[k] * dv[k] > 0.0f);
            const double dx = (double)du[k], dy = (double)dv[k];
            const double e = sqrt(dx * dx + dy * dy);
            gu[k] = on ? (float)((sc * dx) / e) : 0.0f;
            gv[k] = on ? (float)((sc * dy) / e) : 0.0f;
        }
        const int64_t o = img * 2 * p.hw + 4 * q;
        if (VEC) {
            if (p.grad_est != nullptr) {
                *reinterpret_cast<float4*>(p.grad_est + o) = make_float4(gu[0], gu[1], gu[2], gu[3]);
                *reinterpret_cast<float4*>(p.grad_est + o + p.hw) = make_float4(gv[0], gv[1], gv[2], gv[3]);
            }
            if (p.grad_gt != nullptr) {
                *reinterpret_cast<float4*>(p.grad_gt + o) = make_float4(-gu[0], -gu[1], -gu[2], -gu[3]);
                *reinterpret_cast<float4*>(p.grad_gt + o + p.hw) = make_float4(-gv[0], -gv[1], -gv[2], -gv[3]);
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (4 * q + k >= p.hw) continue;
                if (p.grad_est != nullptr) { p.grad_est[o + k] = gu[k]; p.grad_est[o + p.hw + k] = gv[k]; }
                if (p.grad_gt != nullptr) { p.grad_gt[o + k] = -gu[k]; p.grad_gt[o + p.hw + k] = -gv[k]; }
            }
        }
    }
}

int shape_rc(int32_t n, int32_t h, int32_t w) { return dims_ok(n, h, w, 1) ? OFL_OK : OFL_E_SHAPE; }

int64_t blocks_of(int64_t hw, int cap) {
    const int64_t b = ((hw + 3) / 4 + kThreads - 1) / kThreads;
    return b < cap ? b : cap;
}

// the operands both entry points share: flows and masks
int fill_operands(ErrParams* p, const void* est, int64_t est_bs, int32_t est_half, const void* gt, int64_t gt_bs, int32_t gt_half,
                  const uint8_t* est_mask, int64_t est_mask_bs, const uint8_t* gt_mask, int64_t gt_mask_bs, int32_t h, int32_t w) {
    if ((est_half != 0 && est_half != 1) || (gt_half != 0 && gt_half != 1)) return OFL_E_ARG;
    if (est_bs < 0 || gt_bs < 0 || est_mask_bs < 0 || gt_mask_bs < 0) return OFL_E_ARG;
    if (!aligned(est, est_half ? 2 : 4) || !aligned(gt, gt_half ? 2 : 4)) return OFL_E_ARG;
    p->est = est; p->est_bs = est_bs; p->est_half = est_half;
    p->gt = gt; p->gt_bs = gt_bs; p->gt_half = gt_half;
    p->est_mask = est_mask; p->est_mask_bs = est_mask_bs;
    p->gt_mask = gt_mask; p->gt_mask_bs = gt_mask_bs;
    p->hw = (int64_t)h * w;
    p->nblk = 0; p->nthr = 0;
    for (int t = 0; t < kMaxThr; ++t) p->thr[t] = 0.0f;
    p->partial = nullptr; p->map = nullptr; p->out = nullptr; p->scale = nullptr; p->grad_est = nullptr; p->grad_gt = nullptr;
    return OFL_OK;
}

// 16-byte (fp16: 8-byte) accesses of the vector planes and 4-byte accesses of the masks are aligned for every lane of every image
bool inputs_vectorise(const ErrParams& p) {
    if (p.hw % 4 != 0) return false;
    if (p.est_bs % 4 != 0 || p.gt_bs % 4 != 0 || p.est_mask_bs % 4 != 0 || p.gt_mask_bs % 4 != 0) return false;
    if (!aligned(p.est, p.est_half ? 8 : 16) || !aligned(p.gt, p.gt_half ? 8 : 16)) return false;
    return aligned(p.est_mask, 4) && aligned(p.gt_mask, 4);
}

}  // namespace

extern "C" {

__attribute__((visibility("default"))) int64_t ofl_flow_error_workspace_bytes(int32_t n, int32_t h, int32_t w) {
    const int rc = shape_rc(n, h, w);
    if (rc) return rc;
    return (int64_t)n * blocks_of((int64_t)h * w, kMaxBlocks) * kRec * (int64_t)sizeof(double);
}

__attribute__((visibility("default"))) int ofl_flow_error_f64(const void* est, int64_t est_bs, int32_t est_half, const void* gt, int64_t gt_bs,
                                                              int32_t gt_half, const uint8_t* est_mask, int64_t est_mask_bs,
                                                              const uint8_t* gt_mask, int64_t gt_mask_bs, int32_t n_thresholds,
                                                              float t0, float t1, float t2, float t3, void* workspace, float* epe_map,
                                                              double* records,
                                                              int32_t n, int32_t h, int32_t w, void* stream) {
    if (!est || !gt || !workspace || !records) return OFL_E_NULL;
    int rc = shape_rc(n, h, w);
    if (rc) return rc;
    if (n_thresholds < 0 || n_thresholds > kMaxThr) return OFL_E_ARG;
    ErrParams p;
    rc = fill_operands(&p, est, est_bs, est_half, gt, gt_bs, gt_half, est_mask, est_mask_bs, gt_mask, gt_mask_bs, h, w);
    if (rc) return rc;
    if (!aligned(workspace, 8) || !aligned(records, 8) || !aligned(epe_map, 4)) return OFL_E_ARG;
    const float thresholds[kMaxThr] = {t0, t1, t2, t3};
    for (int t = 0; t < n_thresholds; ++t) {
        if (!(thresholds[t] >= 0.0f) || isinf(thresholds[t])) return OFL_E_ARG;      // (NaN fails the first test)
        p.thr[t] = thresholds[t];
    }
    p.nthr = n_thresholds;
    p.nblk = (int32_t)blocks_of(p.hw, kMaxBlocks);
    p.partial = reinterpret_cast<double*>(workspace);
    p.map = epe_map;
    p.out = records;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)p.nblk, (unsigned)n);
    if (inputs_vectorise(p) && aligned(epe_map, 16)) OFL_KLAUNCH(flow_error_kernel<true>, grid, dim3(kThreads), 0, s, p);
    else OFL_KLAUNCH(flow_error_kernel<false>, grid, dim3(kThreads), 0, s, p);
    OFL_KLAUNCH(flow_error_finish_kernel, dim3((unsigned)n), dim3(kThreads), 0, s, p);
    return (int)hipGetLastError();
}

__attribute__((visibility("default"))) int ofl_flow_epe_grad_f32(const void* est, int64_t est_bs, int32_t est_half, const void* gt, int64_t gt_bs,
                                                                 int32_t gt_half, const uint8_t* est_mask, int64_t est_mask_bs,
                                                                 const uint8_t* gt_mask, int64_t gt_mask_bs, const float* scale,
                                                                 float* grad_est, float* grad_gt, int32_t n, int32_t h, int32_t w,
                                                                 void* stream) {
    if (!est || !gt || !scale || (!grad_est && !grad_gt)) return OFL_E_NULL;
    int rc = shape_rc(n, h, w);
    if (rc) return rc;
    ErrParams p;
    rc = fill_operands(&p, est, est_bs, est_half, gt, gt_bs, gt_half, est_mask, est_mask_bs, gt_mask, gt_mask_bs, h, w);
    if (rc) return rc;
    if (!aligned(scale, 4) || !aligned(grad_est, 4) || !aligned(grad_gt, 4)) return OFL_E_ARG;
    p.scale = scale; p.grad_est = grad_est; p.grad_gt = grad_gt;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)blocks_of(p.hw, kMaxGradBlocks), (unsigned)n);
    if (inputs_vectorise(p) && aligned(grad_est, 16) && aligned(grad_gt, 16)) OFL_KLAUNCH(flow_epe_grad_kernel<true>, grid, dim3(kThreads), 0, s, p);
    else OFL_KLAUNCH(flow_epe_grad_kernel<false>, grid, dim3(kThreads), 0, s, p);
    return (int)hipGetLastError();
}

}  // extern "C"
