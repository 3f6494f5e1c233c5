// ofl_consistency.hip -- Flow.consistency / consistency_mask / filter_consistent on gfx950: the forward-backward check of a flow `a`
// (frame 1 -> frame 2) against a flow `back` (frame 2 -> frame 1) in one pass (which DEFINES the numbers;
// tests/consistency_oracle.py is the same definition in NumPy).  An extension: the reference has no such function.
//
//   flow_consistency_kernel          per pixel: the partner (bu, bv) = `back` sampled bilinearly where `a` points and the weight sum mr of
//                                    its valid taps, known = (mr > kValidThr) and a's mask, the round-trip residual (u + bu, v + bv), its
//                                    length e, consistent = known and e^2 <= alpha (|a|^2 + |partner|^2) + beta.  Writes e (0 where not
//                                    known) and the two byte masks, whichever are wanted, and per block ONE record of 8 float64 values
//   flow_consistency_finish_kernel   one block per image: the block records added in ascending block order
//
// The residual and `known` are the vectors and the mask of combine_with(mode 3) bit for bit; the composed flow is never written.  The
// sample (position, taps, weights, the four-term sums) is the one of ofl_loss_common.hpp, which restates the backward warp of
// ofl_kernels.hip; mr here runs the same chain over the tap validities (a tap that back's mask switches off leaves mr only);
// tests/test_gpu_consistency.py compares the two on the device.
//
// One lane takes the 4 pixels 4 q .. 4 q + 3 of an image.  a's planes and mask and the outputs go through 16-byte / 4-byte accesses where
// H*W, the batch strides and the pointers allow (chosen per launch), else one element at a time with bounds checks; the taps of `back`
// are single loads straight from global memory in either form (element alignment is all `back` needs).  Blocks walk an image with a grid
// stride, their number depends on H*W only; the sums are those of ofl_loss_common.hpp.  C ABI: include/oflib_hip.h.
#include "ofl_loss_common.hpp"

namespace {

using namespace ofl_loss;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxBlocks = 256;                    // blocks per image at most (one per CU); 1080p: each walks 7 or 8 steps of 1024 px
constexpr int kRec = OFL_CONSISTENCY_RECORD;       // doubles per record
// slots of a record (include/oflib_hip.h)
enum { R_KNOWN = 0, R_CONS = 1, R_SUM = 2, R_MAX = 3, R_SUM_CONS = 4, R_USED = 5 };

struct ConsParams {
    const void* a; const void* b;                  // [*,2,H,W] fp32 or fp16: the flow and the flow back
    int64_t a_bs, b_bs;                            // elements between images
    const uint8_t* a_mask; const uint8_t* b_mask;  // [*,H,W] bytes or nullptr (all True)
    int64_t a_mask_bs, b_mask_bs;
    int64_t hw;
    int32_t h, w, nblk;
    float flow_sign, alpha, beta;
    float wm1, hm1, half_wm1, half_hm1;
    double* partial;                               // [n][nblk][kRec] or nullptr (no record wanted)
    float* err;                                    // [n][H*W] or nullptr
    uint8_t* cons; uint8_t* known;                 // [n][H*W] bytes or nullptr
    double* out;                                   // [n][kRec]
};

// four consecutive elements p0 .. p0 + 3 of one plane of `a` (`base` + o: its first element); VEC: all four exist and the access is aligned
template <bool VEC, bool HALF>
__device__ __forceinline__ void ld4(const void* base, int64_t o, int64_t p0, int64_t hw, float v[4]) {
    if (VEC) {
        if (HALF) {
            const uint2 u = *reinterpret_cast<const uint2*>(reinterpret_cast<const __half*>(base) + o + p0);
            const __half2 x = *reinterpret_cast<const __half2*>(&u.x), y = *reinterpret_cast<const __half2*>(&u.y);
            v[0] = __low2float(x); v[1] = __high2float(x); v[2] = __low2float(y); v[3] = __high2float(y);
        } else {
            const float4 f = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(base) + o + p0);
            v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = (p0 + k < hw) ? ld_flow<HALF>(base, o + p0 + k) : 0.0f;
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

// the partner of pixel (x, y) whose vector is (u, v): `back` sampled at unnormalise(grid - flow_sign * a) and the weight sum of its valid
// taps, two channels.  The geometry is taps_of() of ofl_loss_common.hpp written out (through Taps the vector kernels take 111 to 122 VGPRs, not 102, by tools/isa_stats.py): a change
// there is made here too.  Taps are clamped into the plane: always addressable
template <bool HALF_B>
__device__ __forceinline__ void partner(const ConsParams& p, const void* bb, const uint8_t* bm, int x, int y, float u, float v,
                                        float& bu, float& bv, float& mr) {
    const int w = p.w, h = p.h;
    const float px = (float)x - p.flow_sign * u;
    const float py = (float)y - p.flow_sign * v;
    const float sx = unnormalise(px, p.wm1, p.half_wm1);
    const float sy = unnormalise(py, p.hm1, p.half_hm1);
    const float x_w = floorf(sx), y_n = floorf(sy);
    const float ww = sx - x_w, e = 1.0f - ww;
    const float nn = sy - y_n, s = 1.0f - nn;
    const float nw = s * e, ne = s * ww, sw = nn * e, se = nn * ww;
    const float x_e = x_w + 1.0f, y_s = y_n + 1.0f;
    const bool x0ok = (x_w > -1.0f) && (x_w < (float)w);
    const bool x1ok = (x_e > -1.0f) && (x_e < (float)w);
    const bool y0ok = (y_n > -1.0f) && (y_n < (float)h);
    const bool y1ok = (y_s > -1.0f) && (y_s < (float)h);
    const int ix0 = x0ok ? (int)x_w : 0, ix1 = x1ok ? (int)x_e : 0;
    const int iy0 = y0ok ? (int)y_n : 0, iy1 = y1ok ? (int)y_s : 0;
    const int64_t o_nw = (int64_t)iy0 * w + ix0, o_ne = (int64_t)iy0 * w + ix1;
    const int64_t o_sw = (int64_t)iy1 * w + ix0, o_se = (int64_t)iy1 * w + ix1;
    const bool k_nw = x0ok && y0ok, k_ne = x1ok && y0ok, k_sw = x0ok && y1ok, k_se = x1ok && y1ok;

    float m_nw, m_ne, m_sw, m_se;
    if (bm) {
        m_nw = k_nw ? (float)(bm[o_nw] != 0) : 0.0f;
        m_ne = k_ne ? (float)(bm[o_ne] != 0) : 0.0f;
        m_sw = k_sw ? (float)(bm[o_sw] != 0) : 0.0f;
        m_se = k_se ? (float)(bm[o_se] != 0) : 0.0f;
    } else {
        m_nw = k_nw ? 1.0f : 0.0f; m_ne = k_ne ? 1.0f : 0.0f;
        m_sw = k_sw ? 1.0f : 0.0f; m_se = k_se ? 1.0f : 0.0f;
    }
    mr = m_nw * nw;
    mr = __builtin_fmaf(m_ne, ne, mr);
    mr = __builtin_fmaf(m_sw, sw, mr);
    mr = __builtin_fmaf(m_se, se, mr);

    float r[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const int64_t pl = (int64_t)c * p.hw;
        const float v_nw = k_nw ? ld_flow<HALF_B>(bb, pl + o_nw) : 0.0f;
        const float v_ne = k_ne ? ld_flow<HALF_B>(bb, pl + o_ne) : 0.0f;
        const float v_sw = k_sw ? ld_flow<HALF_B>(bb, pl + o_sw) : 0.0f;
        const float v_se = k_se ? ld_flow<HALF_B>(bb, pl + o_se) : 0.0f;
        float rr = v_nw * nw;
        rr = __builtin_fmaf(v_ne, ne, rr);
        rr = __builtin_fmaf(v_sw, sw, rr);
        rr = __builtin_fmaf(v_se, se, rr);
        r[c] = rr;
    }
    bu = r[0]; bv = r[1];
}

template <bool VEC, bool HALF_A, bool HALF_B>
__global__ void __launch_bounds__(kThreads) flow_consistency_kernel(ConsParams p) {
    __shared__ double s_red[kWaves * kRec];
    const int64_t img = blockIdx.y;
    const int64_t quads = (p.hw + 3) >> 2, stride = (int64_t)gridDim.x * kThreads;
    const int64_t ao = img * p.a_bs;
    const void* bb = HALF_B ? (const void*)(reinterpret_cast<const __half*>(p.b) + img * p.b_bs)
                            : (const void*)(reinterpret_cast<const float*>(p.b) + img * p.b_bs);
    const uint8_t* bm = p.b_mask ? p.b_mask + img * p.b_mask_bs : nullptr;
    uint32_t nknown = 0u, ncons = 0u;
    double sum = 0.0, sum_cons = 0.0;
    float mx = 0.0f;
    for (int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x; q < quads; q += stride) {
        const int64_t p0 = 4 * q;
        float u[4], v[4], e[4];
        ld4<VEC, HALF_A>(p.a, ao, p0, p.hw, u);
        ld4<VEC, HALF_A>(p.a, ao + p.hw, p0, p.hw, v);
        const uint32_t abits = mask4<VEC>(p.a_mask, img * p.a_mask_bs, p0, p.hw);      // (a pixel past the end has no bit)
        uint32_t kbits = 0u, cbits = 0u;
        int y = (int)((uint32_t)p0 / (uint32_t)p.w), x = (int)((uint32_t)p0 - (uint32_t)y * (uint32_t)p.w);   // (h * w < 2^31)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            e[k] = 0.0f;
            if (VEC || p0 + k < p.hw) {
                float bu, bv, mr;
                partner<HALF_B>(p, bb, bm, x, y, u[k], v[k], bu, bv, mr);
                const bool known = (mr > kValidThr) && ((abits >> k) & 1u);
                const float du = u[k] + bu, dv = v[k] + bv;
                const float e2 = du * du + dv * dv;
                const float ek = sqrt_rn(e2);
                const float m2 = (u[k] * u[k] + v[k] * v[k]) + (bu * bu + bv * bv);
                const float bound = p.alpha * m2 + p.beta;
                const bool cons = known && (e2 <= bound);
                e[k] = known ? ek : 0.0f;
                const double ed = known ? (double)ek : 0.0;
                kbits |= known ? (1u << (8 * k)) : 0u;
                cbits |= cons ? (1u << (8 * k)) : 0u;
                nknown += known ? 1u : 0u;
                ncons += cons ? 1u : 0u;
                sum += ed;
                sum_cons += cons ? ed : 0.0;
                mx = (known && ek > mx) ? ek : mx;
            }
            if (++x == p.w) { x = 0; ++y; }
        }
        const int64_t oo = img * p.hw + p0;
        if (VEC) {
            if (p.err != nullptr) *reinterpret_cast<float4*>(p.err + oo) = make_float4(e[0], e[1], e[2], e[3]);
            if (p.cons != nullptr) *reinterpret_cast<uint32_t*>(p.cons + oo) = cbits;
            if (p.known != nullptr) *reinterpret_cast<uint32_t*>(p.known + oo) = kbits;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (p0 + k >= p.hw) continue;
                if (p.err != nullptr) p.err[oo + k] = e[k];
                if (p.cons != nullptr) p.cons[oo + k] = (uint8_t)((cbits >> (8 * k)) & 1u);
                if (p.known != nullptr) p.known[oo + k] = (uint8_t)((kbits >> (8 * k)) & 1u);
            }
        }
    }
    if (p.partial == nullptr) return;              // (the same for every thread of the launch)
    double rec[kRec];
#pragma unroll
    for (int i = 0; i < kRec; ++i) rec[i] = 0.0;
    rec[R_KNOWN] = (double)nknown; rec[R_CONS] = (double)ncons; rec[R_SUM] = sum; rec[R_MAX] = (double)mx; rec[R_SUM_CONS] = sum_cons;
    reduce_record<kRec, R_USED, R_MAX, kWaves>(rec, s_red, p.partial, img, p.nblk);
}

// one block per image: the block records added in ascending block order (all of them fit one chunk)
__global__ void __launch_bounds__(kThreads) flow_consistency_finish_kernel(ConsParams p) {
    finish_records<kRec, R_MAX, kMaxBlocks, kThreads>(p.partial, p.nblk, p.out);
}

int64_t blocks_of(int64_t hw) {
    const int64_t b = ((hw + 3) / 4 + kThreads - 1) / kThreads;
    return b < kMaxBlocks ? b : kMaxBlocks;
}

// 16-byte (fp16: 8-byte) accesses of a's planes, 4-byte accesses of a's mask and of the byte outputs and 16-byte stores of the map are
// aligned for every lane of every image (`back` and its mask are read one element at a time: nothing to ask of them)
bool vectorises(const ConsParams& p, bool a_half) {
    if (p.hw % 4 != 0 || p.a_bs % 4 != 0 || p.a_mask_bs % 4 != 0) return false;
    return aligned(p.a, a_half ? 8 : 16) && aligned(p.a_mask, 4) && aligned(p.err, 16) && aligned(p.cons, 4) && aligned(p.known, 4);
}

template <bool VEC>
void launch(const ConsParams& p, bool a_half, bool b_half, dim3 grid, hipStream_t s) {
    dispatch_flags(a_half, b_half, [&](auto HALF_A, auto HALF_B) {
        OFL_KLAUNCH((flow_consistency_kernel<VEC, decltype(HALF_A)::value, decltype(HALF_B)::value>), grid, dim3(kThreads), 0, s, p);
    });
}

}  // namespace

extern "C" {

__attribute__((visibility("default"))) int64_t ofl_flow_consistency_workspace_bytes(int32_t n, int32_t h, int32_t w) {
    if (!dims_ok(n, h, w, 2)) return OFL_E_ARG;
    return (int64_t)n * blocks_of((int64_t)h * w) * kRec * (int64_t)sizeof(double);
}

__attribute__((visibility("default"))) int ofl_flow_consistency_f32(const void* a, int64_t a_bs, int32_t a_half, const void* back, int64_t back_bs,
                                                                    int32_t back_half, const uint8_t* a_mask, int64_t a_mask_bs,
                                                                    const uint8_t* back_mask, int64_t back_mask_bs, float flow_sign,
                                                                    float alpha, float beta, void* workspace, float* error,
                                                                    uint8_t* consistent, uint8_t* known, double* record,
                                                                    int32_t n, int32_t h, int32_t w, void* stream) {
    if (!dims_ok(n, h, w, 2)) return OFL_E_ARG;
    if (flow_sign != 1.0f && flow_sign != -1.0f) return OFL_E_ARG;
    if (!(alpha >= 0.0f) || isinf(alpha) || !(beta >= 0.0f) || isinf(beta)) return OFL_E_ARG;      // (NaN fails the first test)
    if (!a || !back) return OFL_E_ARG;
    if (!error && !consistent && !known && !record) return OFL_E_ARG;
    if (record && !workspace) return OFL_E_ARG;
    if ((a_half != 0 && a_half != 1) || (back_half != 0 && back_half != 1)) return OFL_E_ARG;
    if (a_bs < 0 || back_bs < 0 || a_mask_bs < 0 || back_mask_bs < 0) return OFL_E_ARG;
    if (!aligned(a, a_half ? 2 : 4) || !aligned(back, back_half ? 2 : 4)) return OFL_E_ARG;
    if (!aligned(workspace, 8) || !aligned(record, 8) || !aligned(error, 4)) return OFL_E_ARG;
    ConsParams p;
    p.a = a; p.b = back; p.a_bs = a_bs; p.b_bs = back_bs;
    p.a_mask = a_mask; p.b_mask = back_mask; p.a_mask_bs = a_mask_bs; p.b_mask_bs = back_mask_bs;
    p.hw = (int64_t)h * w; p.h = h; p.w = w;
    p.nblk = (int32_t)blocks_of(p.hw);
    p.flow_sign = flow_sign; p.alpha = alpha; p.beta = beta;
    p.wm1 = (float)(w - 1); p.hm1 = (float)(h - 1);
    p.half_wm1 = p.wm1 / 2.0f; p.half_hm1 = p.hm1 / 2.0f;
    p.partial = record ? reinterpret_cast<double*>(workspace) : nullptr;
    p.err = error; p.cons = consistent; p.known = known; p.out = record;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)p.nblk, (unsigned)n);
    if (vectorises(p, a_half != 0)) launch<true>(p, a_half != 0, back_half != 0, grid, s);
    else launch<false>(p, a_half != 0, back_half != 0, grid, s);
    if (record) OFL_KLAUNCH(flow_consistency_finish_kernel, dim3((unsigned)n), dim3(kThreads), 0, s, p);
    return (int)hipGetLastError();
}

}  // extern "C"
