// ofl_chain.hip -- Flow.chain / chain_flows on gfx950: the frame-to-frame flows f_1 .. f_T of a clip composed into the flow from the first
// frame to the last in ONE launch (which DEFINES the numbers; tests/chain_oracle.py is the same definition in NumPy).  An
// extension: the reference composes two flows at a time (combine_with mode 3); this is that fold without its intermediate flows.
//
//   flow_chain_kernel<ALL>   one pixel per lane, consecutive lanes on consecutive pixels.  In mode 3 the accumulated flow is always the
//                            WARPER, so the composition of a sequence is an independent walk per pixel: the running vector and the mask
//                            bit stay in registers, a step is one bilinear sample of the next flow (and the weight test of its mask)
//                            where the walk stands -- taps_of() / sample_of() of ofl_loss_common.hpp, the arithmetic of partner() of
//                            ofl_consistency.hip.  9 B/px per step against the fold's 27 B/px and T - 1 launches.  ALL: every partial
//                            chain is stored as the walk passes it (the dense trajectories of the first frame's pixels)
//
// The T base pointers, batch strides, storage kinds, mask pointers and mask strides travel by value in the kernel arguments, already in
// the order of the walk; they are indexed by the wave-uniform step counter.  Direct global loads of the four taps: no LDS (DESIGN.md 8
// lists the staged gather).  C ABI: include/oflib_hip.h.
#include "ofl_loss_common.hpp"

namespace {

using namespace ofl_loss;

constexpr int kThreads = 256;
constexpr int kMaxT = OFL_CHAIN_MAX_T;

struct Step {
    const void* base;                                       // [*,2,H,W] fp32 or fp16
    const uint8_t* mask;                                    // [*,H,W] bytes or nullptr (all True)
    int64_t bs_kind;                                        // (elements between images) << 1 | (1: fp16)
    int64_t mask_bs;                                        // bytes between the mask's images
};

struct ChainParams {
    Step step[kMaxT];                                       // in the order of the walk: step[0] starts it
    float* out;                                             // [slots][n][2][H*W]
    uint8_t* out_mask;                                      // [slots][n][H*W]
    int64_t hw;
    int32_t t, n, h, w;
    float flow_sign, wm1, hm1, half_wm1, half_hm1;          // (the sample's constants: taps_of)
};

__device__ __forceinline__ float ld_vec(const void* base, bool half, int64_t i) {
    return half ? ld_flow<true>(base, i) : ld_flow<false>(base, i);
}

// the slot of the partial chain that step i (>= 1) of the walk completes: 's' flows walk forward in time, 't' flows backward
__device__ __forceinline__ int slot_of(const ChainParams& p, int i) { return p.flow_sign < 0.0f ? i - 1 : p.t - 1 - i; }

__device__ __forceinline__ void store_px(const ChainParams& p, int slot, int64_t img, int64_t px, float u, float v, bool m) {
    const int64_t o = (int64_t)slot * p.n + img;
    float* q = p.out + o * 2 * p.hw + px;
    q[0] = u;
    q[p.hw] = v;
    p.out_mask[o * p.hw + px] = m ? (uint8_t)1 : (uint8_t)0;
}

template <bool ALL>
__global__ void __launch_bounds__(kThreads) flow_chain_kernel(ChainParams p) {
    const int64_t px = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (px >= p.hw) return;
    const int64_t img = blockIdx.y;
    const int y = (int)(px / p.w), x = (int)(px - (int64_t)y * p.w);
    const int t = p.t;
    float u, v;
    bool m;
    {
        const bool half = (p.step[0].bs_kind & 1) != 0;
        const int64_t o = img * (p.step[0].bs_kind >> 1);
        u = ld_vec(p.step[0].base, half, o + px);
        v = ld_vec(p.step[0].base, half, o + p.hw + px);
        const uint8_t* mk = p.step[0].mask;
        m = mk == nullptr || mk[img * p.step[0].mask_bs + px] != 0;
    }
    for (int i = 1; i < t; ++i) {
        const void* base = p.step[i].base;
        const bool half = (p.step[i].bs_kind & 1) != 0;
        const int64_t o = img * (p.step[i].bs_kind >> 1);
        const uint8_t* mk = p.step[i].mask;
        const Taps tp = taps_of(p, x, y, u, v);
        // (the offsets are clamped into the plane: every load is addressable, a tap outside the frame then reads as 0)
        const float u_nw = ld_vec(base, half, o + tp.o_nw), u_ne = ld_vec(base, half, o + tp.o_ne);
        const float u_sw = ld_vec(base, half, o + tp.o_sw), u_se = ld_vec(base, half, o + tp.o_se);
        const int64_t o1 = o + p.hw;
        const float v_nw = ld_vec(base, half, o1 + tp.o_nw), v_ne = ld_vec(base, half, o1 + tp.o_ne);
        const float v_sw = ld_vec(base, half, o1 + tp.o_sw), v_se = ld_vec(base, half, o1 + tp.o_se);
        float mr = tp.mr;
        if (mk != nullptr) {
            const uint8_t* mi = mk + img * p.step[i].mask_bs;
            const bool k_nw = tp.k_nw && mi[tp.o_nw] != 0, k_ne = tp.k_ne && mi[tp.o_ne] != 0;
            const bool k_sw = tp.k_sw && mi[tp.o_sw] != 0, k_se = tp.k_se && mi[tp.o_se] != 0;
            mr = (k_nw ? 1.0f : 0.0f) * tp.nw;
            mr = __builtin_fmaf(k_ne ? 1.0f : 0.0f, tp.ne, mr);
            mr = __builtin_fmaf(k_sw ? 1.0f : 0.0f, tp.sw, mr);
            mr = __builtin_fmaf(k_se ? 1.0f : 0.0f, tp.se, mr);
        }
        const float bu = sample_of(tp, tp.k_nw ? u_nw : 0.0f, tp.k_ne ? u_ne : 0.0f, tp.k_sw ? u_sw : 0.0f, tp.k_se ? u_se : 0.0f);
        const float bv = sample_of(tp, tp.k_nw ? v_nw : 0.0f, tp.k_ne ? v_ne : 0.0f, tp.k_sw ? v_sw : 0.0f, tp.k_se ? v_se : 0.0f);
        u = u + bu;
        v = v + bv;
        m = m && (mr > kValidThr);
        if (ALL) store_px(p, slot_of(p, i), img, px, u, v, m);
    }
    if (!ALL) store_px(p, 0, img, px, u, v, m);
}

}  // namespace

extern "C" {

__attribute__((visibility("default"))) int ofl_flow_chain_f32(const void* const* flows, const int64_t* flow_bs, const int32_t* flow_half,
                                                              const uint8_t* const* masks, const int64_t* mask_bs, int32_t t,
                                                              float flow_sign, float* out, uint8_t* out_mask, int32_t want_all, int32_t n,
                                                              int32_t h, int32_t w, void* stream) {
    if (t < 2 || t > kMaxT || !dims_ok(n, h, w, 2)) return OFL_E_ARG;
    if (flow_sign != 1.0f && flow_sign != -1.0f) return OFL_E_ARG;
    if (want_all != 0 && want_all != 1) return OFL_E_ARG;
    if (!flows || !flow_bs || !flow_half || (masks && !mask_bs) || !out || !out_mask) return OFL_E_ARG;
    if (!aligned(out, 4)) return OFL_E_ARG;
    ChainParams p;
    for (int i = 0; i < kMaxT; ++i) { p.step[i].base = nullptr; p.step[i].mask = nullptr; p.step[i].bs_kind = 0; p.step[i].mask_bs = 0; }
    for (int i = 0; i < t; ++i) {
        const int k = flow_sign < 0.0f ? i : t - 1 - i;                          // the flow that step i of the walk reads
        if (!flows[k] || (flow_half[k] != 0 && flow_half[k] != 1) || flow_bs[k] < 0 || flow_bs[k] >= (1ll << 62)) return OFL_E_ARG;
        if (!aligned(flows[k], flow_half[k] ? 2 : 4)) return OFL_E_ARG;
        p.step[i].base = flows[k];
        p.step[i].bs_kind = (int64_t)((uint64_t)flow_bs[k] << 1) | flow_half[k];
        if (masks && masks[k]) {
            if (mask_bs[k] < 0) return OFL_E_ARG;
            p.step[i].mask = masks[k];
            p.step[i].mask_bs = mask_bs[k];
        }
    }
    p.out = out; p.out_mask = out_mask;
    p.hw = (int64_t)h * w;
    p.t = t; p.n = n; p.h = h; p.w = w;
    p.flow_sign = flow_sign;
    p.wm1 = (float)(w - 1); p.hm1 = (float)(h - 1);
    p.half_wm1 = p.wm1 / 2.0f; p.half_hm1 = p.hm1 / 2.0f;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((p.hw + kThreads - 1) / kThreads), (unsigned)n);
    if (want_all) OFL_KLAUNCH(flow_chain_kernel<true>, grid, dim3(kThreads), 0, s, p);
    else OFL_KLAUNCH(flow_chain_kernel<false>, grid, dim3(kThreads), 0, s, p);
    return (int)hipGetLastError();
}

}  // extern "C"
