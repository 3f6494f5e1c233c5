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
// The warped image is never written.  The sample (position, taps, weights, the four-term sums and mr) is the one of ofl_loss_common.hpp,
// which restates the backward warp of ofl_kernels.hip; tests/test_gpu_photometric.py compares the two on the device.
//
// One lane takes ONE pixel per round and the lanes of a wave take consecutive pixels of the image (of a row, up to where a row ends),
// the rounds a grid stride apart: on a smooth flow a wave's load of one tap of one plane is one contiguous run of 256 bytes (64 of a uint8
// image), which the four-pixels-per-lane form of ofl_consistency.hip spreads over 1 KiB.  Taps are single loads
// straight from global memory at offsets clamped into the plane: always addressable.  The sums are those of ofl_loss_common.hpp; the number
// of blocks depends on (h, w) only.  C ABI: include/oflib_hip.h.
#include "ofl_loss_common.hpp"

namespace {

using namespace ofl_loss;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxBlocks = 256;                    // forward: blocks per image at most (one per CU); 1080p: each walks 31 or 32 rounds
constexpr int kMaxGradBlocks = 2048;               // backward: nothing to reduce
constexpr int kRec = OFL_PHOTOMETRIC_RECORD;       // doubles per record
constexpr int kMaxChan = 4;
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
                const float v_nw = t.k_nw ? ld_img_unit<U8>(p.other, pl + t.o_nw) : 0.0f;
                const float v_ne = t.k_ne ? ld_img_unit<U8>(p.other, pl + t.o_ne) : 0.0f;
                const float v_sw = t.k_sw ? ld_img_unit<U8>(p.other, pl + t.o_sw) : 0.0f;
                const float v_se = t.k_se ? ld_img_unit<U8>(p.other, pl + t.o_se) : 0.0f;
                const float d = sample_of(t, v_nw, v_ne, v_sw, v_se) - ld_img_unit<U8>(p.img, io + (int64_t)c * p.hw + pix);
                s = s + sqrt_rn(d * d + ee);
            }
            const float rho = known ? s / fc : 0.0f;
            if (p.map != nullptr) p.map[n_img * p.hw + pix] = rho;
            count += known ? 1u : 0u;
            sum += (double)rho;
            mx = (known && rho > mx) ? rho : mx;
        } else {
            double ax = 0.0, ay = 0.0;
            for (int c = 0; c < p.chan; ++c) {
                const int64_t pl = oo + (int64_t)c * p.hw;
                const float v_nw = t.k_nw ? ld_img_unit<U8>(p.other, pl + t.o_nw) : 0.0f;
                const float v_ne = t.k_ne ? ld_img_unit<U8>(p.other, pl + t.o_ne) : 0.0f;
                const float v_sw = t.k_sw ? ld_img_unit<U8>(p.other, pl + t.o_sw) : 0.0f;
                const float v_se = t.k_se ? ld_img_unit<U8>(p.other, pl + t.o_se) : 0.0f;
                const float d = sample_of(t, v_nw, v_ne, v_sw, v_se) - ld_img_unit<U8>(p.img, io + (int64_t)c * p.hw + pix);
                const double dd = (double)d;
                const double den = sqrt(dd * dd + ee64);
                const double q = den != 0.0 ? dd / den : 0.0;
                double gx, gy;
                sample_grad(t, (double)v_nw, (double)v_ne, (double)v_sw, (double)v_se, gx, gy);
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
        __shared__ double s_red[kWaves * kRec];
        double rec[kRec];
#pragma unroll
        for (int i = 0; i < kRec; ++i) rec[i] = 0.0;
        rec[R_COUNT] = (double)count; rec[R_SUM] = sum; rec[R_MAX] = (double)mx;
        reduce_record<kRec, R_USED, R_MAX, kWaves>(rec, s_red, p.partial, n_img, p.nblk);
    }
}

// one block per image: the block records added in ascending block order (all of them fit one chunk)
__global__ void __launch_bounds__(kThreads) flow_photometric_finish_kernel(PhotoParams p) {
    finish_records<kRec, R_MAX, kMaxBlocks, kThreads>(p.partial, p.nblk, p.out);
}

int64_t blocks_of(int64_t hw, int cap) {
    const int64_t b = (hw + kThreads - 1) / kThreads;
    return b < cap ? b : cap;
}

// the operands and the checks both entry points share
int fill_operands(PhotoParams* p, const void* flow, int64_t flow_bs, int32_t flow_half, const uint8_t* mask, int64_t mask_bs,
                  const void* img, int64_t img_bs, const void* other, int64_t other_bs, int32_t channels, int32_t img_u8, float flow_sign,
                  float eps, int32_t n, int32_t h, int32_t w) {
    if (channels < 1 || channels > kMaxChan) return OFL_E_ARG;
    if (!(eps >= 0.0f) || isinf(eps)) return OFL_E_ARG;                                            // (NaN fails the first test)
    p->eps = eps;
    return fill_pair_operands(p, flow, flow_bs, flow_half, mask, mask_bs, img, img_bs, other, other_bs, channels, img_u8, flow_sign, n, h, w);
}

template <bool BWD>
void launch(const PhotoParams& p, bool half, bool u8, dim3 grid, hipStream_t s) {
    dispatch_flags(half, u8, [&](auto HALF, auto U8) {
        OFL_KLAUNCH((flow_photometric_kernel<decltype(HALF)::value, decltype(U8)::value, BWD>), grid, dim3(kThreads), 0, s, p);
    });
}

}  // namespace

extern "C" {

__attribute__((visibility("default"))) int64_t ofl_flow_photometric_workspace_bytes(int32_t n, int32_t h, int32_t w) {
    if (!dims_ok(n, h, w, 2)) return OFL_E_ARG;
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
