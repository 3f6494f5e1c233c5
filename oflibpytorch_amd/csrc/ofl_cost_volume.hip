// ofl_cost_volume.hip -- Flow.cost_volume on gfx950: the local cost volume of PWC-Net, LiteFlowNet, ARFlow and UFlow, warp and correlation
// in one pass (which DEFINES the numbers; tests/cost_volume_oracle.py is the same definition in NumPy).  An extension: the
// reference has no such function.
//
//   flow_cost_volume_kernel<R, HALF>            a block owns a tile of 32 x 16 output pixels.  For a chunk of kChanChunk channels it stages
//                                               W' -- `other` sampled where the flow points, +0 where the pixel is not usable or outside the
//                                               frame -- of the tile and a halo of R pixels in LDS: the geometry of a staged pixel (one
//                                               taps_of()) is computed once per chunk, then four global taps per channel.  Each lane keeps the
//                                               D = (2 R + 1)^2 accumulators of its TWO pixels, one above the other, in registers and walks
//                                               the 2 R + 2 window rows in LDS: a row read serves both pixels.  It loops over the chunks and
//                                               stores D planes
//   flow_cost_volume_grad_kernel<R, HALF, TO_W> the backward with respect to feat (TO_W false) or to the warped tensor W (TO_W true), both
//                                               gathers: each lane loads the D values of gs = g / C of its two pixels ONCE into registers
//                                               (TO_W: plane o at q - o), the block stages W' (TO_W: feat, 0 outside the frame) of the tile
//                                               and halo per chunk, and a lane walks the window once per channel (TO_W: back to front, so
//                                               that o still ascends) into one sum per pixel.  No scatter, no atomics, no workspace
//
//   flow_cost_volume_chain_kernel<HALF>         the vectors the backward of the warp is run on (ofl_warp_bwd_grad_f32 / ofl_splat_sum_f32
//                                               turn d W into d other and d flow): the flow's own as fp32, and a vector that points out of
//                                               the frame where a component is not finite -- such a pixel is not usable, its d W is +0, and a
//                                               NaN weight times that +0 must reach no gradient
//   flow_cost_volume_gate_kernel<HALF>          d flow of that backward, in place: +0 where the pixel is not usable (selected, as in the
//                                               forward: there d W is +0 and the warp's backward would form 0 * tap, NaN for a tap of `other`
//                                               that is not finite and that no usable pixel samples)
//
// The warped tensor is never written.  The sample (position, taps, weights, the four-term sum and mr) is the one of ofl_loss_common.hpp.
// Taps are single loads straight from global memory at offsets clamped into the plane: always addressable.
//
// Geometry.  A lane's two pixels are vertical neighbours and the lanes of a half wave are 32 consecutive pixels of a row: every LDS read
// of a window position is 32 consecutive floats per half wave (free of bank conflicts at any row pitch, so the pitch is not padded), and
// the 2 R + 2 rows x (2 R + 1) columns a lane reads per channel serve 2 D terms (90 reads for 162 terms at R = 4).  32 x 16 outputs over
// 40 x 24 staged pixels is 1.875 warps per output at R = 4.  LDS: kChanChunk planes of (32 + 2 R) x (16 + 2 R) floats, 61 440 B at R = 4:
// two blocks in a CU's 160 KiB, which is what the 2 D accumulators of a lane allow anyway (two waves per SIMD; DESIGN.md 3.24 has the
// register figures of tools/isa_stats.py).
//
// Every product is rounded, then every sum: fp contraction is off (ofl_loss_common.hpp) and no fmaf is written here.  C ABI:
// include/oflib_hip.h.
#include "ofl_loss_common.hpp"

namespace {

using namespace ofl_loss;

constexpr int kThreads = 256;
constexpr int kTileW = 32, kTileH = 16;            // output pixels of a block
constexpr int kPix = 2;                            // pixels per lane: rows 2 k and 2 k + 1 of the tile, k = thread / kTileW
constexpr int kChanChunk = 16;                     // channels staged together
constexpr int kMaxRadius = 4;

static_assert(kThreads * kPix == kTileW * kTileH, "a lane owns kPix vertically adjacent pixels of the tile");

struct CvParams {
    const void* flow;                              // [*,2,H,W] fp32 or fp16
    int64_t flow_bs;                               // elements between images
    const uint8_t* mask;                           // [*,H,W] bytes or nullptr (all True)
    int64_t mask_bs;
    const float* feat; const float* other;         // [*,C,H,W]: the features on the flow's grid, those of the frame it points into
    int64_t feat_bs, other_bs;
    int64_t hw;
    int32_t chan, h, w, tiles_x;
    float flow_sign;
    float wm1, hm1, half_wm1, half_hm1;
    float* out;                                    // forward: [n][D][H*W]
    const float* g;                                // backward: [n][D][H*W], the upstream gradient
    float* grad;                                   // backward: [n][C][H*W]
};

// is the sample of pixel (x, y) of image n_img usable: valid in the mask and the weight sum of its taps inside the frame above kValidThr
template <bool HALF>
__device__ __forceinline__ bool usable_of(const CvParams& p, int64_t n_img, int x, int y, Taps& t) {
    const int64_t pix = (int64_t)y * p.w + x, fo = n_img * p.flow_bs;
    const float u = ld_flow<HALF>(p.flow, fo + pix), v = ld_flow<HALF>(p.flow, fo + p.hw + pix);
    const bool valid = p.mask == nullptr || p.mask[n_img * p.mask_bs + pix] != 0;
    t = taps_of(p, x, y, u, v);
    return (t.mr > kValidThr) && valid;
}

// W' of the channels c0 .. c0 + nc - 1 (plane k of s_w holds channel c0 + k) of the tile at (x0, y0) and R pixels around it: the sample
// where the pixel is usable, +0 elsewhere and outside the frame (selected, not multiplied: a pixel that is not usable loads no sample)
template <int R, bool HALF>
__device__ __forceinline__ void stage_warp(const CvParams& p, int64_t n_img, int x0, int y0, int c0, int nc, float* s_w) {
    constexpr int RW = kTileW + 2 * R, RH = kTileH + 2 * R;
    const float* ot = p.other + n_img * p.other_bs + (int64_t)c0 * p.hw;
    for (int i = threadIdx.x; i < RW * RH; i += kThreads) {
        const int ry = i / RW, rx = i - ry * RW;
        const int x = x0 - R + rx, y = y0 - R + ry;
        Taps t;
        bool us = false;
        if (x >= 0 && x < p.w && y >= 0 && y < p.h) us = usable_of<HALF>(p, n_img, x, y, t);
        if (us) {
#pragma unroll 4
            for (int k = 0; k < nc; ++k) {
                const float* pl = ot + (int64_t)k * p.hw;
                const float v_nw = t.k_nw ? pl[t.o_nw] : 0.0f;
                const float v_ne = t.k_ne ? pl[t.o_ne] : 0.0f;
                const float v_sw = t.k_sw ? pl[t.o_sw] : 0.0f;
                const float v_se = t.k_se ? pl[t.o_se] : 0.0f;
                s_w[k * RW * RH + i] = sample_of(t, v_nw, v_ne, v_sw, v_se);
            }
        } else {
            for (int k = 0; k < nc; ++k) s_w[k * RW * RH + i] = 0.0f;
        }
    }
}

// feat of the same channels and pixels, 0 outside the frame
template <int R>
__device__ __forceinline__ void stage_feat(const CvParams& p, int64_t n_img, int x0, int y0, int c0, int nc, float* s_w) {
    constexpr int RW = kTileW + 2 * R, RH = kTileH + 2 * R;
    const float* ft = p.feat + n_img * p.feat_bs + (int64_t)c0 * p.hw;
    for (int i = threadIdx.x; i < RW * RH; i += kThreads) {
        const int ry = i / RW, rx = i - ry * RW;
        const int x = x0 - R + rx, y = y0 - R + ry;
        const bool in = x >= 0 && x < p.w && y >= 0 && y < p.h;
        const int64_t pix = in ? (int64_t)y * p.w + x : 0;
#pragma unroll 4
        for (int k = 0; k < nc; ++k) s_w[k * RW * RH + i] = in ? ft[(int64_t)k * p.hw + pix] : 0.0f;
    }
}

// One walk of the windows of a lane's two pixels over one staged plane: `s` points at the window's first row and column of the upper
// pixel (pitch RW), f(pixel, o, value) is called for both pixels with o ascending.  FLIP false: window position o holds the staged pixel
// p + o; FLIP true: p - o (the walk goes back to front).  A row read serves both pixels.
template <int R, bool FLIP, class F>
__device__ __forceinline__ void walk(const float* s, F&& f) {
    constexpr int WIN = 2 * R + 1, D = WIN * WIN, RW = kTileW + 2 * R;
#pragma unroll
    for (int jj = 0; jj <= WIN; ++jj) {
        const int j = FLIP ? WIN - jj : jj;        // staged row, counted from the upper pixel's first window row
        float v[WIN];
#pragma unroll
        for (int d = 0; d < WIN; ++d) v[d] = s[j * RW + d];
#pragma unroll
        for (int dd = 0; dd < WIN; ++dd) {
            const int d = FLIP ? WIN - 1 - dd : dd;
            if (j < WIN) f(0, FLIP ? D - 1 - (j * WIN + d) : j * WIN + d, v[d]);
            if (j >= 1) f(1, FLIP ? D - 1 - ((j - 1) * WIN + d) : (j - 1) * WIN + d, v[d]);
        }
    }
}

template <int R, bool HALF>
__global__ void __launch_bounds__(kThreads) flow_cost_volume_kernel(CvParams p) {
    constexpr int WIN = 2 * R + 1, D = WIN * WIN, RW = kTileW + 2 * R, RH = kTileH + 2 * R;
    __shared__ float s_w[kChanChunk * RW * RH];
    const int64_t n_img = blockIdx.y;
    const int ty = (int)(blockIdx.x / (uint32_t)p.tiles_x), tx = (int)(blockIdx.x - (uint32_t)ty * (uint32_t)p.tiles_x);
    const int x0 = tx * kTileW, y0 = ty * kTileH;
    const int lx = threadIdx.x % kTileW, row = kPix * (threadIdx.x / kTileW);
    const int x = x0 + lx, y = y0 + row;
    const bool in0 = x < p.w && y < p.h, in1 = x < p.w && y + 1 < p.h;
    const float* ft = p.feat + n_img * p.feat_bs + (int64_t)y * p.w + x;
    float acc[kPix][D];
#pragma unroll
    for (int o = 0; o < D; ++o) { acc[0][o] = 0.0f; acc[1][o] = 0.0f; }
#pragma unroll 1
    for (int c0 = 0; c0 < p.chan; c0 += kChanChunk) {
        const int nc = p.chan - c0 < kChanChunk ? p.chan - c0 : kChanChunk;
        __syncthreads();                           // (the planes of the chunk before are read to the end)
        stage_warp<R, HALF>(p, n_img, x0, y0, c0, nc, s_w);
        __syncthreads();
        float f0 = in0 ? ft[(int64_t)c0 * p.hw] : 0.0f, f1 = in1 ? ft[(int64_t)c0 * p.hw + p.w] : 0.0f;
#pragma unroll 1
        for (int k = 0; k < nc; ++k) {
            const float a0 = f0, a1 = f1;
            if (k + 1 < nc) {                      // the next channel's two features are on their way during the walk
                f0 = in0 ? ft[(int64_t)(c0 + k + 1) * p.hw] : 0.0f;
                f1 = in1 ? ft[(int64_t)(c0 + k + 1) * p.hw + p.w] : 0.0f;
            }
            walk<R, false>(s_w + k * RW * RH + row * RW + lx, [&](int px, int o, float v) {
                const float prod = (px == 0 ? a0 : a1) * v;
                acc[px][o] = acc[px][o] + prod;
            });
        }
    }
    const float fc = (float)p.chan;
    float* out = p.out + n_img * D * p.hw + (int64_t)y * p.w + x;
    if (in0) {
#pragma unroll
        for (int o = 0; o < D; ++o) out[(int64_t)o * p.hw] = acc[0][o] / fc;
    }
    if (in1) {
#pragma unroll
        for (int o = 0; o < D; ++o) out[(int64_t)o * p.hw + p.w] = acc[1][o] / fc;
    }
}

template <int R, bool HALF, bool TO_W>
__global__ void __launch_bounds__(kThreads) flow_cost_volume_grad_kernel(CvParams p) {
    constexpr int WIN = 2 * R + 1, D = WIN * WIN, RW = kTileW + 2 * R, RH = kTileH + 2 * R;
    __shared__ float s_w[kChanChunk * RW * RH];
    const int64_t n_img = blockIdx.y;
    const int ty = (int)(blockIdx.x / (uint32_t)p.tiles_x), tx = (int)(blockIdx.x - (uint32_t)ty * (uint32_t)p.tiles_x);
    const int x0 = tx * kTileW, y0 = ty * kTileH;
    const int lx = threadIdx.x % kTileW, row = kPix * (threadIdx.x / kTileW);
    const int x = x0 + lx, y = y0 + row;
    const bool in[kPix] = {x < p.w && y < p.h, x < p.w && y + 1 < p.h};
    // gs = g / C of the lane's two pixels: plane o at the pixel itself, or at q - o for the gradient of W (0 outside the frame)
    const float fc = (float)p.chan;
    const float* g = p.g + n_img * D * p.hw;
    float gs[kPix][D];
#pragma unroll
    for (int px = 0; px < kPix; ++px) {
#pragma unroll
        for (int o = 0; o < D; ++o) {
            const int dy = o / WIN - R, dx = o % WIN - R;
            const int gx = TO_W ? x - dx : x, gy = TO_W ? y + px - dy : y + px;
            const bool ok = in[px] && gx >= 0 && gx < p.w && gy >= 0 && gy < p.h;
            gs[px][o] = ok ? g[(int64_t)o * p.hw + (int64_t)gy * p.w + gx] / fc : 0.0f;
        }
    }
    bool keep[kPix] = {in[0], in[1]};              // the gradient of W is +0 where the pixel is not usable
    if (TO_W) {
#pragma unroll
        for (int px = 0; px < kPix; ++px) {
            Taps t;
            if (in[px]) keep[px] = usable_of<HALF>(p, n_img, x, y + px, t);
        }
    }
    float* go = p.grad + n_img * p.chan * p.hw + (int64_t)y * p.w + x;
#pragma unroll 1
    for (int c0 = 0; c0 < p.chan; c0 += kChanChunk) {
        const int nc = p.chan - c0 < kChanChunk ? p.chan - c0 : kChanChunk;
        __syncthreads();                           // (the planes of the chunk before are read to the end)
        if (TO_W) stage_feat<R>(p, n_img, x0, y0, c0, nc, s_w);
        else stage_warp<R, HALF>(p, n_img, x0, y0, c0, nc, s_w);
        __syncthreads();
#pragma unroll 1
        for (int k = 0; k < nc; ++k) {
            float sum[kPix] = {0.0f, 0.0f};
            walk<R, TO_W>(s_w + k * RW * RH + row * RW + lx, [&](int px, int o, float v) {
                const float prod = gs[px][o] * v;
                sum[px] = sum[px] + prod;
            });
            if (in[0]) go[(int64_t)(c0 + k) * p.hw] = keep[0] ? sum[0] : 0.0f;
            if (in[1]) go[(int64_t)(c0 + k) * p.hw + p.w] = keep[1] ? sum[1] : 0.0f;
        }
    }
}

// the x component of the vector a pixel with a non-finite vector gets in the chain: flow_sign * 2^31 puts the sample at x - 2^31, left of
// every legal frame (w < 2^31), so that no tap lies inside the frame
constexpr float kChainAway = 2147483648.0f;

template <bool HALF>
__global__ void __launch_bounds__(kThreads) flow_cost_volume_chain_kernel(CvParams p) {
    const int64_t n_img = blockIdx.y, fo = n_img * p.flow_bs;
    float* out = p.grad + n_img * 2 * p.hw;
    for (int64_t pix = (int64_t)blockIdx.x * kThreads + threadIdx.x; pix < p.hw; pix += (int64_t)gridDim.x * kThreads) {
        float u = ld_flow<HALF>(p.flow, fo + pix), v = ld_flow<HALF>(p.flow, fo + p.hw + pix);
        if (!(__builtin_isfinite(u) && __builtin_isfinite(v))) { u = p.flow_sign * kChainAway; v = 0.0f; }
        out[pix] = u;
        out[p.hw + pix] = v;
    }
}

template <bool HALF>
__global__ void __launch_bounds__(kThreads) flow_cost_volume_gate_kernel(CvParams p) {
    const int64_t n_img = blockIdx.y;
    float* gf = p.grad + n_img * 2 * p.hw;
    for (int64_t pix = (int64_t)blockIdx.x * kThreads + threadIdx.x; pix < p.hw; pix += (int64_t)gridDim.x * kThreads) {
        const int y = (int)(pix / p.w), x = (int)(pix - (int64_t)y * p.w);
        Taps t;
        if (!usable_of<HALF>(p, n_img, x, y, t)) {
            gf[pix] = 0.0f;
            gf[p.hw + pix] = 0.0f;
        }
    }
}

bool radius_ok(int32_t radius) { return radius >= 1 && radius <= kMaxRadius; }

int64_t tiles_of(int32_t extent, int tile) { return ((int64_t)extent + tile - 1) / tile; }

// the flow, its mask and the frame: the operands and the checks every entry point shares
int fill_flow(CvParams* p, const void* flow, int64_t flow_bs, int32_t flow_half, const uint8_t* mask, int64_t mask_bs, float flow_sign,
              int32_t n, int32_t h, int32_t w) {
    if (!dims_ok(n, h, w, 2)) return OFL_E_ARG;
    if (flow_sign != 1.0f && flow_sign != -1.0f) return OFL_E_ARG;
    if (flow == nullptr) return OFL_E_ARG;
    if (flow_half != 0 && flow_half != 1) return OFL_E_ARG;
    if (flow_bs < 0 || mask_bs < 0) return OFL_E_ARG;
    if (!aligned(flow, flow_half ? 2 : 4)) return OFL_E_ARG;
    p->flow = flow; p->flow_bs = flow_bs;
    p->mask = mask; p->mask_bs = mask_bs;
    p->feat = nullptr; p->other = nullptr; p->feat_bs = 0; p->other_bs = 0;
    p->hw = (int64_t)h * w;
    p->chan = 0; p->h = h; p->w = w;
    p->tiles_x = (int32_t)tiles_of(w, kTileW);
    p->flow_sign = flow_sign;
    p->wm1 = (float)(w - 1); p->hm1 = (float)(h - 1);
    p->half_wm1 = p->wm1 / 2.0f; p->half_hm1 = p->hm1 / 2.0f;
    p->out = nullptr; p->g = nullptr; p->grad = nullptr;
    return OFL_OK;
}

// the operands and the checks the volume and its gradients share
int fill_operands(CvParams* p, const void* flow, int64_t flow_bs, int32_t flow_half, const uint8_t* mask, int64_t mask_bs, const float* feat,
                  int64_t feat_bs, const float* other, int64_t other_bs, int32_t channels, float flow_sign, int32_t radius, int32_t n,
                  int32_t h, int32_t w) {
    const int rc = fill_flow(p, flow, flow_bs, flow_half, mask, mask_bs, flow_sign, n, h, w);
    if (rc) return rc;
    if (!radius_ok(radius) || channels < 1) return OFL_E_ARG;
    if (feat == nullptr || other == nullptr) return OFL_E_ARG;
    if (feat_bs < 0 || other_bs < 0) return OFL_E_ARG;
    if (!aligned(feat, 4) || !aligned(other, 4)) return OFL_E_ARG;
    p->feat = feat; p->other = other; p->feat_bs = feat_bs; p->other_bs = other_bs;
    p->chan = channels;
    return OFL_OK;
}

// the grid of the two per-pixel kernels: 256 pixels per block, grid-stride beyond the cap
dim3 pixel_grid_of(int32_t n, int32_t h, int32_t w) {
    const int64_t blocks = ((int64_t)h * w + kThreads - 1) / kThreads;
    return dim3((unsigned)(blocks < 65536 ? blocks : 65536), (unsigned)n);
}

dim3 grid_of(int32_t n, int32_t h, int32_t w) {
    return dim3((unsigned)(tiles_of(w, kTileW) * tiles_of(h, kTileH)), (unsigned)n);     // (h * w < 2^31: under 2^22 tiles)
}

// the radius and the flow's storage to the <R, HALF> instantiation: f(std::integral_constant<int, R>, std::bool_constant<HALF>)
template <class F>
void dispatch(int radius, bool half, F&& f) {
    auto with_r = [&](auto RR) {
        if (half) f(RR, std::true_type{});
        else f(RR, std::false_type{});
    };
    if (radius == 1) with_r(std::integral_constant<int, 1>{});
    else if (radius == 2) with_r(std::integral_constant<int, 2>{});
    else if (radius == 3) with_r(std::integral_constant<int, 3>{});
    else with_r(std::integral_constant<int, 4>{});
}

}  // namespace

extern "C" {

__attribute__((visibility("default"))) int ofl_flow_cost_volume_f32(const void* flow, int64_t flow_bs, int32_t flow_half, const uint8_t* mask,
                                                                    int64_t mask_bs, const float* feat, int64_t feat_bs, const float* other,
                                                                    int64_t other_bs, int32_t channels, float flow_sign, int32_t radius,
                                                                    float* volume, int32_t n, int32_t h, int32_t w, void* stream) {
    CvParams p;
    const int rc = fill_operands(&p, flow, flow_bs, flow_half, mask, mask_bs, feat, feat_bs, other, other_bs, channels, flow_sign, radius,
                                 n, h, w);
    if (rc) return rc;
    if (!volume || !aligned(volume, 4)) return OFL_E_ARG;
    p.out = volume;
    hipStream_t s = (hipStream_t)stream;
    dispatch(radius, flow_half != 0, [&](auto RR, auto HALF) {
        OFL_KLAUNCH((flow_cost_volume_kernel<decltype(RR)::value, decltype(HALF)::value>), grid_of(n, h, w), dim3(kThreads), 0, s, p);
    });
    return (int)hipGetLastError();
}

__attribute__((visibility("default"))) int ofl_flow_cost_volume_grad_f32(const void* flow, int64_t flow_bs, int32_t flow_half,
                                                                         const uint8_t* mask, int64_t mask_bs, const float* feat,
                                                                         int64_t feat_bs, const float* other, int64_t other_bs,
                                                                         int32_t channels, float flow_sign, int32_t radius,
                                                                         const float* grad_volume, float* grad_feat, float* grad_warped,
                                                                         int32_t n, int32_t h, int32_t w, void* stream) {
    CvParams p;
    const int rc = fill_operands(&p, flow, flow_bs, flow_half, mask, mask_bs, feat, feat_bs, other, other_bs, channels, flow_sign, radius,
                                 n, h, w);
    if (rc) return rc;
    if (!grad_volume || !aligned(grad_volume, 4)) return OFL_E_ARG;
    if ((!grad_feat && !grad_warped) || !aligned(grad_feat, 4) || !aligned(grad_warped, 4)) return OFL_E_ARG;
    p.g = grad_volume;
    hipStream_t s = (hipStream_t)stream;
    if (grad_feat) {
        p.grad = grad_feat;
        dispatch(radius, flow_half != 0, [&](auto RR, auto HALF) {
            OFL_KLAUNCH((flow_cost_volume_grad_kernel<decltype(RR)::value, decltype(HALF)::value, false>), grid_of(n, h, w),
                        dim3(kThreads), 0, s, p);
        });
    }
    if (grad_warped) {
        p.grad = grad_warped;
        dispatch(radius, flow_half != 0, [&](auto RR, auto HALF) {
            OFL_KLAUNCH((flow_cost_volume_grad_kernel<decltype(RR)::value, decltype(HALF)::value, true>), grid_of(n, h, w),
                        dim3(kThreads), 0, s, p);
        });
    }
    return (int)hipGetLastError();
}

__attribute__((visibility("default"))) int ofl_flow_cost_volume_chain_f32(const void* flow, int64_t flow_bs, int32_t flow_half, float flow_sign,
                                                                          float* chain, int32_t n, int32_t h, int32_t w, void* stream) {
    CvParams p;
    const int rc = fill_flow(&p, flow, flow_bs, flow_half, nullptr, 0, flow_sign, n, h, w);
    if (rc) return rc;
    if (!chain || !aligned(chain, 4)) return OFL_E_ARG;
    p.grad = chain;
    hipStream_t s = (hipStream_t)stream;
    if (flow_half) OFL_KLAUNCH((flow_cost_volume_chain_kernel<true>), pixel_grid_of(n, h, w), dim3(kThreads), 0, s, p);
    else OFL_KLAUNCH((flow_cost_volume_chain_kernel<false>), pixel_grid_of(n, h, w), dim3(kThreads), 0, s, p);
    return (int)hipGetLastError();
}

__attribute__((visibility("default"))) int ofl_flow_cost_volume_gate_f32(const void* flow, int64_t flow_bs, int32_t flow_half, const uint8_t* mask,
                                                                         int64_t mask_bs, float flow_sign, float* grad_flow, int32_t n,
                                                                         int32_t h, int32_t w, void* stream) {
    CvParams p;
    const int rc = fill_flow(&p, flow, flow_bs, flow_half, mask, mask_bs, flow_sign, n, h, w);
    if (rc) return rc;
    if (!grad_flow || !aligned(grad_flow, 4)) return OFL_E_ARG;
    p.grad = grad_flow;
    hipStream_t s = (hipStream_t)stream;
    if (flow_half) OFL_KLAUNCH((flow_cost_volume_gate_kernel<true>), pixel_grid_of(n, h, w), dim3(kThreads), 0, s, p);
    else OFL_KLAUNCH((flow_cost_volume_gate_kernel<false>), pixel_grid_of(n, h, w), dim3(kThreads), 0, s, p);
    return (int)hipGetLastError();
}

}  // extern "C"
