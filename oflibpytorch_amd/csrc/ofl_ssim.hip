// ofl_ssim.hip -- Flow.ssim / ssim_map / ssim_stats on gfx950: the structural-similarity data term of an unsupervised flow loss, warp and
// windowed comparison in one pass (which DEFINES the numbers; tests/ssim_oracle.py is the same definition in NumPy).  An
// extension: the reference has no such function.
//
//   flow_ssim_kernel<WINDOW, HALF, U8>         a block owns a tile of 64 x 16 output pixels.  It stages, for the tile and a halo of R =
//                                              WINDOW / 2 pixels, every channel X_c of `other` sampled where the flow points, Y_c of `img`
//                                              and the usable byte (in the frame, valid in the mask, sample inside `other`) in LDS: every
//                                              staged pixel is warped ONCE, the channels together.  Each lane then gathers the usable bits
//                                              of the window of each of its four pixels into one 64-bit word and walks the window twice per
//                                              channel out of LDS (dy ascending, dx ascending within it): the means, then the moments
//                                              about them.  Writes rho (0 where not known) if a map is wanted and, per block, ONE record of
//                                              8 float64
//   flow_ssim_finish_kernel                    one block per image: the block records added in ascending block order, from LDS
//   flow_ssim_grad_kernel<WINDOW, HALF, U8>    the backward of the per-image mean with respect to the flow vectors, ONE CHANNEL AT A TIME
//                                              through the same LDS: stages X_c, Y_c of the tile with a halo of 2 R, forms the three
//                                              float64 coefficients a0, a1, a2 of the tile plus a halo of R into LDS, then every pixel box-
//                                              sums them over its window and multiplies by the derivative of its own sample: no scatter, no
//                                              atomics, no workspace
//
// Neither the warped image nor a pooled tensor is written.  The sample (position, taps, weights, the four-term sums and mr) is the one
// of ofl_loss_common.hpp, which restates the backward warp of ofl_kernels.hip; tests/test_gpu_ssim.py compares the two on the device.  A
// uint8 sample s is float(s) / 255.0f (ld_img_unit).  Taps are single loads straight from global memory at offsets clamped into the
// plane: always addressable.
//
// The tile is the one ofl_census.hip arrived at: a row of 64 outputs is one wave, its LDS reads of one window offset are 64 consecutive
// floats (free of bank conflicts at any row pitch, so the pitch is not padded), a wave's map store is one run of 256 bytes, and 64 x 16
// outputs over 70 x 22 staged pixels is 1.50 warps per output at R = 3.  LDS, forward: 6 floats and a byte per staged pixel, 38 768 B
// at R = 3 with the 256 B of the waves' records (four blocks in a CU's 160 KiB).  The backward would need 9 float64 coefficient planes
// of 70 x 22 next to 6 float planes of 76 x 28 with the channels together (164 KB): it runs the channels one after the other through 2
// float planes and 3 float64 planes, 56 112 B at R = 3, and warps a staged pixel once per channel.
// 256 threads, four pixels per lane (rows ly, ly + 4, ly + 8, ly + 12 of the tile).
//
// The sums are those of ofl_loss_common.hpp; the number of blocks depends on (h, w) only.  C ABI: include/oflib_hip.h.
#include "ofl_loss_common.hpp"

namespace {

using namespace ofl_loss;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTileW = 64, kTileH = 16;            // output pixels of a block
constexpr int kRows = kTileH / kWaves;             // pixels per lane
constexpr int kChunk = 256;                        // block records the finish kernel stages at a time
constexpr int kRec = OFL_SSIM_RECORD;              // doubles per record
constexpr int kChan = 3;                           // channels the forward stages together
enum { R_COUNT = 0, R_SUM = 1, R_MAX = 2, R_TERMS = 3, R_USED = 4 };

struct SsimParams {
    const void* flow;                              // [*,2,H,W] fp32 or fp16
    int64_t flow_bs;                               // elements between images
    const uint8_t* mask;                           // [*,H,W] bytes or nullptr (all True)
    int64_t mask_bs;
    const void* img; const void* other;            // [*,C,H,W] fp32 or uint8: the frame on the flow's grid, the frame it points into
    int64_t img_bs, other_bs;
    int64_t hw;
    int32_t chan, h, w, tiles_x, nblk;
    float flow_sign, c1, c2;
    float wm1, hm1, half_wm1, half_hm1;
    double* partial;                               // [n][nblk][kRec] or nullptr (no record wanted)
    float* map;                                    // [n][H*W] or nullptr
    double* out;                                   // [n][kRec]
    const float* scale;                            // backward: [n]
    float* grad;                                   // backward: [n][2][H*W]
};

// X_c, Y_c of the channels c0 .. c0 + NC - 1 (plane k of s_x / s_y holds channel c0 + k; a channel the images do not have is not
// touched) and the usable byte of the tile at (x0, y0) and HALO pixels around it; a pixel outside the frame is not usable, a pixel that
// is not usable loads no image sample
template <int HALO, int NC, bool HALF, bool U8>
__device__ __forceinline__ void stage(const SsimParams& p, int64_t n_img, int x0, int y0, int c0, float* s_x, float* s_y, uint8_t* s_us) {
    constexpr int RW = kTileW + 2 * HALO, RH = kTileH + 2 * HALO;
    const int64_t fo = n_img * p.flow_bs;
    const uint8_t* mk = p.mask ? p.mask + n_img * p.mask_bs : nullptr;
    const int64_t io = n_img * p.img_bs, oo = n_img * p.other_bs;
    for (int i = threadIdx.x; i < RW * RH; i += kThreads) {
        const int ry = i / RW, rx = i - ry * RW;
        const int x = x0 - HALO + rx, y = y0 - HALO + ry;
        float vx[NC], vy[NC];
#pragma unroll
        for (int k = 0; k < NC; ++k) { vx[k] = 0.0f; vy[k] = 0.0f; }
        bool us = false;
        if (x >= 0 && x < p.w && y >= 0 && y < p.h) {
            const int64_t pix = (int64_t)y * p.w + x;
            const float u = ld_flow<HALF>(p.flow, fo + pix), v = ld_flow<HALF>(p.flow, fo + p.hw + pix);
            const bool valid = mk == nullptr || mk[pix] != 0;
            const Taps t = taps_of(p, x, y, u, v);
            us = (t.mr > kValidThr) && valid;
            if (us) {
#pragma unroll
                for (int k = 0; k < NC; ++k) {
                    if (c0 + k < p.chan) {
                        const int64_t pl = oo + (int64_t)(c0 + k) * p.hw;
                        const float v_nw = t.k_nw ? ld_img_unit<U8>(p.other, pl + t.o_nw) : 0.0f;
                        const float v_ne = t.k_ne ? ld_img_unit<U8>(p.other, pl + t.o_ne) : 0.0f;
                        const float v_sw = t.k_sw ? ld_img_unit<U8>(p.other, pl + t.o_sw) : 0.0f;
                        const float v_se = t.k_se ? ld_img_unit<U8>(p.other, pl + t.o_se) : 0.0f;
                        vx[k] = sample_of(t, v_nw, v_ne, v_sw, v_se);
                        vy[k] = ld_img_unit<U8>(p.img, io + (int64_t)(c0 + k) * p.hw + pix);
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            if (c0 + k < p.chan) { s_x[k * RW * RH + i] = vx[k]; s_y[k * RW * RH + i] = vy[k]; }
        }
        s_us[i] = us ? 1 : 0;
    }
}

// the usable bits of the window around the staged pixel at index c (pitch RW): bit (dy + R) * WINDOW + dx + R, the centre included
template <int R, int RW>
__device__ __forceinline__ uint64_t window_bits(const uint8_t* s_us, int c) {
    constexpr int WIN = 2 * R + 1;
    uint64_t m = 0;
#pragma unroll
    for (int dy = -R; dy <= R; ++dy) {
        uint32_t row = 0;
#pragma unroll
        for (int dx = -R; dx <= R; ++dx) row |= (s_us[c + dy * RW + dx] != 0 ? 1u : 0u) << (dx + R);
        m |= (uint64_t)row << ((dy + R) * WIN);
    }
    return m;
}

// d_c = clamp((1 - ssim_c) / 2) of the window `m` around index c of one channel's planes: fp32, one rounding per operation, two walks
template <int R, int RW>
__device__ __forceinline__ float walk(const float* s_x, const float* s_y, int c, uint64_t m, float fn, float c1, float c2) {
    constexpr int WIN = 2 * R + 1;
    float sx = 0.0f, sy = 0.0f;
#pragma unroll 1
    for (int dy = -R; dy <= R; ++dy) {
        const uint32_t row = (uint32_t)(m >> ((dy + R) * WIN));
#pragma unroll
        for (int dx = -R; dx <= R; ++dx) {
            if ((row >> (dx + R)) & 1u) {
                const int o = c + dy * RW + dx;
                sx = sx + s_x[o];
                sy = sy + s_y[o];
            }
        }
    }
    const float mux = sx / fn, muy = sy / fn;
    float vxx = 0.0f, vyy = 0.0f, vxy = 0.0f;
#pragma unroll 1
    for (int dy = -R; dy <= R; ++dy) {
        const uint32_t row = (uint32_t)(m >> ((dy + R) * WIN));
#pragma unroll
        for (int dx = -R; dx <= R; ++dx) {
            if ((row >> (dx + R)) & 1u) {
                const int o = c + dy * RW + dx;
                const float ax = s_x[o] - mux, ay = s_y[o] - muy;
                vxx = vxx + ax * ax;
                vyy = vyy + ay * ay;
                vxy = vxy + ax * ay;
            }
        }
    }
    const float oxx = vxx / fn, oyy = vyy / fn, oxy = vxy / fn;
    const float l1 = (2.0f * mux) * muy + c1;
    const float l2 = (mux * mux + muy * muy) + c1;
    const float s1 = 2.0f * oxy + c2;
    const float s2 = (oxx + oyy) + c2;
    const float ssim = (l1 * s1) / (l2 * s2);
    const float d = (1.0f - ssim) * 0.5f;
    return d < 0.0f ? 0.0f : (d > 1.0f ? 1.0f : d);    // (comparisons: a NaN passes through)
}

template <int WINDOW, bool HALF, bool U8>
__global__ void __launch_bounds__(kThreads) flow_ssim_kernel(SsimParams p) {
    constexpr int R = WINDOW / 2, RW = kTileW + 2 * R, RH = kTileH + 2 * R;
    __shared__ float s_x[kChan * RW * RH];
    __shared__ float s_y[kChan * RW * RH];
    __shared__ uint8_t s_us[RW * RH];
    __shared__ double s_red[kWaves * kRec];
    const int64_t n_img = blockIdx.y;
    const int ty = (int)(blockIdx.x / (uint32_t)p.tiles_x), tx = (int)(blockIdx.x - (uint32_t)ty * (uint32_t)p.tiles_x);
    const int x0 = tx * kTileW, y0 = ty * kTileH;
    stage<R, kChan, HALF, U8>(p, n_img, x0, y0, 0, s_x, s_y, s_us);
    __syncthreads();
    const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
    const int x = x0 + lx;
    const float fc = (float)p.chan;
    uint32_t count = 0u, terms = 0u;
    double sum = 0.0;
    float mx = 0.0f;
#pragma unroll 1
    for (int k = 0; k < kRows; ++k) {
        const int row = ly + k * kWaves, y = y0 + row;
        if (x < p.w && y < p.h) {
            const int c = (row + R) * RW + lx + R;
            const bool known = s_us[c] != 0;
            int n = 0;
            float rho = 0.0f;
            if (known) {
                const uint64_t m = window_bits<R, RW>(s_us, c);
                n = __popcll(m);
                const float fn = (float)n;
                float acc = walk<R, RW>(s_x, s_y, c, m, fn, p.c1, p.c2);
                if (p.chan == 3) {
                    acc = acc + walk<R, RW>(s_x + RW * RH, s_y + RW * RH, c, m, fn, p.c1, p.c2);
                    acc = acc + walk<R, RW>(s_x + 2 * RW * RH, s_y + 2 * RW * RH, c, m, fn, p.c1, p.c2);
                }
                rho = acc / fc;
            }
            if (p.map != nullptr) p.map[n_img * p.hw + (int64_t)y * p.w + x] = known ? rho : 0.0f;
            count += known ? 1u : 0u;
            terms += (uint32_t)n;
            sum += known ? (double)rho : 0.0;
            mx = (known && rho > mx) ? rho : mx;
        }
    }
    if (p.partial == nullptr) return;              // (the same for every thread of the launch)
    double rec[kRec];
#pragma unroll
    for (int i = 0; i < kRec; ++i) rec[i] = 0.0;
    rec[R_COUNT] = (double)count; rec[R_SUM] = sum; rec[R_MAX] = (double)mx; rec[R_TERMS] = (double)terms;
    reduce_record<kRec, R_USED, R_MAX, kWaves>(rec, s_red, p.partial, n_img, p.nblk);
}

// one block per image: the block records added in ascending block order, kChunk of them through LDS at a time
__global__ void __launch_bounds__(kThreads) flow_ssim_finish_kernel(SsimParams p) {
    finish_records<kRec, R_MAX, kChunk, kThreads>(p.partial, p.nblk, p.out);
}

template <int WINDOW, bool HALF, bool U8>
__global__ void __launch_bounds__(kThreads) flow_ssim_grad_kernel(SsimParams p) {
    constexpr int R = WINDOW / 2, H2 = 2 * R;
    constexpr int RW = kTileW + 2 * H2, RH = kTileH + 2 * H2;      // staged: the tile and 2 R around it
    constexpr int KW = kTileW + 2 * R, KH = kTileH + 2 * R;        // coefficients: the tile and R around it
    __shared__ float s_x[RW * RH];
    __shared__ float s_y[RW * RH];
    __shared__ uint8_t s_us[RW * RH];
    __shared__ double s_a0[KW * KH];
    __shared__ double s_a1[KW * KH];
    __shared__ double s_a2[KW * KH];
    const int64_t n_img = blockIdx.y;
    const int ty = (int)(blockIdx.x / (uint32_t)p.tiles_x), tx = (int)(blockIdx.x - (uint32_t)ty * (uint32_t)p.tiles_x);
    const int x0 = tx * kTileW, y0 = ty * kTileH;
    const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
    const int x = x0 + lx;
    const double c1 = (double)p.c1, c2 = (double)p.c2;
    const int64_t fo = n_img * p.flow_bs, oo = n_img * p.other_bs;
    double gx_acc[kRows], gy_acc[kRows];
#pragma unroll
    for (int k = 0; k < kRows; ++k) { gx_acc[k] = 0.0; gy_acc[k] = 0.0; }
#pragma unroll 1
    for (int ch = 0; ch < p.chan; ++ch) {
        __syncthreads();                           // (the planes of the channel before are read to the end)
        stage<H2, 1, HALF, U8>(p, n_img, x0, y0, ch, s_x, s_y, s_us);
        __syncthreads();
        // a0, a1, a2 of every centre of the tile plus R, float64 on the fp32 X, Y of the forward by the same two walks; 0 where the
        // centre is not known.  The image's scale and -1 / (2 C) are applied at the end
        for (int i = threadIdx.x; i < KW * KH; i += kThreads) {
            const int ky = i / KW, kx = i - ky * KW;
            const int c = (ky + R) * RW + kx + R;
            double a0 = 0.0, a1 = 0.0, a2 = 0.0;
            if (s_us[c] != 0) {
                const uint64_t m = window_bits<R, RW>(s_us, c);
                const double dn = (double)__popcll(m);
                double sx = 0.0, sy = 0.0;
#pragma unroll 1
                for (int dy = -R; dy <= R; ++dy) {
                    const uint32_t row = (uint32_t)(m >> ((dy + R) * WINDOW));
#pragma unroll
                    for (int dx = -R; dx <= R; ++dx) {
                        if ((row >> (dx + R)) & 1u) {
                            const int o = c + dy * RW + dx;
                            sx += (double)s_x[o];
                            sy += (double)s_y[o];
                        }
                    }
                }
                const double mux = sx / dn, muy = sy / dn;
                double vxx = 0.0, vyy = 0.0, vxy = 0.0;
#pragma unroll 1
                for (int dy = -R; dy <= R; ++dy) {
                    const uint32_t row = (uint32_t)(m >> ((dy + R) * WINDOW));
#pragma unroll
                    for (int dx = -R; dx <= R; ++dx) {
                        if ((row >> (dx + R)) & 1u) {
                            const int o = c + dy * RW + dx;
                            const double ax = (double)s_x[o] - mux, ay = (double)s_y[o] - muy;
                            vxx += ax * ax;
                            vyy += ay * ay;
                            vxy += ax * ay;
                        }
                    }
                }
                const double A = (2.0 * mux) * muy + c1, D = (mux * mux + muy * muy) + c1;
                const double B = 2.0 * (vxy / dn) + c2, E = (vxx / dn + vyy / dn) + c2;
                const double de = D * E, tn = 2.0 / dn;
                a0 = tn * (((B * muy / de - A * B * mux / (D * de)) - A * muy / de) + A * B * mux / (de * E));
                a1 = tn * (A / de);
                a2 = -(tn * (A * B / (de * E)));
            }
            s_a0[i] = a0; s_a1[i] = a1; s_a2[i] = a2;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kRows; ++k) {
            const int row = ly + k * kWaves, y = y0 + row;
            const int c = (row + H2) * RW + lx + H2;
            if (x < p.w && y < p.h && s_us[c] != 0) {
                const int ck = (row + R) * KW + lx + R;
                double t0 = 0.0, t1 = 0.0, t2 = 0.0;
#pragma unroll 1
                for (int dy = -R; dy <= R; ++dy) {
#pragma unroll
                    for (int dx = -R; dx <= R; ++dx) {
                        const int o = ck + dy * KW + dx;
                        t0 += s_a0[o]; t1 += s_a1[o]; t2 += s_a2[o];
                    }
                }
                const double dX = (t0 + t1 * (double)s_y[c]) + t2 * (double)s_x[c];   // sum over p of d ssim_c(p) / d X_c(x)
                // the derivative of the pixel's own sample
                const int64_t pix = (int64_t)y * p.w + x;
                const float u = ld_flow<HALF>(p.flow, fo + pix), v = ld_flow<HALF>(p.flow, fo + p.hw + pix);
                const Taps t = taps_of(p, x, y, u, v);
                const int64_t pl = oo + (int64_t)ch * p.hw;
                const double v_nw = t.k_nw ? (double)ld_img_unit<U8>(p.other, pl + t.o_nw) : 0.0;
                const double v_ne = t.k_ne ? (double)ld_img_unit<U8>(p.other, pl + t.o_ne) : 0.0;
                const double v_sw = t.k_sw ? (double)ld_img_unit<U8>(p.other, pl + t.o_sw) : 0.0;
                const double v_se = t.k_se ? (double)ld_img_unit<U8>(p.other, pl + t.o_se) : 0.0;
                double gx, gy;
                sample_grad(t, v_nw, v_ne, v_sw, v_se, gx, gy);
                gx_acc[k] += dX * gx;
                gy_acc[k] += dX * gy;
            }
        }
    }
    // dL/dX_c = -scale / (2 C) * dX;  dX_c / d flow = -flow_sign * (gx_c, gy_c).  s_us still holds the last channel's bytes (the same
    // for every channel)
    const double sc = (double)p.scale[n_img] * (double)p.flow_sign / (2.0 * (double)p.chan);
#pragma unroll
    for (int k = 0; k < kRows; ++k) {
        const int row = ly + k * kWaves, y = y0 + row;
        if (!(x < p.w && y < p.h)) continue;
        float* go = p.grad + n_img * 2 * p.hw + (int64_t)y * p.w + x;
        const bool known = s_us[(row + H2) * RW + lx + H2] != 0;
        go[0] = known ? (float)(sc * gx_acc[k]) : 0.0f;            // not known: exactly +0
        go[p.hw] = known ? (float)(sc * gy_acc[k]) : 0.0f;
    }
}

bool window_ok(int32_t window) { return window == 3 || window == 5 || window == 7; }

int64_t tiles_of(int32_t extent, int tile) { return ((int64_t)extent + tile - 1) / tile; }

// the operands and the checks both entry points share
int fill_operands(SsimParams* p, const void* flow, int64_t flow_bs, int32_t flow_half, const uint8_t* mask, int64_t mask_bs,
                  const void* img, int64_t img_bs, const void* other, int64_t other_bs, int32_t channels, int32_t img_u8, float flow_sign,
                  int32_t window, float c1, float c2, int32_t n, int32_t h, int32_t w) {
    if (!window_ok(window)) return OFL_E_ARG;
    if (channels != 1 && channels != 3) return OFL_E_ARG;
    if (!(c1 > 0.0f) || isinf(c1) || !(c2 > 0.0f) || isinf(c2)) return OFL_E_ARG;          // (NaN fails)
    const int rc = fill_pair_operands(p, flow, flow_bs, flow_half, mask, mask_bs, img, img_bs, other, other_bs, channels, img_u8, flow_sign,
                                      n, h, w);
    if (rc) return rc;
    p->tiles_x = (int32_t)tiles_of(w, kTileW);
    p->nblk = (int32_t)(tiles_of(w, kTileW) * tiles_of(h, kTileH));        // (h * w < 2^31: under 2^27)
    p->c1 = c1; p->c2 = c2;
    return OFL_OK;
}

template <int WINDOW, bool BWD>
void launch_window(const SsimParams& p, bool half, bool u8, dim3 grid, hipStream_t s) {
    dispatch_flags(half, u8, [&](auto HALF, auto U8) {
        constexpr bool kHalf = decltype(HALF)::value, kU8 = decltype(U8)::value;
        if constexpr (BWD) OFL_KLAUNCH((flow_ssim_grad_kernel<WINDOW, kHalf, kU8>), grid, dim3(kThreads), 0, s, p);
        else OFL_KLAUNCH((flow_ssim_kernel<WINDOW, kHalf, kU8>), grid, dim3(kThreads), 0, s, p);
    });
}

template <bool BWD>
void launch(const SsimParams& p, int window, bool half, bool u8, dim3 grid, hipStream_t s) {
    if (window == 3) launch_window<3, BWD>(p, half, u8, grid, s);
    else if (window == 5) launch_window<5, BWD>(p, half, u8, grid, s);
    else launch_window<7, BWD>(p, half, u8, grid, s);
}

}  // namespace

extern "C" {

__attribute__((visibility("default"))) int64_t ofl_flow_ssim_workspace_bytes(int32_t n, int32_t h, int32_t w, int32_t window) {
    if (!dims_ok(n, h, w, 2) || !window_ok(window)) return OFL_E_ARG;
    return (int64_t)n * tiles_of(w, kTileW) * tiles_of(h, kTileH) * kRec * (int64_t)sizeof(double);
}

__attribute__((visibility("default"))) int ofl_flow_ssim_f64(const void* flow, int64_t flow_bs, int32_t flow_half, const uint8_t* mask,
                                                             int64_t mask_bs, const void* img, int64_t img_bs, const void* other,
                                                             int64_t other_bs, int32_t channels, int32_t img_u8, float flow_sign,
                                                             int32_t window, float c1, float c2, void* workspace, float* ssim_map,
                                                             double* records, int32_t n, int32_t h, int32_t w, void* stream) {
    SsimParams p;
    const int rc = fill_operands(&p, flow, flow_bs, flow_half, mask, mask_bs, img, img_bs, other, other_bs, channels, img_u8, flow_sign,
                                 window, c1, c2, n, h, w);
    if (rc) return rc;
    if (!ssim_map && !records) return OFL_E_ARG;
    if (records && !workspace) return OFL_E_ARG;
    if (!aligned(workspace, 8) || !aligned(records, 8) || !aligned(ssim_map, 4)) return OFL_E_ARG;
    p.partial = records ? reinterpret_cast<double*>(workspace) : nullptr;
    p.map = ssim_map;
    p.out = records;
    hipStream_t s = (hipStream_t)stream;
    launch<false>(p, window, flow_half != 0, img_u8 != 0, dim3((unsigned)p.nblk, (unsigned)n), s);
    if (records) OFL_KLAUNCH(flow_ssim_finish_kernel, dim3((unsigned)n), dim3(kThreads), 0, s, p);
    return (int)hipGetLastError();
}

__attribute__((visibility("default"))) int ofl_flow_ssim_grad_f32(const void* flow, int64_t flow_bs, int32_t flow_half, const uint8_t* mask,
                                                                  int64_t mask_bs, const void* img, int64_t img_bs, const void* other,
                                                                  int64_t other_bs, int32_t channels, int32_t img_u8, float flow_sign,
                                                                  int32_t window, float c1, float c2, const float* scale, float* grad,
                                                                  int32_t n, int32_t h, int32_t w, void* stream) {
    SsimParams p;
    const int rc = fill_operands(&p, flow, flow_bs, flow_half, mask, mask_bs, img, img_bs, other, other_bs, channels, img_u8, flow_sign,
                                 window, c1, c2, n, h, w);
    if (rc) return rc;
    if (!scale || !grad || !aligned(scale, 4) || !aligned(grad, 4)) return OFL_E_ARG;
    p.scale = scale; p.grad = grad;
    hipStream_t s = (hipStream_t)stream;
    launch<true>(p, window, flow_half != 0, img_u8 != 0, dim3((unsigned)p.nblk, (unsigned)n), s);
    return (int)hipGetLastError();
}

}  // extern "C"
