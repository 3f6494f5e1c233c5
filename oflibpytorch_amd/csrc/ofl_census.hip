// ofl_census.hip -- Flow.census / census_map / census_stats on gfx950: the census data term of an unsupervised flow loss, warp and
// comparison of ternary census signatures in one pass (which DEFINES the numbers; tests/census_oracle.py is the same
// definition in NumPy).  An extension: the reference has no such function.
//
//   flow_census_kernel<PATCH, HALF, U8>        a block owns a tile of 64 x 16 output pixels.  It stages, for the tile and a halo of R =
//                                              PATCH / 2 pixels, the grey Gw of `other` sampled where the flow points, the grey Gi of `img`
//                                              and the usable byte (in the frame, valid in the mask, sample inside `other`) in LDS: every
//                                              staged pixel is warped ONCE.  Each lane then walks the patch of its four pixels out of LDS
//                                              (dy ascending, dx ascending within it), rho = pow(hd + eps, q) in float64 rounded once.
//                                              Writes rho (0 where not known) if a map is wanted and, per block, ONE record of 8 float64
//   flow_census_finish_kernel                  one block per image: the block records added in ascending block order, from LDS
//   flow_census_grad_kernel<PATCH, HALF, U8>   the backward of the per-image mean with respect to the flow vectors.  Stages the tile with
//                                              a halo of 2 R, recomputes kappa(p) = q b^(q-1) / n of the tile plus a halo of R into LDS
//                                              (float64), then every pixel gathers dL/dGw over its patch and multiplies by the derivative
//                                              of its own sample: no scatter, no atomics, no workspace
//
// The warped image is never written, nor any tensor of patch^2 - 1 channels.  The sample (position, taps, weights, the four-term sums and mr) is
// the one of ofl_loss_common.hpp, which restates the backward warp of ofl_kernels.hip; tests/test_gpu_census.py compares the two on the
// device.  A uint8 sample stays on the scale 0 .. 255 here (ld_img_raw).  Taps are single loads straight from global memory at offsets
// clamped into the plane: always addressable.
//
// The tile.  A pixel of the staged region costs a warp (two flow loads, a mask byte, 4 taps x C planes, the position chain with its two
// divisions); the walk costs patch^2 - 1 terms of three divisions and two roots each and dominates.  64 x 16 outputs over 70 x 22 staged
// pixels is 1.50 warps per output at R = 3 (32 x 8 over 38 x 14: 2.08; 64 x 4 over 70 x 10: 2.73).  A row of 64 outputs is one wave: its
// LDS reads of one patch offset are 64 consecutive floats, 32 distinct banks for each 32-lane half, free of conflicts at any row pitch,
// so the pitch is not padded (70 floats at R = 3); the usable bytes of a wave are 16 consecutive words, read as broadcasts.  LDS: 2 floats
// and a byte per staged pixel, 14 128 B forward at R = 3 with the 256 B of the waves' records; the backward stages 76 x 28 pixels and
// 70 x 22 float64 kappa, 31 472 B.
// 256 threads, four pixels per lane (rows ly, ly + 4, ly + 8, ly + 12 of the tile), so that a wave's map store is one run of 256 bytes.
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
constexpr int kRec = OFL_CENSUS_RECORD;            // doubles per record
constexpr float kSoft = 0.81f;                     // the constant under the root of the soft sign
constexpr float kGreyR = 0.299f, kGreyG = 0.587f, kGreyB = 0.114f;
enum { R_COUNT = 0, R_SUM = 1, R_MAX = 2, R_TERMS = 3, R_USED = 4 };

struct CensusParams {
    const void* flow;                              // [*,2,H,W] fp32 or fp16
    int64_t flow_bs;                               // elements between images
    const uint8_t* mask;                           // [*,H,W] bytes or nullptr (all True)
    int64_t mask_bs;
    const void* img; const void* other;            // [*,C,H,W] fp32 or uint8: the frame on the flow's grid, the frame it points into
    int64_t img_bs, other_bs;
    int64_t hw;
    int32_t chan, h, w, tiles_x, nblk;
    float flow_sign, thresh, eps, q;
    float wm1, hm1, half_wm1, half_hm1;
    double* partial;                               // [n][nblk][kRec] or nullptr (no record wanted)
    float* map;                                    // [n][H*W] or nullptr
    double* out;                                   // [n][kRec]
    const float* scale;                            // backward: [n]
    float* grad;                                   // backward: [n][2][H*W]
};

// grey of up to three channel values; float32 images are brought to the scale 0 .. 255
template <bool U8>
__device__ __forceinline__ float grey_of(const float (&v)[3], int chan) {
    const float g = chan == 1 ? v[0] : (kGreyR * v[0] + kGreyG * v[1]) + kGreyB * v[2];
    return U8 ? g : 255.0f * g;
}

// Gw, Gi and the usable byte of the tile at (x0, y0) and HALO pixels around it; a pixel outside the frame is not usable
template <int HALO, bool HALF, bool U8>
__device__ __forceinline__ void stage(const CensusParams& p, int64_t n_img, int x0, int y0, float* s_gw, float* s_gi, uint8_t* s_us) {
    constexpr int RW = kTileW + 2 * HALO, RH = kTileH + 2 * HALO;
    const int64_t fo = n_img * p.flow_bs;
    const uint8_t* mk = p.mask ? p.mask + n_img * p.mask_bs : nullptr;
    const int64_t io = n_img * p.img_bs, oo = n_img * p.other_bs;
    for (int i = threadIdx.x; i < RW * RH; i += kThreads) {
        const int ry = i / RW, rx = i - ry * RW;
        const int x = x0 - HALO + rx, y = y0 - HALO + ry;
        float gw = 0.0f, gi = 0.0f;
        bool us = false;
        if (x >= 0 && x < p.w && y >= 0 && y < p.h) {
            const int64_t pix = (int64_t)y * p.w + x;
            const float u = ld_flow<HALF>(p.flow, fo + pix), v = ld_flow<HALF>(p.flow, fo + p.hw + pix);
            const bool valid = mk == nullptr || mk[pix] != 0;
            const Taps t = taps_of(p, x, y, u, v);
            us = (t.mr > kValidThr) && valid;
            if (us) {
                float vw[3] = {0.0f, 0.0f, 0.0f}, vi[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    if (c < p.chan) {
                        const int64_t pl = oo + (int64_t)c * p.hw;
                        const float v_nw = t.k_nw ? ld_img_raw<U8>(p.other, pl + t.o_nw) : 0.0f;
                        const float v_ne = t.k_ne ? ld_img_raw<U8>(p.other, pl + t.o_ne) : 0.0f;
                        const float v_sw = t.k_sw ? ld_img_raw<U8>(p.other, pl + t.o_sw) : 0.0f;
                        const float v_se = t.k_se ? ld_img_raw<U8>(p.other, pl + t.o_se) : 0.0f;
                        vw[c] = sample_of(t, v_nw, v_ne, v_sw, v_se);
                        vi[c] = ld_img_raw<U8>(p.img, io + (int64_t)c * p.hw + pix);
                    }
                }
                gw = grey_of<U8>(vw, p.chan);
                gi = grey_of<U8>(vi, p.chan);
            }
        }
        s_gw[i] = gw; s_gi[i] = gi; s_us[i] = us ? 1 : 0;
    }
}

// the soft sign of a grey difference
__device__ __forceinline__ float soft_sign(float d) { return d / sqrt_rn(kSoft + d * d); }

// the fp32 sum of the terms of the patch around the staged pixel at index c (pitch RW), in the order of the definition, and their
// number n
template <int R, int RW>
__device__ __forceinline__ float walk(const float* s_gw, const float* s_gi, const uint8_t* s_us, int c, float thresh, int* n_out) {
    const float gw0 = s_gw[c], gi0 = s_gi[c];
    float sum = 0.0f;
    int n = 0;
#pragma unroll 1
    for (int dy = -R; dy <= R; ++dy) {
#pragma unroll
        for (int dx = -R; dx <= R; ++dx) {
            const int o = c + dy * RW + dx;
            if ((dy != 0 || dx != 0) && s_us[o] != 0) {
                const float tw = soft_sign(s_gw[o] - gw0);
                const float ti = soft_sign(s_gi[o] - gi0);
                const float e = ti - tw;
                const float s = e * e;
                sum = sum + s / (thresh + s);
                ++n;
            }
        }
    }
    *n_out = n;
    return sum;
}

template <int PATCH, bool HALF, bool U8>
__global__ void __launch_bounds__(kThreads) flow_census_kernel(CensusParams p) {
    constexpr int R = PATCH / 2, RW = kTileW + 2 * R, RH = kTileH + 2 * R;
    __shared__ float s_gw[RW * RH];
    __shared__ float s_gi[RW * RH];
    __shared__ uint8_t s_us[RW * RH];
    __shared__ double s_red[kWaves * kRec];
    const int64_t n_img = blockIdx.y;
    const int ty = (int)(blockIdx.x / (uint32_t)p.tiles_x), tx = (int)(blockIdx.x - (uint32_t)ty * (uint32_t)p.tiles_x);
    const int x0 = tx * kTileW, y0 = ty * kTileH;
    stage<R, HALF, U8>(p, n_img, x0, y0, s_gw, s_gi, s_us);
    __syncthreads();
    const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
    const int x = x0 + lx;
    const double q = (double)p.q;
    uint32_t count = 0u, terms = 0u;
    double sum = 0.0;
    float mx = 0.0f;
#pragma unroll 1
    for (int k = 0; k < kRows; ++k) {
        const int row = ly + k * kWaves, y = y0 + row;
        if (x < p.w && y < p.h) {
            const int c = (row + R) * RW + lx + R;
            int n = 0;
            float rho = 0.0f;
            if (s_us[c] != 0) {
                const float tot = walk<R, RW>(s_gw, s_gi, s_us, c, p.thresh, &n);
                if (n > 0) {
                    const float b = tot / (float)n + p.eps;
                    rho = (float)pow((double)b, q);
                }
            }
            const bool known = n > 0;
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
__global__ void __launch_bounds__(kThreads) flow_census_finish_kernel(CensusParams p) {
    finish_records<kRec, R_MAX, kChunk, kThreads>(p.partial, p.nblk, p.out);
}

template <int PATCH, bool HALF, bool U8>
__global__ void __launch_bounds__(kThreads) flow_census_grad_kernel(CensusParams p) {
    constexpr int R = PATCH / 2, H2 = 2 * R;
    constexpr int RW = kTileW + 2 * H2, RH = kTileH + 2 * H2;      // staged: the tile and 2 R around it
    constexpr int KW = kTileW + 2 * R, KH = kTileH + 2 * R;        // kappa: the tile and R around it
    __shared__ float s_gw[RW * RH];
    __shared__ float s_gi[RW * RH];
    __shared__ uint8_t s_us[RW * RH];
    __shared__ double s_kap[KW * KH];
    const int64_t n_img = blockIdx.y;
    const int ty = (int)(blockIdx.x / (uint32_t)p.tiles_x), tx = (int)(blockIdx.x - (uint32_t)ty * (uint32_t)p.tiles_x);
    const int x0 = tx * kTileW, y0 = ty * kTileH;
    stage<H2, HALF, U8>(p, n_img, x0, y0, s_gw, s_gi, s_us);
    __syncthreads();
    // kappa(p) = q b^(q - 1) / n on the fp32 b of the forward, 0 where p is not known; the image's scale is applied at the end
    const double q = (double)p.q;
    for (int i = threadIdx.x; i < KW * KH; i += kThreads) {
        const int ky = i / KW, kx = i - ky * KW;
        const int c = (ky + R) * RW + kx + R;
        double kap = 0.0;
        if (s_us[c] != 0) {
            int n = 0;
            const float tot = walk<R, RW>(s_gw, s_gi, s_us, c, p.thresh, &n);
            if (n > 0) {
                const float b = tot / (float)n + p.eps;
                kap = q * pow((double)b, q - 1.0) / (double)n;
            }
        }
        s_kap[i] = kap;
    }
    __syncthreads();
    const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
    const int x = x0 + lx;
    const double th = (double)p.thresh, soft = (double)kSoft;
    const double sc = (double)p.scale[n_img] * (double)(-p.flow_sign) * (U8 ? 1.0 : 255.0);
    const double wr = p.chan == 1 ? 1.0 : (double)kGreyR, wg = (double)kGreyG, wb = (double)kGreyB;
    const int64_t fo = n_img * p.flow_bs, oo = n_img * p.other_bs;
#pragma unroll 1
    for (int k = 0; k < kRows; ++k) {
        const int row = ly + k * kWaves, y = y0 + row;
        if (!(x < p.w && y < p.h)) continue;
        const int64_t pix = (int64_t)y * p.w + x;
        float* go = p.grad + n_img * 2 * p.hw + pix;
        const int c = (row + H2) * RW + lx + H2;
        const int ck = (row + R) * KW + lx + R;
        int n = 0;
        double acc = 0.0;
        if (s_us[c] != 0) {
            // for usable x and usable x + o:  k_{-o}(x + o) = -k_o(x) exactly, so both sums of the definition run over the terms of x
            const double gw0 = (double)s_gw[c], gi0 = (double)s_gi[c], kap0 = s_kap[ck];
#pragma unroll 1
            for (int dy = -R; dy <= R; ++dy) {
#pragma unroll
                for (int dx = -R; dx <= R; ++dx) {
                    const int o = c + dy * RW + dx;
                    if ((dy != 0 || dx != 0) && s_us[o] != 0) {
                        const double dw = (double)s_gw[o] - gw0, di = (double)s_gi[o] - gi0;
                        const double cw = soft + dw * dw, rw = sqrt(cw);
                        const double e = di / sqrt(soft + di * di) - dw / rw;
                        const double ts = th + e * e;
                        const double kk = (th / (ts * ts)) * (-2.0 * e) * (soft / (cw * rw));
                        acc += kk * (s_kap[ck + dy * KW + dx] + kap0);
                        ++n;
                    }
                }
            }
        }
        if (n == 0) {                              // not known: exactly +0
            go[0] = 0.0f; go[p.hw] = 0.0f;
            continue;
        }
        // the derivative of the pixel's own sample
        const float u = ld_flow<HALF>(p.flow, fo + pix), v = ld_flow<HALF>(p.flow, fo + p.hw + pix);
        const Taps t = taps_of(p, x, y, u, v);
        double ax = 0.0, ay = 0.0;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            if (ch < p.chan) {
                const int64_t pl = oo + (int64_t)ch * p.hw;
                const double v_nw = t.k_nw ? (double)ld_img_raw<U8>(p.other, pl + t.o_nw) : 0.0;
                const double v_ne = t.k_ne ? (double)ld_img_raw<U8>(p.other, pl + t.o_ne) : 0.0;
                const double v_sw = t.k_sw ? (double)ld_img_raw<U8>(p.other, pl + t.o_sw) : 0.0;
                const double v_se = t.k_se ? (double)ld_img_raw<U8>(p.other, pl + t.o_se) : 0.0;
                double gx, gy;
                sample_grad(t, v_nw, v_ne, v_sw, v_se, gx, gy);
                const double wc = ch == 0 ? wr : (ch == 1 ? wg : wb);
                ax = ch == 0 ? wc * gx : ax + wc * gx;
                ay = ch == 0 ? wc * gy : ay + wc * gy;
            }
        }
        const double dg = -acc;                    // dL/dGw(x) / scale
        go[0] = (float)(sc * (dg * ax));
        go[p.hw] = (float)(sc * (dg * ay));
    }
}

bool patch_ok(int32_t patch) { return patch == 3 || patch == 5 || patch == 7; }

int64_t tiles_of(int32_t extent, int tile) { return ((int64_t)extent + tile - 1) / tile; }

// the operands and the checks both entry points share
int fill_operands(CensusParams* p, const void* flow, int64_t flow_bs, int32_t flow_half, const uint8_t* mask, int64_t mask_bs,
                  const void* img, int64_t img_bs, const void* other, int64_t other_bs, int32_t channels, int32_t img_u8, float flow_sign,
                  int32_t patch, float thresh, float eps, float q, int32_t n, int32_t h, int32_t w) {
    if (!patch_ok(patch)) return OFL_E_ARG;
    if (channels != 1 && channels != 3) return OFL_E_ARG;
    if (!(thresh > 0.0f) || isinf(thresh) || !(eps > 0.0f) || isinf(eps) || !(q > 0.0f) || !(q <= 1.0f)) return OFL_E_ARG;  // (NaN fails)
    const int rc = fill_pair_operands(p, flow, flow_bs, flow_half, mask, mask_bs, img, img_bs, other, other_bs, channels, img_u8, flow_sign,
                                      n, h, w);
    if (rc) return rc;
    p->tiles_x = (int32_t)tiles_of(w, kTileW);
    p->nblk = (int32_t)(tiles_of(w, kTileW) * tiles_of(h, kTileH));        // (h * w < 2^31: under 2^27)
    p->thresh = thresh; p->eps = eps; p->q = q;
    return OFL_OK;
}

template <int PATCH, bool BWD>
void launch_patch(const CensusParams& p, bool half, bool u8, dim3 grid, hipStream_t s) {
    dispatch_flags(half, u8, [&](auto HALF, auto U8) {
        constexpr bool kHalf = decltype(HALF)::value, kU8 = decltype(U8)::value;
        if constexpr (BWD) OFL_KLAUNCH((flow_census_grad_kernel<PATCH, kHalf, kU8>), grid, dim3(kThreads), 0, s, p);
        else OFL_KLAUNCH((flow_census_kernel<PATCH, kHalf, kU8>), grid, dim3(kThreads), 0, s, p);
    });
}

template <bool BWD>
void launch(const CensusParams& p, int patch, bool half, bool u8, dim3 grid, hipStream_t s) {
    if (patch == 3) launch_patch<3, BWD>(p, half, u8, grid, s);
    else if (patch == 5) launch_patch<5, BWD>(p, half, u8, grid, s);
    else launch_patch<7, BWD>(p, half, u8, grid, s);
}

}  // namespace

extern "C" {

__attribute__((visibility("default"))) int64_t ofl_flow_census_workspace_bytes(int32_t n, int32_t h, int32_t w, int32_t patch) {
    if (!dims_ok(n, h, w, 2) || !patch_ok(patch)) return OFL_E_ARG;
    return (int64_t)n * tiles_of(w, kTileW) * tiles_of(h, kTileH) * kRec * (int64_t)sizeof(double);
}

__attribute__((visibility("default"))) int ofl_flow_census_f64(const void* flow, int64_t flow_bs, int32_t flow_half, const uint8_t* mask,
                                                               int64_t mask_bs, const void* img, int64_t img_bs, const void* other,
                                                               int64_t other_bs, int32_t channels, int32_t img_u8, float flow_sign,
                                                               int32_t patch, float thresh, float eps, float q, void* workspace,
                                                               float* census_map, double* records, int32_t n, int32_t h, int32_t w,
                                                               void* stream) {
    CensusParams p;
    const int rc = fill_operands(&p, flow, flow_bs, flow_half, mask, mask_bs, img, img_bs, other, other_bs, channels, img_u8, flow_sign,
                                 patch, thresh, eps, q, n, h, w);
    if (rc) return rc;
    if (!census_map && !records) return OFL_E_ARG;
    if (records && !workspace) return OFL_E_ARG;
    if (!aligned(workspace, 8) || !aligned(records, 8) || !aligned(census_map, 4)) return OFL_E_ARG;
    p.partial = records ? reinterpret_cast<double*>(workspace) : nullptr;
    p.map = census_map;
    p.out = records;
    hipStream_t s = (hipStream_t)stream;
    launch<false>(p, patch, flow_half != 0, img_u8 != 0, dim3((unsigned)p.nblk, (unsigned)n), s);
    if (records) OFL_KLAUNCH(flow_census_finish_kernel, dim3((unsigned)n), dim3(kThreads), 0, s, p);
    return (int)hipGetLastError();
}

__attribute__((visibility("default"))) int ofl_flow_census_grad_f32(const void* flow, int64_t flow_bs, int32_t flow_half, const uint8_t* mask,
                                                                    int64_t mask_bs, const void* img, int64_t img_bs, const void* other,
                                                                    int64_t other_bs, int32_t channels, int32_t img_u8, float flow_sign,
                                                                    int32_t patch, float thresh, float eps, float q, const float* scale,
                                                                    float* grad, int32_t n, int32_t h, int32_t w, void* stream) {
    CensusParams p;
    const int rc = fill_operands(&p, flow, flow_bs, flow_half, mask, mask_bs, img, img_bs, other, other_bs, channels, img_u8, flow_sign,
                                 patch, thresh, eps, q, n, h, w);
    if (rc) return rc;
    if (!scale || !grad || !aligned(scale, 4) || !aligned(grad, 4)) return OFL_E_ARG;
    p.scale = scale; p.grad = grad;
    hipStream_t s = (hipStream_t)stream;
    launch<true>(p, patch, flow_half != 0, img_u8 != 0, dim3((unsigned)p.nblk, (unsigned)n), s);
    return (int)hipGetLastError();
}

}  // extern "C"
