// ofl_smoothness.hip -- Flow.smoothness / smoothness_map / smoothness_stats on gfx950: the edge-aware first- or second-order smoothness
// penalty of a flow, weighted down where a guidance image has an edge (which DEFINES the numbers;
// tests/smoothness_oracle.py is the same definition in NumPy).  An extension: the reference has no such function.
//
//   flow_smoothness_kernel<ORDER, IMG, false>   one pass over the flow, its mask and the image: per pixel the x and the y term in fp32
//                                               (their sum optionally stored as a map) and, per block, ONE record of 8 float64 values
//   flow_smoothness_finish_kernel               one block per image: the block records added in ascending block order, from LDS
//   flow_smoothness_kernel<ORDER, IMG, true>    the backward of the per-image mean: every output pixel GATHERS the 4 (order 1) or 6
//                                               (order 2) terms that read it, recomputed from the inputs; no scatter, no atomics
//
// Both are stencils.  A block of 256 lanes takes tiles of kTH x kTW = 8 x 128 pixels: the planes of the tile (u, v, a validity byte, the
// image planes as fp32) are staged in LDS with a halo of 0 / 1 (forward, order 1: right and lower neighbour), 1 (forward order 2, backward
// order 1) or 2 pixels (backward order 2), and every tap is an LDS read.  A lane stages and computes the 4 consecutive pixels
// 4 q .. 4 q + 3 of a row: 16-byte loads and stores (8 bytes of an fp16-stored flow, 4 of the mask or a uint8 image) where the width,
// the batch strides and the pointers allow (chosen per launch, a uniform branch), else one element at a time with bounds checks -- the
// same pixels in the same lanes, so the choice never changes a bit.  The validity byte is 0 outside the frame: a term whose taps are all
// valid exists.  Blocks walk the tiles of an image with a grid stride; their number depends on (h, w) only.  The sums are those of
// ofl_loss_common.hpp.  C ABI: include/oflib_hip.h.
#include "ofl_loss_common.hpp"

namespace {

using namespace ofl_loss;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTH = 8, kTW = 128;                  // the tile: one quad of a row per lane
constexpr int kQuadsPerRow = kTW / 4;
constexpr int kPad = 4;                            // LDS columns before the tile's first: the interior stays 16-byte aligned
constexpr int kLW = kPad + kTW + 4;                // LDS row length
constexpr int kMaxBlocks = 256;                    // forward: blocks per image at most (one per CU)
constexpr int kMaxGradBlocks = 1024;               // backward: nothing to reduce (1080p: 2025 tiles, every block takes 1 or 2)
constexpr int kRec = OFL_SMOOTHNESS_RECORD;        // doubles per record
constexpr int kMaxChan = 4;
enum { R_COUNT_X = 0, R_COUNT_Y = 1, R_SUM_X = 2, R_SUM_Y = 3, R_MAX = 4 };
enum { IMG_NONE = 0, IMG_F32 = 1, IMG_U8 = 2 };

struct SmoothParams {
    const void* flow;                              // [*,2,H,W] fp32 or fp16
    int64_t flow_bs;                               // elements between images
    int32_t flow_half;
    const uint8_t* mask;                           // [*,H,W] bytes or nullptr (all True)
    int64_t mask_bs;
    const void* img;                               // [*,C,H,W] fp32 or uint8, or nullptr
    int64_t img_bs;
    int32_t chan;
    int32_t vec;                                   // 16-byte form
    int32_t h, w;
    int32_t tiles_x, tiles;
    int32_t nblk;
    float alpha, eps;
    double* partial;                               // [n][nblk][kRec]
    float* map;                                    // [n][H][W] or nullptr
    double* out;                                   // [n][kRec]
    const float* scale;                            // backward: [n]
    float* grad;                                   // backward: [n][2][H][W]
};

// halo of the tile: pixels above / left (HT) and below / right (HB) that the taps of the tile's terms reach
template <int ORDER, bool BWD> struct Halo {
    static constexpr int HT = BWD ? ORDER : ORDER - 1;
    static constexpr int HB = BWD ? ORDER : 1;
    static constexpr int ROWS = kTH + HT + HB;
};

template <int IMG, int ROWS>
struct Tile {
    float u[ROWS * kLW];
    float v[ROWS * kLW];
    float img[IMG == IMG_NONE ? 1 : kMaxChan][IMG == IMG_NONE ? 4 : ROWS * kLW];
    uint8_t valid[ROWS * kLW];
};

enum { K_FLOAT = 0, K_HALF = 1, K_U8 = 2 };

// one element of a plane as the tile holds it
template <int KIND>
__device__ __forceinline__ float ld1(const void* base, int64_t o) {
    if (KIND == K_FLOAT) return reinterpret_cast<const float*>(base)[o];
    if (KIND == K_HALF) return __half2float(reinterpret_cast<const __half*>(base)[o]);
    return (float)reinterpret_cast<const uint8_t*>(base)[o] / 255.0f;
}

// four consecutive, existing, aligned elements
template <int KIND>
__device__ __forceinline__ void ld4(const void* base, int64_t o, float x[4]) {
    if (KIND == K_FLOAT) {
        const float4 f = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(base) + o);
        x[0] = f.x; x[1] = f.y; x[2] = f.z; x[3] = f.w;
    } else if (KIND == K_HALF) {
        const uint2 q = *reinterpret_cast<const uint2*>(reinterpret_cast<const __half*>(base) + o);
        const __half2 a = *reinterpret_cast<const __half2*>(&q.x), b = *reinterpret_cast<const __half2*>(&q.y);
        x[0] = __low2float(a); x[1] = __high2float(a); x[2] = __low2float(b); x[3] = __high2float(b);
    } else {
        const uint32_t m = *reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint8_t*>(base) + o);
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = (float)((m >> (8 * k)) & 0xffu) / 255.0f;
    }
}

// One plane of the tile at (ty0, tx0) with its halo into LDS: the quads of the tile's columns (all rows, halo rows included) by 16-byte
// loads where `vec`, then the halo columns one element each.  Outside the frame: 0.  `base` + o: the plane's first element.
template <int KIND, int HT, int HB>
__device__ __forceinline__ void stage_plane(float* dst, const void* base, int64_t o, int ty0, int tx0, int h, int w, bool vec) {
    constexpr int ROWS = kTH + HT + HB;
    for (int i = threadIdx.x; i < ROWS * kQuadsPerRow; i += kThreads) {
        const int r = i / kQuadsPerRow, q = i % kQuadsPerRow;
        const int gy = ty0 - HT + r, gx = tx0 + 4 * q;
        float x[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (gy >= 0 && gy < h && gx < w) {
            const int64_t e = o + (int64_t)gy * w + gx;
            if (vec) {
                ld4<KIND>(base, e, x);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (gx + k < w) x[k] = ld1<KIND>(base, e + k);
            }
        }
        *reinterpret_cast<float4*>(dst + r * kLW + kPad + 4 * q) = make_float4(x[0], x[1], x[2], x[3]);
    }
    for (int i = threadIdx.x; i < ROWS * (HT + HB); i += kThreads) {
        const int r = i / (HT + HB), c = i % (HT + HB);
        const int col = c < HT ? c - HT : kTW + (c - HT);
        const int gy = ty0 - HT + r, gx = tx0 + col;
        float x = 0.0f;
        if (gy >= 0 && gy < h && gx >= 0 && gx < w) x = ld1<KIND>(base, o + (int64_t)gy * w + gx);
        dst[r * kLW + kPad + col] = x;
    }
}

// The validity byte of the tile and its halo: 1 where the pixel lies in the frame and the mask (nullptr: all True) is not 0.
template <int HT, int HB>
__device__ __forceinline__ void stage_valid(uint8_t* dst, const uint8_t* mask, int64_t o, int ty0, int tx0, int h, int w, bool vec) {
    constexpr int ROWS = kTH + HT + HB;
    for (int i = threadIdx.x; i < ROWS * kQuadsPerRow; i += kThreads) {
        const int r = i / kQuadsPerRow, q = i % kQuadsPerRow;
        const int gy = ty0 - HT + r, gx = tx0 + 4 * q;
        uint32_t bytes = 0u;
        if (gy >= 0 && gy < h && gx < w) {
            const int64_t e = o + (int64_t)gy * w + gx;
            if (mask == nullptr) {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (gx + k < w) bytes |= 1u << (8 * k);
            } else if (vec) {
                const uint32_t m = *reinterpret_cast<const uint32_t*>(mask + e);
#pragma unroll
                for (int k = 0; k < 4; ++k) bytes |= ((m >> (8 * k)) & 0xffu) ? (1u << (8 * k)) : 0u;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (gx + k < w && mask[e + k] != 0) bytes |= 1u << (8 * k);
            }
        }
        *reinterpret_cast<uint32_t*>(dst + r * kLW + kPad + 4 * q) = bytes;
    }
    for (int i = threadIdx.x; i < ROWS * (HT + HB); i += kThreads) {
        const int r = i / (HT + HB), c = i % (HT + HB);
        const int col = c < HT ? c - HT : kTW + (c - HT);
        const int gy = ty0 - HT + r, gx = tx0 + col;
        uint8_t b = 0;
        if (gy >= 0 && gy < h && gx >= 0 && gx < w) b = (mask == nullptr || mask[o + (int64_t)gy * w + gx] != 0) ? 1 : 0;
        dst[r * kLW + kPad + col] = b;
    }
}

template <int ORDER, int IMG, bool BWD>
__device__ __forceinline__ void stage_tile(Tile<IMG, Halo<ORDER, BWD>::ROWS>& t, const SmoothParams& p, int64_t img, int ty0, int tx0) {
    constexpr int HT = Halo<ORDER, BWD>::HT, HB = Halo<ORDER, BWD>::HB;
    const int64_t hw = (int64_t)p.h * p.w;
    const bool vec = p.vec != 0;
    if (p.flow_half) {
        stage_plane<K_HALF, HT, HB>(t.u, p.flow, img * p.flow_bs, ty0, tx0, p.h, p.w, vec);
        stage_plane<K_HALF, HT, HB>(t.v, p.flow, img * p.flow_bs + hw, ty0, tx0, p.h, p.w, vec);
    } else {
        stage_plane<K_FLOAT, HT, HB>(t.u, p.flow, img * p.flow_bs, ty0, tx0, p.h, p.w, vec);
        stage_plane<K_FLOAT, HT, HB>(t.v, p.flow, img * p.flow_bs + hw, ty0, tx0, p.h, p.w, vec);
    }
    stage_valid<HT, HB>(t.valid, p.mask, img * p.mask_bs, ty0, tx0, p.h, p.w, vec);
    if (IMG != IMG_NONE) {
        for (int c = 0; c < p.chan; ++c)
            stage_plane<IMG == IMG_U8 ? K_U8 : K_FLOAT, HT, HB>(t.img[c], p.img, img * p.img_bs + c * hw, ty0, tx0, p.h, p.w, vec);
    }
}

// The term attributed to LDS position `at` along `step` (1: x, kLW: y): its validity, the fp32 differences and the weight.
template <int ORDER, int IMG, int ROWS>
__device__ __forceinline__ bool term(const Tile<IMG, ROWS>& t, const SmoothParams& p, int at, int step, float& du, float& dv, float& wgt) {
    const int lo = ORDER == 1 ? at : at - step, hi = at + step;
    bool valid = t.valid[at] != 0 && t.valid[hi] != 0;
    if (ORDER == 2) valid = valid && t.valid[lo] != 0;
    if (ORDER == 1) {
        du = t.u[hi] - t.u[at];
        dv = t.v[hi] - t.v[at];
    } else {
        du = (t.u[lo] - (t.u[at] + t.u[at])) + t.u[hi];
        dv = (t.v[lo] - (t.v[at] + t.v[at])) + t.v[hi];
    }
    wgt = 1.0f;
    if (IMG != IMG_NONE) {
        float s = 0.0f;
        for (int c = 0; c < p.chan; ++c) s = s + fabsf(t.img[c][hi] - t.img[c][lo]);
        float g = s / (float)p.chan;
        if (ORDER == 2) g = g * 0.5f;
        wgt = valid ? (float)exp((double)(-(p.alpha * g))) : 1.0f;      // (an invalid term is +0 whatever its weight)
    }
    return valid;
}

// the forward value of a term: w (sqrt(du du + eps eps) + sqrt(dv dv + eps eps)), +0 where not valid
template <int IMG>
__device__ __forceinline__ float term_value(bool valid, float du, float dv, float wgt, float ee) {
    const float r = sqrt_rn(du * du + ee) + sqrt_rn(dv * dv + ee);
    const float tv = IMG == IMG_NONE ? r : wgt * r;
    return valid ? tv : 0.0f;
}

// d term / d its difference, per component, in float64: (w d) / sqrt(d d + eps eps), 0 where the root is 0 or the term is not valid
__device__ __forceinline__ double term_q(bool valid, float d, float wgt, double ee) {
    const double dd = (double)d;
    const double den = sqrt(dd * dd + ee);
    return (valid && den != 0.0) ? ((double)wgt * dd) / den : 0.0;
}

template <int ORDER, int IMG, bool BWD>
__global__ void __launch_bounds__(kThreads) flow_smoothness_kernel(SmoothParams p) {
    constexpr int HT = Halo<ORDER, BWD>::HT;
    __shared__ __attribute__((aligned(16))) Tile<IMG, Halo<ORDER, BWD>::ROWS> t;
    __shared__ double s_red[kWaves * kRec];
    const int64_t img = blockIdx.y;
    const int64_t hw = (int64_t)p.h * p.w;
    const int row = threadIdx.x / kQuadsPerRow, quad = threadIdx.x % kQuadsPerRow;
    const float ee = p.eps * p.eps;
    const double ee64 = (double)p.eps * (double)p.eps;
    const double sc = BWD ? (double)p.scale[img] : 0.0;
    uint32_t cnt_x = 0u, cnt_y = 0u;
    double sum_x = 0.0, sum_y = 0.0;
    float mx = 0.0f;
    for (int tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
        const int ty0 = (tile / p.tiles_x) * kTH, tx0 = (tile % p.tiles_x) * kTW;
        stage_tile<ORDER, IMG, BWD>(t, p, img, ty0, tx0);
        __syncthreads();
        const int gy = ty0 + row, gx = tx0 + 4 * quad;
        const int at0 = (row + HT) * kLW + kPad + 4 * quad;
        if (gy < p.h && gx < p.w) {
            if (!BWD) {
                float m[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    float du, dv, wg;
                    const bool vx = term<ORDER, IMG, Halo<ORDER, BWD>::ROWS>(t, p, at0 + k, 1, du, dv, wg);
                    const float tx = term_value<IMG>(vx, du, dv, wg, ee);
                    const bool vy = term<ORDER, IMG, Halo<ORDER, BWD>::ROWS>(t, p, at0 + k, kLW, du, dv, wg);
                    const float ty = term_value<IMG>(vy, du, dv, wg, ee);
                    cnt_x += vx ? 1u : 0u;
                    cnt_y += vy ? 1u : 0u;
                    sum_x += (double)tx;
                    sum_y += (double)ty;
                    mx = (vx && tx > mx) ? tx : mx;
                    mx = (vy && ty > mx) ? ty : mx;
                    m[k] = tx + ty;
                }
                if (p.map != nullptr) {
                    float* mo = p.map + img * hw + (int64_t)gy * p.w + gx;
                    if (p.vec) {
                        *reinterpret_cast<float4*>(mo) = make_float4(m[0], m[1], m[2], m[3]);
                    } else {
#pragma unroll
                        for (int k = 0; k < 4; ++k)
                            if (gx + k < p.w) mo[k] = m[k];
                    }
                }
            } else {
                float gu[4], gv[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    // x before y, lower term index first: order 1 the terms at s - 1 (+1) and s (-1); order 2 at s - 1 (+1), s (-2), s + 1 (+1)
                    double au = 0.0, av = 0.0;
                    bool any = false;
#pragma unroll
                    for (int dir = 0; dir < 2; ++dir) {
                        const int step = dir == 0 ? 1 : kLW;
#pragma unroll
                        for (int j = -1; j <= ORDER - 1; ++j) {
                            const double coef = ORDER == 1 ? (j < 0 ? 1.0 : -1.0) : (j == 0 ? -2.0 : 1.0);
                            float du, dv, wg;
                            const bool vt = term<ORDER, IMG, Halo<ORDER, BWD>::ROWS>(t, p, at0 + k + j * step, step, du, dv, wg);
                            any = any || vt;
                            au += coef * term_q(vt, du, wg, ee64);
                            av += coef * term_q(vt, dv, wg, ee64);
                        }
                    }
                    gu[k] = any ? (float)(sc * au) : 0.0f;
                    gv[k] = any ? (float)(sc * av) : 0.0f;
                }
                float* go = p.grad + img * 2 * hw + (int64_t)gy * p.w + gx;
                if (p.vec) {
                    *reinterpret_cast<float4*>(go) = make_float4(gu[0], gu[1], gu[2], gu[3]);
                    *reinterpret_cast<float4*>(go + hw) = make_float4(gv[0], gv[1], gv[2], gv[3]);
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (gx + k < p.w) { go[k] = gu[k]; go[hw + k] = gv[k]; }
                }
            }
        }
        __syncthreads();
    }
    if (BWD) return;
    double rec[kRec];
#pragma unroll
    for (int i = 0; i < kRec; ++i) rec[i] = 0.0;
    rec[R_COUNT_X] = (double)cnt_x; rec[R_COUNT_Y] = (double)cnt_y; rec[R_SUM_X] = sum_x; rec[R_SUM_Y] = sum_y; rec[R_MAX] = (double)mx;
    reduce_record<kRec, R_MAX + 1, R_MAX, kWaves>(rec, s_red, p.partial, img, p.nblk);
}

// one block per image: the block records added in ascending block order (all of them fit one chunk)
__global__ void __launch_bounds__(kThreads) flow_smoothness_finish_kernel(SmoothParams p) {
    finish_records<kRec, R_MAX, kMaxBlocks, kThreads>(p.partial, p.nblk, p.out);
}

int64_t tiles_of(int32_t h, int32_t w) { return (int64_t)((h + kTH - 1) / kTH) * ((w + kTW - 1) / kTW); }

int64_t blocks_of(int32_t h, int32_t w, int cap) {
    const int64_t t = tiles_of(h, w);
    return t < cap ? t : cap;
}

// the operands and the checks both entry points share
int fill_operands(SmoothParams* p, const void* flow, int64_t flow_bs, int32_t flow_half, const uint8_t* mask, int64_t mask_bs,
                  const void* img, int64_t img_bs, int32_t img_channels, int32_t img_u8, int32_t order, float alpha, float eps,
                  int32_t n, int32_t h, int32_t w) {
    if (!dims_ok(n, h, w, 1)) return OFL_E_ARG;
    if (order != 1 && order != 2) return OFL_E_ARG;
    if (!(alpha >= 0.0f) || isinf(alpha) || !(eps >= 0.0f) || isinf(eps)) return OFL_E_ARG;      // (NaN fails the first test)
    if (flow == nullptr || (flow_half != 0 && flow_half != 1) || flow_bs < 0 || mask_bs < 0) return OFL_E_ARG;
    if (!aligned(flow, flow_half ? 2 : 4)) return OFL_E_ARG;
    if (img != nullptr) {
        if (img_channels < 1 || img_channels > kMaxChan || (img_u8 != 0 && img_u8 != 1) || img_bs < 0) return OFL_E_ARG;
        if (!aligned(img, img_u8 ? 1 : 4)) return OFL_E_ARG;
    }
    p->flow = flow; p->flow_bs = flow_bs; p->flow_half = flow_half;
    p->mask = mask; p->mask_bs = mask_bs;
    p->img = img; p->img_bs = img ? img_bs : 0; p->chan = img ? img_channels : 0;
    p->h = h; p->w = w;
    p->tiles_x = (w + kTW - 1) / kTW;
    p->tiles = (int32_t)tiles_of(h, w);
    p->nblk = 0;
    p->alpha = alpha; p->eps = eps;
    p->partial = nullptr; p->map = nullptr; p->out = nullptr; p->scale = nullptr; p->grad = nullptr;
    // 16-byte (fp16: 8-byte) accesses of the vector planes, 4-byte accesses of the mask and a uint8 image are aligned for every quad
    bool vec = w % 4 == 0 && flow_bs % 4 == 0 && mask_bs % 4 == 0 && aligned(flow, flow_half ? 8 : 16) && aligned(mask, 4);
    if (img != nullptr) vec = vec && img_bs % 4 == 0 && aligned(img, img_u8 ? 4 : 16);
    p->vec = vec ? 1 : 0;
    return OFL_OK;
}

template <bool BWD>
void launch(const SmoothParams& p, int order, int kind, dim3 grid, hipStream_t s) {
#define OFL_SMOOTH_CASE(O, I) \
    if (order == O && kind == I) { OFL_KLAUNCH((flow_smoothness_kernel<O, I, BWD>), grid, dim3(kThreads), 0, s, p); return; }
    OFL_SMOOTH_CASE(1, IMG_NONE) OFL_SMOOTH_CASE(1, IMG_F32) OFL_SMOOTH_CASE(1, IMG_U8)
    OFL_SMOOTH_CASE(2, IMG_NONE) OFL_SMOOTH_CASE(2, IMG_F32) OFL_SMOOTH_CASE(2, IMG_U8)
#undef OFL_SMOOTH_CASE
}

}  // namespace

extern "C" {

__attribute__((visibility("default"))) int64_t ofl_flow_smoothness_workspace_bytes(int32_t n, int32_t h, int32_t w) {
    if (!dims_ok(n, h, w, 1)) return OFL_E_ARG;
    return (int64_t)n * blocks_of(h, w, kMaxBlocks) * kRec * (int64_t)sizeof(double);
}

__attribute__((visibility("default"))) int ofl_flow_smoothness_f64(const void* flow, int64_t flow_bs, int32_t flow_half, const uint8_t* mask,
                                                                   int64_t mask_bs, const void* img, int64_t img_bs, int32_t img_channels,
                                                                   int32_t img_u8, int32_t order, float alpha, float eps, void* workspace,
                                                                   float* smoothness_map, double* records, int32_t n, int32_t h, int32_t w,
                                                                   void* stream) {
    SmoothParams p;
    const int rc = fill_operands(&p, flow, flow_bs, flow_half, mask, mask_bs, img, img_bs, img_channels, img_u8, order, alpha, eps, n, h, w);
    if (rc) return rc;
    if (!workspace || !records || !aligned(workspace, 8) || !aligned(records, 8) || !aligned(smoothness_map, 4)) return OFL_E_ARG;
    if (!aligned(smoothness_map, 16)) p.vec = 0;
    p.nblk = (int32_t)blocks_of(h, w, kMaxBlocks);
    p.partial = reinterpret_cast<double*>(workspace);
    p.map = smoothness_map;
    p.out = records;
    hipStream_t s = (hipStream_t)stream;
    launch<false>(p, order, img == nullptr ? IMG_NONE : (img_u8 ? IMG_U8 : IMG_F32), dim3((unsigned)p.nblk, (unsigned)n), s);
    OFL_KLAUNCH(flow_smoothness_finish_kernel, dim3((unsigned)n), dim3(kThreads), 0, s, p);
    return (int)hipGetLastError();
}

__attribute__((visibility("default"))) int ofl_flow_smoothness_grad_f32(const void* flow, int64_t flow_bs, int32_t flow_half,
                                                                        const uint8_t* mask, int64_t mask_bs, const void* img,
                                                                        int64_t img_bs, int32_t img_channels, int32_t img_u8, int32_t order,
                                                                        float alpha, float eps, const float* scale, float* grad, int32_t n,
                                                                        int32_t h, int32_t w, void* stream) {
    SmoothParams p;
    const int rc = fill_operands(&p, flow, flow_bs, flow_half, mask, mask_bs, img, img_bs, img_channels, img_u8, order, alpha, eps, n, h, w);
    if (rc) return rc;
    if (!scale || !grad || !aligned(scale, 4) || !aligned(grad, 4)) return OFL_E_ARG;
    if (!aligned(grad, 16)) p.vec = 0;
    p.scale = scale; p.grad = grad;
    hipStream_t s = (hipStream_t)stream;
    launch<true>(p, order, img == nullptr ? IMG_NONE : (img_u8 ? IMG_U8 : IMG_F32),
                 dim3((unsigned)blocks_of(h, w, kMaxGradBlocks), (unsigned)n), s);
    return (int)hipGetLastError();
}

}  // extern "C"
