// ofl_arrows.hip -- Flow.visualise_arrows (flow_class.py:1358-1496) on gfx950: the flow as arrows on a grid of points, drawn by a
// small tile rasteriser.  The reference's own NumPy steps are kept bit for bit (threshold, cartToPolar in OpenCV's FMA form, the
// 99th percentile of the grid magnitudes, the fp32 scaling, np.round of the end points, the hue, the painter's order, the red
// grid pixels, the mask halving and borders); the anti-aliased line itself is DEFINED in DESIGN.md 3.11 (not OpenCV's LINE_AA):
// an arrow is three capsules, its coverage alpha = clamp(t / 2 + 0.5 - d, 0, 1) with d the distance to the nearest of the three
// segments, all of it in float64 with + - * / sqrt only and no contraction, so that tests/arrows_oracle.py follows every bit.
//
//   ofl_arrows_scale_f32   sample the grid points, one block selects the 99th percentile of the N*P magnitudes (exact order
//                          statistics by a radix select on the fp32 bit patterns), scaling = grid_dist / percentile in fp32
//   ofl_arrows_plan        one record per (image, grid point): end points, barbs, colour, thickness, bounding boxes; the number
//                          of arrows whose box touches each 64 x 16 output tile; the exclusive scan of those counts
//   ofl_arrows_u8          fill the tile lists (sized from the counts), then one block per tile GATHERS: background in
//                          registers, the tile's arrows in painter's order (a short list ordered by counting, a long one through
//                          LDS bitmap windows: any length), red grid pixels at their place in the order, mask halving, borders
// C ABI: include/oflib_hip.h.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <float.h>
#include <stdint.h>

#include "oflib_hip.h"

#pragma clang fp contract(off)

// the launch recorder of ofl_kernels.hip (ofl_last_kernel_name)
extern const void* g_ofl_last_kernel;
#define OFL_KLAUNCH(K, ...) do { g_ofl_last_kernel = (const void*)(K); hipLaunchKernelGGL(K, __VA_ARGS__); } while (0)

namespace {

constexpr float kZeroThr = 1e-3f;      // utils.py:23, :642
constexpr int kThreads = 256;
constexpr int kTileW = 64, kTileH = 16;           // the house tile: 256 threads x 4 pixels of a row
constexpr int kSelThreads = 1024;
constexpr int kBins0 = 2048, kBins12 = 1024;      // radix select: bits 30..20, 19..10, 9..0
constexpr int kHeader = 16;                        // workspace header: [0] [1] the list entries of all tiles (int64)
constexpr int kRec = 20;                           // int32 words of one arrow record
constexpr int kWin = 32 * kThreads;                // grid-point indices one bitmap window covers (one word per thread)
constexpr int kStage = 64;                         // records staged in LDS per round
constexpr float kFar = 1048576.0f;                 // 2^20: longer arrows are skipped (every integer below stays exact)
enum { R_P1X = 0, R_P1Y, R_P2X, R_P2Y, R_BPX, R_BPY, R_BMX, R_BMY, R_BX0, R_BY0, R_BX1, R_BY1, R_TX0, R_TY0, R_TX1, R_TY1,
       R_COL, R_THICK, R_LISTED, R_PAD };

// ---- cv2.cartToPolar(x, y, angleInDegrees=True) in OpenCV's SIMD (FMA) form, as ofl_visualise.hip and tests/vis_oracle.py
constexpr float kRad2Deg = (float)(180.0 / 3.141592653589793);
constexpr float kP1 = 0.9997878412794807f * kRad2Deg;
constexpr float kP3 = -0.3258083974640975f * kRad2Deg;
constexpr float kP5 = 0.1555786518463281f * kRad2Deg;
constexpr float kP7 = -0.04432655554792128f * kRad2Deg;

__device__ __forceinline__ float thr(float u) { return (u < kZeroThr && u > -kZeroThr) ? 0.0f : u; }

__device__ __forceinline__ float cart_mag(float x, float y) { return sqrtf(fmaf(x, x, y * y)); }

__device__ __forceinline__ float cart_angle(float x, float y) {
    const float ax = fabsf(x), ay = fabsf(y);
    const float c = fminf(ax, ay) / (fmaxf(ax, ay) + (float)DBL_EPSILON);
    const float cc = c * c;
    float a = fmaf(fmaf(fmaf(cc, kP7, kP5), cc, kP3), cc, kP1) * c;
    if (!(ax >= ay)) a = 90.0f - a;
    if (x < 0.0f) a = 180.0f - a;
    if (y < 0.0f) a = 360.0f - a;
    return a;
}

// grid rows / columns: arange(g // 2, size - 1, g)
__host__ __device__ __forceinline__ int grid_count(int size, int g) {
    const int span = size - 1 - g / 2;
    return span <= 0 ? 0 : (span + g - 1) / g;
}

struct Geometry {
    int32_t n, h, w, g;
    int32_t rows, cols;        // grid points per column / row
    int32_t tx, ty;            // tiles per row / column
    int64_t hw;
};

struct Workspace {
    int32_t* header;
    unsigned long long* img_total;   // [n] list entries of each image
    unsigned long long* img_base;    // [n] exclusive scan of them
    float* mags;               // [n * P]
    int32_t* recs;             // [n * P * kRec]
    uint32_t* counts;          // [n * T]
    uint32_t* offsets;         // [n * T]
    uint32_t* cursor;          // [n * T]
};

__host__ __device__ inline Workspace carve(int32_t* ws, const Geometry& g) {
    const int64_t m = (int64_t)g.n * g.rows * g.cols, nt = (int64_t)g.n * g.tx * g.ty;
    Workspace r;
    r.header = ws;
    r.img_total = reinterpret_cast<unsigned long long*>(ws + kHeader);
    r.img_base = r.img_total + g.n;
    int32_t* rest = ws + kHeader + 4 * (int64_t)g.n;
    r.mags = reinterpret_cast<float*>(rest);
    r.recs = rest + m;
    r.counts = reinterpret_cast<uint32_t*>(rest + m + m * kRec);
    r.offsets = r.counts + nt;
    r.cursor = r.offsets + nt;
    return r;
}

struct FlowIn {
    const void* flow;
    int64_t bs;
    int half;
};

__device__ __forceinline__ float flow_at(const FlowIn& f, int64_t hw, int img, int plane, int64_t q) {
    const int64_t o = (int64_t)img * f.bs + plane * hw + q;
    if (f.half) return __half2float(reinterpret_cast<const __half*>(f.flow)[o]);
    return reinterpret_cast<const float*>(f.flow)[o];
}

// ---- the magnitudes of the thresholded flow at the grid points ----------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) arrows_sample_kernel(FlowIn f, Geometry g, float* mags) {
    const int64_t p = (int64_t)g.rows * g.cols;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= p * g.n) return;
    const int img = (int)(i / p);
    const int j = (int)(i - (int64_t)img * p);
    const int y = g.g / 2 + (j / g.cols) * g.g, x = g.g / 2 + (j % g.cols) * g.g;
    const int64_t q = (int64_t)y * g.w + x;
    mags[i] = cart_mag(thr(flow_at(f, g.hw, img, 0, q)), thr(flow_at(f, g.hw, img, 1, q)));
}

// ---- np.percentile(mags, 99) (numpy 2.2.6, 'linear', fp32) by one block, then scaling = fp32(grid_dist) / percentile ------------
// bin of hist[0 .. nb) that holds 0-based rank `rank`, and the rank left inside it (block-wide: nb / 1024 bins per thread)
__device__ void find_bin(const uint32_t* hist, int nb, uint32_t rank, uint32_t* s_part, uint32_t* out_bin, uint32_t* out_left) {
    const int per = nb / kSelThreads;
    uint32_t sum = 0u;
    for (int i = 0; i < per; ++i) sum += hist[threadIdx.x * per + i];
    s_part[threadIdx.x] = sum;
    __syncthreads();
    for (int off = 1; off < kSelThreads; off <<= 1) {          // inclusive Hillis-Steele scan
        const uint32_t v = threadIdx.x >= (unsigned)off ? s_part[threadIdx.x - off] : 0u;
        __syncthreads();
        s_part[threadIdx.x] += v;
        __syncthreads();
    }
    const uint32_t incl = s_part[threadIdx.x], excl = incl - sum;
    if (rank >= excl && rank < incl) {                          // exactly one thread (rank < the number of values)
        uint32_t c = excl;
        for (int i = 0; i < per; ++i) {
            const uint32_t h = hist[threadIdx.x * per + i];
            if (rank < c + h) { *out_bin = (uint32_t)(threadIdx.x * per + i); *out_left = rank - c; break; }
            c += h;
        }
    }
    __syncthreads();
}

__global__ void __launch_bounds__(kSelThreads) arrows_select_kernel(const float* mags, uint32_t m, float grid_dist, float* scaling) {
    __shared__ uint32_t hist[kBins0];
    __shared__ uint32_t s_part[kSelThreads];
    __shared__ uint32_t s_bin, s_left, s_min;
    // the virtual index (m - 1) * q in fp32; previous = floor, next = previous + 1, both the last index at or past m - 1
    const float qf = 99.0f / 100.0f;
    const float vi = (float)(m - 1u) * qf;
    uint32_t k0, k1;
    float gamma;
    if (vi >= (float)(m - 1u)) {
        k0 = k1 = m - 1u;
        gamma = (float)((double)vi - (-1.0));
    } else {
        const double prev = floor((double)vi);
        k0 = (uint32_t)prev;
        k1 = k0 + 1u;
        gamma = (float)((double)vi - prev);
    }
    uint32_t pfx = 0u, rank = k0;
    for (int level = 0; level < 3; ++level) {
        const int nb = level == 0 ? kBins0 : kBins12;
        for (int i = threadIdx.x; i < nb; i += kSelThreads) hist[i] = 0u;
        __syncthreads();
        for (uint32_t i0 = threadIdx.x; i0 < m; i0 += kSelThreads * 8) {      // eight independent loads in flight
            uint32_t bits[8];
            for (int u = 0; u < 8; ++u) {
                const uint32_t i = i0 + (uint32_t)u * kSelThreads;
                bits[u] = i < m ? __float_as_uint(mags[i]) : 0xffffffffu;       // (no magnitude has the sign bit)
            }
            for (int u = 0; u < 8; ++u) {
                if (bits[u] == 0xffffffffu) continue;
                if (level == 0) atomicAdd(&hist[bits[u] >> 20], 1u);
                else if (level == 1) { if ((bits[u] >> 20) == pfx) atomicAdd(&hist[(bits[u] >> 10) & 1023u], 1u); }
                else if ((bits[u] >> 10) == pfx) atomicAdd(&hist[bits[u] & 1023u], 1u);
            }
        }
        __syncthreads();
        find_bin(hist, nb, rank, s_part, &s_bin, &s_left);
        pfx = level == 0 ? s_bin : ((pfx << 10) | s_bin);
        rank = s_left;
        if (level < 2) __syncthreads();
    }
    const uint32_t v0 = pfx;
    uint32_t v1 = v0;
    const bool need_next = k1 != k0 && rank + 1u >= hist[v0 & 1023u];       // the next order statistic is a larger value
    if (threadIdx.x == 0) s_min = 0xffffffffu;
    __syncthreads();
    if (need_next) {
        uint32_t mine = 0xffffffffu;
        for (uint32_t i = threadIdx.x; i < m; i += kSelThreads) {
            const uint32_t bits = __float_as_uint(mags[i]);
            if (bits > v0 && bits < mine) mine = bits;
        }
        if (mine != 0xffffffffu) atomicMin(&s_min, mine);
        __syncthreads();
        v1 = s_min;
    }
    if (threadIdx.x == 0) {
        const float a = __uint_as_float(v0), b = __uint_as_float(v1);
        const float d = b - a;                                               // numpy's _lerp in fp32, with its t >= 0.5 branch
        const float pct = gamma >= 0.5f ? b - d * (1.0f - gamma) : a + d * gamma;
        *scaling = grid_dist / pct;
    }
}

// ---- one record per (image, grid point) -------------------------------------------------------------------------------------------
struct PlanParams {
    FlowIn f;
    Geometry g;
    const float* scaling;
    int32_t* recs;
    uint32_t* counts;
    int32_t ref_s;             // 1: 's' (grid point -> end point, thickness 1), 0: 't'
    int32_t colour;            // packed b | g << 8 | r << 16, or -1: the hue of the direction
    int32_t thickness;
    float tip_size;            // fp32(sqrt(thickness) * 3.5)
};

// flow_class.py:1333-1349 for (h, 255, 255): the colour Flow.visualise('bgr') paints for that hue at full saturation
__device__ __forceinline__ int32_t hue_bgr(float hue) {
    const float h = hue / 180.0f, s = 255.0f / 255.0f, v = 255.0f / 255.0f;
    const float h6 = h * 6.0f;
    int64_t i = (int64_t)h6;
    const double f = (double)h6 - (double)i;
    const double t = 1.0 - f;
    i %= 6;
    const double sd = (double)s, vd = (double)v;
    double c[4];
    c[0] = (1.0 - sd * 0.0) * vd;
    c[1] = (1.0 - sd * 1.0) * vd;
    c[2] = (1.0 - sd * f) * vd;
    c[3] = (1.0 - sd * t) * vd;
    int r0, r1, r2;
    switch ((int)i) {
        case 0: r0 = 0; r1 = 3; r2 = 1; break;
        case 1: r0 = 2; r1 = 0; r2 = 1; break;
        case 2: r0 = 1; r1 = 0; r2 = 3; break;
        case 3: r0 = 1; r1 = 2; r2 = 0; break;
        case 4: r0 = 3; r1 = 1; r2 = 0; break;
        default: r0 = 0; r1 = 1; r2 = 2; break;
    }
    const int32_t r = (int32_t)rint(c[r0] * 255.0), gch = (int32_t)rint(c[r1] * 255.0), b = (int32_t)rint(c[r2] * 255.0);
    return b | (gch << 8) | (r << 16);
}

__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int imax(int a, int b) { return a > b ? a : b; }

__global__ void __launch_bounds__(kThreads) arrows_records_kernel(PlanParams p) {
    const Geometry& g = p.g;
    const int64_t pts = (int64_t)g.rows * g.cols;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= pts * g.n) return;
    const int img = (int)(i / pts);
    const int j = (int)(i - (int64_t)img * pts);
    const int gy = g.g / 2 + (j / g.cols) * g.g, gx = g.g / 2 + (j % g.cols) * g.g;
    const int64_t q = (int64_t)gy * g.w + gx;
    const float fx = thr(flow_at(p.f, g.hw, img, 0, q)), fy = thr(flow_at(p.f, g.hw, img, 1, q));
    const float s = *p.scaling;
    const float smag = cart_mag(fx, fy) * s;                   // flow_mags *= scaling (fp32)
    int32_t* rec = p.recs + i * kRec;
    // drawn iff the scaled magnitude is > 0.5; skipped when it is not finite or beyond 2^20 pixels
    bool listed = smag > 0.5f && smag <= kFar;
    int32_t r[kRec];
    for (int k = 0; k < kRec; ++k) r[k] = 0;
    if (listed) {
        const float sx = fx * s, sy = fy * s;                  // f *= scaling (fp32)
        // np.round(i_pt +- f[::-1]).astype('i'): int32 + fp32 promotes to float64; half to even
        const double sign = p.ref_s ? 1.0 : -1.0;
        const int ex = (int)rint((double)gx + sign * (double)sx), ey = (int)rint((double)gy + sign * (double)sy);
        const int p1x = p.ref_s ? gx : ex, p1y = p.ref_s ? gy : ey, p2x = p.ref_s ? ex : gx, p2y = p.ref_s ? ey : gy;
        const double tip_length = (double)(p.tip_size / smag);  // float(tip_size / np.float32): an fp32 division
        const double k = tip_length * 0.7071067811865476;
        const double dx = (double)(p1x - p2x), dy = (double)(p1y - p2y);
        const int bpx = (int)rint((double)p2x + k * (dx - dy)), bpy = (int)rint((double)p2y + k * (dx + dy));
        const int bmx = (int)rint((double)p2x + k * (dx + dy)), bmy = (int)rint((double)p2y + k * (dy - dx));
        const int t = p.ref_s ? 1 : p.thickness;
        const int pad = t / 2 + 1;                              // >= t / 2 + 0.5: no pixel outside has alpha > 0
        const int tx0 = imax(imin(imin(p2x, bpx), bmx) - pad, 0), tx1 = imin(imax(imax(p2x, bpx), bmx) + pad, g.w - 1);
        const int ty0 = imax(imin(imin(p2y, bpy), bmy) - pad, 0), ty1 = imin(imax(imax(p2y, bpy), bmy) + pad, g.h - 1);
        const int sx0 = imax(imin(p1x, p2x) - pad, 0), sx1 = imin(imax(p1x, p2x) + pad, g.w - 1);
        const int sy0 = imax(imin(p1y, p2y) - pad, 0), sy1 = imin(imax(p1y, p2y) + pad, g.h - 1);
        // (an empty box has x0 > x1 or y0 > y1; the union of an empty and a full one is the full one)
        const bool tip_in = tx0 <= tx1 && ty0 <= ty1, shaft_in = sx0 <= sx1 && sy0 <= sy1;
        int bx0 = sx0, bx1 = sx1, by0 = sy0, by1 = sy1;
        if (tip_in && shaft_in) { bx0 = imin(sx0, tx0); bx1 = imax(sx1, tx1); by0 = imin(sy0, ty0); by1 = imax(sy1, ty1); }
        else if (tip_in) { bx0 = tx0; bx1 = tx1; by0 = ty0; by1 = ty1; }
        listed = tip_in || shaft_in;
        r[R_P1X] = p1x; r[R_P1Y] = p1y; r[R_P2X] = p2x; r[R_P2Y] = p2y;
        r[R_BPX] = bpx; r[R_BPY] = bpy; r[R_BMX] = bmx; r[R_BMY] = bmy;
        r[R_BX0] = bx0; r[R_BY0] = by0; r[R_BX1] = bx1; r[R_BY1] = by1;
        r[R_TX0] = tx0; r[R_TY0] = ty0; r[R_TX1] = tx1; r[R_TY1] = ty1;
        r[R_THICK] = t;
        if (p.colour >= 0) {
            r[R_COL] = p.colour;
        } else {
            const float ang = cart_angle(fx, fy);              // of the unscaled vector, as the reference
            // uint8(np.round(np.mod(ang, 360) / 2)): the angle lies in [0, 360]
            r[R_COL] = hue_bgr(rintf((ang >= 360.0f ? ang - 360.0f : ang) / 2.0f));
        }
        r[R_LISTED] = listed ? 1 : 0;
    }
    int4* dst = reinterpret_cast<int4*>(rec);
    for (int k = 0; k < kRec / 4; ++k) dst[k] = make_int4(r[4 * k], r[4 * k + 1], r[4 * k + 2], r[4 * k + 3]);
    if (!listed) return;
    uint32_t* counts = p.counts + (int64_t)img * g.tx * g.ty;
    for (int ty = r[R_BY0] / kTileH; ty <= r[R_BY1] / kTileH; ++ty)
        for (int tx = r[R_BX0] / kTileW; tx <= r[R_BX1] / kTileW; ++tx) atomicAdd(&counts[ty * g.tx + tx], 1u);
}

// exclusive scan of the tile counts of one image per block (offsets inside the image), and the image's sum
__global__ void __launch_bounds__(kThreads) arrows_scan_image_kernel(const uint32_t* counts, uint32_t* offsets, int32_t tiles,
                                                                     unsigned long long* img_total) {
    __shared__ uint32_t part[kThreads];
    const int64_t t0 = (int64_t)blockIdx.x * tiles;
    unsigned long long carry = 0ull;
    for (int base = 0; base < tiles; base += kThreads) {
        const int i = base + (int)threadIdx.x;
        const uint32_t v = i < tiles ? counts[t0 + i] : 0u;
        part[threadIdx.x] = v;
        __syncthreads();
        for (int off = 1; off < kThreads; off <<= 1) {
            const uint32_t a = threadIdx.x >= (unsigned)off ? part[threadIdx.x - off] : 0u;
            __syncthreads();
            part[threadIdx.x] += a;
            __syncthreads();
        }
        if (i < tiles) offsets[t0 + i] = (uint32_t)(carry + part[threadIdx.x] - v);
        carry += part[kThreads - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0) img_total[blockIdx.x] = carry;
}

// exclusive scan of the images' sums by one block; header[0..1] = the sum of all (int64)
__global__ void __launch_bounds__(kSelThreads) arrows_scan_kernel(const unsigned long long* counts, unsigned long long* offsets,
                                                                  int64_t nt, int32_t* header) {
    __shared__ unsigned long long part[kSelThreads];
    const int64_t chunk = (nt + kSelThreads - 1) / kSelThreads;
    const int64_t lo = (int64_t)threadIdx.x * chunk, hi = lo + chunk < nt ? lo + chunk : nt;
    unsigned long long sum = 0ull;
    for (int64_t i = lo; i < hi; ++i) sum += counts[i];
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int off = 1; off < kSelThreads; off <<= 1) {
        const unsigned long long v = threadIdx.x >= (unsigned)off ? part[threadIdx.x - off] : 0ull;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    unsigned long long c = part[threadIdx.x] - sum;
    for (int64_t i = lo; i < hi; ++i) { offsets[i] = c; c += counts[i]; }
    if (threadIdx.x == kSelThreads - 1) *reinterpret_cast<long long*>(header) = (long long)part[threadIdx.x];
}

// ---- fill: every listed arrow appends its grid-point index to the list of each tile its box touches ----------------------------
struct FillParams {
    Geometry g;
    const int32_t* recs;
    const uint32_t* offsets;
    const unsigned long long* img_base;
    uint32_t* cursor;
    int32_t* list;
    int64_t list_ints;
};

__global__ void __launch_bounds__(kThreads) arrows_fill_kernel(FillParams p) {
    const Geometry& g = p.g;
    const int64_t pts = (int64_t)g.rows * g.cols;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= pts * g.n) return;
    const int32_t* rec = p.recs + i * kRec;
    if (!rec[R_LISTED]) return;
    const int img = (int)(i / pts);
    const int j = (int)(i - (int64_t)img * pts);
    const int64_t t0 = (int64_t)img * g.tx * g.ty;
    for (int ty = rec[R_BY0] / kTileH; ty <= rec[R_BY1] / kTileH; ++ty)
        for (int tx = rec[R_BX0] / kTileW; tx <= rec[R_BX1] / kTileW; ++tx) {
            const int64_t t = t0 + ty * g.tx + tx;
            const int64_t at = (int64_t)p.img_base[img] + p.offsets[t] + atomicAdd(&p.cursor[t], 1u);
            if (at < p.list_ints) p.list[at] = j;
        }
}

// ---- raster: one block per 64 x 16 tile, each thread owns four pixels of a row ---------------------------------------------------
struct RasterParams {
    Geometry g;
    const int32_t* recs;
    const uint32_t* counts;
    const uint32_t* offsets;
    const unsigned long long* img_base;
    const int32_t* list;
    int64_t list_ints;
    const uint8_t* img;        // nullptr: white
    int64_t img_bs;            // bytes between images (0: one image for the batch)
    int img_layout;            // 0 3-H-W planes, 1 H-W-3
    const uint8_t* mask;       // nullptr: all True
    int64_t mask_bs;
    int show_mask, borders;
    uint8_t* out;
    int layout;                // 0 N-3-H-W, 1 N-H-W-3
    int vec_in, vec_out;
};

__device__ __forceinline__ bool mask_at(const RasterParams& p, int img, int64_t q) {
    return p.mask == nullptr || p.mask[img * p.mask_bs + q] != 0;
}

// squared distance of the pixel centre (qx, qy) to the segment a -> a + e (integers held in float64: every product and sum
// below 2^53 is exact); +inf where it is surely >= r2 (lim = r2 * L2 with a margin far above the rounding of either side)
__device__ __forceinline__ double seg_d2(double qx, double qy, double ax, double ay, double ex, double ey, double l2, double lim) {
    const double dx = qx - ax, dy = qy - ay;
    const double u = dx * ex + dy * ey;
    if (u <= 0.0 || l2 == 0.0) return dx * dx + dy * dy;
    if (u >= l2) {
        const double fx = dx - ex, fy = dy - ey;
        return fx * fx + fy * fy;
    }
    const double cr = dx * ey - dy * ex;
    const double c2 = cr * cr;
    if (c2 > lim) return HUGE_VAL;
    return c2 / l2;
}

// blend the m staged records (ascending grid-point index) into the thread's four pixels
__device__ __forceinline__ void paint_staged(int m, const int32_t* s_idx, const int32_t* s_rec, int y, int x0, int wave_y0,
                                             int (&c)[4][3], int (&red)[4]) {
    for (int r = 0; r < m; ++r) {
        const int32_t* rec = s_rec + r * kRec;
        if (rec[R_BY1] < wave_y0 || rec[R_BY0] > wave_y0 + 3) continue;      // (wave-uniform)
        if (y < rec[R_BY0] || y > rec[R_BY1] || x0 > rec[R_BX1] || x0 + 3 < rec[R_BX0]) continue;
        const int j = s_idx[r];
        const double p1x = rec[R_P1X], p1y = rec[R_P1Y], p2x = rec[R_P2X], p2y = rec[R_P2Y];
        const double bpx = rec[R_BPX], bpy = rec[R_BPY], bmx = rec[R_BMX], bmy = rec[R_BMY];
        const double e0x = p2x - p1x, e0y = p2y - p1y, e1x = p2x - bpx, e1y = p2y - bpy, e2x = p2x - bmx, e2y = p2y - bmy;
        const double l0 = e0x * e0x + e0y * e0y, l1 = e1x * e1x + e1y * e1y, l2 = e2x * e2x + e2y * e2y;
        const double rad = (double)rec[R_THICK] / 2.0 + 0.5, r2 = rad * rad;
        const double m0 = r2 * l0 * 1.0000001, m1 = r2 * l1 * 1.0000001, m2 = r2 * l2 * 1.0000001;
        const bool tip_row = y >= rec[R_TY0] && y <= rec[R_TY1];
        const double qy = (double)y;
        const int col = rec[R_COL];
        for (int k = 0; k < 4; ++k) {
            const int x = x0 + k;
            if (x < rec[R_BX0] || x > rec[R_BX1]) continue;
            const double qx = (double)x;
            double d2 = seg_d2(qx, qy, p1x, p1y, e0x, e0y, l0, m0);
            if (tip_row && x >= rec[R_TX0] && x <= rec[R_TX1]) {
                d2 = fmin(d2, seg_d2(qx, qy, bpx, bpy, e1x, e1y, l1, m1));
                d2 = fmin(d2, seg_d2(qx, qy, bmx, bmy, e2x, e2y, l2, m2));
            }
            if (!(d2 < r2)) continue;                    // d >= t / 2 + 0.5: alpha = 0, the pixel keeps its value
            if (red[k] >= 0 && red[k] < j) { c[k][0] = 0; c[k][1] = 0; c[k][2] = 255; red[k] = -1; }
            const double alpha = fmin(fmax(rad - sqrt(d2), 0.0), 1.0);
            for (int ch = 0; ch < 3; ++ch) {
                const double old = (double)c[k][ch];
                c[k][ch] = (int)rint(old + alpha * ((double)((col >> (8 * ch)) & 255) - old));
            }
        }
    }
}

__global__ void __launch_bounds__(kThreads) arrows_raster_kernel(RasterParams p) {
    __shared__ uint32_t bitmap[kThreads];
    __shared__ uint32_t scan[kThreads];
    __shared__ int32_t s_idx[kStage];
    __shared__ int32_t s_rec[kStage * kRec];
    __shared__ int32_t s_lo, s_hi;
    const Geometry& g = p.g;
    const int img = blockIdx.z;
    const int64_t tile = ((int64_t)img * g.ty + blockIdx.y) * g.tx + blockIdx.x;
    const int y = blockIdx.y * kTileH + (int)threadIdx.x / 16;
    const int x0 = blockIdx.x * kTileW + ((int)threadIdx.x % 16) * 4;
    const bool row_in = y < g.h;
    const int64_t q0 = (int64_t)y * g.w + x0;
    // background
    int c[4][3];
    for (int k = 0; k < 4; ++k) c[k][0] = c[k][1] = c[k][2] = 255;
    if (p.img != nullptr && row_in && x0 < g.w) {
        const uint8_t* src = p.img + (int64_t)img * p.img_bs;
        if (p.vec_in) {
            if (p.img_layout == 0) {
                for (int ch = 0; ch < 3; ++ch) {
                    const uint32_t wd = *reinterpret_cast<const uint32_t*>(src + ch * g.hw + q0);
                    for (int k = 0; k < 4; ++k) c[k][ch] = (int)((wd >> (8 * k)) & 255u);
                }
            } else {
                const uint32_t* s32 = reinterpret_cast<const uint32_t*>(src + q0 * 3);
                const uint32_t wd[3] = {s32[0], s32[1], s32[2]};
                for (int b = 0; b < 12; ++b) c[b / 3][b % 3] = (int)((wd[b >> 2] >> (8 * (b & 3))) & 255u);
            }
        } else {
            for (int k = 0; k < 4; ++k)
                if (x0 + k < g.w)
                    for (int ch = 0; ch < 3; ++ch)
                        c[k][ch] = p.img_layout == 0 ? src[ch * g.hw + q0 + k] : src[(q0 + k) * 3 + ch];
        }
    }
    // the grid point of each pixel (its index in the painter's order), or -1
    int red[4];
    {
        const int oy = y - g.g / 2;
        const bool gy_ok = row_in && oy >= 0 && oy % g.g == 0 && oy / g.g < g.rows;
        for (int k = 0; k < 4; ++k) {
            const int ox = x0 + k - g.g / 2;
            red[k] = (gy_ok && ox >= 0 && ox % g.g == 0 && ox / g.g < g.cols) ? (oy / g.g) * g.cols + ox / g.g : -1;
        }
    }
    // the tile's list: indices of the image's grid points, in the order the fill wrote them
    int64_t off = (int64_t)p.img_base[img] + p.offsets[tile];
    int64_t len = (int64_t)p.counts[tile];
    if (off + len > p.list_ints) len = p.list_ints > off ? p.list_ints - off : 0;
    const int32_t* list = p.list + off;
    const int64_t rec0 = (int64_t)img * g.rows * g.cols;
    const int wave_y0 = blockIdx.y * kTileH + ((int)threadIdx.x / 64) * 4;
    if (len <= kStage) {
        // the usual tile: a short list, put in order by counting the smaller entries (the indices are distinct)
        const int m = (int)len;
        if ((int)threadIdx.x < m) scan[threadIdx.x] = (uint32_t)list[threadIdx.x];
        __syncthreads();
        if ((int)threadIdx.x < m) {
            const uint32_t v = scan[threadIdx.x];
            int rank = 0;
            for (int k = 0; k < m; ++k) rank += scan[k] < v ? 1 : 0;
            s_idx[rank] = (int)v;
        }
        __syncthreads();
        for (int i = threadIdx.x; i < m * kRec; i += kThreads) s_rec[i] = p.recs[(rec0 + s_idx[i / kRec]) * kRec + i % kRec];
        __syncthreads();
        paint_staged(m, s_idx, s_rec, y, x0, wave_y0, c, red);
        len = 0;                                                  // (nothing left for the windows below)
    }
    if (threadIdx.x == 0) { s_lo = 0x7fffffff; s_hi = -1; }
    __syncthreads();
    {
        int lo = 0x7fffffff, hi = -1;
        for (int64_t i = threadIdx.x; i < len; i += kThreads) { const int j = list[i]; lo = imin(lo, j); hi = imax(hi, j); }
        if (hi >= 0) { atomicMin(&s_lo, lo); atomicMax(&s_hi, hi); }
    }
    __syncthreads();
    const int j_lo = s_lo, j_hi = s_hi;
    for (int64_t base = len > 0 ? (int64_t)(j_lo / kWin) * kWin : 1; base <= j_hi; base += kWin) {
        // ascending order without a sort: the window's indices as bits, then the bits in order
        bitmap[threadIdx.x] = 0u;
        __syncthreads();
        for (int64_t i = threadIdx.x; i < len; i += kThreads) {
            const int64_t d = (int64_t)list[i] - base;
            if (d >= 0 && d < kWin) atomicOr(&bitmap[d >> 5], 1u << (d & 31));
        }
        __syncthreads();
        const uint32_t word = bitmap[threadIdx.x];
        const uint32_t mine = (uint32_t)__popc(word);
        scan[threadIdx.x] = mine;
        __syncthreads();
        for (int o = 1; o < kThreads; o <<= 1) {
            const uint32_t v = threadIdx.x >= (unsigned)o ? scan[threadIdx.x - o] : 0u;
            __syncthreads();
            scan[threadIdx.x] += v;
            __syncthreads();
        }
        const int total = (int)scan[kThreads - 1];
        const int first = (int)(scan[threadIdx.x] - mine);
        for (int sub = 0; sub < total; sub += kStage) {
            uint32_t wd = word;
            for (int s = first; wd != 0u; ++s, wd &= wd - 1u)
                if (s >= sub && s < sub + kStage) s_idx[s - sub] = (int)(base + 32 * (int)threadIdx.x + (__ffs((int)wd) - 1));
            __syncthreads();
            const int m = imin(kStage, total - sub);
            for (int i = threadIdx.x; i < m * kRec; i += kThreads) s_rec[i] = p.recs[(rec0 + s_idx[i / kRec]) * kRec + i % kRec];
            __syncthreads();
            paint_staged(m, s_idx, s_rec, y, x0, wave_y0, c, red);
            __syncthreads();
        }
    }
    if (!row_in || x0 >= g.w) return;
    uint8_t o[4][3];
    for (int k = 0; k < 4; ++k) {
        if (red[k] >= 0) { c[k][0] = 0; c[k][1] = 0; c[k][2] = 255; }
        const bool exists = x0 + k < g.w;
        if (exists && p.show_mask && !mask_at(p, img, q0 + k))
            for (int ch = 0; ch < 3; ++ch) { const int hv = c[k][ch] >> 1; c[k][ch] = hv + ((c[k][ch] & 1) & (hv & 1)); }   // np.round(0.5 * px)
        if (exists && p.borders && mask_at(p, img, q0 + k)) {
            const int x = x0 + k;
            const bool edge = y == 0 || x == 0 || y == g.h - 1 || x == g.w - 1;
            if (edge || !mask_at(p, img, q0 + k - 1) || !mask_at(p, img, q0 + k + 1) || !mask_at(p, img, q0 + k - g.w) ||
                !mask_at(p, img, q0 + k + g.w))
                c[k][0] = c[k][1] = c[k][2] = 0;
        }
        for (int ch = 0; ch < 3; ++ch) o[k][ch] = (uint8_t)c[k][ch];
    }
    if (p.layout == 0) {
        uint8_t* dst = p.out + (int64_t)img * 3 * g.hw + q0;
        for (int ch = 0; ch < 3; ++ch) {
            if (p.vec_out) {
                *reinterpret_cast<uint32_t*>(dst + ch * g.hw) =
                    (uint32_t)o[0][ch] | ((uint32_t)o[1][ch] << 8) | ((uint32_t)o[2][ch] << 16) | ((uint32_t)o[3][ch] << 24);
            } else {
                for (int k = 0; k < 4; ++k) if (x0 + k < g.w) dst[ch * g.hw + k] = o[k][ch];
            }
        }
    } else {
        uint8_t* dst = p.out + ((int64_t)img * g.hw + q0) * 3;
        if (p.vec_out) {
            uint32_t wd[3] = {0u, 0u, 0u};
            for (int b = 0; b < 12; ++b) wd[b >> 2] |= (uint32_t)o[b / 3][b % 3] << (8 * (b & 3));
            uint32_t* d32 = reinterpret_cast<uint32_t*>(dst);
            d32[0] = wd[0]; d32[1] = wd[1]; d32[2] = wd[2];
        } else {
            for (int k = 0; k < 4; ++k)
                if (x0 + k < g.w) { dst[3 * k] = o[k][0]; dst[3 * k + 1] = o[k][1]; dst[3 * k + 2] = o[k][2]; }
        }
    }
}

// n, h, w, grid_dist -> geometry, or an OFL_E_* code
int make_geometry(int32_t n, int32_t h, int32_t w, int32_t grid_dist, Geometry* out) {
    if (n < 1 || h < 2 || w < 2 || n > 65535) return OFL_E_SHAPE;
    if ((int64_t)h * w >= (1ll << 31)) return OFL_E_SHAPE;
    if (grid_dist < 1 || grid_dist > (h < w ? h : w) / 2) return OFL_E_ARG;
    Geometry g;
    g.n = n; g.h = h; g.w = w; g.g = grid_dist; g.hw = (int64_t)h * w;
    g.rows = grid_count(h, grid_dist); g.cols = grid_count(w, grid_dist);
    g.tx = (w + kTileW - 1) / kTileW; g.ty = (h + kTileH - 1) / kTileH;
    if (g.ty > 65535 || (int64_t)g.tx * g.ty >= (1ll << 31)) return OFL_E_SHAPE;
    if ((int64_t)n * g.rows * g.cols >= (1ll << 31)) return OFL_E_SHAPE;
    *out = g;
    return OFL_OK;
}

int64_t workspace_ints(const Geometry& g) {
    const int64_t m = (int64_t)g.n * g.rows * g.cols, nt = (int64_t)g.n * g.tx * g.ty;
    return kHeader + 4 * (int64_t)g.n + m + m * kRec + 3 * nt;
}

bool aligned(const void* ptr, int a) { return ((uintptr_t)ptr % (uintptr_t)a) == 0; }

}  // namespace

extern "C" {

__attribute__((visibility("default"))) int64_t ofl_arrows_workspace_ints(int32_t n, int32_t h, int32_t w, int32_t grid_dist) {
    Geometry g;
    const int rc = make_geometry(n, h, w, grid_dist, &g);
    if (rc) return rc;
    return workspace_ints(g);
}

__attribute__((visibility("default"))) int ofl_arrows_scale_f32(const void* flow, int64_t flow_bs, int32_t flow_half,
                                                                int32_t grid_dist, int32_t* workspace, float* scaling, int32_t n,
                                                                int32_t h, int32_t w, void* stream) {
    if (!flow || !workspace || !scaling) return OFL_E_NULL;
    Geometry g;
    const int rc = make_geometry(n, h, w, grid_dist, &g);
    if (rc) return rc;
    if ((flow_half != 0 && flow_half != 1) || flow_bs < 0) return OFL_E_ARG;
    const Workspace ws = carve(workspace, g);
    const FlowIn f{flow, flow_bs, flow_half};
    const int64_t m = (int64_t)n * g.rows * g.cols;
    hipStream_t s = (hipStream_t)stream;
    OFL_KLAUNCH(arrows_sample_kernel, dim3((unsigned)((m + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, f, g, ws.mags);
    OFL_KLAUNCH(arrows_select_kernel, dim3(1), dim3(kSelThreads), 0, s, (const float*)ws.mags, (uint32_t)m, (float)grid_dist, scaling);
    return (int)hipGetLastError();
}

__attribute__((visibility("default"))) int ofl_arrows_plan(const void* flow, int64_t flow_bs, int32_t flow_half, int32_t ref_s,
                                                           int32_t grid_dist, const float* scaling, int32_t colour,
                                                           int32_t thickness, float tip_size, int32_t* workspace, int32_t n,
                                                           int32_t h, int32_t w, void* stream) {
    if (!flow || !workspace || !scaling) return OFL_E_NULL;
    Geometry g;
    const int rc = make_geometry(n, h, w, grid_dist, &g);
    if (rc) return rc;
    if ((flow_half != 0 && flow_half != 1) || flow_bs < 0 || (ref_s != 0 && ref_s != 1)) return OFL_E_ARG;
    if (thickness < 1 || thickness > 32767 || colour < -1 || colour > 0xffffff || !(tip_size > 0.0f)) return OFL_E_ARG;
    const Workspace ws = carve(workspace, g);
    const int64_t m = (int64_t)n * g.rows * g.cols, nt = (int64_t)n * g.tx * g.ty;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(ws.counts, 0, (size_t)nt * sizeof(uint32_t), s);
    if (e != hipSuccess) return (int)e;
    PlanParams p;
    p.f = FlowIn{flow, flow_bs, flow_half}; p.g = g; p.scaling = scaling; p.recs = ws.recs; p.counts = ws.counts;
    p.ref_s = ref_s; p.colour = colour; p.thickness = thickness; p.tip_size = tip_size;
    OFL_KLAUNCH(arrows_records_kernel, dim3((unsigned)((m + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, p);
    OFL_KLAUNCH(arrows_scan_image_kernel, dim3((unsigned)n), dim3(kThreads), 0, s, (const uint32_t*)ws.counts, ws.offsets,
                g.tx * g.ty, ws.img_total);
    OFL_KLAUNCH(arrows_scan_kernel, dim3(1), dim3(kSelThreads), 0, s, (const unsigned long long*)ws.img_total, ws.img_base,
                (int64_t)n, ws.header);
    return (int)hipGetLastError();
}

__attribute__((visibility("default"))) int ofl_arrows_u8(const uint8_t* img, int64_t img_bs, int32_t img_layout,
                                                         const uint8_t* mask, int64_t mask_bs, int32_t show_mask,
                                                         int32_t show_mask_borders, int32_t grid_dist, int32_t* workspace,
                                                         int32_t* list, int64_t list_ints, int32_t layout, uint8_t* out,
                                                         int32_t n, int32_t h, int32_t w, void* stream) {
    if (!workspace || !out || (!list && list_ints > 0)) return OFL_E_NULL;
    Geometry g;
    const int rc = make_geometry(n, h, w, grid_dist, &g);
    if (rc) return rc;
    if (layout < 0 || layout > 1 || img_layout < 0 || img_layout > 1) return OFL_E_ARG;
    if ((show_mask != 0 && show_mask != 1) || (show_mask_borders != 0 && show_mask_borders != 1)) return OFL_E_ARG;
    if (img_bs < 0 || mask_bs < 0 || list_ints < 0) return OFL_E_ARG;
    const Workspace ws = carve(workspace, g);
    const int64_t m = (int64_t)n * g.rows * g.cols, nt = (int64_t)n * g.tx * g.ty;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(ws.cursor, 0, (size_t)nt * sizeof(uint32_t), s);
    if (e != hipSuccess) return (int)e;
    FillParams fp;
    fp.g = g; fp.recs = ws.recs; fp.offsets = ws.offsets; fp.img_base = ws.img_base; fp.cursor = ws.cursor; fp.list = list; fp.list_ints = list_ints;
    if (list_ints > 0)
        OFL_KLAUNCH(arrows_fill_kernel, dim3((unsigned)((m + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, fp);
    RasterParams p;
    p.g = g; p.recs = ws.recs; p.counts = ws.counts; p.offsets = ws.offsets; p.img_base = ws.img_base; p.list = list; p.list_ints = list_ints;
    p.img = img; p.img_bs = img_bs; p.img_layout = img_layout; p.mask = mask; p.mask_bs = mask_bs;
    p.show_mask = show_mask; p.borders = show_mask_borders; p.out = out; p.layout = layout;
    p.vec_in = img != nullptr && w % 4 == 0 && img_bs % 4 == 0 && aligned(img, 4);
    p.vec_out = w % 4 == 0 && aligned(out, 4);
    OFL_KLAUNCH(arrows_raster_kernel, dim3((unsigned)g.tx, (unsigned)g.ty, (unsigned)n), dim3(kThreads), 0, s, p);
    return (int)hipGetLastError();
}

}  // extern "C"
