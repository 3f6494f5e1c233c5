// ofl_visualise.hip -- Flow.visualise (flow_class.py:1246-1356) on gfx950: the HSV colour coding of a flow field and its
// per-image range (the 99th percentile of the magnitudes), without a host round trip.
//
//   ofl_visualise_range_f32   <- the `range_max is None` loop (flow_class.py:1300-1309): np.percentile(m, 99) of numpy 2.2.6
//                                ('linear': virtual index (n - 1) * q in fp32, _get_gamma, _lerp with its t >= 0.5 branch), the
//                                np.max fallback and the final 1.  An exact order statistic by a three-level radix select on the
//                                fp32 bit patterns (magnitudes are >= 0, so they sort as uint32): 11 + 10 + 10 bits, integer
//                                histograms per block in LDS, one atomicAdd per non-empty bin into a per-image histogram.
//   ofl_visualise_u8          <- everything after it: threshold_vectors, cv2.cartToPolar (restated below), the HSV planes, the
//                                mask value 180, the mask borders of findContours / drawContours, np.round for 'hsv', the
//                                float64 HSV -> RGB of :1333-1349 for 'rgb' / 'bgr'.
//
// Bit-exact with the reference's NumPy: fp32 where NumPy computes in fp32, fp64 where it promotes, the only fused multiply-adds
// the explicit fmaf of OpenCV's SIMD cartToPolar.  C ABI: include/oflib_hip.h.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <float.h>
#include <stdint.h>

#include "oflib_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr float kZeroThr = 1e-3f;      // utils.py:23, :642 (compared in fp32, as the kernels of ofl_kernels.hip do)
constexpr int kThreads = 256;
constexpr int kQuadsPerThread = 16;    // histogram passes: 256 threads x 16 quads = 16 384 pixels per block
constexpr int kBins0 = 2048;           // level 0: bits 30..20 (sign bit is 0)
constexpr int kBins12 = 1024;          // levels 1 and 2: bits 19..10, 9..0
// per image workspace (int32): H0[2048], H1[2][1024], H2[2][1024], meta[kMeta]
constexpr int kMeta = 16;
constexpr int kWsInts = kBins0 + 2 * kBins12 + 2 * kBins12 + kMeta;
constexpr int kOffH1 = kBins0, kOffH2 = kBins0 + 2 * kBins12, kOffMeta = kBins0 + 4 * kBins12;
// meta: [0] count of values, [1] max (fp32 bits), [2] [3] prefix of target 0 / 1, [4] [5] rank left in the prefix's bin
enum { M_COUNT = 0, M_MAX = 1, M_PFX = 2, M_RANK = 4 };

// ---- cv2.cartToPolar(x, y, angleInDegrees=True), restated from OpenCV 4.x mathfuncs_core.simd.hpp (fastAtan32 / magnitude).
// OpenCV's x86 build runs its AVX2 path (FMA) on all but the last len % 8 values of a row and a scalar tail without FMA.  The
// reference's rows are the W values of an image row.  THE choice of this file: every value takes the SIMD (FMA) form,
// as the oracle (tests/vis_oracle.py, OFL_CART_FMA) does.  Restated, not checked against an OpenCV build.
#define OFL_CART_FMA 1
constexpr float kRad2Deg = (float)(180.0 / 3.141592653589793);
constexpr float kP1 = 0.9997878412794807f * kRad2Deg;
constexpr float kP3 = -0.3258083974640975f * kRad2Deg;
constexpr float kP5 = 0.1555786518463281f * kRad2Deg;
constexpr float kP7 = -0.04432655554792128f * kRad2Deg;

__device__ __forceinline__ float thr(float u) { return (u < kZeroThr && u > -kZeroThr) ? 0.0f : u; }

__device__ __forceinline__ float cart_mag(float x, float y) {
#if OFL_CART_FMA
    return sqrtf(fmaf(x, x, y * y));
#else
    return sqrtf(x * x + y * y);
#endif
}

__device__ __forceinline__ float cart_angle(float x, float y) {
    const float ax = fabsf(x), ay = fabsf(y);
    const float c = fminf(ax, ay) / (fmaxf(ax, ay) + (float)DBL_EPSILON);
    const float cc = c * c;
#if OFL_CART_FMA
    float a = fmaf(fmaf(fmaf(cc, kP7, kP5), cc, kP3), cc, kP1) * c;
#else
    float a = (((kP7 * cc + kP5) * cc + kP3) * cc + kP1) * c;
#endif
    if (!(ax >= ay)) a = 90.0f - a;
    if (x < 0.0f) a = 180.0f - a;
    if (y < 0.0f) a = 360.0f - a;
    return a;
}

__device__ __forceinline__ float magnitude_of(float x, float y) { return cart_mag(thr(x), thr(y)); }

// ---- loads: `Q` = 4 consecutive pixels of one image; the vector form needs H*W % 4 == 0 and 16 / 8-byte aligned planes
template <bool HALF>
struct Loader {
    const void* flow;
    int64_t bs;
    int64_t hw;
    __device__ __forceinline__ float ld(int64_t img, int plane, int64_t p) const {
        const int64_t o = img * bs + plane * hw + p;
        if (HALF) return __half2float(reinterpret_cast<const __half*>(flow)[o]);
        return reinterpret_cast<const float*>(flow)[o];
    }
    // four pixels p0 .. p0+3 of plane `plane`; `vec`: all four exist and the address is aligned
    __device__ __forceinline__ void ld4(int64_t img, int plane, int64_t p0, bool vec, float v[4]) const {
        const int64_t o = img * bs + plane * hw + p0;
        if (vec) {
            if (HALF) {
                const uint2 u = *reinterpret_cast<const uint2*>(reinterpret_cast<const __half*>(flow) + o);
                const __half2 a = *reinterpret_cast<const __half2*>(&u.x), b = *reinterpret_cast<const __half2*>(&u.y);
                v[0] = __low2float(a); v[1] = __high2float(a); v[2] = __low2float(b); v[3] = __high2float(b);
            } else {
                const float4 f = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(flow) + o);
                v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
            }
        } else {
            for (int k = 0; k < 4; ++k) v[k] = (p0 + k < hw) ? ld(img, plane, p0 + k) : 0.0f;
        }
    }
};

struct RangeParams {
    const void* flow;
    int64_t flow_bs;
    const uint8_t* mask;   // nullptr: every pixel counts
    int64_t mask_bs;
    uint32_t* ws;
    double* range_max;
    int32_t* counts;
    int32_t n, h, w;
    int64_t hw;
    int vec;
};

// one LDS histogram add per lane; a wave whose active lanes all name one bin adds once (a constant-magnitude flow puts every
// pixel of an image in one bin).  Called by every lane of the wave.
__device__ __forceinline__ void hist_add(uint32_t* hist, uint32_t bin, bool active) {
    const unsigned long long act = __ballot(active);
    if (act == 0ull) return;
    const int first = __ffsll((long long)act) - 1;
    const uint32_t b0 = (uint32_t)__shfl((int)bin, first);
    if (__all(!active || bin == b0)) {
        if ((int)__lane_id() == first) atomicAdd(&hist[b0], (uint32_t)__popcll(act));
    } else if (active) {
        atomicAdd(&hist[bin], 1u);
    }
}

// LEVEL 0: histogram of bits 30..20 of every counted magnitude, count and max.  LEVEL 1 / 2: histograms of bits 19..10 / 9..0
// of the magnitudes whose higher bits equal the prefix of target 0 / 1 (one histogram when both targets share their prefix).
template <bool HALF, int LEVEL>
__global__ void __launch_bounds__(kThreads) vis_range_hist_kernel(RangeParams p) {
    __shared__ uint32_t hist[LEVEL == 0 ? kBins0 : 2 * kBins12];
    __shared__ uint32_t s_count, s_max;
    const int img = blockIdx.y;
    uint32_t* ws = p.ws + (int64_t)img * kWsInts;
    const int nb = LEVEL == 0 ? kBins0 : 2 * kBins12;
    for (int i = threadIdx.x; i < nb; i += kThreads) hist[i] = 0u;
    if (threadIdx.x == 0) { s_count = 0u; s_max = 0u; }
    uint32_t pfx0 = 0u, pfx1 = 0u;
    bool same = true;
    if (LEVEL > 0) {
        pfx0 = ws[kOffMeta + M_PFX];
        pfx1 = ws[kOffMeta + M_PFX + 1];
        same = pfx0 == pfx1;
        if (ws[kOffMeta + M_COUNT] == 0u) return;              // (block-uniform: nothing to select)
    }
    __syncthreads();
    const Loader<HALF> L{p.flow, p.flow_bs, p.hw};
    const int64_t quads = (p.hw + 3) / 4;
    const int64_t q_begin = (int64_t)blockIdx.x * kThreads * kQuadsPerThread;
    uint32_t my_count = 0u, my_max = 0u;
    for (int it = 0; it < kQuadsPerThread; ++it) {
        const int64_t q = q_begin + (int64_t)it * kThreads + threadIdx.x;
        if (q_begin + (int64_t)it * kThreads >= quads) break;  // (wave-uniform: the whole step is past the end)
        const bool inq = q < quads;
        const int64_t p0 = 4 * q;
        float x[4] = {0.f, 0.f, 0.f, 0.f}, y[4] = {0.f, 0.f, 0.f, 0.f};
        uint32_t mbits = 0u;
        if (inq) {
            L.ld4(img, 0, p0, p.vec, x);
            L.ld4(img, 1, p0, p.vec, y);
            for (int k = 0; k < 4; ++k) {
                const bool exists = p0 + k < p.hw;
                const bool counted = exists && (p.mask == nullptr || p.mask[img * p.mask_bs + p0 + k] != 0);
                if (counted) mbits |= 1u << k;
            }
        }
        for (int k = 0; k < 4; ++k) {
            const bool counted = (mbits >> k) & 1u;
            const uint32_t bits = __float_as_uint(magnitude_of(x[k], y[k]));
            if (LEVEL == 0) {
                if (counted) { ++my_count; my_max = bits > my_max ? bits : my_max; }
                hist_add(hist, bits >> 20, counted);
            } else if (LEVEL == 1) {
                hist_add(hist, (bits >> 10) & 1023u, counted && (bits >> 20) == pfx0);
                if (!same) hist_add(hist + kBins12, (bits >> 10) & 1023u, counted && (bits >> 20) == pfx1);
            } else {
                hist_add(hist, bits & 1023u, counted && (bits >> 10) == pfx0);
                if (!same) hist_add(hist + kBins12, bits & 1023u, counted && (bits >> 10) == pfx1);
            }
        }
    }
    if (LEVEL == 0) {
        // wave reduction of count / max, then one LDS atomic per wave
        for (int off = 32; off > 0; off >>= 1) {
            my_count += (uint32_t)__shfl_xor((int)my_count, off);
            const uint32_t o = (uint32_t)__shfl_xor((int)my_max, off);
            my_max = o > my_max ? o : my_max;
        }
        if (__lane_id() == 0) { atomicAdd(&s_count, my_count); atomicMax(&s_max, my_max); }
    }
    __syncthreads();
    uint32_t* gh = ws + (LEVEL == 0 ? 0 : (LEVEL == 1 ? kOffH1 : kOffH2));
    const int used = LEVEL == 0 ? kBins0 : (same ? kBins12 : 2 * kBins12);
    for (int i = threadIdx.x; i < used; i += kThreads) {
        const uint32_t c = hist[i];
        if (c) atomicAdd(&gh[i], c);
    }
    if (LEVEL == 0 && threadIdx.x == 0) {
        if (s_count) atomicAdd(&ws[kOffMeta + M_COUNT], s_count);
        atomicMax(&ws[kOffMeta + M_MAX], s_max);
    }
}

// the bin of `hist[0 .. nb)` holding 0-based rank `rank` and the rank left inside it (block-wide: 256 threads, nb / 256 bins each)
__device__ void find_bin(const uint32_t* hist, int nb, uint32_t rank, uint32_t* s_part, uint32_t* out_bin, uint32_t* out_left) {
    const int per = nb / kThreads;
    uint32_t sum = 0u;
    for (int i = 0; i < per; ++i) sum += hist[threadIdx.x * per + i];
    s_part[threadIdx.x] = sum;
    __syncthreads();
    for (int off = 1; off < kThreads; off <<= 1) {            // inclusive Hillis-Steele scan
        const uint32_t v = threadIdx.x >= (unsigned)off ? s_part[threadIdx.x - off] : 0u;
        __syncthreads();
        s_part[threadIdx.x] += v;
        __syncthreads();
    }
    const uint32_t incl = s_part[threadIdx.x];
    const uint32_t excl = incl - sum;
    if (rank >= excl && rank < incl) {                          // exactly one thread
        uint32_t c = excl;
        for (int i = 0; i < per; ++i) {
            const uint32_t h = hist[threadIdx.x * per + i];
            if (rank < c + h) { *out_bin = (uint32_t)(threadIdx.x * per + i); *out_left = rank - c; break; }
            c += h;
        }
    }
    __syncthreads();
}

// numpy 2.2.6 np.percentile(m, 99) of n fp32 values, 'linear': q = float32(0.99) (99 / float32(100)); the virtual index
// (n - 1) * q in fp32; previous = floor, next = previous + 1, both the last index when the virtual index is >= n - 1.
struct VIndex {
    float vi;
    uint32_t k0, k1;
    float gamma;
};

__device__ __forceinline__ VIndex virtual_index(uint32_t n) {
    VIndex r;
    const float q = 99.0f / 100.0f;
    r.vi = (float)(n - 1u) * q;
    const double prev = floor((double)r.vi);
    if (r.vi >= (float)(n - 1u)) {                               // indexes_above_bounds: both -1
        r.k0 = r.k1 = n - 1u;
        r.gamma = (float)((double)r.vi - (-1.0));               // _get_gamma sees the -1 (its value cannot matter: b - a = 0)
    } else {
        r.k0 = (uint32_t)prev;
        r.k1 = r.k0 + 1u;
        r.gamma = (float)((double)r.vi - prev);
    }
    return r;
}

// numpy's _lerp in fp32: a + (b - a) * t, or b - (b - a) * (1 - t) where t >= 0.5
__device__ __forceinline__ float np_lerp(float a, float b, float t) {
    const float d = b - a;
    if (t >= 0.5f) return b - d * (1.0f - t);
    return a + d * t;
}

// LEVEL 0 / 1: choose the bin of both targets at this level, extend their prefixes.  LEVEL 2: the two order statistics are
// known: lerp, the `> 0` / max / 1 fallback, range_max as float64.
template <int LEVEL>
__global__ void __launch_bounds__(kThreads) vis_range_select_kernel(RangeParams p) {
    __shared__ uint32_t s_part[kThreads];
    __shared__ uint32_t s_bin[2], s_left[2];
    const int img = blockIdx.x;
    uint32_t* ws = p.ws + (int64_t)img * kWsInts;
    uint32_t* meta = ws + kOffMeta;
    const uint32_t n = meta[M_COUNT];
    if (LEVEL == 0 && threadIdx.x == 0 && p.counts) p.counts[img] = (int32_t)n;
    if (n == 0u) {                                               // (the host raises numpy's IndexError for it)
        if (LEVEL == 2 && threadIdx.x == 0) p.range_max[img] = 1.0;
        return;
    }
    uint32_t rank0, rank1;
    const VIndex vx = virtual_index(n);
    if (LEVEL == 0) {
        rank0 = vx.k0; rank1 = vx.k1;
    } else {
        rank0 = meta[M_RANK]; rank1 = meta[M_RANK + 1];
    }
    const uint32_t pfx0 = meta[M_PFX], pfx1 = meta[M_PFX + 1];
    const bool same = LEVEL == 0 || pfx0 == pfx1;
    const uint32_t* h0 = ws + (LEVEL == 0 ? 0 : (LEVEL == 1 ? kOffH1 : kOffH2));
    const uint32_t* h1 = same ? h0 : h0 + kBins12;
    const int nb = LEVEL == 0 ? kBins0 : kBins12;
    find_bin(h0, nb, rank0, s_part, &s_bin[0], &s_left[0]);
    find_bin(h1, nb, rank1, s_part, &s_bin[1], &s_left[1]);
    if (threadIdx.x != 0) return;
    uint32_t np0, np1;
    if (LEVEL == 0) {
        np0 = s_bin[0]; np1 = s_bin[1];
    } else {
        np0 = (pfx0 << 10) | s_bin[0]; np1 = (pfx1 << 10) | s_bin[1];
    }
    if (LEVEL < 2) {
        meta[M_PFX] = np0; meta[M_PFX + 1] = np1;
        meta[M_RANK] = s_left[0]; meta[M_RANK + 1] = s_left[1];
        return;
    }
    const float a = __uint_as_float(np0), b = __uint_as_float(np1);
    const float pct = np_lerp(a, b, vx.gamma);
    const float mx = __uint_as_float(meta[M_MAX]);
    double r;
    if (pct > 0.0f) r = (double)pct;
    else if (mx > 0.0f) r = (double)mx;
    else r = 1.0;
    p.range_max[img] = r;
}

// ---- the colour kernel ------------------------------------------------------------------------------------------------
struct ColourParams {
    const void* flow;
    int64_t flow_bs;
    const uint8_t* mask;   // nullptr: all True
    int64_t mask_bs;
    const double* range_max;
    uint8_t* out;
    int32_t n, h, w;
    int64_t hw;
    int vec;               // H*W % 4 == 0, aligned planes and output
    int show_mask, borders;
    int mode;              // 0 hsv, 1 rgb, 2 bgr
    int layout;            // 0 N-3-H-W planes, 1 N-H-W-3
};

__device__ __forceinline__ bool mask_at(const ColourParams& p, int img, int64_t q) {
    return p.mask == nullptr || p.mask[img * p.mask_bs + q] != 0;
}

// findContours(RETR_TREE, CHAIN_APPROX_SIMPLE) + drawContours(..., thickness 1) on the 0-framed mask: the True pixels with a
// 4-neighbour that is False or outside the image
__device__ __forceinline__ bool on_border(const ColourParams& p, int img, int64_t q) {
    if (!mask_at(p, img, q)) return false;
    const int64_t r = q / p.w, c = q - r * p.w;
    if (r == 0 || c == 0 || r == p.h - 1 || c == p.w - 1) return true;
    return !mask_at(p, img, q - 1) || !mask_at(p, img, q + 1) || !mask_at(p, img, q - p.w) || !mask_at(p, img, q + p.w);
}

// the three bytes of one pixel
__device__ __forceinline__ void colour_pixel(const ColourParams& p, float x, float y, bool valid, bool border, double rmax,
                                             uint8_t o[3]) {
    x = thr(x);
    y = thr(y);
    const float mag = cart_mag(x, y);
    float ang = cart_angle(x, y);
    // np.mod(ang, 360) / 2: the angle lies in [0, 360] (360.0f only from 360 - a with a below half an ulp)
    float hue = (ang >= 360.0f ? ang - 360.0f : ang) / 2.0f;
    float val = (p.show_mask && !valid) ? 180.0f : 255.0f;
    // np.clip(mag * 255 / range_max, 0, 255): the product in fp32, the division in float64, stored as fp32
    const double s64 = (double)(mag * 255.0f) / rmax;
    float sat = (float)fmin(fmax(s64, 0.0), 255.0);
    if (border) { hue = 0.0f; sat = 0.0f; val = 0.0f; }
    if (p.mode == 0) {
        o[0] = (uint8_t)rintf(hue); o[1] = (uint8_t)rintf(sat); o[2] = (uint8_t)rintf(val);
        return;
    }
    // flow_class.py:1333-1349: h, s, v in fp32; i = int(h * 6.) (fp32 product), f = h * 6. - i in float64
    const float h = hue / 180.0f, s = sat / 255.0f, v = val / 255.0f;
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
    // the `order` table: 0:v 1:p 2:q 3:t
    int r0, r1, r2;
    switch ((int)i) {
        case 0: r0 = 0; r1 = 3; r2 = 1; break;
        case 1: r0 = 2; r1 = 0; r2 = 1; break;
        case 2: r0 = 1; r1 = 0; r2 = 3; break;
        case 3: r0 = 1; r1 = 2; r2 = 0; break;
        case 4: r0 = 3; r1 = 1; r2 = 0; break;
        default: r0 = 0; r1 = 1; r2 = 2; break;
    }
    const uint8_t a0 = (uint8_t)rint(c[r0] * 255.0), a1 = (uint8_t)rint(c[r1] * 255.0), a2 = (uint8_t)rint(c[r2] * 255.0);
    if (p.mode == 2) { o[0] = a2; o[1] = a1; o[2] = a0; }
    else { o[0] = a0; o[1] = a1; o[2] = a2; }
}

template <bool HALF>
__global__ void __launch_bounds__(kThreads) vis_colour_kernel(ColourParams p) {
    const int img = blockIdx.y;
    const int64_t quads = (p.hw + 3) / 4;
    const int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (q >= quads) return;
    const int64_t p0 = 4 * q;
    const Loader<HALF> L{p.flow, p.flow_bs, p.hw};
    float x[4], y[4];
    L.ld4(img, 0, p0, p.vec, x);
    L.ld4(img, 1, p0, p.vec, y);
    const double rmax = p.range_max[img];
    uint8_t o[4][3];
    for (int k = 0; k < 4; ++k) {
        const bool exists = p0 + k < p.hw;
        const bool valid = !exists || !p.show_mask || mask_at(p, img, p0 + k);
        const bool border = exists && p.borders && on_border(p, img, p0 + k);
        colour_pixel(p, x[k], y[k], valid, border, rmax, o[k]);
    }
    if (p.layout == 0) {                                         // N-3-H-W
        uint8_t* base = p.out + (int64_t)img * 3 * p.hw + p0;
        for (int ch = 0; ch < 3; ++ch) {
            if (p.vec) {
                const uint32_t word = (uint32_t)o[0][ch] | ((uint32_t)o[1][ch] << 8) | ((uint32_t)o[2][ch] << 16) | ((uint32_t)o[3][ch] << 24);
                *reinterpret_cast<uint32_t*>(base + ch * p.hw) = word;
            } else {
                for (int k = 0; k < 4; ++k) if (p0 + k < p.hw) base[ch * p.hw + k] = o[k][ch];
            }
        }
    } else {                                                     // N-H-W-3
        uint8_t* base = p.out + ((int64_t)img * p.hw + p0) * 3;
        if (p.vec) {
            uint32_t wd[3] = {0u, 0u, 0u};
            for (int b = 0; b < 12; ++b) wd[b >> 2] |= (uint32_t)o[b / 3][b % 3] << (8 * (b & 3));
            uint32_t* dst = reinterpret_cast<uint32_t*>(base);
            dst[0] = wd[0]; dst[1] = wd[1]; dst[2] = wd[2];
        } else {
            for (int k = 0; k < 4; ++k)
                if (p0 + k < p.hw) { base[3 * k] = o[k][0]; base[3 * k + 1] = o[k][1]; base[3 * k + 2] = o[k][2]; }
        }
    }
}

int dims_ok(int32_t n, int32_t h, int32_t w) {
    if (n < 1 || h < 1 || w < 1 || n > 65535) return OFL_E_SHAPE;
    if ((int64_t)h * w >= (1ll << 31)) return OFL_E_SHAPE;
    return OFL_OK;
}

bool aligned(const void* ptr, int a) { return ((uintptr_t)ptr % (uintptr_t)a) == 0; }

}  // namespace

extern "C" {

__attribute__((visibility("default"))) int64_t ofl_visualise_workspace_ints(int32_t n) {
    if (n < 1 || n > 65535) return OFL_E_SHAPE;
    return (int64_t)n * kWsInts;
}

__attribute__((visibility("default"))) int ofl_visualise_range_f32(const void* flow, int64_t flow_bs, int32_t flow_half,
                                                                   const uint8_t* mask, int64_t mask_bs, int32_t* workspace,
                                                                   double* range_max, int32_t* counts, int32_t n, int32_t h,
                                                                   int32_t w, void* stream) {
    if (!flow || !workspace || !range_max) return OFL_E_NULL;
    int rc = dims_ok(n, h, w);
    if (rc) return rc;
    if (flow_half != 0 && flow_half != 1) return OFL_E_ARG;
    if (flow_bs < 0 || mask_bs < 0) return OFL_E_ARG;
    RangeParams p;
    p.flow = flow; p.flow_bs = flow_bs; p.mask = mask; p.mask_bs = mask_bs; p.ws = reinterpret_cast<uint32_t*>(workspace);
    p.range_max = range_max; p.counts = counts; p.n = n; p.h = h; p.w = w; p.hw = (int64_t)h * w;
    const int elem = flow_half ? 2 : 4;
    p.vec = (p.hw % 4 == 0) && (flow_bs % 4 == 0) && aligned(flow, 4 * elem);
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(workspace, 0, (size_t)n * kWsInts * sizeof(int32_t), s);
    if (e != hipSuccess) return (int)e;
    const int64_t quads = (p.hw + 3) / 4;
    const unsigned bx = (unsigned)((quads + (int64_t)kThreads * kQuadsPerThread - 1) / ((int64_t)kThreads * kQuadsPerThread));
    const dim3 grid(bx, (unsigned)n), block(kThreads);
    if (flow_half) {
        hipLaunchKernelGGL((vis_range_hist_kernel<true, 0>), grid, block, 0, s, p);
        hipLaunchKernelGGL(vis_range_select_kernel<0>, dim3(n), block, 0, s, p);
        hipLaunchKernelGGL((vis_range_hist_kernel<true, 1>), grid, block, 0, s, p);
        hipLaunchKernelGGL(vis_range_select_kernel<1>, dim3(n), block, 0, s, p);
        hipLaunchKernelGGL((vis_range_hist_kernel<true, 2>), grid, block, 0, s, p);
    } else {
        hipLaunchKernelGGL((vis_range_hist_kernel<false, 0>), grid, block, 0, s, p);
        hipLaunchKernelGGL(vis_range_select_kernel<0>, dim3(n), block, 0, s, p);
        hipLaunchKernelGGL((vis_range_hist_kernel<false, 1>), grid, block, 0, s, p);
        hipLaunchKernelGGL(vis_range_select_kernel<1>, dim3(n), block, 0, s, p);
        hipLaunchKernelGGL((vis_range_hist_kernel<false, 2>), grid, block, 0, s, p);
    }
    hipLaunchKernelGGL(vis_range_select_kernel<2>, dim3(n), block, 0, s, p);
    return (int)hipGetLastError();
}

__attribute__((visibility("default"))) int ofl_visualise_u8(const void* flow, int64_t flow_bs, int32_t flow_half,
                                                            const uint8_t* mask, int64_t mask_bs, int32_t show_mask,
                                                            int32_t show_mask_borders, const double* range_max, int32_t mode,
                                                            int32_t layout, uint8_t* out, int32_t n, int32_t h, int32_t w,
                                                            void* stream) {
    if (!flow || !range_max || !out) return OFL_E_NULL;
    int rc = dims_ok(n, h, w);
    if (rc) return rc;
    if (flow_half != 0 && flow_half != 1) return OFL_E_ARG;
    if (mode < 0 || mode > 2 || layout < 0 || layout > 1) return OFL_E_ARG;
    if (show_mask != 0 && show_mask != 1) return OFL_E_ARG;
    if (show_mask_borders != 0 && show_mask_borders != 1) return OFL_E_ARG;
    if (flow_bs < 0 || mask_bs < 0) return OFL_E_ARG;
    ColourParams p;
    p.flow = flow; p.flow_bs = flow_bs; p.mask = mask; p.mask_bs = mask_bs; p.range_max = range_max; p.out = out;
    p.n = n; p.h = h; p.w = w; p.hw = (int64_t)h * w; p.show_mask = show_mask; p.borders = show_mask_borders;
    p.mode = mode; p.layout = layout;
    const int elem = flow_half ? 2 : 4;
    p.vec = (p.hw % 4 == 0) && (flow_bs % 4 == 0) && aligned(flow, 4 * elem) && aligned(out, 4);
    const int64_t quads = (p.hw + 3) / 4;
    const dim3 grid((unsigned)((quads + kThreads - 1) / kThreads), (unsigned)n), block(kThreads);
    if (flow_half) hipLaunchKernelGGL(vis_colour_kernel<true>, grid, block, 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(vis_colour_kernel<false>, grid, block, 0, (hipStream_t)stream, p);
    return (int)hipGetLastError();
}

}  // extern "C"
