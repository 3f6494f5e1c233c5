// ofl_matrix.hip -- Flow.matrix (flow_class.py:1566-1646) on gfx950: a similarity (dof 4), an affine map (dof 6) or a homography
// (dof 8) fitted to the point pairs of a flow field, by least squares ('lms') or by a robust search over K fixed hypotheses
// ('ransac', 'lmeds') followed by one least-squares fit of the winner's inliers.  The definition is DESIGN.md section 3.10 (restated, not
// checked against OpenCV); tests/matrix_oracle.py is the same definition in NumPy.
//
//   mat_rowcount_kernel / mat_init_kernel   valid pixels per row, their prefix sums, n_valid, status "too few points"
//   mat_hyp_kernel                          one thread per (image, k): draws m pixels, solves the minimal system in float64
//   mat_score_kernel                        RANSAC: inlier counts of the K hypotheses, fp32 residuals, integer atomics only
//   mat_hist_kernel / mat_select_kernel     LMedS: the exact median residual of every hypothesis by a radix select (11 + 10 + 10 bits)
//   mat_winner_kernel                       arg max count / arg min median, lowest k on ties; the model and threshold of the refit
//   mat_sums_kernel / mat_finish_kernel     the float64 sums of a least-squares fit (over all valid pixels, or over the inliers
//                                           of a model) as per-block partials added in index order, and the solve
//
// No float atomics; the block-to-pixel assignment depends on (H, W) only; nothing is indexed or seeded by the image: the result
// of image i is bitwise independent of the batch.  C ABI: include/oflib_hip.h.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "oflib_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kQuadsPerThread = 16;                   // 256 threads x 16 quads = 16 384 pixels per block
constexpr int kBlockQuads = kThreads * kQuadsPerThread;
constexpr int kNS = 24;                               // sums per block slot (14 used by the first pass, 24 by the DLT pass)
constexpr int kKRansac = 256, kKLmeds = 128;          // hypotheses per image
constexpr int kG = 4;                                 // LMedS: hypotheses per histogram block (4 x 2048 x 4 B = 32 KB of LDS)
constexpr int kBins = 2048;                           // level 0: bits 30..20; levels 1 / 2: two targets x 1024 bins (19..10, 9..0)
constexpr int kHypStride = 12;                        // nine fp32 entries, threshold / padding
constexpr uint64_t kSeed = 0x0F1E2D3C4B5A6978ull;
constexpr float kRansacThr = 9.0f;                    // 3 px, squared
enum { METHOD_LMS = 0, METHOD_RANSAC = 1, METHOD_LMEDS = 2 };
enum { ST_OK = 0, ST_FEW_POINTS = 1, ST_NO_HYPOTHESIS = 2, ST_REFIT_SINGULAR = 3 };
enum { I_NVALID = 0, I_WINNER = 1, I_INLIERS = 2, I_STATUS = 3 };

struct MatParams {
    const void* flow;
    int64_t flow_bs;
    const uint8_t* mask;     // nullptr: every pixel counts
    int64_t mask_bs;
    int32_t n, h, w;
    int64_t hw;
    int vec, ref_s, dof, m, method, K, nblk;
    int pass;                // sums / finish: 0 first- and second-order sums, 1 the DLT sums in normalised coordinates
    int use_pred;            // sums: only pixels whose residual under model[img] is <= its threshold
    double cx, cy;           // the shift of the least-squares coordinates: the image centre
    double* partial;         // [n][nblk][kNS]
    double* norm;            // [n][8]: mean x, mean y, scale of src; the same of dst
    float* model;            // [n][kHypStride]: the winner, [9] its threshold
    float* hyp;              // [n][K][kHypStride]
    int32_t* hvalid;         // [n][K]
    uint32_t* score;         // [n][K]: inlier count (RANSAC) / bits of the median (LMedS)
    int32_t* rowoff;         // [n][h + 1]: valid pixels before row r (masked only)
    uint32_t* hist;          // [n][K][kBins]
    uint32_t* meta;          // [n][K][4]: prefix of target 0 / 1, rank left of target 0 / 1
    int32_t* info;           // [n][4]: n_valid, winner k, inliers, status
    double* out;             // [n][9]
};

// ---- loads (as in ofl_visualise.hip): four consecutive pixels of one plane ------------------------------------------------
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

// the point pair of pixel q with vector (u, v), in float64 (flow_class.py:1600-1610)
__device__ __forceinline__ void make_pair(const MatParams& p, uint32_t q, float u, float v, double& sx, double& sy, double& dx,
                                          double& dy) {
    const uint32_t r = q / (uint32_t)p.w, c = q - r * (uint32_t)p.w;
    const double gx = (double)c, gy = (double)r;
    if (p.ref_s) { sx = gx; sy = gy; dx = gx + (double)u; dy = gy + (double)v; }
    else { dx = gx; dy = gy; sx = gx - (double)u; sy = gy - (double)v; }
}

// the fp32 squared reprojection residual, in THE operation order of DESIGN.md 3.10; not finite -> +inf
template <bool PROJ>
__device__ __forceinline__ float resid(const float* hm, float sx, float sy, float dx, float dy) {
    float px = (hm[0] * sx + hm[1] * sy) + hm[2];
    float py = (hm[3] * sx + hm[4] * sy) + hm[5];
    if (PROJ) {
        const float wz = (hm[6] * sx + hm[7] * sy) + hm[8];
        px = px / wz;
        py = py / wz;
    }
    const float ex = px - dx, ey = py - dy;
    const float r = ex * ex + ey * ey;
    return (r <= FLT_MAX) ? r : __uint_as_float(0x7f800000u);
}

// the tile of one thread: four pixels as fp32 point pairs and their valid bits
template <bool HALF>
__device__ __forceinline__ uint32_t load_tile(const MatParams& p, const Loader<HALF>& L, int img, int64_t q, int64_t quads,
                                              float sx[4], float sy[4], float dx[4], float dy[4]) {
    uint32_t bits = 0u;
    float u[4] = {0.f, 0.f, 0.f, 0.f}, v[4] = {0.f, 0.f, 0.f, 0.f};
    const int64_t p0 = 4 * q;
    if (q < quads) {
        L.ld4(img, 0, p0, p.vec, u);
        L.ld4(img, 1, p0, p.vec, v);
        for (int k = 0; k < 4; ++k) {
            const bool exists = p0 + k < p.hw;
            if (exists && (p.mask == nullptr || p.mask[img * p.mask_bs + p0 + k] != 0)) bits |= 1u << k;
        }
    }
    for (int k = 0; k < 4; ++k) {
        double a, b, c, d;
        make_pair(p, (uint32_t)(p0 + k), u[k], v[k], a, b, c, d);
        sx[k] = (float)a; sy[k] = (float)b; dx[k] = (float)c; dy[k] = (float)d;
    }
    return bits;
}

// ---- valid pixels per row, prefix sums, n_valid ---------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) mat_rowcount_kernel(MatParams p) {
    const int img = blockIdx.y;
    const int row = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (row >= p.h) return;                                       // (wave-uniform)
    const uint8_t* mrow = p.mask + img * p.mask_bs + (int64_t)row * p.w;
    int c = 0;
    for (int x = threadIdx.x & 63; x < p.w; x += 64) c += mrow[x] != 0;
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
    if ((threadIdx.x & 63) == 0) p.rowoff[(int64_t)img * (p.h + 1) + row + 1] = c;
}

// one block per image: rowoff[r + 1] becomes the count of valid pixels in rows 0 .. r; n_valid; status
__global__ void __launch_bounds__(kThreads) mat_init_kernel(MatParams p) {
    __shared__ int s_part[kThreads];
    const int img = blockIdx.x;
    int total;
    if (p.mask == nullptr) {
        total = (int)p.hw;
    } else {
        int32_t* ro = p.rowoff + (int64_t)img * (p.h + 1);
        const int per = (p.h + kThreads - 1) / kThreads;
        const int r0 = threadIdx.x * per, r1 = min(r0 + per, p.h);
        int sum = 0;
        for (int r = r0; r < r1; ++r) sum += ro[r + 1];
        s_part[threadIdx.x] = sum;
        __syncthreads();
        for (int off = 1; off < kThreads; off <<= 1) {
            const int v = threadIdx.x >= (unsigned)off ? s_part[threadIdx.x - off] : 0;
            __syncthreads();
            s_part[threadIdx.x] += v;
            __syncthreads();
        }
        int run = s_part[threadIdx.x] - sum;
        for (int r = r0; r < r1; ++r) { run += ro[r + 1]; ro[r + 1] = run; }
        total = s_part[kThreads - 1];
    }
    if (threadIdx.x == 0) {
        p.info[img * 4 + I_NVALID] = total;
        p.info[img * 4 + I_WINNER] = -1;
        if (total < p.m) p.info[img * 4 + I_STATUS] = ST_FEW_POINTS;
    }
}

// ---- hypotheses -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t draw_hash(uint32_t k, uint32_t j) {        // splitmix64 of a counter
    uint64_t z = kSeed + (uint64_t)(k * 8u + j + 1u) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// the r-th valid pixel of image img in row-major order
__device__ uint32_t locate(const MatParams& p, int img, uint32_t r) {
    if (p.mask == nullptr) return r;
    const int32_t* ro = p.rowoff + (int64_t)img * (p.h + 1);
    int lo = 0, hi = p.h - 1;                                    // the row with ro[row] <= r < ro[row + 1]
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((uint32_t)ro[mid + 1] > r) hi = mid; else lo = mid + 1;
    }
    uint32_t left = r - (uint32_t)ro[lo];
    const uint8_t* mrow = p.mask + img * p.mask_bs + (int64_t)lo * p.w;
    int x = 0;
    for (; x < p.w - 1; ++x) {
        if (mrow[x] != 0) {
            if (left == 0u) break;
            --left;
        }
    }
    return (uint32_t)lo * (uint32_t)p.w + (uint32_t)x;
}

// |cross| of (b - a) and (c - a) against the size of its two products
__device__ __forceinline__ bool collinear(double ax, double ay, double bx, double by, double cx, double cy) {
    const double t1 = (bx - ax) * (cy - ay), t2 = (by - ay) * (cx - ax);
    return fabs(t1 - t2) <= 1e-6 * (fabs(t1) + fabs(t2));
}

// Gaussian elimination with partial pivoting, NR right-hand sides, in THE order of DESIGN.md 3.10: for each column the pivot is
// the first row of largest |a|; rows are swapped; each lower row i gets f = a[i][col] / a[col][col], then a[i][j] -= f * a[col][j]
// for j = col + 1 .. N - 1 and b[i][r] -= f * b[col][r]; back substitution from the last row, s -= a[i][j] * x[j] for j ascending,
// x[i] = s / a[i][i].  false: a zero or non-finite pivot.
template <int N, int NR>
__device__ bool gauss_solve(double* a, double* b, double* x) {
    for (int col = 0; col < N; ++col) {
        int piv = col;
        double best = fabs(a[col * N + col]);
        for (int i = col + 1; i < N; ++i) {
            const double v = fabs(a[i * N + col]);
            if (v > best) { best = v; piv = i; }
        }
        if (!(best > 0.0) || !(best <= DBL_MAX)) return false;
        if (piv != col) {
            for (int j = 0; j < N; ++j) { const double t = a[col * N + j]; a[col * N + j] = a[piv * N + j]; a[piv * N + j] = t; }
            for (int r = 0; r < NR; ++r) { const double t = b[col * NR + r]; b[col * NR + r] = b[piv * NR + r]; b[piv * NR + r] = t; }
        }
        for (int i = col + 1; i < N; ++i) {
            const double f = a[i * N + col] / a[col * N + col];
            for (int j = col + 1; j < N; ++j) a[i * N + j] -= f * a[col * N + j];
            for (int r = 0; r < NR; ++r) b[i * NR + r] -= f * b[col * NR + r];
        }
    }
    for (int r = 0; r < NR; ++r) {
        for (int i = N - 1; i >= 0; --i) {
            double s = b[i * NR + r];
            for (int j = i + 1; j < N; ++j) s -= a[i * N + j] * x[j * NR + r];
            x[i * NR + r] = s / a[i * N + i];
        }
    }
    return true;
}

template <bool HALF>
__global__ void __launch_bounds__(64) mat_hyp_kernel(MatParams p) {
    const int img = blockIdx.y;
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= p.K) return;
    float* hout = p.hyp + ((int64_t)img * p.K + k) * kHypStride;
    int32_t* vout = p.hvalid + (int64_t)img * p.K + k;
    for (int i = 0; i < kHypStride; ++i) hout[i] = 0.0f;
    *vout = 0;
    if (p.info[img * 4 + I_STATUS] != ST_OK) return;
    const uint32_t nv = (uint32_t)p.info[img * 4 + I_NVALID];
    const Loader<HALF> L{p.flow, p.flow_bs, p.hw};
    const int m = p.m;
    uint32_t q[4];
    double sx[4], sy[4], dx[4], dy[4];
    for (int j = 0; j < m; ++j) {
        q[j] = locate(p, img, (uint32_t)(draw_hash((uint32_t)k, (uint32_t)j) % (uint64_t)nv));
        make_pair(p, q[j], L.ld(img, 0, q[j]), L.ld(img, 1, q[j]), sx[j], sy[j], dx[j], dy[j]);
    }
    for (int j = 1; j < m; ++j)
        for (int i = 0; i < j; ++i)
            if (q[i] == q[j]) return;
    for (int c = 2; c < m; ++c)
        for (int b = 1; b < c; ++b)
            for (int a = 0; a < b; ++a)
                if (collinear(sx[a], sy[a], sx[b], sy[b], sx[c], sy[c]) || collinear(dx[a], dy[a], dx[b], dy[b], dx[c], dy[c])) return;
    double hm[9] = {0, 0, 0, 0, 0, 0, 0, 0, 1};
    if (m == 2) {
        const double ex = sx[1] - sx[0], ey = sy[1] - sy[0], fu = dx[1] - dx[0], fv = dy[1] - dy[0];
        const double den = ex * ex + ey * ey;
        if (!(den > 0.0)) return;
        const double a = (ex * fu + ey * fv) / den, b = (ex * fv - ey * fu) / den;
        hm[0] = a; hm[1] = -b; hm[2] = dx[0] - (a * sx[0] - b * sy[0]);
        hm[3] = b; hm[4] = a; hm[5] = dy[0] - (b * sx[0] + a * sy[0]);
    } else if (m == 3) {
        double a[9], b[6], x[6];
        for (int j = 0; j < 3; ++j) {
            a[j * 3] = sx[j]; a[j * 3 + 1] = sy[j]; a[j * 3 + 2] = 1.0;
            b[j * 2] = dx[j]; b[j * 2 + 1] = dy[j];
        }
        if (!gauss_solve<3, 2>(a, b, x)) return;
        hm[0] = x[0]; hm[1] = x[2]; hm[2] = x[4];
        hm[3] = x[1]; hm[4] = x[3]; hm[5] = x[5];
    } else {
        // h33 = 1: rows [x y 1 0 0 0 -ux -uy] = u and [0 0 0 x y 1 -vx -vy] = v for each of the four pairs
        double a[64], b[8], x[8];
        for (int j = 0; j < 4; ++j) {
            double* r0 = a + (2 * j) * 8;
            double* r1 = a + (2 * j + 1) * 8;
            r0[0] = sx[j]; r0[1] = sy[j]; r0[2] = 1.0; r0[3] = 0.0; r0[4] = 0.0; r0[5] = 0.0; r0[6] = -(dx[j] * sx[j]); r0[7] = -(dx[j] * sy[j]);
            r1[0] = 0.0; r1[1] = 0.0; r1[2] = 0.0; r1[3] = sx[j]; r1[4] = sy[j]; r1[5] = 1.0; r1[6] = -(dy[j] * sx[j]); r1[7] = -(dy[j] * sy[j]);
            b[2 * j] = dx[j]; b[2 * j + 1] = dy[j];
        }
        if (!gauss_solve<8, 1>(a, b, x)) return;
        for (int i = 0; i < 8; ++i) hm[i] = x[i];
    }
    bool fin = true;
    for (int i = 0; i < 9; ++i) fin = fin && (fabs(hm[i]) <= (double)FLT_MAX);
    if (!fin) return;
    for (int i = 0; i < 9; ++i) hout[i] = (float)hm[i];
    *vout = 1;
}

// ---- RANSAC scoring -------------------------------------------------------------------------------------------------------
// Each block walks its 16 384 pixels in steps of 1024 (four per thread, in registers) and scores all K hypotheses, held in
// LDS, on each step.  A wave's counts live in K / 64 registers per lane (lane l of register j: hypothesis 64 j + l), so the
// hypothesis loop touches neither LDS (beyond the broadcast read of nine floats) nor global memory.
template <bool HALF, bool PROJ, int K>
__global__ void __launch_bounds__(kThreads) mat_score_kernel(MatParams p) {
    __shared__ float s_h[K * kHypStride];
    const int img = blockIdx.y;
    if (p.info[img * 4 + I_STATUS] != ST_OK) return;              // (block-uniform)
    const float* hsrc = p.hyp + (int64_t)img * K * kHypStride;
    for (int i = threadIdx.x; i < K * kHypStride; i += kThreads) s_h[i] = hsrc[i];
    __syncthreads();
    const Loader<HALF> L{p.flow, p.flow_bs, p.hw};
    const int64_t quads = (p.hw + 3) / 4;
    const int64_t q_begin = (int64_t)blockIdx.x * kBlockQuads;
    const int lane = threadIdx.x & 63;
    uint32_t cnt[K / 64];
    for (int j = 0; j < K / 64; ++j) cnt[j] = 0u;
    for (int it = 0; it < kQuadsPerThread; ++it) {
        if (q_begin + (int64_t)it * kThreads >= quads) break;     // (block-uniform)
        float sx[4], sy[4], dx[4], dy[4];
        const uint32_t bits = load_tile<HALF>(p, L, img, q_begin + (int64_t)it * kThreads + threadIdx.x, quads, sx, sy, dx, dy);
#pragma unroll
        for (int j = 0; j < K / 64; ++j) {
            for (int kk = 0; kk < 64; ++kk) {
                const float* hm = s_h + (j * 64 + kk) * kHypStride;
                uint32_t c = 0u;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const bool inl = ((bits >> e) & 1u) && resid<PROJ>(hm, sx[e], sy[e], dx[e], dy[e]) <= kRansacThr;
                    c += (uint32_t)__popcll(__ballot(inl));
                }
                cnt[j] += (lane == kk) ? c : 0u;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < K / 64; ++j)
        if (cnt[j]) atomicAdd(&p.score[(int64_t)img * K + j * 64 + lane], cnt[j]);
}

// ---- LMedS medians --------------------------------------------------------------------------------------------------------
// one LDS histogram add per lane; a wave whose active lanes all name one bin adds once (as in ofl_visualise.hip)
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

// grid (pixel blocks, K / kG, N).  LEVEL 0: bits 30..20 of every valid pixel's residual under each of the group's kG hypotheses;
// LEVEL 1 / 2: bits 19..10 / 9..0 of the residuals whose higher bits equal the prefix of target 0 (bins 0..1023) / target 1
// (bins 1024..2047, only when the prefixes differ).  Residuals are recomputed, never stored.
template <bool HALF, bool PROJ, int LEVEL>
__global__ void __launch_bounds__(kThreads) mat_hist_kernel(MatParams p) {
    __shared__ uint32_t hist[kG * kBins];
    __shared__ float s_h[kG * kHypStride];
    __shared__ uint32_t s_pfx[kG * 2];
    const int img = blockIdx.z;
    if (p.info[img * 4 + I_STATUS] != ST_OK) return;              // (block-uniform)
    const int k0 = blockIdx.y * kG;
    for (int i = threadIdx.x; i < kG * kBins; i += kThreads) hist[i] = 0u;
    if (threadIdx.x < kG * kHypStride) s_h[threadIdx.x] = p.hyp[((int64_t)img * p.K + k0) * kHypStride + threadIdx.x];
    if (threadIdx.x < kG * 2) s_pfx[threadIdx.x] = p.meta[((int64_t)img * p.K + k0 + (threadIdx.x >> 1)) * 4 + (threadIdx.x & 1)];
    __syncthreads();
    const Loader<HALF> L{p.flow, p.flow_bs, p.hw};
    const int64_t quads = (p.hw + 3) / 4;
    const int64_t q_begin = (int64_t)blockIdx.x * kBlockQuads;
    for (int it = 0; it < kQuadsPerThread; ++it) {
        if (q_begin + (int64_t)it * kThreads >= quads) break;     // (block-uniform)
        float sx[4], sy[4], dx[4], dy[4];
        const uint32_t bits = load_tile<HALF>(p, L, img, q_begin + (int64_t)it * kThreads + threadIdx.x, quads, sx, sy, dx, dy);
        for (int g = 0; g < kG; ++g) {
            const float* hm = s_h + g * kHypStride;
            uint32_t* hg = hist + g * kBins;
            const uint32_t pfx0 = s_pfx[2 * g], pfx1 = s_pfx[2 * g + 1];
            const bool same = pfx0 == pfx1;
            for (int e = 0; e < 4; ++e) {
                const bool valid = (bits >> e) & 1u;
                const uint32_t rb = __float_as_uint(resid<PROJ>(hm, sx[e], sy[e], dx[e], dy[e]));
                if (LEVEL == 0) {
                    hist_add(hg, rb >> 20, valid);
                } else if (LEVEL == 1) {
                    hist_add(hg, (rb >> 10) & 1023u, valid && (rb >> 20) == pfx0);
                    if (!same) hist_add(hg + 1024, (rb >> 10) & 1023u, valid && (rb >> 20) == pfx1);
                } else {
                    hist_add(hg, rb & 1023u, valid && (rb >> 10) == pfx0);
                    if (!same) hist_add(hg + 1024, rb & 1023u, valid && (rb >> 10) == pfx1);
                }
            }
        }
    }
    __syncthreads();
    uint32_t* gh = p.hist + ((int64_t)img * p.K + k0) * kBins;
    for (int i = threadIdx.x; i < kG * kBins; i += kThreads) {
        const uint32_t c = hist[i];
        if (c) atomicAdd(&gh[i], c);
    }
}

// the bin of `hist[0 .. nb)` holding 0-based rank `rank` and the rank left inside it (block-wide, nb / 256 bins per thread)
__device__ void find_bin(const uint32_t* hist, int nb, uint32_t rank, uint32_t* s_part, uint32_t* out_bin, uint32_t* out_left) {
    const int per = nb / kThreads;
    uint32_t sum = 0u;
    for (int i = 0; i < per; ++i) sum += hist[threadIdx.x * per + i];
    s_part[threadIdx.x] = sum;
    __syncthreads();
    for (int off = 1; off < kThreads; off <<= 1) {
        const uint32_t v = threadIdx.x >= (unsigned)off ? s_part[threadIdx.x - off] : 0u;
        __syncthreads();
        s_part[threadIdx.x] += v;
        __syncthreads();
    }
    const uint32_t incl = s_part[threadIdx.x];
    const uint32_t excl = incl - sum;
    if (rank >= excl && rank < incl) {                            // exactly one thread
        uint32_t c = excl;
        for (int i = 0; i < per; ++i) {
            const uint32_t hv = hist[threadIdx.x * per + i];
            if (rank < c + hv) { *out_bin = (uint32_t)(threadIdx.x * per + i); *out_left = rank - c; break; }
            c += hv;
        }
    }
    __syncthreads();
}

// grid (K, N): narrows both targets of one hypothesis by the level's bits and clears its histogram for the next level;
// LEVEL 2 writes the median: sorted[n / 2] for odd n, the fp32 mean of the two middle values for even n
template <int LEVEL>
__global__ void __launch_bounds__(kThreads) mat_select_kernel(MatParams p) {
    __shared__ uint32_t s_part[kThreads];
    __shared__ uint32_t s_bin[2], s_left[2];
    const int img = blockIdx.y, k = blockIdx.x;
    if (p.info[img * 4 + I_STATUS] != ST_OK) return;              // (block-uniform)
    const uint32_t n = (uint32_t)p.info[img * 4 + I_NVALID];
    uint32_t* hist = p.hist + ((int64_t)img * p.K + k) * kBins;
    uint32_t* meta = p.meta + ((int64_t)img * p.K + k) * 4;
    const uint32_t pfx0 = meta[0], pfx1 = meta[1];
    uint32_t rank0, rank1;
    if (LEVEL == 0) { rank0 = (n - 1u) >> 1; rank1 = n >> 1; }
    else { rank0 = meta[2]; rank1 = meta[3]; }
    const bool same = LEVEL == 0 || pfx0 == pfx1;
    const int nb = LEVEL == 0 ? kBins : 1024;
    find_bin(hist, nb, rank0, s_part, &s_bin[0], &s_left[0]);
    find_bin(same ? hist : hist + 1024, nb, rank1, s_part, &s_bin[1], &s_left[1]);
    for (int i = threadIdx.x; i < kBins; i += kThreads) hist[i] = 0u;
    if (threadIdx.x != 0) return;
    uint32_t np0, np1;
    if (LEVEL == 0) { np0 = s_bin[0]; np1 = s_bin[1]; }
    else { np0 = (pfx0 << 10) | s_bin[0]; np1 = (pfx1 << 10) | s_bin[1]; }
    if (LEVEL < 2) {
        meta[0] = np0; meta[1] = np1; meta[2] = s_left[0]; meta[3] = s_left[1];
        return;
    }
    const float a = __uint_as_float(np0), b = __uint_as_float(np1);
    const float med = (n & 1u) ? b : (a + b) / 2.0f;
    p.score[(int64_t)img * p.K + k] = __float_as_uint(med);
}

// ---- winner ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) mat_winner_kernel(MatParams p) {
    const int img = blockIdx.x;
    if (threadIdx.x != 0) return;
    if (p.info[img * 4 + I_STATUS] != ST_OK) return;
    const uint32_t* sc = p.score + (int64_t)img * p.K;
    const int32_t* hv = p.hvalid + (int64_t)img * p.K;
    int best = -1;
    uint32_t bs = 0u;
    float bm = 0.0f;
    for (int k = 0; k < p.K; ++k) {
        if (!hv[k]) continue;
        if (p.method == METHOD_RANSAC) {
            if (best < 0 || sc[k] > bs) { best = k; bs = sc[k]; }
        } else {
            const float med = __uint_as_float(sc[k]);
            if (best < 0 || med < bm) { best = k; bm = med; }
        }
    }
    if (best < 0) { p.info[img * 4 + I_STATUS] = ST_NO_HYPOTHESIS; return; }
    p.info[img * 4 + I_WINNER] = best;
    float* mo = p.model + (int64_t)img * kHypStride;
    const float* hb = p.hyp + ((int64_t)img * p.K + best) * kHypStride;
    for (int i = 0; i < 9; ++i) mo[i] = hb[i];
    float thr = kRansacThr;
    if (p.method == METHOD_LMEDS) {
        const double nv = (double)p.info[img * 4 + I_NVALID];
        const double sigma = fmax(2.5 * 1.4826 * (1.0 + 5.0 / (nv - (double)p.m)) * sqrt((double)bm), 0.001);
        thr = (float)(sigma * sigma);
    }
    mo[9] = thr;
}

// ---- least squares --------------------------------------------------------------------------------------------------------
// pass 0: count, Sx, Sy, Su, Sv, Sxx, Sxy, Syy, Sxu, Sxv, Syu, Syv, Suu, Svv of the shifted pairs (x, y) -> (u, v);
// pass 1: for w in {1, u, v, uu + vv} the six sums of w * {xx, xy, x, yy, y, 1} in normalised coordinates (the 9 x 9 A^T A of
// the DLT has no other entries).  Per-thread float64 accumulators, wave butterfly, waves added in order, one slot per block.
template <bool HALF, bool PROJ, int PASS>
__global__ void __launch_bounds__(kThreads) mat_sums_kernel(MatParams p) {
    constexpr int NS = PASS == 0 ? 14 : 24;
    __shared__ double s_red[(kThreads / 64) * NS];
    const int img = blockIdx.y;
    if (p.info[img * 4 + I_STATUS] != ST_OK) return;              // (block-uniform)
    const Loader<HALF> L{p.flow, p.flow_bs, p.hw};
    const int64_t quads = (p.hw + 3) / 4;
    const int64_t q_begin = (int64_t)blockIdx.x * kBlockQuads;
    float hm[9];
    float thr = 0.0f;
    if (p.use_pred) {
        for (int i = 0; i < 9; ++i) hm[i] = p.model[(int64_t)img * kHypStride + i];
        thr = p.model[(int64_t)img * kHypStride + 9];
    }
    double nm[6] = {0, 0, 1, 0, 0, 1};
    if (PASS == 1) for (int i = 0; i < 6; ++i) nm[i] = p.norm[(int64_t)img * 8 + i];
    double acc[NS];
    for (int i = 0; i < NS; ++i) acc[i] = 0.0;
    for (int it = 0; it < kQuadsPerThread; ++it) {
        const int64_t q = q_begin + (int64_t)it * kThreads + threadIdx.x;
        if (q_begin + (int64_t)it * kThreads >= quads) break;     // (block-uniform)
        if (q >= quads) continue;
        const int64_t p0 = 4 * q;
        float fu[4], fv[4];
        L.ld4(img, 0, p0, p.vec, fu);
        L.ld4(img, 1, p0, p.vec, fv);
        for (int e = 0; e < 4; ++e) {
            if (p0 + e >= p.hw) continue;
            if (p.mask != nullptr && p.mask[img * p.mask_bs + p0 + e] == 0) continue;
            double sx, sy, dx, dy;
            make_pair(p, (uint32_t)(p0 + e), fu[e], fv[e], sx, sy, dx, dy);
            if (p.use_pred && !(resid<PROJ>(hm, (float)sx, (float)sy, (float)dx, (float)dy) <= thr)) continue;
            double x = sx - p.cx, y = sy - p.cy, u = dx - p.cx, v = dy - p.cy;
            if (PASS == 0) {
                acc[0] += 1.0; acc[1] += x; acc[2] += y; acc[3] += u; acc[4] += v;
                acc[5] += x * x; acc[6] += x * y; acc[7] += y * y;
                acc[8] += x * u; acc[9] += x * v; acc[10] += y * u; acc[11] += y * v;
                acc[12] += u * u; acc[13] += v * v;
            } else {
                x = (x - nm[0]) * nm[2]; y = (y - nm[1]) * nm[2];
                u = (u - nm[3]) * nm[5]; v = (v - nm[4]) * nm[5];
                const double pp[6] = {x * x, x * y, x, y * y, y, 1.0};
                const double ww[4] = {1.0, u, v, u * u + v * v};
                for (int a = 0; a < 4; ++a)
                    for (int b = 0; b < 6; ++b) acc[a * 6 + b] += ww[a] * pp[b];
            }
        }
    }
    for (int i = 0; i < NS; ++i)
        for (int off = 32; off > 0; off >>= 1) acc[i] += __shfl_xor(acc[i], off);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) for (int i = 0; i < NS; ++i) s_red[wave * NS + i] = acc[i];
    __syncthreads();
    if (threadIdx.x < NS) {
        double s = s_red[threadIdx.x];
        for (int wv = 1; wv < kThreads / 64; ++wv) s += s_red[wv * NS + threadIdx.x];
        p.partial[((int64_t)img * p.nblk + blockIdx.x) * kNS + threadIdx.x] = s;
    }
}

__device__ void mul33(const double* a, const double* b, double* c) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) c[i * 3 + j] = (a[i * 3] * b[j] + a[i * 3 + 1] * b[3 + j]) + a[i * 3 + 2] * b[6 + j];
}

// the eigenvector of the smallest eigenvalue of the symmetric 9 x 9 `a` (destroyed): cyclic Jacobi, 16 sweeps at most
__device__ void jacobi_smallest(double* a, double* vec) {
    double v[81];
    for (int i = 0; i < 81; ++i) v[i] = (i % 10 == 0) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 16; ++sweep) {
        double off = 0.0;
        for (int i = 0; i < 9; ++i)
            for (int j = i + 1; j < 9; ++j) off += a[i * 9 + j] * a[i * 9 + j];
        if (off == 0.0) break;
        for (int pi = 0; pi < 8; ++pi) {
            for (int qi = pi + 1; qi < 9; ++qi) {
                const double apq = a[pi * 9 + qi];
                if (apq == 0.0) continue;
                const double theta = (a[qi * 9 + qi] - a[pi * 9 + pi]) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int r = 0; r < 9; ++r) {                     // A <- A J
                    const double arp = a[r * 9 + pi], arq = a[r * 9 + qi];
                    a[r * 9 + pi] = c * arp - s * arq;
                    a[r * 9 + qi] = s * arp + c * arq;
                }
                for (int r = 0; r < 9; ++r) {                     // A <- J^T A
                    const double apr = a[pi * 9 + r], aqr = a[qi * 9 + r];
                    a[pi * 9 + r] = c * apr - s * aqr;
                    a[qi * 9 + r] = s * apr + c * aqr;
                }
                for (int r = 0; r < 9; ++r) {
                    const double vrp = v[r * 9 + pi], vrq = v[r * 9 + qi];
                    v[r * 9 + pi] = c * vrp - s * vrq;
                    v[r * 9 + qi] = s * vrp + c * vrq;
                }
            }
        }
    }
    int best = 0;
    for (int i = 1; i < 9; ++i) if (a[i * 9 + i] < a[best * 9 + best]) best = i;
    for (int r = 0; r < 9; ++r) vec[r] = v[r * 9 + best];
}

// one block per image: the block slots added in index order, then the solve of (dof, pass)
__global__ void __launch_bounds__(64) mat_finish_kernel(MatParams p) {
    __shared__ double s_sum[kNS];
    const int img = blockIdx.x;
    int32_t* info = p.info + img * 4;
    if (info[I_STATUS] != ST_OK) return;                          // (block-uniform)
    if (threadIdx.x < kNS) {
        double s = 0.0;
        const double* part = p.partial + (int64_t)img * p.nblk * kNS + threadIdx.x;
        for (int b = 0; b < p.nblk; ++b) s += part[(int64_t)b * kNS];
        s_sum[threadIdx.x] = s;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const double* S = s_sum;
    double* out = p.out + (int64_t)img * 9;
    const int fail = p.use_pred ? ST_REFIT_SINGULAR : ST_FEW_POINTS;
    double M[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (p.pass == 0) {
        const double cnt = S[0];
        if (p.use_pred) info[I_INLIERS] = (int32_t)cnt; else { info[I_NVALID] = (int32_t)cnt; info[I_WINNER] = -1; info[I_INLIERS] = (int32_t)cnt; }
        if (cnt < (double)p.m) { info[I_STATUS] = fail; return; }
        if (p.dof == 4) {
            const double mx = S[1] / cnt, my = S[2] / cnt, mu = S[3] / cnt, mv = S[4] / cnt;
            const double cxx = S[5] - S[1] * mx, cyy = S[7] - S[2] * my;
            const double cxu = S[8] - S[1] * mu, cxv = S[9] - S[1] * mv, cyu = S[10] - S[2] * mu, cyv = S[11] - S[2] * mv;
            const double den = cxx + cyy;
            if (!(den > 0.0)) { info[I_STATUS] = ST_REFIT_SINGULAR; return; }
            const double a = (cxu + cyv) / den, b = (cxv - cyu) / den;
            M[0] = a; M[1] = -b; M[2] = mu - (a * mx - b * my);
            M[3] = b; M[4] = a; M[5] = mv - (b * mx + a * my);
        } else if (p.dof == 6) {
            double a[9] = {S[5], S[6], S[1], S[6], S[7], S[2], S[1], S[2], cnt};
            double b[6] = {S[8], S[9], S[10], S[11], S[3], S[4]};
            double x[6];
            if (!gauss_solve<3, 2>(a, b, x)) { info[I_STATUS] = ST_REFIT_SINGULAR; return; }
            M[0] = x[0]; M[1] = x[2]; M[2] = x[4];
            M[3] = x[1]; M[4] = x[3]; M[5] = x[5];
        } else {
            // the normalisation of the DLT: centroid to the origin, mean squared distance 2, src and dst separately
            const double mx = S[1] / cnt, my = S[2] / cnt, mu = S[3] / cnt, mv = S[4] / cnt;
            const double vs = ((S[5] - S[1] * mx) + (S[7] - S[2] * my)) / cnt;
            const double vd = ((S[12] - S[3] * mu) + (S[13] - S[4] * mv)) / cnt;
            if (!(vs > 0.0) || !(vd > 0.0)) { info[I_STATUS] = ST_REFIT_SINGULAR; return; }
            double* nm = p.norm + (int64_t)img * 8;
            nm[0] = mx; nm[1] = my; nm[2] = sqrt(2.0 / vs);
            nm[3] = mu; nm[4] = mv; nm[5] = sqrt(2.0 / vd);
            return;
        }
        // back from the shifted coordinates: t = t' + c - A c
        M[2] = M[2] + p.cx - (M[0] * p.cx + M[1] * p.cy);
        M[5] = M[5] + p.cy - (M[3] * p.cx + M[4] * p.cy);
    } else {
        double a[81];
        for (int i = 0; i < 81; ++i) a[i] = 0.0;
        // P = [[xx xy x] [xy yy y] [x y 1]] from {xx, xy, x, yy, y, 1}
        const int pidx[9] = {0, 1, 2, 1, 3, 4, 2, 4, 5};
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) {
                const int e = pidx[i * 3 + j];
                a[i * 9 + j] = S[e];
                a[(3 + i) * 9 + 3 + j] = S[e];
                a[i * 9 + 6 + j] = -S[6 + e];
                a[(6 + j) * 9 + i] = -S[6 + e];
                a[(3 + i) * 9 + 6 + j] = -S[12 + e];
                a[(6 + j) * 9 + 3 + i] = -S[12 + e];
                a[(6 + i) * 9 + 6 + j] = S[18 + e];
            }
        }
        double hn[9];
        jacobi_smallest(a, hn);
        const double* nm = p.norm + (int64_t)img * 8;
        const double ts[9] = {nm[2], 0, -(nm[2] * nm[0]), 0, nm[2], -(nm[2] * nm[1]), 0, 0, 1};
        const double tdi[9] = {1.0 / nm[5], 0, nm[3], 0, 1.0 / nm[5], nm[4], 0, 0, 1};
        const double tc[9] = {1, 0, p.cx, 0, 1, p.cy, 0, 0, 1};
        const double tci[9] = {1, 0, -p.cx, 0, 1, -p.cy, 0, 0, 1};
        double t1[9], t2[9];
        mul33(hn, ts, t1);
        mul33(tdi, t1, t2);
        mul33(t2, tci, t1);
        mul33(tc, t1, t2);
        const double h33 = t2[8];
        bool ok = h33 != 0.0;
        for (int i = 0; i < 9; ++i) { M[i] = t2[i] / h33; ok = ok && (fabs(M[i]) <= DBL_MAX); }
        if (!ok) { info[I_STATUS] = ST_REFIT_SINGULAR; return; }
    }
    for (int i = 0; i < 9; ++i) out[i] = M[i];
}

int dims_ok(int32_t n, int32_t h, int32_t w) {
    if (n < 1 || h < 1 || w < 1 || n > 65535) return OFL_E_SHAPE;
    if ((int64_t)h * w >= (1ll << 31)) return OFL_E_SHAPE;
    return OFL_OK;
}

int args_ok(int32_t dof, int32_t method) {
    if (dof != 4 && dof != 6 && dof != 8) return OFL_E_ARG;
    if (method < METHOD_LMS || method > METHOD_LMEDS) return OFL_E_ARG;
    return OFL_OK;
}

bool aligned(const void* ptr, int a) { return ((uintptr_t)ptr % (uintptr_t)a) == 0; }

int hypotheses(int32_t method) { return method == METHOD_RANSAC ? kKRansac : (method == METHOD_LMEDS ? kKLmeds : 0); }

int64_t blocks_of(int32_t h, int32_t w) {
    const int64_t quads = ((int64_t)h * w + 3) / 4;
    return (quads + kBlockQuads - 1) / kBlockQuads;
}

int64_t up8(int64_t b) { return (b + 7) / 8 * 8; }

// the workspace: byte offsets of its arrays (all multiples of 8)
struct Layout {
    int64_t partial, norm, model, hyp, hvalid, score, rowoff, meta, hist, total;
};

Layout layout_of(int32_t n, int32_t h, int32_t w, int32_t method) {
    Layout l;
    const int64_t K = hypotheses(method);
    int64_t o = 0;
    l.partial = o; o += up8((int64_t)n * blocks_of(h, w) * kNS * 8);
    l.norm = o; o += (int64_t)n * 8 * 8;
    l.model = o; o += up8((int64_t)n * kHypStride * 4);
    l.hyp = o; o += up8((int64_t)n * K * kHypStride * 4);
    l.hvalid = o; o += up8((int64_t)n * K * 4);
    l.score = o; o += up8((int64_t)n * K * 4);
    l.rowoff = o; o += up8(K ? (int64_t)n * (h + 1) * 4 : 0);
    l.meta = o; o += up8(method == METHOD_LMEDS ? (int64_t)n * K * 4 * 4 : 0);
    l.hist = o; o += up8(method == METHOD_LMEDS ? (int64_t)n * K * kBins * 4 : 0);
    l.total = o > 0 ? o : 8;
    return l;
}

template <bool HALF, bool PROJ>
void launch_all(MatParams p, hipStream_t s) {
    const dim3 block(kThreads);
    const dim3 pix((unsigned)p.nblk, (unsigned)p.n);
    if (p.method != METHOD_LMS) {
        if (p.mask) hipLaunchKernelGGL(mat_rowcount_kernel, dim3((unsigned)((p.h + 3) / 4), (unsigned)p.n), block, 0, s, p);
        hipLaunchKernelGGL(mat_init_kernel, dim3(p.n), block, 0, s, p);
        hipLaunchKernelGGL(mat_hyp_kernel<HALF>, dim3((unsigned)((p.K + 63) / 64), (unsigned)p.n), dim3(64), 0, s, p);
        if (p.method == METHOD_RANSAC) {
            hipLaunchKernelGGL((mat_score_kernel<HALF, PROJ, kKRansac>), pix, block, 0, s, p);
        } else {
            const dim3 hg((unsigned)p.nblk, (unsigned)(p.K / kG), (unsigned)p.n), sg((unsigned)p.K, (unsigned)p.n);
            hipLaunchKernelGGL((mat_hist_kernel<HALF, PROJ, 0>), hg, block, 0, s, p);
            hipLaunchKernelGGL(mat_select_kernel<0>, sg, block, 0, s, p);
            hipLaunchKernelGGL((mat_hist_kernel<HALF, PROJ, 1>), hg, block, 0, s, p);
            hipLaunchKernelGGL(mat_select_kernel<1>, sg, block, 0, s, p);
            hipLaunchKernelGGL((mat_hist_kernel<HALF, PROJ, 2>), hg, block, 0, s, p);
            hipLaunchKernelGGL(mat_select_kernel<2>, sg, block, 0, s, p);
        }
        hipLaunchKernelGGL(mat_winner_kernel, dim3(p.n), dim3(64), 0, s, p);
        p.use_pred = 1;
    }
    p.pass = 0;
    hipLaunchKernelGGL((mat_sums_kernel<HALF, PROJ, 0>), pix, block, 0, s, p);
    hipLaunchKernelGGL(mat_finish_kernel, dim3(p.n), dim3(64), 0, s, p);
    if (p.dof == 8) {
        p.pass = 1;
        hipLaunchKernelGGL((mat_sums_kernel<HALF, PROJ, 1>), pix, block, 0, s, p);
        hipLaunchKernelGGL(mat_finish_kernel, dim3(p.n), dim3(64), 0, s, p);
    }
}

}  // namespace

extern "C" {

__attribute__((visibility("default"))) int64_t ofl_matrix_workspace_bytes(int32_t n, int32_t h, int32_t w, int32_t dof,
                                                                          int32_t method) {
    int rc = dims_ok(n, h, w);
    if (rc) return rc;
    rc = args_ok(dof, method);
    if (rc) return rc;
    return layout_of(n, h, w, method).total;
}

__attribute__((visibility("default"))) int ofl_matrix_fit_f64(const void* flow, int64_t flow_bs, int32_t flow_half, int32_t ref,
                                                              const uint8_t* mask, int64_t mask_bs, int32_t n, int32_t h, int32_t w,
                                                              int32_t dof, int32_t method, void* workspace, double* out_matrix,
                                                              int32_t* out_info, void* stream) {
    if (!flow || !workspace || !out_matrix || !out_info) return OFL_E_NULL;
    int rc = dims_ok(n, h, w);
    if (rc) return rc;
    rc = args_ok(dof, method);
    if (rc) return rc;
    if (flow_half != 0 && flow_half != 1) return OFL_E_ARG;
    if (ref != 0 && ref != 1) return OFL_E_ARG;
    if (flow_bs < 0 || mask_bs < 0) return OFL_E_ARG;
    if (!aligned(workspace, 8)) return OFL_E_ARG;
    const Layout l = layout_of(n, h, w, method);
    char* ws = reinterpret_cast<char*>(workspace);
    MatParams p;
    p.flow = flow; p.flow_bs = flow_bs; p.mask = mask; p.mask_bs = mask_bs; p.n = n; p.h = h; p.w = w; p.hw = (int64_t)h * w;
    const int elem = flow_half ? 2 : 4;
    p.vec = (p.hw % 4 == 0) && (flow_bs % 4 == 0) && aligned(flow, 4 * elem);
    p.ref_s = ref; p.dof = dof; p.m = dof / 2; p.method = method; p.K = hypotheses(method); p.nblk = (int)blocks_of(h, w);
    p.pass = 0; p.use_pred = 0;
    p.cx = 0.5 * (double)(w - 1); p.cy = 0.5 * (double)(h - 1);
    p.partial = reinterpret_cast<double*>(ws + l.partial);
    p.norm = reinterpret_cast<double*>(ws + l.norm);
    p.model = reinterpret_cast<float*>(ws + l.model);
    p.hyp = reinterpret_cast<float*>(ws + l.hyp);
    p.hvalid = reinterpret_cast<int32_t*>(ws + l.hvalid);
    p.score = reinterpret_cast<uint32_t*>(ws + l.score);
    p.rowoff = reinterpret_cast<int32_t*>(ws + l.rowoff);
    p.meta = reinterpret_cast<uint32_t*>(ws + l.meta);
    p.hist = reinterpret_cast<uint32_t*>(ws + l.hist);
    p.info = out_info;
    p.out = out_matrix;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(workspace, 0, (size_t)l.total, s);
    if (e != hipSuccess) return (int)e;
    e = hipMemsetAsync(out_info, 0, (size_t)n * 4 * sizeof(int32_t), s);
    if (e != hipSuccess) return (int)e;
    e = hipMemsetAsync(out_matrix, 0, (size_t)n * 9 * sizeof(double), s);
    if (e != hipSuccess) return (int)e;
    if (flow_half) {
        if (dof == 8) launch_all<true, true>(p, s); else launch_all<true, false>(p, s);
    } else {
        if (dof == 8) launch_all<false, true>(p, s); else launch_all<false, false>(p, s);
    }
    return (int)hipGetLastError();
}

}  // extern "C"
