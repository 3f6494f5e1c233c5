// ofl_mesh.hip -- the triangle-mesh interpolator of DESIGN.md 3.12 on gfx950: what apply_flow(ref='s') and track_pts(ref='t') compute
// when PURE_PYTORCH is unset and set_mesh_interpolation() is on (the reference calls scipy.interpolate.griddata there, utils.py:577-600
// and :1020-1032).  The warped pixel grid's own quads are the mesh: every quad with four usable vertices is split along its locally
// Delaunay diagonal into two triangles, numbered 2 q and 2 q + 1; a query takes the barycentric interpolation of the LOWEST-numbered
// triangle that contains it (edges included), or 0 where none does.  Everything that decides coverage or forms a weight is float64 with
// + - * / only, in ONE operation order and without contraction, so that tests/mesh_oracle.py follows every bit.
//
//   ofl_mesh_plan     one thread per quad: its box, the number of quads whose box touches each tile; the exclusive scan of the counts
//   ofl_mesh_apply    fill the tile lists (sized from the counts), then one block per 64 x 16 tile GATHERS: the tile's quads are walked by
//                     the block's threads, every pixel of the tile keeps the lowest triangle that contains it (an LDS plane, atomicMin:
//                     the minimum does not depend on the order), then each pixel interpolates all C channels from its triangle's three
//                     source pixels and writes its output once
//   ofl_mesh_points   the same lists over 8 x 8 tiles, then one thread per query point walks its tile's list
// The list entry is the quad's number (4 bytes): the vertices are re-read from the flow and the split is re-derived where they are needed,
// which costs a few cached loads and ~30 float64 operations and saves a 100-byte triangle record per quad and tile.
// C ABI: include/oflib_hip.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "oflib_hip.h"

#pragma clang fp contract(off)

// the launch recorder of ofl_kernels.hip (ofl_last_kernel_name)
extern const void* g_ofl_last_kernel;
#define OFL_KLAUNCH(K, ...) do { g_ofl_last_kernel = (const void*)(K); hipLaunchKernelGGL(K, __VA_ARGS__); } while (0)

namespace {

constexpr int kThreads = 256;
constexpr int kTileW = 64, kTileH = 16;           // the house tile of the raster kernel
constexpr int kPtTile = 8;                         // the point query's tiles: a point walks ~ 2 * 8 * 8 triangles
constexpr int kScanThreads = 1024;
constexpr int kHeader = 16;                        // workspace header: [0] [1] the list entries of all tiles (int64)
constexpr uint32_t kNone = 0xffffffffu;

struct Geo {
    int32_t nf, h, w;          // flow images (each has its own mesh), frame
    int32_t tw, th, tx, ty;    // tile size, tiles per row / column
    int32_t points;            // 0: pixel queries (boxes hold pixel centres), 1: point queries (boxes hold real positions)
    int64_t hw;
};

struct FlowIn {
    const float* flow;         // [nf, 2, h, w]
    int64_t bs;
    double sign;               // vertices are grid + sign * flow
    const uint8_t* mask;       // [nf, h, w] or nullptr: every vertex usable
    int64_t mbs;
};

struct Workspace {
    int32_t* header;
    unsigned long long* offsets;   // [nt]
    uint32_t* counts;              // [nt]
    uint32_t* cursor;              // [nt]
};

__host__ __device__ inline Workspace carve(int32_t* ws, const Geo& g) {
    const int64_t nt = (int64_t)g.nf * g.tx * g.ty;
    Workspace r;
    r.header = ws;
    r.offsets = reinterpret_cast<unsigned long long*>(ws + kHeader);
    r.counts = reinterpret_cast<uint32_t*>(ws + kHeader + 2 * nt);
    r.cursor = r.counts + nt;
    return r;
}

// ---- the definition; tests/mesh_oracle.py restates each function below operation for operation ----------------
struct Quad { double ax, ay, bx, by, cx, cy, dx, dy; };    // A (i, j)  B (i, j + 1)  C (i + 1, j + 1)  D (i + 1, j)
struct Tri { double x0, y0, x1, y1, x2, y2; };

__device__ __forceinline__ bool finite64(double v) { return v - v == 0.0; }

__device__ __forceinline__ bool load_vertex(const FlowIn& f, const Geo& g, int img, int i, int j, double* x, double* y) {
    const int64_t q = (int64_t)i * g.w + j;
    if (f.mask != nullptr && f.mask[(int64_t)img * f.mbs + q] == 0) return false;
    const float* p = f.flow + (int64_t)img * f.bs;
    *x = (double)j + f.sign * (double)p[q];
    *y = (double)i + f.sign * (double)p[g.hw + q];
    return finite64(*x) && finite64(*y);
}

// the four vertices of quad (i, j); false: one of them is masked out or not finite, the quad gives no triangle
__device__ __forceinline__ bool load_quad(const FlowIn& f, const Geo& g, int img, int i, int j, Quad* q) {
    bool ok = load_vertex(f, g, img, i, j, &q->ax, &q->ay);
    ok = load_vertex(f, g, img, i, j + 1, &q->bx, &q->by) && ok;
    ok = load_vertex(f, g, img, i + 1, j + 1, &q->cx, &q->cy) && ok;
    ok = load_vertex(f, g, img, i + 1, j, &q->dx, &q->dy) && ok;
    return ok;
}

// E(P, Q; X): > 0 on one side of the line P -> Q, < 0 on the other
__device__ __forceinline__ double edge_fn(double px, double py, double qx, double qy, double x, double y) {
    return (qx - px) * (y - py) - (qy - py) * (x - px);
}

// true: D lies strictly inside the circle through A, B, C -- the diagonal A-C is not locally Delaunay, the quad is split along
// B-D.  A tie (co-circular, or A, B, C collinear) keeps A-C.
__device__ __forceinline__ bool split_bd(const Quad& q) {
    const double adx = q.ax - q.dx, ady = q.ay - q.dy, bdx = q.bx - q.dx, bdy = q.by - q.dy, cdx = q.cx - q.dx, cdy = q.cy - q.dy;
    const double ad2 = adx * adx + ady * ady, bd2 = bdx * bdx + bdy * bdy, cd2 = cdx * cdx + cdy * cdy;
    const double det = (ad2 * (bdx * cdy - bdy * cdx) + bd2 * (cdx * ady - cdy * adx)) + cd2 * (adx * bdy - ady * bdx);
    const double o = edge_fn(q.ax, q.ay, q.bx, q.by, q.cx, q.cy);
    return (det > 0.0 && o > 0.0) || (det < 0.0 && o < 0.0);
}

// triangle k of the quad: A-C split (A, B, C) (A, C, D); B-D split (A, B, D) (B, C, D)
__device__ __forceinline__ Tri make_tri(const Quad& q, bool bd, int k) {
    Tri t;
    if (k == 0) {
        t.x0 = q.ax; t.y0 = q.ay; t.x1 = q.bx; t.y1 = q.by;
        t.x2 = bd ? q.dx : q.cx; t.y2 = bd ? q.dy : q.cy;
    } else {
        t.x0 = bd ? q.bx : q.ax; t.y0 = bd ? q.by : q.ay;
        t.x1 = q.cx; t.y1 = q.cy; t.x2 = q.dx; t.y2 = q.dy;
    }
    return t;
}

__device__ __forceinline__ double tri_area2(const Tri& t) { return edge_fn(t.x0, t.y0, t.x1, t.y1, t.x2, t.y2); }

// the three edge functions of the query, e_m opposite vertex m.  An edge is ALWAYS evaluated from its vertex with the lower pixel
// index to the one with the higher and negated for the triangle that runs it the other way, so the two triangles that share an edge see
// exactly opposite values: a query on it is inside both, one just off it inside exactly one -- the mesh has no cracks.  In both splits
// triangle 0 runs 0 -> 1 -> 2 upwards except 2 -> 0, triangle 1 runs 0 -> 1 upwards and 1 -> 2, 2 -> 0 downwards.
__device__ __forceinline__ void tri_edges(const Tri& t, int k, double x, double y, double* e0, double* e1, double* e2) {
    *e0 = k == 0 ? edge_fn(t.x1, t.y1, t.x2, t.y2, x, y) : -edge_fn(t.x2, t.y2, t.x1, t.y1, x, y);
    *e1 = -edge_fn(t.x0, t.y0, t.x2, t.y2, x, y);
    *e2 = edge_fn(t.x0, t.y0, t.x1, t.y1, x, y);
}

__device__ __forceinline__ bool tri_inside(double a2, double e0, double e1, double e2) {
    return a2 > 0.0 ? (e0 >= 0.0 && e1 >= 0.0 && e2 >= 0.0) : (e0 <= 0.0 && e1 <= 0.0 && e2 <= 0.0);
}

__device__ __forceinline__ double min3(double a, double b, double c) { return fmin(fmin(a, b), c); }
__device__ __forceinline__ double max3(double a, double b, double c) { return fmax(fmax(a, b), c); }

// the cells [x0, x1] x [y0, y1] of the frame a box of positions touches: pixel queries -- the pixel centres inside the box; point
// queries -- the unit cells (floor of a position) the box overlaps.  false: none.
__device__ __forceinline__ bool box_cells(const Geo& g, double minx, double maxx, double miny, double maxy, int* x0, int* x1, int* y0,
                                          int* y1) {
    const double lx = fmax(g.points ? floor(minx) : ceil(minx), 0.0), hx = fmin(floor(maxx), (double)(g.w - 1));
    const double ly = fmax(g.points ? floor(miny) : ceil(miny), 0.0), hy = fmin(floor(maxy), (double)(g.h - 1));
    if (!(lx <= hx && ly <= hy)) return false;
    *x0 = (int)lx; *x1 = (int)hx; *y0 = (int)ly; *y1 = (int)hy;
    return true;
}

__device__ __forceinline__ bool quad_cells(const Geo& g, const Quad& q, int* x0, int* x1, int* y0, int* y1) {
    return box_cells(g, fmin(fmin(q.ax, q.bx), fmin(q.cx, q.dx)), fmax(fmax(q.ax, q.bx), fmax(q.cx, q.dx)),
                     fmin(fmin(q.ay, q.by), fmin(q.cy, q.dy)), fmax(fmax(q.ay, q.by), fmax(q.cy, q.dy)), x0, x1, y0, y1);
}

// ---- plan: count, scan ---------------------------------------------------------------------------------------------------------
// One thread per (image, quad).  A quad is listed in EVERY tile its box touches, however many: the lists are sized from these
// counts, nothing is capped (a flow that stretches one quad over the whole frame costs one entry per tile of the frame).
template <bool kFill>
__global__ void __launch_bounds__(kThreads) mesh_list_kernel(FlowIn f, Geo g, uint32_t* counts, const unsigned long long* offsets,
                                                             uint32_t* cursor, int32_t* list, int64_t list_ints) {
    const int64_t quads = (int64_t)(g.h - 1) * (g.w - 1);
    const int64_t id = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (id >= quads * g.nf) return;
    const int img = (int)(id / quads);
    const int qn = (int)(id - (int64_t)img * quads);
    Quad q;
    if (!load_quad(f, g, img, qn / (g.w - 1), qn % (g.w - 1), &q)) return;
    int x0, x1, y0, y1;
    if (!quad_cells(g, q, &x0, &x1, &y0, &y1)) return;
    const int64_t t0 = (int64_t)img * g.tx * g.ty;
    for (int ty = y0 / g.th; ty <= y1 / g.th; ++ty)
        for (int tx = x0 / g.tw; tx <= x1 / g.tw; ++tx) {
            const int64_t t = t0 + (int64_t)ty * g.tx + tx;
            if (!kFill) {
                atomicAdd(&counts[t], 1u);
            } else {
                const int64_t at = (int64_t)offsets[t] + atomicAdd(&cursor[t], 1u);
                if (at < list_ints) list[at] = qn;
            }
        }
}

// exclusive scan of the tile counts by one block; header[0..1] = their sum (int64)
__global__ void __launch_bounds__(kScanThreads) mesh_scan_kernel(const uint32_t* counts, unsigned long long* offsets, int64_t nt,
                                                                 int32_t* header) {
    __shared__ unsigned long long part[kScanThreads];
    const int64_t chunk = (nt + kScanThreads - 1) / kScanThreads;
    const int64_t lo = (int64_t)threadIdx.x * chunk < nt ? (int64_t)threadIdx.x * chunk : nt;
    const int64_t hi = lo + chunk < nt ? lo + chunk : nt;
    unsigned long long sum = 0ull;
    for (int64_t i = lo; i < hi; ++i) sum += counts[i];
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int off = 1; off < kScanThreads; off <<= 1) {
        const unsigned long long v = threadIdx.x >= (unsigned)off ? part[threadIdx.x - off] : 0ull;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    unsigned long long c = part[threadIdx.x] - sum;
    for (int64_t i = lo; i < hi; ++i) { offsets[i] = c; c += counts[i]; }
    if (threadIdx.x == kScanThreads - 1) *reinterpret_cast<long long*>(header) = (long long)part[threadIdx.x];
}

// ---- raster: one block per 64 x 16 tile ---------------------------------------------------------------------------------------------
struct RasterParams {
    FlowIn f;
    Geo g;
    const uint32_t* counts;
    const unsigned long long* offsets;
    const int32_t* list;
    int64_t list_ints;
    const void* src;           // [*, c, h, w] float or uint8
    int64_t src_bs;            // elements between images (0: one image for the batch)
    void* dst;                 // [n, c, h, w], the type of src
    uint8_t* inside;           // [n, h, w] or nullptr
    int32_t* owner;            // [n, h, w] or nullptr: the number of the triangle each pixel took, -1: none
    int32_t c, round_mode;
};

__device__ __forceinline__ double src_at(const float* s, int64_t i) { return (double)s[i]; }
__device__ __forceinline__ double src_at(const uint8_t* s, int64_t i) { return (double)s[i]; }

// the float64 value goes to float32 (the reference's result array has the target's type), then integer targets are rounded half to
// even and uint8 is clamped (utils.py:612-618)
__device__ __forceinline__ float finish(double v, int round_mode) {
    float r = (float)v;
    if (round_mode != OFL_ROUND_NONE) r = rintf(r);
    if (round_mode == OFL_ROUND_U8) r = r > 0.0f ? fminf(r, 255.0f) : 0.0f;       // (everything not above 0, -0.0 included, is +0.0)
    return r;
}
__device__ __forceinline__ void store(float* d, int64_t i, float v) { d[i] = v; }
__device__ __forceinline__ void store(uint8_t* d, int64_t i, float v) { d[i] = (uint8_t)v; }

template <typename T>
__global__ void __launch_bounds__(kThreads) mesh_raster_kernel(RasterParams p) {
    __shared__ uint32_t s_owner[kTileW * kTileH];
    const Geo& g = p.g;
    const int img = blockIdx.z;
    const int fimg = g.nf == 1 ? 0 : img;
    const int64_t tile = ((int64_t)fimg * g.ty + blockIdx.y) * g.tx + blockIdx.x;
    const int tx0 = blockIdx.x * kTileW, ty0 = blockIdx.y * kTileH;
    const int tx1 = min(tx0 + kTileW, g.w) - 1, ty1 = min(ty0 + kTileH, g.h) - 1;
    for (int i = threadIdx.x; i < kTileW * kTileH; i += kThreads) s_owner[i] = kNone;
    __syncthreads();
    // every pixel of the tile keeps the lowest triangle that contains it
    const int64_t off = (int64_t)p.offsets[tile];
    int64_t len = (int64_t)p.counts[tile];
    if (off + len > p.list_ints) len = p.list_ints > off ? p.list_ints - off : 0;
    for (int64_t e = threadIdx.x; e < len; e += kThreads) {
        const int qn = p.list[off + e];
        Quad q;
        if (!load_quad(p.f, g, fimg, qn / (g.w - 1), qn % (g.w - 1), &q)) continue;
        const bool bd = split_bd(q);
        for (int k = 0; k < 2; ++k) {
            const Tri t = make_tri(q, bd, k);
            const double a2 = tri_area2(t);
            if (a2 == 0.0) continue;                                  // a zero-area triangle is dropped
            int x0, x1, y0, y1;
            if (!box_cells(g, min3(t.x0, t.x1, t.x2), max3(t.x0, t.x1, t.x2), min3(t.y0, t.y1, t.y2), max3(t.y0, t.y1, t.y2), &x0, &x1,
                           &y0, &y1))
                continue;
            x0 = max(x0, tx0); x1 = min(x1, tx1); y0 = max(y0, ty0); y1 = min(y1, ty1);
            const uint32_t id = 2u * (uint32_t)qn + (uint32_t)k;
            for (int y = y0; y <= y1; ++y)
                for (int x = x0; x <= x1; ++x) {
                    double e0, e1, e2;
                    tri_edges(t, k, (double)x, (double)y, &e0, &e1, &e2);
                    if (tri_inside(a2, e0, e1, e2)) atomicMin(&s_owner[(y - ty0) * kTileW + (x - tx0)], id);
                }
        }
    }
    __syncthreads();
    // each pixel interpolates all channels from its triangle's three source pixels
    const T* src = reinterpret_cast<const T*>(p.src) + (int64_t)img * p.src_bs;
    T* dst = reinterpret_cast<T*>(p.dst) + (int64_t)img * p.c * g.hw;
    for (int r = 0; r < kTileW * kTileH / kThreads; ++r) {
        const int local = r * kThreads + (int)threadIdx.x;
        const int y = ty0 + local / kTileW, x = tx0 + local % kTileW;
        if (y >= g.h || x >= g.w) continue;
        const int64_t px = (int64_t)y * g.w + x;
        const uint32_t id = s_owner[local];
        if (p.inside != nullptr) p.inside[(int64_t)img * g.hw + px] = id != kNone ? 1 : 0;
        if (p.owner != nullptr) p.owner[(int64_t)img * g.hw + px] = id != kNone ? (int32_t)id : -1;
        if (id == kNone) {
            for (int ch = 0; ch < p.c; ++ch) store(dst, ch * g.hw + px, 0.0f);
            continue;
        }
        const int qn = (int)(id >> 1), k = (int)(id & 1u);
        const int qi = qn / (g.w - 1), qj = qn % (g.w - 1);
        Quad q;
        load_quad(p.f, g, fimg, qi, qj, &q);
        const bool bd = split_bd(q);
        const Tri t = make_tri(q, bd, k);
        const double a2 = tri_area2(t);
        double e0, e1, e2;
        tri_edges(t, k, (double)x, (double)y, &e0, &e1, &e2);
        const double w0 = e0 / a2, w1 = e1 / a2, w2 = e2 / a2;
        const int64_t pa = (int64_t)qi * g.w + qj;
        const int64_t s0 = (k == 1 && bd) ? pa + 1 : pa;
        const int64_t s1 = k == 0 ? pa + 1 : pa + g.w + 1;
        const int64_t s2 = (k == 0 && !bd) ? pa + g.w + 1 : pa + g.w;
        for (int ch = 0; ch < p.c; ++ch) {
            const int64_t co = ch * g.hw;
            const double v = (w0 * src_at(src, co + s0) + w1 * src_at(src, co + s1)) + w2 * src_at(src, co + s2);
            store(dst, co + px, finish(v, p.round_mode));
        }
    }
}

// ---- point queries: one thread per (image, point) -----------------------------------------------------------------------------------
struct PointParams {
    FlowIn f;
    Geo g;
    const uint32_t* counts;
    const unsigned long long* offsets;
    const int32_t* list;
    int64_t list_ints;
    const double* pts;         // [*, m, 2] (y, x)
    int64_t pts_bs;            // doubles between images (0: one set for the batch)
    double* vecs;              // [nf, m, 2] (y, x): the interpolated flow vector
    uint8_t* inside;           // [nf, m]
    int32_t m;
};

__global__ void __launch_bounds__(kThreads) mesh_points_kernel(PointParams p) {
    const Geo& g = p.g;
    const int64_t id = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (id >= (int64_t)g.nf * p.m) return;
    const int img = (int)(id / p.m);
    const int j = (int)(id - (int64_t)img * p.m);
    const double y = p.pts[(int64_t)img * p.pts_bs + 2 * (int64_t)j], x = p.pts[(int64_t)img * p.pts_bs + 2 * (int64_t)j + 1];
    uint32_t best = kNone;
    // a point outside the frame (or NaN) is in no tile
    if (x >= 0.0 && x <= (double)(g.w - 1) && y >= 0.0 && y <= (double)(g.h - 1)) {
        const int64_t tile = ((int64_t)img * g.ty + (int)y / g.th) * g.tx + (int)x / g.tw;
        const int64_t off = (int64_t)p.offsets[tile];
        int64_t len = (int64_t)p.counts[tile];
        if (off + len > p.list_ints) len = p.list_ints > off ? p.list_ints - off : 0;
        for (int64_t e = 0; e < len; ++e) {
            const int qn = p.list[off + e];
            if (2u * (uint32_t)qn >= best) continue;
            Quad q;
            if (!load_quad(p.f, g, img, qn / (g.w - 1), qn % (g.w - 1), &q)) continue;
            const bool bd = split_bd(q);
            for (int k = 0; k < 2; ++k) {
                const uint32_t tid = 2u * (uint32_t)qn + (uint32_t)k;
                if (tid >= best) continue;
                const Tri t = make_tri(q, bd, k);
                const double a2 = tri_area2(t);
                if (a2 == 0.0) continue;
                // candidates are the queries inside the triangle's box, as for pixels
                if (x < min3(t.x0, t.x1, t.x2) || x > max3(t.x0, t.x1, t.x2) || y < min3(t.y0, t.y1, t.y2) || y > max3(t.y0, t.y1, t.y2))
                    continue;
                double e0, e1, e2;
                tri_edges(t, k, x, y, &e0, &e1, &e2);
                if (tri_inside(a2, e0, e1, e2)) best = tid;
            }
        }
    }
    double vy = 0.0, vx = 0.0;
    if (best != kNone) {
        const int qn = (int)(best >> 1), k = (int)(best & 1u);
        const int qi = qn / (g.w - 1), qj = qn % (g.w - 1);
        Quad q;
        load_quad(p.f, g, img, qi, qj, &q);
        const bool bd = split_bd(q);
        const Tri t = make_tri(q, bd, k);
        const double a2 = tri_area2(t);
        double e0, e1, e2;
        tri_edges(t, k, x, y, &e0, &e1, &e2);
        const double w0 = e0 / a2, w1 = e1 / a2, w2 = e2 / a2;
        const int64_t pa = (int64_t)qi * g.w + qj;
        const int64_t s0 = (k == 1 && bd) ? pa + 1 : pa;
        const int64_t s1 = k == 0 ? pa + 1 : pa + g.w + 1;
        const int64_t s2 = (k == 0 && !bd) ? pa + g.w + 1 : pa + g.w;
        const float* fl = p.f.flow + (int64_t)img * p.f.bs;
        vx = (w0 * (double)fl[s0] + w1 * (double)fl[s1]) + w2 * (double)fl[s2];
        vy = (w0 * (double)fl[g.hw + s0] + w1 * (double)fl[g.hw + s1]) + w2 * (double)fl[g.hw + s2];
    }
    p.vecs[2 * id] = vy;
    p.vecs[2 * id + 1] = vx;
    p.inside[id] = best != kNone ? 1 : 0;
}

// nf, h, w, points -> geometry, or an OFL_E_* code
int make_geo(int32_t nf, int32_t h, int32_t w, int32_t points, Geo* out) {
    if (nf < 1 || h < 2 || w < 2 || nf > 65535) return OFL_E_SHAPE;
    if ((int64_t)h * w >= (1ll << 30)) return OFL_E_SHAPE;            // triangle numbers 2 q + 1 stay below 2^31
    if (points != 0 && points != 1) return OFL_E_ARG;
    Geo g;
    g.nf = nf; g.h = h; g.w = w; g.hw = (int64_t)h * w; g.points = points;
    g.tw = points ? kPtTile : kTileW; g.th = points ? kPtTile : kTileH;
    g.tx = (w + g.tw - 1) / g.tw; g.ty = (h + g.th - 1) / g.th;
    if (g.ty > 65535 || (int64_t)nf * g.tx * g.ty >= (1ll << 31)) return OFL_E_SHAPE;
    if ((int64_t)nf * (h - 1) * (w - 1) >= (1ll << 31) * (int64_t)kThreads) return OFL_E_SHAPE;
    *out = g;
    return OFL_OK;
}

bool sign_ok(float s) { return s == 1.0f || s == -1.0f; }

// the fill of the lists the plan counted
int fill_lists(const FlowIn& f, const Geo& g, const Workspace& ws, int32_t* list, int64_t list_ints, hipStream_t s) {
    const int64_t nt = (int64_t)g.nf * g.tx * g.ty, m = (int64_t)g.nf * (g.h - 1) * (g.w - 1);
    hipError_t e = hipMemsetAsync(ws.cursor, 0, (size_t)nt * sizeof(uint32_t), s);
    if (e != hipSuccess) return (int)e;
    if (list_ints > 0)
        OFL_KLAUNCH(mesh_list_kernel<true>, dim3((unsigned)((m + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, f, g, ws.counts,
                    (const unsigned long long*)ws.offsets, ws.cursor, list, list_ints);
    return 0;
}

}  // namespace

extern "C" {

__attribute__((visibility("default"))) int64_t ofl_mesh_workspace_ints(int32_t nf, int32_t h, int32_t w, int32_t points) {
    Geo g;
    const int rc = make_geo(nf, h, w, points, &g);
    if (rc) return rc;
    return kHeader + 4 * (int64_t)g.nf * g.tx * g.ty;
}

__attribute__((visibility("default"))) int ofl_mesh_plan(const float* flow, int64_t flow_bs, float flow_sign, const uint8_t* mask,
                                                         int64_t mask_bs, int32_t points, int32_t* workspace, int32_t nf, int32_t h,
                                                         int32_t w, void* stream) {
    if (!flow || !workspace) return OFL_E_NULL;
    Geo g;
    const int rc = make_geo(nf, h, w, points, &g);
    if (rc) return rc;
    if (!sign_ok(flow_sign) || flow_bs < 0 || mask_bs < 0) return OFL_E_ARG;
    const Workspace ws = carve(workspace, g);
    const FlowIn f{flow, flow_bs, (double)flow_sign, mask, mask_bs};
    const int64_t nt = (int64_t)nf * g.tx * g.ty, m = (int64_t)nf * (h - 1) * (w - 1);
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(ws.counts, 0, (size_t)nt * sizeof(uint32_t), s);
    if (e != hipSuccess) return (int)e;
    OFL_KLAUNCH(mesh_list_kernel<false>, dim3((unsigned)((m + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, f, g, ws.counts,
                (const unsigned long long*)nullptr, (uint32_t*)nullptr, (int32_t*)nullptr, (int64_t)0);
    OFL_KLAUNCH(mesh_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, (const uint32_t*)ws.counts, ws.offsets, nt, ws.header);
    return (int)hipGetLastError();
}

__attribute__((visibility("default"))) int ofl_mesh_apply(const float* flow, int64_t flow_bs, float flow_sign, const uint8_t* mask,
                                                          int64_t mask_bs, const void* src, int64_t src_bs, int32_t src_u8,
                                                          int32_t round_mode, int32_t* workspace, int32_t* list, int64_t list_ints,
                                                          void* dst, uint8_t* inside, int32_t* owner, int32_t nf, int32_t n, int32_t c,
                                                          int32_t h, int32_t w, void* stream) {
    if (!flow || !workspace || !src || !dst || (!list && list_ints > 0)) return OFL_E_NULL;
    Geo g;
    const int rc = make_geo(nf, h, w, 0, &g);
    if (rc) return rc;
    if (n < 1 || n > 65535 || c < 1 || (nf != 1 && nf != n)) return OFL_E_SHAPE;
    if (!sign_ok(flow_sign) || flow_bs < 0 || mask_bs < 0 || src_bs < 0 || list_ints < 0) return OFL_E_ARG;
    if ((src_u8 != 0 && src_u8 != 1) || round_mode < OFL_ROUND_NONE || round_mode > OFL_ROUND_U8) return OFL_E_ARG;
    if (src_u8 && round_mode != OFL_ROUND_U8) return OFL_E_ARG;
    const Workspace ws = carve(workspace, g);
    const FlowIn f{flow, flow_bs, (double)flow_sign, mask, mask_bs};
    hipStream_t s = (hipStream_t)stream;
    const int frc = fill_lists(f, g, ws, list, list_ints, s);
    if (frc) return frc;
    RasterParams p;
    p.f = f; p.g = g; p.counts = ws.counts; p.offsets = ws.offsets; p.list = list; p.list_ints = list_ints;
    p.src = src; p.src_bs = src_bs; p.dst = dst; p.inside = inside; p.owner = owner; p.c = c; p.round_mode = round_mode;
    const dim3 grid((unsigned)g.tx, (unsigned)g.ty, (unsigned)n);
    if (src_u8) OFL_KLAUNCH(mesh_raster_kernel<uint8_t>, grid, dim3(kThreads), 0, s, p);
    else OFL_KLAUNCH(mesh_raster_kernel<float>, grid, dim3(kThreads), 0, s, p);
    return (int)hipGetLastError();
}

__attribute__((visibility("default"))) int ofl_mesh_points(const float* flow, int64_t flow_bs, float flow_sign, const uint8_t* mask,
                                                           int64_t mask_bs, const double* pts, int64_t pts_bs, int32_t* workspace,
                                                           int32_t* list, int64_t list_ints, double* vecs, uint8_t* inside, int32_t nf,
                                                           int32_t m, int32_t h, int32_t w, void* stream) {
    if (!flow || !workspace || !pts || !vecs || !inside || (!list && list_ints > 0)) return OFL_E_NULL;
    Geo g;
    const int rc = make_geo(nf, h, w, 1, &g);
    if (rc) return rc;
    if (m < 1 || (int64_t)nf * m >= (1ll << 31)) return OFL_E_SHAPE;
    if (!sign_ok(flow_sign) || flow_bs < 0 || mask_bs < 0 || pts_bs < 0 || list_ints < 0) return OFL_E_ARG;
    const Workspace ws = carve(workspace, g);
    const FlowIn f{flow, flow_bs, (double)flow_sign, mask, mask_bs};
    hipStream_t s = (hipStream_t)stream;
    const int frc = fill_lists(f, g, ws, list, list_ints, s);
    if (frc) return frc;
    PointParams p;
    p.f = f; p.g = g; p.counts = ws.counts; p.offsets = ws.offsets; p.list = list; p.list_ints = list_ints;
    p.pts = pts; p.pts_bs = pts_bs; p.vecs = vecs; p.inside = inside; p.m = m;
    OFL_KLAUNCH(mesh_points_kernel, dim3((unsigned)(((int64_t)nf * m + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, p);
    return (int)hipGetLastError();
}

}  // extern "C"
