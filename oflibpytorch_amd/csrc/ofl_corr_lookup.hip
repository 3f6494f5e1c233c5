// ofl_corr_lookup.hip -- Flow.corr_lookup on gfx950: the correlation lookup of RAFT, GMA, SEA-RAFT and CRAFT computed on the fly at the
// looked-up positions, without the all-pairs volume (which DEFINES the numbers; tests/corr_lookup_oracle.py is the same
// definition in NumPy).  An extension: the reference has no such function.
//
//   flow_corr_lookup_kernel<R, HALF>             one launch per pyramid level, one pixel per lane, a block owns a tile of 32 x 8 pixels.
//                                                A lane keeps the (2 R + 2)^2 node sums K[j,i] = sum_c feat_c(p) * other_l[c, node] of its
//                                                pixel in registers and walks the channels once: the feature of the next channel is on
//                                                its way while the nodes of this one are loaded straight from global memory at offsets
//                                                clamped into the plane (always addressable; a node outside the frame is selected out).
//                                                After the last channel the (2 R + 1)^2 bilinear combinations and the division, stored
//                                                plane by plane into the level's channel slice of the result
//   flow_corr_lookup_nodes_kernel<R, HALF>       the backward's per-pixel pass of a level: Gn[j,i](p), the gradient of the node sums, from
//                                                the (2 R + 1)^2 planes of gs = g / sqrt(C) into the workspace [n][(2 R + 2)^2][H W], and
//                                                (when d other is wanted) the 64-bit key of the pixel's window
//   flow_corr_lookup_grad_feat_kernel<R, HALF>   d feat: the forward's walk with Gn (read once into registers) in place of feat and one
//                                                sum per channel, which continues the stored sum of the level before
//   flow_corr_lookup_grad_other_kernel<R>        d other_l, a gather: one lane per element q of the level and chunk of kChanChunk channels.
//                                                Node (j, i) of pixel p is q exactly when p's window starts in cell q - (j, i); the pixels
//                                                of a cell are a run of the sorted keys, in ascending raster order
//
// No float atomics and no scatter anywhere: every sum has one owner and a fixed order, the same bits on any run and in any batch.  The
// keys are sorted by torch.sort between the nodes pass and the gather (they are unique: the order is determined).  The position
// arithmetic (win_of, nodes_of) is shared by all four kernels, so that they agree on every floor and every inside test.
//
// Every product is rounded, then every sum: fp contraction is off (ofl_loss_common.hpp); the only fused multiply-adds are the three of
// sample_of().  C ABI: include/oflib_hip.h.
#include "ofl_loss_common.hpp"

namespace {

using namespace ofl_loss;

constexpr int kThreads = 256;
constexpr int kTileW = 32, kTileH = 8;             // output pixels of a block: one per lane
constexpr int kChanChunk = 8;                      // channels a lane of the d other gather sums together
constexpr int kListStep = 4;                       // entries of a cell's list whose loads the gather issues together
constexpr int kMaxRadius = 4;
constexpr int kWavesPerSimd = 3;                   // the walk kernels are compiled for three waves per SIMD (168 VGPRs; 100 sums at R = 4)
constexpr int kMaxLevel = 5;                       // level index l of 2^-l: 0 .. 5, six levels
constexpr int kMaxLevelExtent = 1 << 24;           // a level's height and width: a node's column and row are exact in float32

static_assert(kThreads == kTileW * kTileH, "a lane owns one pixel of the tile");

struct ClParams {
    const void* flow;                              // [*,2,H,W] fp32 or fp16
    int64_t flow_bs;                               // elements between images
    const uint8_t* mask;                           // [*,H,W] bytes or nullptr (all True)
    int64_t mask_bs;
    const float* feat; const float* other;         // [*,C,H,W] on the flow's grid; [*,C,hl,wl], the level
    int64_t feat_bs, other_bs;
    int64_t hw, hwl;
    int32_t chan, h, w, hl, wl, tiles_x;
    float flow_sign, scale;                        // scale: 2^-l
    float* out; int64_t out_bs;                    // forward: the level's slice [n][D][H W] of the result, elements between images
    const float* g; int64_t g_bs;                  // nodes pass: the level's slice of the upstream gradient
    float* gn;                                     // [n][(2 R + 2)^2][H W]: written by the nodes pass, read by both gradients
    int64_t* keys;                                 // [n][H W] or nullptr
    int64_t cells;                                 // cells of the padded grid of a level, plus the sentinel: the key's image stride
    float* grad;                                   // d feat [n][C][H W] or d other [n][C][hl wl]
    int32_t accumulate;                            // d feat: continue the stored sums
    const int64_t* order; const int64_t* starts;   // d other: pixel n H W + p per sorted key; the first sorted key >= k H W, k = 0 .. n cells
    int64_t total;                                 // n H W
};

// The window of pixel (x, y): weights and floors in `t` (nw, ne, sw, se, x_w, y_n, sx, sy; the other fields are not set); returns
// `usable`: valid in the mask and both components finite.  float32 steps as in the head of taps_of(), without the normalise round trip
template <bool HALF>
__device__ __forceinline__ bool win_of(const ClParams& p, int64_t n_img, int x, int y, Taps& t) {
    const int64_t pix = (int64_t)y * p.w + x, fo = n_img * p.flow_bs;
    const float u = ld_flow<HALF>(p.flow, fo + pix), v = ld_flow<HALF>(p.flow, fo + p.hw + pix);
    const bool valid = p.mask == nullptr || p.mask[n_img * p.mask_bs + pix] != 0;
    const float px = (float)x - p.flow_sign * u;
    const float py = (float)y - p.flow_sign * v;
    t.sx = px * p.scale; t.sy = py * p.scale;
    t.x_w = floorf(t.sx); t.y_n = floorf(t.sy);
    const float ww = t.sx - t.x_w, e = 1.0f - ww;
    const float nn = t.sy - t.y_n, s = 1.0f - nn;
    t.nw = s * e; t.ne = s * ww; t.sw = nn * e; t.se = nn * ww;
    return valid && __builtin_isfinite(u) && __builtin_isfinite(v);
}

// The 2 R + 2 node columns and rows of a window: offsets clamped into the plane (column; row times the pitch) and the bits of those
// inside the frame -- float compares, the conversion only where the node is inside.  A pixel that is not usable has no node.
template <int R>
struct Nodes {
    int ix[2 * R + 2], ro[2 * R + 2];
    uint32_t cm, rm;
};

template <int R>
__device__ __forceinline__ Nodes<R> nodes_of(const ClParams& p, const Taps& t, bool usable) {
    Nodes<R> nd;
    nd.cm = 0; nd.rm = 0;
    const float fw = (float)p.wl, fh = (float)p.hl;
#pragma unroll
    for (int i = 0; i < 2 * R + 2; ++i) {
        const float cx = t.x_w + (float)(i - R), cy = t.y_n + (float)(i - R);
        const bool xok = usable && (cx > -1.0f) && (cx < fw);
        const bool yok = usable && (cy > -1.0f) && (cy < fh);
        nd.ix[i] = xok ? (int)cx : 0;
        nd.ro[i] = yok ? (int)cy * p.wl : 0;       // (hl * wl < 2^31)
        nd.cm |= (xok ? 1u : 0u) << i;
        nd.rm |= (yok ? 1u : 0u) << i;
    }
    return nd;
}

// One walk over the nodes of a window in a level plane `pl`: f(j * (2 R + 2) + i, inside, value), j then i ascending; the value of a
// node outside the frame is that of some element of the plane and is to be selected out
template <int R, class F>
__device__ __forceinline__ void walk_nodes(const float* pl, const Nodes<R>& nd, F&& f) {
    constexpr int NW = 2 * R + 2;
#pragma unroll
    for (int j = 0; j < NW; ++j) {
        uint32_t row = ((nd.rm >> j) & 1u) ? nd.cm : 0u;
        int ro = nd.ro[j];
        // (no instruction: the row's offset and mask count as made HERE, in the channel loop.  Otherwise the (2 R + 2)^2 node offsets
        // and inside tests, which do not depend on the channel, are all formed ahead of the loop and kept next to the sums: 168 VGPRs
        // and 596 B of scratch at R = 4)
        asm volatile("" : "+v"(ro), "+v"(row));
#pragma unroll
        for (int i = 0; i < NW; ++i) f(j * NW + i, ((row >> i) & 1u) != 0, pl[ro + nd.ix[i]]);
    }
}

template <int R, bool HALF>
__global__ void __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(kWavesPerSimd))) flow_corr_lookup_kernel(ClParams p) {
    constexpr int NW = 2 * R + 2, WIN = 2 * R + 1;
    const int64_t n_img = blockIdx.y;
    const int ty = (int)(blockIdx.x / (uint32_t)p.tiles_x), tx = (int)(blockIdx.x - (uint32_t)ty * (uint32_t)p.tiles_x);
    const int x = tx * kTileW + (int)(threadIdx.x % kTileW), y = ty * kTileH + (int)(threadIdx.x / kTileW);
    if (x >= p.w || y >= p.h) return;              // (no barrier in this kernel)
    Taps t;
    const bool us = win_of<HALF>(p, n_img, x, y, t);
    const Nodes<R> nd = nodes_of<R>(p, t, us);
    const int64_t pix = (int64_t)y * p.w + x;
    const float* ft = p.feat + n_img * p.feat_bs + pix;
    const float* ot = p.other + n_img * p.other_bs;
    float K[NW * NW];
#pragma unroll
    for (int k = 0; k < NW * NW; ++k) K[k] = 0.0f;
    float f_next = ft[0];
#pragma unroll 1
    for (int c = 0; c < p.chan; ++c) {
        const float f = f_next;
        if (c + 1 < p.chan) f_next = ft[(int64_t)(c + 1) * p.hw];     // the next channel's feature is on its way during the walk
        walk_nodes<R>(ot + (int64_t)c * p.hwl, nd, [&](int k, bool ok, float v) {
            const float prod = f * v;
            const float sum = K[k] + prod;
            K[k] = ok ? sum : K[k];                // a node outside the frame: +0, selected
        });
    }
    const float root = sqrt_rn((float)p.chan);
    float* out = p.out + n_img * p.out_bs + pix;
#pragma unroll
    for (int ox = 0; ox < WIN; ++ox) {             // the x offset is the outer index: RAFT's order
#pragma unroll
        for (int oy = 0; oy < WIN; ++oy) {
            const float val = sample_of(t, K[oy * NW + ox], K[oy * NW + ox + 1], K[(oy + 1) * NW + ox], K[(oy + 1) * NW + ox + 1]) / root;
            out[(int64_t)(ox * WIN + oy) * p.hw] = us ? val : 0.0f;
        }
    }
}

template <int R, bool HALF>
__global__ void __launch_bounds__(kThreads) flow_corr_lookup_nodes_kernel(ClParams p) {
    constexpr int NW = 2 * R + 2, WIN = 2 * R + 1;
    const int64_t n_img = blockIdx.y;
    const float root = sqrt_rn((float)p.chan);
    for (int64_t pix = (int64_t)blockIdx.x * kThreads + threadIdx.x; pix < p.hw; pix += (int64_t)gridDim.x * kThreads) {
        const int y = (int)(pix / p.w), x = (int)(pix - (int64_t)y * p.w);
        Taps t;
        const bool us = win_of<HALF>(p, n_img, x, y, t);
        float* gn = p.gn + n_img * (NW * NW) * p.hw + pix;
        if (us) {
            const float* g = p.g + n_img * p.g_bs + pix;
            float gs[WIN * WIN];                   // entry (dx, dy) at (dx + R) WIN + dy + R
#pragma unroll
            for (int o = 0; o < WIN * WIN; ++o) gs[o] = g[(int64_t)o * p.hw] / root;
#pragma unroll
            for (int j = 0; j < NW; ++j) {
#pragma unroll
                for (int i = 0; i < NW; ++i) {
                    float s = 0.0f;
                    if (j <= 2 * R && i <= 2 * R) { const float a = gs[i * WIN + j] * t.nw; s = s + a; }
                    if (j <= 2 * R && i >= 1) { const float a = gs[(i - 1) * WIN + j] * t.ne; s = s + a; }
                    if (j >= 1 && i <= 2 * R) { const float a = gs[i * WIN + j - 1] * t.sw; s = s + a; }
                    if (j >= 1 && i >= 1) { const float a = gs[(i - 1) * WIN + j - 1] * t.se; s = s + a; }
                    gn[(int64_t)(j * NW + i) * p.hw] = s;
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < NW * NW; ++k) gn[(int64_t)k * p.hw] = 0.0f;
        }
        if (p.keys != nullptr) {
            // the window's base (y_n - R, x_w - R) on the level's grid padded by 2 R + 1 to the north and west; the sentinel cell, the
            // last of the image, where the pixel is not usable or no node of its window lies in the frame
            const Nodes<R> nd = nodes_of<R>(p, t, us);
            const bool hit = nd.cm != 0 && nd.rm != 0;
            const int bx = hit ? (int)t.x_w - R : 0, by = hit ? (int)t.y_n - R : 0;
            const int64_t cell = hit ? (int64_t)(by + WIN) * (p.wl + WIN) + (bx + WIN) : p.cells - 1;
            p.keys[n_img * p.hw + pix] = (n_img * p.cells + cell) * p.hw + pix;
        }
    }
}

template <int R, bool HALF>
__global__ void __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(kWavesPerSimd))) flow_corr_lookup_grad_feat_kernel(ClParams p) {
    constexpr int NW = 2 * R + 2;
    const int64_t n_img = blockIdx.y;
    const int ty = (int)(blockIdx.x / (uint32_t)p.tiles_x), tx = (int)(blockIdx.x - (uint32_t)ty * (uint32_t)p.tiles_x);
    const int x = tx * kTileW + (int)(threadIdx.x % kTileW), y = ty * kTileH + (int)(threadIdx.x / kTileW);
    if (x >= p.w || y >= p.h) return;              // (no barrier in this kernel)
    Taps t;
    const bool us = win_of<HALF>(p, n_img, x, y, t);
    const Nodes<R> nd = nodes_of<R>(p, t, us);
    const int64_t pix = (int64_t)y * p.w + x;
    const float* gn = p.gn + n_img * (NW * NW) * p.hw + pix;
    const float* ot = p.other + n_img * p.other_bs;
    float* go = p.grad + n_img * p.chan * p.hw + pix;
    float G[NW * NW];
#pragma unroll
    for (int k = 0; k < NW * NW; ++k) G[k] = gn[(int64_t)k * p.hw];
#pragma unroll 1
    for (int c = 0; c < p.chan; ++c) {
        float acc = p.accumulate ? go[(int64_t)c * p.hw] : 0.0f;
        walk_nodes<R>(ot + (int64_t)c * p.hwl, nd, [&](int k, bool ok, float v) {
            const float prod = G[k] * v;
            const float sum = acc + prod;
            acc = ok ? sum : acc;                  // nodes outside the frame are skipped
        });
        go[(int64_t)c * p.hw] = us ? acc : 0.0f;
    }
}

template <int R>
__global__ void __launch_bounds__(kThreads) flow_corr_lookup_grad_other_kernel(ClParams p) {
    constexpr int NW = 2 * R + 2, WIN = 2 * R + 1;
    const int64_t n_img = blockIdx.z;
    const int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (q >= p.hwl) return;                        // (no barrier in this kernel)
    const int qy = (int)(q / p.wl), qx = (int)(q - (int64_t)qy * p.wl);
    const int c0 = (int)blockIdx.y * kChanChunk;
    const float* gn = p.gn + n_img * (NW * NW) * p.hw;
    const float* ft = p.feat + n_img * p.feat_bs + (int64_t)c0 * p.hw;
    const int64_t* st = p.starts + n_img * p.cells;
    const int64_t first = n_img * p.hw;
    float acc[kChanChunk];
#pragma unroll
    for (int k = 0; k < kChanChunk; ++k) acc[k] = 0.0f;
#pragma unroll 1
    for (int j = 0; j < NW; ++j) {
#pragma unroll 1
        for (int i = 0; i < NW; ++i) {
            const int64_t cell = (int64_t)(qy - j + WIN) * (p.wl + WIN) + (qx - i + WIN);      // (never the sentinel)
            int64_t s = st[cell], e = st[cell + 1];
            s = s < 0 ? 0 : s;
            e = e > p.total ? p.total : e;         // a list is a run of the sorted keys: what is handed in cannot lead outside them
            const float* gp = gn + (int64_t)(j * NW + i) * p.hw;
            // kListStep entries of the list at a time: their loads are independent of the sums and go out together, the sums then
            // take them in list order (one entry at a time the walk is a chain of three load latencies per term)
            for (; s < e; s += kListStep) {
                int64_t pix[kListStep];
                bool ok[kListStep];
                float gv[kListStep], fv[kListStep][kChanChunk];
#pragma unroll
                for (int u = 0; u < kListStep; ++u) {
                    const int64_t at = s + u < e ? p.order[s + u] - first : -1;
                    ok[u] = at >= 0 && at < p.hw;
                    pix[u] = ok[u] ? at : 0;
                }
#pragma unroll
                for (int u = 0; u < kListStep; ++u) {
                    gv[u] = gp[pix[u]];
#pragma unroll
                    for (int k = 0; k < kChanChunk; ++k) fv[u][k] = c0 + k < p.chan ? ft[(int64_t)k * p.hw + pix[u]] : 0.0f;
                }
#pragma unroll
                for (int u = 0; u < kListStep; ++u) {
#pragma unroll
                    for (int k = 0; k < kChanChunk; ++k) {
                        const float prod = gv[u] * fv[u][k];
                        const float sum = acc[k] + prod;
                        acc[k] = ok[u] ? sum : acc[k];
                    }
                }
            }
        }
    }
    float* go = p.grad + (n_img * p.chan + c0) * p.hwl + q;
#pragma unroll
    for (int k = 0; k < kChanChunk; ++k) {
        if (c0 + k < p.chan) go[(int64_t)k * p.hwl] = acc[k];
    }
}

int64_t tiles_of(int32_t extent, int tile) { return ((int64_t)extent + tile - 1) / tile; }

// cells of a level's padded grid plus the sentinel; 0 where the level or the radius is not accepted
int64_t cells_of(int32_t hl, int32_t wl, int32_t radius) {
    if (radius < 1 || radius > kMaxRadius || hl < 1 || wl < 1 || hl > kMaxLevelExtent || wl > kMaxLevelExtent) return 0;
    if ((int64_t)hl * wl >= (1ll << 31)) return 0;
    return ((int64_t)hl + 2 * radius + 1) * ((int64_t)wl + 2 * radius + 1) + 1;
}

// the frame, the level and the window: the fields and the checks every entry point shares
int fill_frame(ClParams* p, int32_t channels, int32_t radius, int32_t level, int32_t hl, int32_t wl, int32_t n, int32_t h, int32_t w) {
    if (!dims_ok(n, h, w, 1)) return OFL_E_ARG;
    if (channels < 1 || level < 0 || level > kMaxLevel) return OFL_E_ARG;
    const int64_t cells = cells_of(hl, wl, radius);
    if (cells == 0) return OFL_E_ARG;
    if ((double)n * (double)cells * (double)h * (double)w >= 4.0e18) return OFL_E_ARG;       // the keys are 63-bit
    p->flow = nullptr; p->flow_bs = 0; p->mask = nullptr; p->mask_bs = 0;
    p->feat = nullptr; p->other = nullptr; p->feat_bs = 0; p->other_bs = 0;
    p->hw = (int64_t)h * w; p->hwl = (int64_t)hl * wl;
    p->chan = channels; p->h = h; p->w = w; p->hl = hl; p->wl = wl;
    p->tiles_x = (int32_t)tiles_of(w, kTileW);
    p->flow_sign = 0.0f;
    p->scale = 1.0f / (float)(1 << level);
    p->out = nullptr; p->out_bs = 0; p->g = nullptr; p->g_bs = 0; p->gn = nullptr; p->keys = nullptr;
    p->cells = cells;
    p->grad = nullptr; p->accumulate = 0; p->order = nullptr; p->starts = nullptr;
    p->total = (int64_t)n * p->hw;
    return OFL_OK;
}

int fill_flow(ClParams* p, const void* flow, int64_t flow_bs, int32_t flow_half, const uint8_t* mask, int64_t mask_bs, float flow_sign) {
    if (flow_sign != 1.0f && flow_sign != -1.0f) return OFL_E_ARG;
    if (flow == nullptr) return OFL_E_ARG;
    if (flow_half != 0 && flow_half != 1) return OFL_E_ARG;
    if (flow_bs < 0 || mask_bs < 0) return OFL_E_ARG;
    if (!aligned(flow, flow_half ? 2 : 4)) return OFL_E_ARG;
    p->flow = flow; p->flow_bs = flow_bs;
    p->mask = mask; p->mask_bs = mask_bs;
    p->flow_sign = flow_sign;
    return OFL_OK;
}

// the grid of the per-pixel pass: 256 pixels per block, grid-stride beyond the cap
dim3 pixel_grid_of(int32_t n, int32_t h, int32_t w) {
    const int64_t blocks = ((int64_t)h * w + kThreads - 1) / kThreads;
    return dim3((unsigned)(blocks < 65536 ? blocks : 65536), (unsigned)n);
}

dim3 grid_of(int32_t n, int32_t h, int32_t w) {
    return dim3((unsigned)(tiles_of(w, kTileW) * tiles_of(h, kTileH)), (unsigned)n);     // (h * w < 2^31: under 2^23 tiles)
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

__attribute__((visibility("default"))) int64_t ofl_flow_corr_lookup_cells(int32_t level_h, int32_t level_w, int32_t radius) {
    const int64_t cells = cells_of(level_h, level_w, radius);
    return cells == 0 ? (int64_t)OFL_E_ARG : cells;
}

__attribute__((visibility("default"))) int ofl_flow_corr_lookup_f32(const void* flow, int64_t flow_bs, int32_t flow_half, const uint8_t* mask,
                                                                    int64_t mask_bs, const float* feat, int64_t feat_bs, const float* other,
                                                                    int64_t other_bs, int32_t channels, float flow_sign, int32_t radius,
                                                                    int32_t level, int32_t level_h, int32_t level_w, float* out,
                                                                    int64_t out_bs, int32_t n, int32_t h, int32_t w, void* stream) {
    ClParams p;
    int rc = fill_frame(&p, channels, radius, level, level_h, level_w, n, h, w);
    if (rc) return rc;
    rc = fill_flow(&p, flow, flow_bs, flow_half, mask, mask_bs, flow_sign);
    if (rc) return rc;
    if (feat == nullptr || other == nullptr || out == nullptr) return OFL_E_ARG;
    if (feat_bs < 0 || other_bs < 0) return OFL_E_ARG;
    if (!aligned(feat, 4) || !aligned(other, 4) || !aligned(out, 4)) return OFL_E_ARG;
    const int64_t d = (int64_t)(2 * radius + 1) * (2 * radius + 1);
    if (out_bs < d * p.hw) return OFL_E_ARG;
    p.feat = feat; p.feat_bs = feat_bs; p.other = other; p.other_bs = other_bs;
    p.out = out; p.out_bs = out_bs;
    hipStream_t s = (hipStream_t)stream;
    dispatch(radius, flow_half != 0, [&](auto RR, auto HALF) {
        OFL_KLAUNCH((flow_corr_lookup_kernel<decltype(RR)::value, decltype(HALF)::value>), grid_of(n, h, w), dim3(kThreads), 0, s, p);
    });
    return (int)hipGetLastError();
}

__attribute__((visibility("default"))) int ofl_flow_corr_lookup_nodes_f32(const void* flow, int64_t flow_bs, int32_t flow_half,
                                                                          const uint8_t* mask, int64_t mask_bs, int32_t channels,
                                                                          float flow_sign, int32_t radius, int32_t level, int32_t level_h,
                                                                          int32_t level_w, const float* grad_out, int64_t grad_bs,
                                                                          float* nodes, int64_t* keys, int32_t n, int32_t h, int32_t w,
                                                                          void* stream) {
    ClParams p;
    int rc = fill_frame(&p, channels, radius, level, level_h, level_w, n, h, w);
    if (rc) return rc;
    rc = fill_flow(&p, flow, flow_bs, flow_half, mask, mask_bs, flow_sign);
    if (rc) return rc;
    if (grad_out == nullptr || nodes == nullptr) return OFL_E_ARG;
    if (!aligned(grad_out, 4) || !aligned(nodes, 4) || !aligned(keys, 8)) return OFL_E_ARG;
    const int64_t d = (int64_t)(2 * radius + 1) * (2 * radius + 1);
    if (grad_bs < d * p.hw) return OFL_E_ARG;
    p.g = grad_out; p.g_bs = grad_bs; p.gn = nodes; p.keys = keys;
    hipStream_t s = (hipStream_t)stream;
    dispatch(radius, flow_half != 0, [&](auto RR, auto HALF) {
        OFL_KLAUNCH((flow_corr_lookup_nodes_kernel<decltype(RR)::value, decltype(HALF)::value>), pixel_grid_of(n, h, w), dim3(kThreads), 0,
                    s, p);
    });
    return (int)hipGetLastError();
}

__attribute__((visibility("default"))) int ofl_flow_corr_lookup_grad_feat_f32(const void* flow, int64_t flow_bs, int32_t flow_half,
                                                                              const uint8_t* mask, int64_t mask_bs, const float* other,
                                                                              int64_t other_bs, int32_t channels, float flow_sign,
                                                                              int32_t radius, int32_t level, int32_t level_h,
                                                                              int32_t level_w, const float* nodes, float* grad_feat,
                                                                              int32_t accumulate, int32_t n, int32_t h, int32_t w,
                                                                              void* stream) {
    ClParams p;
    int rc = fill_frame(&p, channels, radius, level, level_h, level_w, n, h, w);
    if (rc) return rc;
    rc = fill_flow(&p, flow, flow_bs, flow_half, mask, mask_bs, flow_sign);
    if (rc) return rc;
    if (other == nullptr || nodes == nullptr || grad_feat == nullptr) return OFL_E_ARG;
    if (other_bs < 0 || (accumulate != 0 && accumulate != 1)) return OFL_E_ARG;
    if (!aligned(other, 4) || !aligned(nodes, 4) || !aligned(grad_feat, 4)) return OFL_E_ARG;
    p.other = other; p.other_bs = other_bs;
    p.gn = const_cast<float*>(nodes); p.grad = grad_feat; p.accumulate = accumulate;
    hipStream_t s = (hipStream_t)stream;
    dispatch(radius, flow_half != 0, [&](auto RR, auto HALF) {
        OFL_KLAUNCH((flow_corr_lookup_grad_feat_kernel<decltype(RR)::value, decltype(HALF)::value>), grid_of(n, h, w), dim3(kThreads), 0, s,
                    p);
    });
    return (int)hipGetLastError();
}

__attribute__((visibility("default"))) int ofl_flow_corr_lookup_grad_other_f32(const float* feat, int64_t feat_bs, int32_t channels,
                                                                               int32_t radius, int32_t level_h, int32_t level_w,
                                                                               const float* nodes, const int64_t* order,
                                                                               const int64_t* starts, float* grad_other, int32_t n,
                                                                               int32_t h, int32_t w, void* stream) {
    ClParams p;
    const int rc = fill_frame(&p, channels, radius, 0, level_h, level_w, n, h, w);
    if (rc) return rc;
    if (feat == nullptr || nodes == nullptr || order == nullptr || starts == nullptr || grad_other == nullptr) return OFL_E_ARG;
    if (feat_bs < 0) return OFL_E_ARG;
    if (!aligned(feat, 4) || !aligned(nodes, 4) || !aligned(order, 8) || !aligned(starts, 8) || !aligned(grad_other, 4)) return OFL_E_ARG;
    const int64_t chunks = ((int64_t)channels + kChanChunk - 1) / kChanChunk;
    if (chunks > 65535) return OFL_E_ARG;
    p.feat = feat; p.feat_bs = feat_bs;
    p.gn = const_cast<float*>(nodes); p.order = order; p.starts = starts; p.grad = grad_other;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((p.hwl + kThreads - 1) / kThreads), (unsigned)chunks, (unsigned)n);
    auto launch = [&](auto RR) {
        OFL_KLAUNCH((flow_corr_lookup_grad_other_kernel<decltype(RR)::value>), grid, dim3(kThreads), 0, s, p);
    };
    if (radius == 1) launch(std::integral_constant<int, 1>{});
    else if (radius == 2) launch(std::integral_constant<int, 2>{});
    else if (radius == 3) launch(std::integral_constant<int, 3>{});
    else launch(std::integral_constant<int, 4>{});
    return (int)hipGetLastError();
}

}  // extern "C"
