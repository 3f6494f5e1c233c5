// ofl_local_match.hip -- Flow.match_local on gfx950: the local matching of GMFlow's and UniMatch's refinement stage -- warp the other
// frame's features by the flow, correlate every pixel with the (2 r + 1)^2 window of the warped features around it, take the softmax of
// the window over sqrt(C) and add the expected offset to the flow -- in one pass, without the warped tensor, the D planes of the volume
// or the unfold (which DEFINES the numbers; tests/local_match_oracle.py is the same definition in NumPy).  An extension:
// the reference has no such function.
//
//   flow_local_match_kernel<R, HALF, GRAD>        a tile of kTileW x kTileH pixels, one per lane (the shape of flow_propagate_local_kernel,
//                                                 ofl_propagate.hip).  For a chunk of kChanChunk channels the block stages W' -- `other`
//                                                 sampled where the flow points, +0 where the pixel is not usable or outside the frame --
//                                                 of the tile and a halo of R pixels in LDS (the staging of ofl_cost_volume.hip: one
//                                                 taps_of() per staged pixel and chunk, four global taps per channel); the D dot products
//                                                 of a lane's pixel stay in registers.  The logits then go into a lane-private LDS column
//                                                 that reuses the staging buffer, and the two passes of the softmax over the positions
//                                                 INSIDE the frame (a coordinate test; a position outside takes no part) or, with GRAD,
//                                                 dss of every offset walk them in rolled loops
//   flow_local_match_gather_kernel<R, HALF, TO_W> the gradients with respect to feat (TO_W false) and to the warped tensor W (TO_W true)
//                                                 as gathers from that workspace: flow_cost_volume_grad_kernel of ofl_cost_volume.hip with
//                                                 dss in the place of g / C -- a tile of kGTileW x kGTileH pixels, two per lane, one above
//                                                 the other
//
// d other and the warp's part of d flow come from d W through the backward of the cost volume, unchanged (ofl_flow_cost_volume_chain_f32,
// ofl_warp_bwd_grad_f32, ofl_flow_cost_volume_gate_f32).  No float atomics and no scatter: every sum has one owner and a fixed order that
// no tile size enters.  usable_of / stage_warp / stage_feat / walk are those of ofl_cost_volume.hip, e_of is that of ofl_propagate.hip,
// copied (the tile has become a template argument): those files' code is left as it was compiled.
//
// LDS.  The forward parks D logits per pixel: D * kThreads floats, 41 472 B at R = 4 for 128 pixels.  The 32 x 16 tile of the cost
// volume (512 pixels, 165 888 B) does not fit what a block may declare; 32 x 4 does, and the staged chunk ((32 + 2 R) x (4 + 2 R) x
// kChanChunk floats, 30 720 B at R = 4) fits inside it.  The gathers keep the cost volume's tile and its 61 440 B.
//
// Every product is rounded, then every sum: fp contraction is off (ofl_loss_common.hpp) and no fmaf is written here.  C ABI:
// include/oflib_hip.h.
#include "ofl_loss_common.hpp"

namespace {

using namespace ofl_loss;

constexpr int kTileW = 32, kTileH = 4;             // the forward's tile: one pixel per thread
constexpr int kThreads = kTileW * kTileH;
constexpr int kChanChunk = 16;                     // channels staged together, forward and gathers
constexpr int kGTileW = 32, kGTileH = 16;          // the gathers' tile
constexpr int kGThreads = 256;
constexpr int kPix = 2;                            // pixels per lane of a gather: rows 2 k and 2 k + 1 of its tile, k = thread / kGTileW
constexpr int kMaxRadius = 4;
constexpr int kLdsLimit = 64 * 1024;               // bytes of LDS a block may declare

static_assert(kGThreads * kPix == kGTileW * kGTileH, "a lane of a gather owns kPix vertically adjacent pixels of the tile");
static_assert((2 * kMaxRadius + 1) * (2 * kMaxRadius + 1) * kThreads * 4 <= kLdsLimit, "the parked logits of the forward's tile");
static_assert(kChanChunk * (kTileW + 2 * kMaxRadius) * (kTileH + 2 * kMaxRadius) * 4 <= kLdsLimit, "the forward's staged chunk");
static_assert(kChanChunk * (kGTileW + 2 * kMaxRadius) * (kGTileH + 2 * kMaxRadius) * 4 <= kLdsLimit, "the gathers' staged chunk");

struct LmParams {
    const void* flow;                              // [*,2,H,W] fp32 or fp16
    int64_t flow_bs;                               // elements between images
    const uint8_t* mask;                           // [*,H,W] bytes or nullptr (all True)
    int64_t mask_bs;
    const float* feat; const float* other;         // [*,C,H,W]: the features on the flow's grid, those of the frame it points into
    int64_t feat_bs, other_bs;
    int64_t hw, nhw;                               // H W; n H W
    int32_t chan, h, w, tiles_x;
    float flow_sign;
    float wm1, hm1, half_wm1, half_hm1;
    float* out;                                    // forward: [n][2][H W]
    float* prob;                                   // forward: [n][H W]; or nullptr
    double* ws_d;                                  // the statistics' float64 part [3][n][H W]: S, ox, oy; or nullptr
    float* ws_m;                                   // their float32 part [n][H W]: m
    const float* g;                                // backward: the upstream gradient [n][2][H W]
    float* scratch;                                // backward: dss [n][D][H W]
    float* grad;                                   // backward: d feat or d W [n][C][H W]
};

// is the sample of pixel (x, y) of image n_img usable: valid in the mask and the weight sum of its taps inside the frame above kValidThr
// (ofl_cost_volume.hip)
template <bool HALF>
__device__ __forceinline__ bool usable_of(const LmParams& p, int64_t n_img, int x, int y, Taps& t) {
    const int64_t pix = (int64_t)y * p.w + x, fo = n_img * p.flow_bs;
    const float u = ld_flow<HALF>(p.flow, fo + pix), v = ld_flow<HALF>(p.flow, fo + p.hw + pix);
    const bool valid = p.mask == nullptr || p.mask[n_img * p.mask_bs + pix] != 0;
    t = taps_of(p, x, y, u, v);
    return (t.mr > kValidThr) && valid;
}

// W' of the channels c0 .. c0 + nc - 1 (plane k of s_w holds channel c0 + k) of the TW x TH tile at (x0, y0) and R pixels around it: the
// sample where the pixel is usable, +0 elsewhere and outside the frame (selected, not multiplied: a pixel that is not usable loads no
// sample)
template <int R, bool HALF, int TW, int TH, int THREADS>
__device__ __forceinline__ void stage_warp(const LmParams& p, int64_t n_img, int x0, int y0, int c0, int nc, float* s_w) {
    constexpr int RW = TW + 2 * R, RH = TH + 2 * R;
    const float* ot = p.other + n_img * p.other_bs + (int64_t)c0 * p.hw;
    for (int i = threadIdx.x; i < RW * RH; i += THREADS) {
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
template <int R, int TW, int TH, int THREADS>
__device__ __forceinline__ void stage_feat(const LmParams& p, int64_t n_img, int x0, int y0, int c0, int nc, float* s_w) {
    constexpr int RW = TW + 2 * R, RH = TH + 2 * R;
    const float* ft = p.feat + n_img * p.feat_bs + (int64_t)c0 * p.hw;
    for (int i = threadIdx.x; i < RW * RH; i += THREADS) {
        const int ry = i / RW, rx = i - ry * RW;
        const int x = x0 - R + rx, y = y0 - R + ry;
        const bool in = x >= 0 && x < p.w && y >= 0 && y < p.h;
        const int64_t pix = in ? (int64_t)y * p.w + x : 0;
#pragma unroll 4
        for (int k = 0; k < nc; ++k) s_w[k * RW * RH + i] = in ? ft[(int64_t)k * p.hw + pix] : 0.0f;
    }
}

// e = exp((double)s - (double)m) in float64 (ofl_propagate.hip)
__device__ __forceinline__ double e_of(float s, float m) { return exp((double)s - (double)m); }

template <int R>
struct Local {
    static constexpr int kSide = 2 * R + 1;
    static constexpr int kD = kSide * kSide;
    static constexpr int kHaloW = kTileW + 2 * R;
    static constexpr int kHaloH = kTileH + 2 * R;
    static constexpr int kHalo = kHaloW * kHaloH;
    static constexpr int kLds = kChanChunk * kHalo > kD * kThreads ? kChanChunk * kHalo : kD * kThreads;    // floats: W', then the logits
};

template <int R, bool HALF, bool GRAD>
__global__ void __launch_bounds__(kThreads) flow_local_match_kernel(LmParams p) {
    using L = Local<R>;
    __shared__ float s_buf[L::kLds];
    const int64_t n_img = blockIdx.y;
    const int tid = (int)threadIdx.x;
    const int lx = tid % kTileW, ly = tid / kTileW;
    const int tile_y = (int)(blockIdx.x / (unsigned)p.tiles_x), tile_x = (int)(blockIdx.x - (unsigned)tile_y * (unsigned)p.tiles_x);
    const int x0 = tile_x * kTileW, y0 = tile_y * kTileH;
    const int x = x0 + lx, y = y0 + ly;
    const bool live = x < p.w && y < p.h;
    // (a lane beyond the frame computes on the nearest pixel's features and stores nothing; its window is taken at (x, y) all the same)
    const int64_t pix = (int64_t)(y < p.h ? y : p.h - 1) * p.w + (x < p.w ? x : p.w - 1);
    const float* own = p.feat + n_img * p.feat_bs + pix;
    const float root = sqrt_rn((float)p.chan);
    float acc[L::kD];
#pragma unroll
    for (int o = 0; o < L::kD; ++o) acc[o] = 0.0f;
#pragma unroll 1
    for (int c0 = 0; c0 < p.chan; c0 += kChanChunk) {
        const int cc = p.chan - c0 < kChanChunk ? p.chan - c0 : kChanChunk;
        __syncthreads();                           // (the chunk before has been read)
        stage_warp<R, HALF, kTileW, kTileH, kThreads>(p, n_img, x0, y0, c0, cc, s_buf);
        __syncthreads();
#pragma unroll 1
        for (int c = 0; c < cc; ++c) {
            const float fv = own[(int64_t)(c0 + c) * p.hw];
            const float* base = s_buf + c * L::kHalo + ly * L::kHaloW + lx;
#pragma unroll
            for (int o = 0; o < L::kD; ++o) {
                const float prod = fv * base[(o / L::kSide) * L::kHaloW + o % L::kSide];
                acc[o] = acc[o] + prod;
            }
        }
    }
    __syncthreads();                               // (the last chunk has been read: the buffer becomes the logits' columns)
    float* col = s_buf + tid;
#pragma unroll
    for (int o = 0; o < L::kD; ++o) col[o * kThreads] = acc[o] / root;
    // (from here on a lane reads its own column only: no barrier)
    if (!GRAD) {
        float m = 0.0f;
        bool started = false;
        {
            int dy = -R, dx = -R;
#pragma unroll 1
            for (int o = 0; o < L::kD; ++o) {
                const int qy = y + dy, qx = x + dx;
                if (qy >= 0 && qy < p.h && qx >= 0 && qx < p.w) {
                    const float s = col[o * kThreads];
                    if (!started) { m = s; started = true; }
                    else if (s > m) m = s;
                }
                if (++dx > R) { dx = -R; ++dy; }
            }
        }
        double S = 0.0, X = 0.0, Y = 0.0;
        {
            int dy = -R, dx = -R;
#pragma unroll 1
            for (int o = 0; o < L::kD; ++o) {
                const int qy = y + dy, qx = x + dx;
                if (qy >= 0 && qy < p.h && qx >= 0 && qx < p.w) {
                    const double e = e_of(col[o * kThreads], m);
                    const double ex = e * (double)dx, ey = e * (double)dy;
                    S = S + e; X = X + ex; Y = Y + ey;
                }
                if (++dx > R) { dx = -R; ++dy; }
            }
        }
        if (!live) return;
        const double ox = X / S, oy = Y / S;
        const int64_t fo = n_img * p.flow_bs;
        const double u = (double)ld_flow<HALF>(p.flow, fo + pix), v = (double)ld_flow<HALF>(p.flow, fo + p.hw + pix);
        const double sg = -(double)p.flow_sign;
        const double mx = sg * ox, my = sg * oy;
        float* out = p.out + n_img * 2 * p.hw + pix;
        out[0] = (float)(u + mx);
        out[p.hw] = (float)(v + my);
        if (p.prob != nullptr) p.prob[n_img * p.hw + pix] = (float)(1.0 / S);
        if (p.ws_d != nullptr) {
            double* wd = p.ws_d + n_img * p.hw + pix;
            wd[0] = S; wd[p.nhw] = ox; wd[2 * p.nhw] = oy;
            p.ws_m[n_img * p.hw + pix] = m;
        }
    } else {
        const double* wd = p.ws_d + n_img * p.hw + pix;
        const float m = p.ws_m[n_img * p.hw + pix];
        const double S = wd[0], ox = wd[p.nhw], oy = wd[2 * p.nhw];
        const float* g = p.g + n_img * 2 * p.hw + pix;
        const double sg = -(double)p.flow_sign;
        const double Gx = sg * (double)g[0], Gy = sg * (double)g[p.hw];
        float* sc = p.scratch + n_img * L::kD * p.hw + pix;
        int dy = -R, dx = -R;
#pragma unroll 1
        for (int o = 0; o < L::kD; ++o) {
            const int qy = y + dy, qx = x + dx;
            const bool in = qy >= 0 && qy < p.h && qx >= 0 && qx < p.w;
            const double wt = e_of(col[o * kThreads], m) / S;
            const double ax = Gx * ((double)dx - ox), ay = Gy * ((double)dy - oy);
            const double t = ax + ay;
            const float ds = (float)(wt * t);
            if (live) sc[(int64_t)o * p.hw] = in ? ds / root : 0.0f;   // (a position outside the frame has no gradient: selected)
            if (++dx > R) { dx = -R; ++dy; }
        }
    }
}

// One walk of the windows of a lane's two pixels over one staged plane: `s` points at the window's first row and column of the upper
// pixel (pitch RW), f(pixel, o, value) is called for both pixels with o ascending.  FLIP false: window position o holds the staged pixel
// p + o; FLIP true: p - o (the walk goes back to front).  A row read serves both pixels.  (ofl_cost_volume.hip)
template <int R, bool FLIP, class F>
__device__ __forceinline__ void walk(const float* s, F&& f) {
    constexpr int WIN = 2 * R + 1, D = WIN * WIN, RW = kGTileW + 2 * R;
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

template <int R, bool HALF, bool TO_W>
__global__ void __launch_bounds__(kGThreads) flow_local_match_gather_kernel(LmParams p) {
    constexpr int WIN = 2 * R + 1, D = WIN * WIN, RW = kGTileW + 2 * R, RH = kGTileH + 2 * R;
    __shared__ float s_w[kChanChunk * RW * RH];
    const int64_t n_img = blockIdx.y;
    const int ty = (int)(blockIdx.x / (uint32_t)p.tiles_x), tx = (int)(blockIdx.x - (uint32_t)ty * (uint32_t)p.tiles_x);
    const int x0 = tx * kGTileW, y0 = ty * kGTileH;
    const int lx = threadIdx.x % kGTileW, row = kPix * (threadIdx.x / kGTileW);
    const int x = x0 + lx, y = y0 + row;
    const bool in[kPix] = {x < p.w && y < p.h, x < p.w && y + 1 < p.h};
    // dss of the lane's two pixels: plane o at the pixel itself, or at q - o for the gradient of W (0 where that is outside the frame)
    const float* sc = p.scratch + n_img * D * p.hw;
    float d[kPix][D];
#pragma unroll
    for (int px = 0; px < kPix; ++px) {
#pragma unroll
        for (int o = 0; o < D; ++o) {
            const int dy = o / WIN - R, dx = o % WIN - R;
            const int gx = TO_W ? x - dx : x, gy = TO_W ? y + px - dy : y + px;
            const bool ok = in[px] && gx >= 0 && gx < p.w && gy >= 0 && gy < p.h;
            d[px][o] = ok ? sc[(int64_t)o * p.hw + (int64_t)gy * p.w + gx] : 0.0f;
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
        if (TO_W) stage_feat<R, kGTileW, kGTileH, kGThreads>(p, n_img, x0, y0, c0, nc, s_w);
        else stage_warp<R, HALF, kGTileW, kGTileH, kGThreads>(p, n_img, x0, y0, c0, nc, s_w);
        __syncthreads();
#pragma unroll 1
        for (int k = 0; k < nc; ++k) {
            float sum[kPix] = {0.0f, 0.0f};
            walk<R, TO_W>(s_w + k * RW * RH + row * RW + lx, [&](int px, int o, float v) {
                const float prod = d[px][o] * v;
                sum[px] = sum[px] + prod;
            });
            if (in[0]) go[(int64_t)(c0 + k) * p.hw] = keep[0] ? sum[0] : 0.0f;
            if (in[1]) go[(int64_t)(c0 + k) * p.hw + p.w] = keep[1] ? sum[1] : 0.0f;
        }
    }
}

int64_t tiles_of(int32_t extent, int tile) { return ((int64_t)extent + tile - 1) / tile; }

// the operands and the checks both entry points share
int fill_operands(LmParams* p, const void* flow, int64_t flow_bs, int32_t flow_half, const uint8_t* mask, int64_t mask_bs, const float* feat,
                  int64_t feat_bs, const float* other, int64_t other_bs, int32_t channels, float flow_sign, int32_t radius, int32_t n,
                  int32_t h, int32_t w) {
    if (!dims_ok(n, h, w, 2)) return OFL_E_ARG;
    if (flow_sign != 1.0f && flow_sign != -1.0f) return OFL_E_ARG;
    if (flow == nullptr || feat == nullptr || other == nullptr) return OFL_E_ARG;
    if (flow_half != 0 && flow_half != 1) return OFL_E_ARG;
    if (radius < 1 || radius > kMaxRadius || channels < 1) return OFL_E_ARG;
    if (flow_bs < 0 || mask_bs < 0 || feat_bs < 0 || other_bs < 0) return OFL_E_ARG;
    if (!aligned(flow, flow_half ? 2 : 4) || !aligned(feat, 4) || !aligned(other, 4)) return OFL_E_ARG;
    p->flow = flow; p->flow_bs = flow_bs;
    p->mask = mask; p->mask_bs = mask_bs;
    p->feat = feat; p->other = other; p->feat_bs = feat_bs; p->other_bs = other_bs;
    p->hw = (int64_t)h * w; p->nhw = (int64_t)n * p->hw;
    p->chan = channels; p->h = h; p->w = w;
    p->tiles_x = (int32_t)tiles_of(w, kTileW);
    p->flow_sign = flow_sign;
    p->wm1 = (float)(w - 1); p->hm1 = (float)(h - 1);
    p->half_wm1 = p->wm1 / 2.0f; p->half_hm1 = p->hm1 / 2.0f;
    p->out = nullptr; p->prob = nullptr; p->ws_d = nullptr; p->ws_m = nullptr; p->g = nullptr; p->scratch = nullptr; p->grad = nullptr;
    return OFL_OK;
}

// the statistics [3][n][H W] float64, then [n][H W] float32
void fill_workspace(LmParams* p, void* workspace) {
    p->ws_d = reinterpret_cast<double*>(workspace);
    p->ws_m = workspace == nullptr ? nullptr : reinterpret_cast<float*>(p->ws_d + 3 * p->nhw);
}

dim3 grid_of(int32_t n, int32_t h, int32_t w) {
    return dim3((unsigned)(tiles_of(w, kTileW) * tiles_of(h, kTileH)), (unsigned)n);        // (h * w < 2^31: under 2^24 tiles)
}

dim3 gather_grid_of(int32_t n, int32_t h, int32_t w) {
    return dim3((unsigned)(tiles_of(w, kGTileW) * tiles_of(h, kGTileH)), (unsigned)n);
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

__attribute__((visibility("default"))) int ofl_flow_local_match_f32(const void* flow, int64_t flow_bs, int32_t flow_half, const uint8_t* mask,
                                                                    int64_t mask_bs, const float* feat, int64_t feat_bs, const float* other,
                                                                    int64_t other_bs, int32_t channels, float flow_sign, int32_t radius,
                                                                    float* out, float* prob, void* workspace, int32_t n, int32_t h,
                                                                    int32_t w, void* stream) {
    LmParams p;
    const int rc = fill_operands(&p, flow, flow_bs, flow_half, mask, mask_bs, feat, feat_bs, other, other_bs, channels, flow_sign, radius,
                                 n, h, w);
    if (rc) return rc;
    if (out == nullptr) return OFL_E_ARG;
    if (!aligned(out, 4) || !aligned(prob, 4) || !aligned(workspace, 8)) return OFL_E_ARG;
    p.out = out; p.prob = prob;
    fill_workspace(&p, workspace);
    hipStream_t s = (hipStream_t)stream;
    dispatch(radius, flow_half != 0, [&](auto RR, auto HALF) {
        OFL_KLAUNCH((flow_local_match_kernel<decltype(RR)::value, decltype(HALF)::value, false>), grid_of(n, h, w), dim3(kThreads), 0, s,
                    p);
    });
    return (int)hipGetLastError();
}

__attribute__((visibility("default"))) int ofl_flow_local_match_grad_f32(const void* flow, int64_t flow_bs, int32_t flow_half,
                                                                         const uint8_t* mask, int64_t mask_bs, const float* feat,
                                                                         int64_t feat_bs, const float* other, int64_t other_bs,
                                                                         int32_t channels, float flow_sign, int32_t radius,
                                                                         const void* workspace, const float* grad_out, float* scratch,
                                                                         float* grad_feat, float* grad_warped, int32_t n, int32_t h,
                                                                         int32_t w, void* stream) {
    LmParams p;
    const int rc = fill_operands(&p, flow, flow_bs, flow_half, mask, mask_bs, feat, feat_bs, other, other_bs, channels, flow_sign, radius,
                                 n, h, w);
    if (rc) return rc;
    if (workspace == nullptr || grad_out == nullptr || scratch == nullptr) return OFL_E_ARG;
    if (grad_feat == nullptr && grad_warped == nullptr) return OFL_E_ARG;
    if (!aligned(workspace, 8) || !aligned(grad_out, 4) || !aligned(scratch, 4) || !aligned(grad_feat, 4) || !aligned(grad_warped, 4)) {
        return OFL_E_ARG;
    }
    fill_workspace(&p, const_cast<void*>(workspace));
    p.g = grad_out; p.scratch = scratch;
    hipStream_t s = (hipStream_t)stream;
    dispatch(radius, flow_half != 0, [&](auto RR, auto HALF) {
        OFL_KLAUNCH((flow_local_match_kernel<decltype(RR)::value, decltype(HALF)::value, true>), grid_of(n, h, w), dim3(kThreads), 0, s, p);
    });
    p.tiles_x = (int32_t)tiles_of(w, kGTileW);
    if (grad_feat != nullptr) {
        p.grad = grad_feat;
        dispatch(radius, flow_half != 0, [&](auto RR, auto HALF) {
            OFL_KLAUNCH((flow_local_match_gather_kernel<decltype(RR)::value, decltype(HALF)::value, false>), gather_grid_of(n, h, w),
                        dim3(kGThreads), 0, s, p);
        });
    }
    if (grad_warped != nullptr) {
        p.grad = grad_warped;
        dispatch(radius, flow_half != 0, [&](auto RR, auto HALF) {
            OFL_KLAUNCH((flow_local_match_gather_kernel<decltype(RR)::value, decltype(HALF)::value, true>), gather_grid_of(n, h, w),
                        dim3(kGThreads), 0, s, p);
        });
    }
    return (int)hipGetLastError();
}

}  // extern "C"
