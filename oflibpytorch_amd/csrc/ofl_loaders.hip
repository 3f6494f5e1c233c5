// ofl_loaders.hip -- the device half of the dataset loaders: Flow.from_kitti / Flow.from_sintel on gfx950.
// The host has inflated and unfiltered the file (ofl_png_host.cpp) or read the .flo payload; what the reference then does in NumPy --
// channel flip, float64 copy, (x - 2^15) / 64, the valid write, the transpose to planes, the fp32 conversion -- and what Flow(...) adds
// (the finiteness and zero-flow passes over the planes) is ONE streaming pass here: raw samples in, flow planes, mask and the flag word
// of flow_flags_kernel out.
//
// Both the raw image ([h, w, 3] x 16 bit, or [h, w, 2] x fp32) and the planes are dense, so a pixel's place in each is its flat index
// p = y * w + x: one lane takes the 4 pixels 4 g .. 4 g + 3 (24 B of KITTI samples, 32 B of .flo pairs), the last lane of an image the
// h * w % 4 that are left, one by one.  A wave reads one contiguous run (1536 / 2048 B) and writes three contiguous runs (2 x 1024 B of
// planes, 256 B of mask).  Loads are 16 + 8 bytes per lane (KITTI: 24 g is a multiple of 8, of 16 for every other lane -- the 16-byte
// half sits wherever it is aligned) or 2 x 16 bytes (.flo) when the image's first byte is aligned for them, else per sample; stores are
// 16 bytes per plane (4 for the mask) where the plane's first element is aligned, else per element.  The conditions are per image
// (block-uniform): with h * w % 4 != 0 the images of a batch differ in alignment.  No LDS except the block's flag word.
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
constexpr int kMaxBlocksX = 2048;                  // 8 per CU: a larger image is walked with a grid stride
constexpr float kZeroThr = 1e-3f;                  // utils.py:23, :642 (as in ofl_kernels.hip)

typedef uint32_t u4 __attribute__((ext_vector_type(4)));
typedef uint32_t u2 __attribute__((ext_vector_type(2)));

// the bits flow_flags_kernel sets for one vector: a COPY of flag_bits in ofl_kernels.hip (which points back here) -- change both;
// tests/test_gpu_loaders.py holds the two to each other word for word
__device__ __forceinline__ int flag_bits(float u, float v, bool valid) {
    int f = 0;
    const bool nf = !(isfinite(u) && isfinite(v));
    const bool nz = !(u == 0.0f) || !(v == 0.0f);
    const bool nzt = !((u < kZeroThr) && (u > -kZeroThr)) || !((v < kZeroThr) && (v > -kZeroThr));
    if (nf) f |= OFL_FLAG_NONFINITE;
    if (nz) f |= OFL_FLAG_NZ | (valid ? OFL_FLAG_NZ_MASKED : 0);
    if (nzt) f |= OFL_FLAG_NZ_THR | (valid ? OFL_FLAG_NZ_THR_MASKED : 0);
    return f;
}

// OR of the lanes' words over the wave (5 ballots), of the waves' words in LDS, then one atomic per block on the image's word
__device__ __forceinline__ void publish_flags(int32_t* addr, int f) {
    __shared__ int bflags;
    int r = 0;
#pragma unroll
    for (int b = 0; b < 5; ++b)
        if (__ballot((f >> b) & 1) != 0ull) r |= (1 << b);
    if (threadIdx.x == 0) bflags = 0;
    __syncthreads();
    if ((threadIdx.x & 63) == 0 && r != 0) atomicOr(&bflags, r);
    __syncthreads();
    if (threadIdx.x == 0 && bflags != 0) atomicOr(addr, bflags);
}

__device__ __forceinline__ float kitti_value(uint32_t sample) {      // (x - 2^15) / 64: an integer below 2^16 times 2^-6, exact in fp32
    return (float)((int)sample - 32768) * 0.015625f;
}

// big-endian 16-bit sample k (0 .. 11: R G B of 4 pixels) out of the 6 little-endian dwords of a group
__device__ __forceinline__ uint32_t be16(const uint32_t (&d)[6], int k) {
    const uint32_t half = (d[k >> 1] >> ((k & 1) * 16)) & 0xffffu;
    return ((half & 0xffu) << 8) | (half >> 8);
}

struct Planes {
    float* u; float* v; uint8_t* m;      // this image's planes
    bool vec_f, vec_m;                   // 16-byte plane stores / 4-byte mask stores are aligned
};

__device__ __forceinline__ Planes image_planes(float* vecs, uint8_t* mask, int64_t n, int64_t hw) {
    Planes o;
    o.u = vecs + n * 2 * hw;
    o.v = o.u + hw;
    o.m = mask ? mask + n * hw : nullptr;
    o.vec_f = (((uintptr_t)o.u | (uintptr_t)o.v) & 15) == 0;
    o.vec_m = ((uintptr_t)o.m & 3) == 0;
    return o;
}

// 4 pixels of both planes and of the mask; the vectors travel as 32-bit patterns (a .flo value is stored exactly as it came)
__device__ __forceinline__ void store_group(const Planes& o, int64_t p, const u4 u, const u4 v, const uint32_t m4) {
    uint32_t* pu = reinterpret_cast<uint32_t*>(o.u);
    uint32_t* pv = reinterpret_cast<uint32_t*>(o.v);
    if (o.vec_f) {
        *reinterpret_cast<u4*>(pu + p) = u;
        *reinterpret_cast<u4*>(pv + p) = v;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) { pu[p + k] = u[k]; pv[p + k] = v[k]; }
    }
    if (o.m) {
        if (o.vec_m) *reinterpret_cast<uint32_t*>(o.m + p) = m4;
        else {
#pragma unroll
            for (int k = 0; k < 4; ++k) o.m[p + k] = (uint8_t)((m4 >> (8 * k)) & 0xffu);
        }
    }
}

// raw: n images of hw pixels x 3 samples x 2 bytes (big-endian), raw_bs bytes apart
__global__ __launch_bounds__(kThreads) void decode_kitti_kernel(const uint8_t* __restrict__ raw, int64_t raw_bs, float* __restrict__ vecs,
                                                                uint8_t* __restrict__ mask, int32_t* __restrict__ flags, int64_t hw) {
    const int64_t n = blockIdx.y;
    const uint8_t* src = raw + n * raw_bs;
    const Planes o = image_planes(vecs, mask, n, hw);
    const bool vec_in = ((uintptr_t)src & 7) == 0;                        // then every group (24 g bytes in) is 8-byte aligned
    const int64_t groups = (hw + 3) >> 2, stride = (int64_t)gridDim.x * blockDim.x;
    int f = 0;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += stride) {
        const int64_t p = 4 * g;
        const uint8_t* s = src + 6 * p;
        if (p + 4 <= hw) {
            uint32_t d[6];
            if (vec_in) {
                // 24 bytes as one 16-byte and one 8-byte load, the 16-byte one where it is aligned: first for a group that starts on a
                // multiple of 16, last for one that starts 8 past it (lanes alternate)
                const bool late = ((uintptr_t)s & 8) != 0;
                const u4 q = *reinterpret_cast<const u4*>(s + (late ? 8 : 0));
                const u2 t = *reinterpret_cast<const u2*>(s + (late ? 0 : 16));
                d[0] = late ? t[0] : q[0]; d[1] = late ? t[1] : q[1];
                d[2] = late ? q[0] : q[2]; d[3] = late ? q[1] : q[3];
                d[4] = late ? q[2] : t[0]; d[5] = late ? q[3] : t[1];
            } else {
#pragma unroll
                for (int k = 0; k < 6; ++k)
                    d[k] = (uint32_t)s[4 * k] | ((uint32_t)s[4 * k + 1] << 8) | ((uint32_t)s[4 * k + 2] << 16) | ((uint32_t)s[4 * k + 3] << 24);
            }
            u4 ub, vb;
            uint32_t m4 = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float u = kitti_value(be16(d, 3 * k)), v = kitti_value(be16(d, 3 * k + 1));
                const bool valid = be16(d, 3 * k + 2) > 0u;
                ub[k] = __float_as_uint(u);
                vb[k] = __float_as_uint(v);
                m4 |= (valid ? 1u : 0u) << (8 * k);
                f |= flag_bits(u, v, o.m ? valid : true);
            }
            store_group(o, p, ub, vb, m4);
        } else {
            for (int64_t q = p; q < hw; ++q) {                            // the image's last 1 .. 3 pixels
                const uint8_t* t = src + 6 * q;
                const float u = kitti_value(((uint32_t)t[0] << 8) | t[1]), v = kitti_value(((uint32_t)t[2] << 8) | t[3]);
                const bool valid = (((uint32_t)t[4] << 8) | t[5]) > 0u;
                o.u[q] = u;
                o.v[q] = v;
                if (o.m) o.m[q] = valid ? 1 : 0;
                f |= flag_bits(u, v, o.m ? valid : true);
            }
        }
    }
    publish_flags(&flags[n], f);
}

// raw: n images of hw interleaved (u, v) pairs, raw_bs dwords apart; the values travel as bit patterns
__global__ __launch_bounds__(kThreads) void decode_flo_kernel(const uint32_t* __restrict__ raw, int64_t raw_bs, const uint8_t* __restrict__ grey,
                                                              int64_t grey_bs, float* __restrict__ vecs, uint8_t* __restrict__ mask,
                                                              int32_t* __restrict__ flags, int64_t hw) {
    const int64_t n = blockIdx.y;
    const uint32_t* src = raw + n * raw_bs;
    const uint8_t* gr = grey ? grey + n * grey_bs : nullptr;
    const Planes o = image_planes(vecs, mask, n, hw);
    const bool vec_in = ((uintptr_t)src & 15) == 0, vec_g = ((uintptr_t)gr & 3) == 0;
    const int64_t groups = (hw + 3) >> 2, stride = (int64_t)gridDim.x * blockDim.x;
    int f = 0;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += stride) {
        const int64_t p = 4 * g;
        const uint32_t* s = src + 2 * p;
        if (p + 4 <= hw) {
            u4 a, b;
            if (vec_in) {
                a = *reinterpret_cast<const u4*>(s);
                b = *reinterpret_cast<const u4*>(s + 4);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) { a[k] = s[k]; b[k] = s[4 + k]; }
            }
            uint32_t g4 = 0;                                              // grey 0 = valid; no grey plane: all valid
            if (gr) {
                if (vec_g) g4 = *reinterpret_cast<const uint32_t*>(gr + p);
                else g4 = (uint32_t)gr[p] | ((uint32_t)gr[p + 1] << 8) | ((uint32_t)gr[p + 2] << 16) | ((uint32_t)gr[p + 3] << 24);
            }
            const u4 ub = {a[0], a[2], b[0], b[2]}, vb = {a[1], a[3], b[1], b[3]};
            uint32_t m4 = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool valid = ((g4 >> (8 * k)) & 0xffu) == 0u;
                m4 |= (valid ? 1u : 0u) << (8 * k);
                f |= flag_bits(__uint_as_float(ub[k]), __uint_as_float(vb[k]), valid);
            }
            store_group(o, p, ub, vb, m4);
        } else {
            for (int64_t q = p; q < hw; ++q) {                            // the image's last 1 .. 3 pixels
                const uint32_t ub = src[2 * q], vb = src[2 * q + 1];
                const bool valid = gr ? gr[q] == 0 : true;
                reinterpret_cast<uint32_t*>(o.u)[q] = ub;
                reinterpret_cast<uint32_t*>(o.v)[q] = vb;
                if (o.m) o.m[q] = valid ? 1 : 0;
                f |= flag_bits(__uint_as_float(ub), __uint_as_float(vb), valid);
            }
        }
    }
    publish_flags(&flags[n], f);
}

// shape checks and the launch grid shared by both entry points
inline int loader_grid(int32_t n, int32_t h, int32_t w, int64_t* hw, dim3* grid) {
    if (n < 1 || h < 1 || w < 1 || n > 65535 || (int64_t)h * w >= (1ll << 31)) return OFL_E_SHAPE;
    *hw = (int64_t)h * w;
    const int64_t blocks = ((*hw + 3) / 4 + kThreads - 1) / kThreads;
    *grid = dim3((unsigned)(blocks < kMaxBlocksX ? blocks : kMaxBlocksX), (unsigned)n);
    return OFL_OK;
}

}  // namespace

extern "C" {

__attribute__((visibility("default"))) int ofl_decode_kitti(const uint8_t* raw, int64_t raw_bs, float* vecs, uint8_t* mask, int32_t* flags,
                                                            int32_t n, int32_t h, int32_t w, void* stream) {
    if (!raw || !vecs || !flags) return OFL_E_NULL;
    int64_t hw;
    dim3 grid;
    const int rc = loader_grid(n, h, w, &hw, &grid);
    if (rc) return rc;
    if (raw_bs < 6 * hw || ((uintptr_t)vecs & 3) != 0 || ((uintptr_t)flags & 3) != 0) return OFL_E_ARG;
    hipStream_t s = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(flags, 0, sizeof(int32_t) * (size_t)n, s);
    if (e != hipSuccess) return (int)e;
    OFL_KLAUNCH(decode_kitti_kernel, grid, dim3(kThreads), 0, s, raw, raw_bs, vecs, mask, flags, hw);
    return (int)hipGetLastError();
}

__attribute__((visibility("default"))) int ofl_decode_flo(const float* raw, int64_t raw_bs, const uint8_t* grey, int64_t grey_bs, float* vecs,
                                                          uint8_t* mask, int32_t* flags, int32_t n, int32_t h, int32_t w, void* stream) {
    if (!raw || !vecs || !flags) return OFL_E_NULL;
    int64_t hw;
    dim3 grid;
    const int rc = loader_grid(n, h, w, &hw, &grid);
    if (rc) return rc;
    if (raw_bs < 2 * hw || ((uintptr_t)raw & 3) != 0 || ((uintptr_t)vecs & 3) != 0 || ((uintptr_t)flags & 3) != 0) return OFL_E_ARG;
    if ((grey != nullptr) != (mask != nullptr) || (grey && grey_bs < hw)) return OFL_E_ARG;
    hipStream_t s = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(flags, 0, sizeof(int32_t) * (size_t)n, s);
    if (e != hipSuccess) return (int)e;
    OFL_KLAUNCH(decode_flo_kernel, grid, dim3(kThreads), 0, s, reinterpret_cast<const uint32_t*>(raw), raw_bs, grey, grey_bs, vecs, mask,
                flags, hw);
    return (int)hipGetLastError();
}

}  // extern "C"
