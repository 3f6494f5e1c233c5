// ofl_png_host.cpp -- the host half of the dataset loaders: PNG scanline unfiltering and the 8-bit grey value of a pixel.
// Plain C++: no HIP call, no allocation, no global state; it is linked into libofl_hip.so and also compiles on its own with the host
// compiler (tests/test_png_host.py, tools/png_unfilter_check.cpp).  The binding parses the chunks and inflates the IDAT stream
// (zlib); what is left is sequential per byte lane -- every byte of a Sub / Average / Paeth row depends on the one `bpp` bytes before it --
// which is hopeless in an interpreter and a poor fit for a GPU.
// Every length is the caller's; all indices are formed from the validated geometry, never from the image bytes, so nothing is read or
// written beyond the buffers whatever the bytes say.
// C ABI: include/oflib_hip.h.
#include <stdint.h>

#include "oflib_hip.h"

#define OFL_EXPORT extern "C" __attribute__((visibility("default")))

namespace {

constexpr int32_t kMaxSide = 1 << 24;           // row_bytes <= 2^27, an image <= 2^51 bytes: no int64 overflow below

// channels of a colour type, 0 for one PNG does not define
inline int png_channels(int32_t colour_type) {
    switch (colour_type) {
        case 0: return 1;       // grey
        case 2: return 3;       // R G B
        case 3: return 1;       // palette index
        case 4: return 2;       // grey, alpha
        case 6: return 4;       // R G B A
        default: return 0;
    }
}

inline bool png_depth_ok(int32_t colour_type, int32_t d) {
    switch (colour_type) {
        case 0: return d == 1 || d == 2 || d == 4 || d == 8 || d == 16;
        case 3: return d == 1 || d == 2 || d == 4 || d == 8;
        case 2: case 4: case 6: return d == 8 || d == 16;
        default: return false;
    }
}

// geometry checks shared by both entry points: 0 and row_bytes, or an OFL_E_* code
inline int png_geometry(int32_t width, int32_t height, int32_t bit_depth, int32_t colour_type, int64_t* row_bytes) {
    if (width < 1 || height < 1 || width > kMaxSide || height > kMaxSide) return OFL_E_SHAPE;
    if (!png_depth_ok(colour_type, bit_depth)) return OFL_E_ARG;
    *row_bytes = ((int64_t)width * png_channels(colour_type) * bit_depth + 7) / 8;
    return OFL_OK;
}

inline int paeth(int a, int b, int c) {
    const int p = a + b - c;
    const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

}  // namespace

OFL_EXPORT int ofl_png_unfilter(const uint8_t* inflated, int64_t inflated_len, int32_t width, int32_t height, int32_t bit_depth,
                                int32_t colour_type, uint8_t* out, int64_t out_len) {
    if (!inflated || !out) return OFL_E_NULL;
    int64_t rb = 0;
    const int rc = png_geometry(width, height, bit_depth, colour_type, &rb);
    if (rc != OFL_OK) return rc;
    if (inflated_len != (int64_t)height * (rb + 1) || out_len != (int64_t)height * rb) return OFL_E_SHAPE;
    const int bits = png_channels(colour_type) * bit_depth;
    const int64_t bpp = bits < 8 ? 1 : bits / 8;                  // the filter's "previous pixel" distance in bytes
    for (int64_t r = 0; r < height; ++r) {
        const uint8_t* in = inflated + r * (rb + 1);
        const int ft = in[0];
        ++in;
        uint8_t* cur = out + r * rb;
        const uint8_t* up = r > 0 ? cur - rb : nullptr;           // (the row above the first one is all zero)
        switch (ft) {
            case 0:
                for (int64_t i = 0; i < rb; ++i) cur[i] = in[i];
                break;
            case 1:
                for (int64_t i = 0; i < rb; ++i) cur[i] = (uint8_t)(in[i] + (i >= bpp ? cur[i - bpp] : 0));
                break;
            case 2:
                for (int64_t i = 0; i < rb; ++i) cur[i] = (uint8_t)(in[i] + (up ? up[i] : 0));
                break;
            case 3:
                for (int64_t i = 0; i < rb; ++i) {
                    const int a = i >= bpp ? cur[i - bpp] : 0, b = up ? up[i] : 0;
                    cur[i] = (uint8_t)(in[i] + ((a + b) >> 1));
                }
                break;
            case 4:
                for (int64_t i = 0; i < rb; ++i) {
                    const int a = i >= bpp ? cur[i - bpp] : 0, b = up ? up[i] : 0, c = (up && i >= bpp) ? up[i - bpp] : 0;
                    cur[i] = (uint8_t)(in[i] + paeth(a, b, c));
                }
                break;
            default:
                return OFL_E_ARG;
        }
    }
    return OFL_OK;
}

OFL_EXPORT int ofl_png_grey8(const uint8_t* raw, int64_t raw_len, int32_t width, int32_t height, int32_t bit_depth, int32_t colour_type,
                             const uint8_t* palette, int32_t palette_entries, uint8_t* grey, int64_t grey_len) {
    if (!raw || !grey) return OFL_E_NULL;
    int64_t rb = 0;
    const int rc = png_geometry(width, height, bit_depth, colour_type, &rb);
    if (rc != OFL_OK) return rc;
    if (raw_len != (int64_t)height * rb || grey_len != (int64_t)height * width) return OFL_E_SHAPE;
    if (colour_type == 4 || ((colour_type == 2 || colour_type == 6) && bit_depth != 8)) return OFL_E_UNSUPPORTED;
    if (colour_type == 3 && (!palette || palette_entries < 1 || palette_entries > 256)) return palette ? OFL_E_ARG : OFL_E_NULL;
    // OpenCV's 8-bit cvtColor weights.  UNVERIFIED against cv2.imread(path, 0) for colour / palette masks: its PNG reader may let libpng
    // convert (png_set_rgb_to_gray), which can differ by one level at nearly black pixels
    auto luma = [](int r, int g, int b) { return (uint8_t)((4899 * r + 9617 * g + 1868 * b + 8192) >> 14); };
    for (int64_t y = 0; y < height; ++y) {
        const uint8_t* row = raw + y * rb;
        uint8_t* dst = grey + y * width;
        if (colour_type == 0 && bit_depth == 16) {
            for (int64_t x = 0; x < width; ++x) dst[x] = row[2 * x];                       // the high byte
        } else if (colour_type == 2 || colour_type == 6) {
            const int ch = colour_type == 2 ? 3 : 4;
            for (int64_t x = 0; x < width; ++x) dst[x] = luma(row[ch * x], row[ch * x + 1], row[ch * x + 2]);
        } else {                                                                         // grey or palette index of 1 / 2 / 4 / 8 bits
            const int d = bit_depth, per = 8 / d, top = (1 << d) - 1, scale = 255 / top;
            for (int64_t x = 0; x < width; ++x) {
                const int s = (row[x / per] >> (8 - d - (int)(x % per) * d)) & top;      // most significant bits first
                if (colour_type == 0) {
                    dst[x] = (uint8_t)(s * scale);
                } else {
                    if (s >= palette_entries) return OFL_E_ARG;
                    dst[x] = luma(palette[3 * s], palette[3 * s + 1], palette[3 * s + 2]);
                }
            }
        }
    }
    return OFL_OK;
}
