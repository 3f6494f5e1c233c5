// png_unfilter_check.cpp -- stand-alone driver for the host PNG code (oflibpytorch_amd/csrc/ofl_png_host.cpp), meant to be built with
// the host compiler and -fsanitize=address,undefined (tests/test_png_host.py does; no GPU, no Python in the process):
//
//     g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include tools/png_unfilter_check.cpp \
//         oflibpytorch_amd/csrc/ofl_png_host.cpp -o png_unfilter_check
//     png_unfilter_check INFLATED_FILE WIDTH HEIGHT BIT_DEPTH COLOUR_TYPE
//
// INFLATED_FILE holds the inflated IDAT stream of an image with that header.  The program decodes it, then every single-byte mutation
// from a fixed set, every filter byte set to 0 .. 7, every truncation, and output buffers that are too short -- each time from heap
// buffers of EXACTLY the stated lengths, so that one byte read or written beyond them is a sanitizer report.  Exit status 0: every call
// returned what the header documents.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "oflib_hip.h"

static int failures = 0;

static void expect(bool ok, const char* what, long long detail) {
    if (!ok) {
        fprintf(stderr, "png_unfilter_check: %s (%lld)\n", what, detail);
        ++failures;
    }
}

// one call on exact-size heap copies
static int run(const uint8_t* in, int64_t in_len, int w, int h, int depth, int ct, int64_t out_len, std::vector<uint8_t>* keep = nullptr) {
    uint8_t* src = (uint8_t*)malloc(in_len > 0 ? (size_t)in_len : 1);
    uint8_t* dst = (uint8_t*)malloc(out_len > 0 ? (size_t)out_len : 1);
    if (in_len > 0) memcpy(src, in, (size_t)in_len);
    const int rc = ofl_png_unfilter(src, in_len, w, h, depth, ct, dst, out_len);
    if (rc == OFL_OK && keep) keep->assign(dst, dst + out_len);
    free(src);
    free(dst);
    return rc;
}

static int run_grey(const std::vector<uint8_t>& raw, int w, int h, int depth, int ct, const uint8_t* palette, int entries, int64_t grey_len) {
    uint8_t* src = (uint8_t*)malloc(raw.empty() ? 1 : raw.size());
    uint8_t* dst = (uint8_t*)malloc(grey_len > 0 ? (size_t)grey_len : 1);
    uint8_t* pal = palette ? (uint8_t*)malloc((size_t)entries * 3) : nullptr;
    if (!raw.empty()) memcpy(src, raw.data(), raw.size());
    if (pal) memcpy(pal, palette, (size_t)entries * 3);
    const int rc = ofl_png_grey8(src, (int64_t)raw.size(), w, h, depth, ct, pal, entries, dst, grey_len);
    free(src);
    free(dst);
    free(pal);
    return rc;
}

int main(int argc, char** argv) {
    if (argc != 6) {
        fprintf(stderr, "usage: %s INFLATED_FILE WIDTH HEIGHT BIT_DEPTH COLOUR_TYPE\n", argv[0]);
        return 2;
    }
    const int w = atoi(argv[2]), h = atoi(argv[3]), depth = atoi(argv[4]), ct = atoi(argv[5]);
    FILE* f = fopen(argv[1], "rb");
    if (!f) {
        fprintf(stderr, "png_unfilter_check: cannot open %s\n", argv[1]);
        return 2;
    }
    std::vector<uint8_t> in;
    uint8_t buf[4096];
    for (size_t got; (got = fread(buf, 1, sizeof buf, f)) > 0;) in.insert(in.end(), buf, buf + got);
    fclose(f);
    const int channels = ct == 0 || ct == 3 ? 1 : ct == 2 ? 3 : ct == 4 ? 2 : 4;
    const int64_t rb = ((int64_t)w * channels * depth + 7) / 8, n = (int64_t)in.size(), out_len = rb * h;
    expect(n == (rb + 1) * h, "the file's length does not match the header", n);
    if (failures) return 1;

    // 1. the image as it is
    std::vector<uint8_t> raw;
    expect(run(in.data(), n, w, h, depth, ct, out_len, &raw) == OFL_OK, "the unmodified image is rejected", 0);
    const bool grey_ok = ct == 0 || ct == 3 || ((ct == 2 || ct == 6) && depth == 8);
    uint8_t palette[256 * 3];
    for (int i = 0; i < 256 * 3; ++i) palette[i] = (uint8_t)(i * 7);
    if (!raw.empty()) {
        const int rc = run_grey(raw, w, h, depth, ct, palette, 256, (int64_t)w * h);
        expect(rc == (grey_ok ? OFL_OK : OFL_E_UNSUPPORTED), "grey conversion of the unmodified image", rc);
        expect(run_grey(raw, w, h, depth, ct, palette, 256, (int64_t)w * h - 1) == OFL_E_SHAPE, "a short grey buffer is accepted", 0);
        if (ct == 3) expect(run_grey(raw, w, h, depth, ct, nullptr, 0, (int64_t)w * h) == OFL_E_NULL, "a missing palette is accepted", 0);
    }

    // 2. single-byte mutations: any byte may change the pixels, only a filter byte above 4 may change the status
    std::vector<uint8_t> m = in;
    static const uint8_t flips[] = {0x01, 0x80, 0xff};
    for (int64_t i = 0; i < n; ++i) {
        const bool is_filter = i % (rb + 1) == 0;
        for (uint8_t x : flips) {
            m[i] = in[i] ^ x;
            const int rc = run(m.data(), n, w, h, depth, ct, out_len);
            expect(rc == ((is_filter && m[i] > 4) ? OFL_E_ARG : OFL_OK), "status after a byte flip at", i);
        }
        if (is_filter) {
            for (int v = 0; v < 8; ++v) {
                m[i] = (uint8_t)v;
                const int rc = run(m.data(), n, w, h, depth, ct, out_len);
                expect(rc == (v > 4 ? OFL_E_ARG : OFL_OK), "status after a filter byte rewrite at", i);
            }
        }
        m[i] = in[i];
    }

    // 3. truncations and short / long outputs: a length error, and not one byte touched beyond the buffers
    for (int64_t len = 0; len < n; ++len)
        expect(run(in.data(), len, w, h, depth, ct, out_len) == OFL_E_SHAPE, "a truncated stream is accepted at length", len);
    for (int64_t len = 0; len < out_len; len += (out_len > 64 ? out_len / 64 : 1))
        expect(run(in.data(), n, w, h, depth, ct, len) == OFL_E_SHAPE, "a short output is accepted at length", len);
    expect(run(in.data(), n, w, h, depth, ct, out_len + 1) == OFL_E_SHAPE, "a long output is accepted", 0);

    // 4. a header that disagrees with the bytes
    expect(run(in.data(), n, w + 8, h, depth, ct, out_len) == OFL_E_SHAPE, "a wider header is accepted", 0);      // (8 pixels: at least a byte)
    expect(run(in.data(), n, w, h + 1, depth, ct, out_len) == OFL_E_SHAPE, "a taller header is accepted", 0);
    expect(run(in.data(), n, 0, h, depth, ct, out_len) == OFL_E_SHAPE, "zero width is accepted", 0);
    expect(run(in.data(), n, w, 0, depth, ct, out_len) == OFL_E_SHAPE, "zero height is accepted", 0);
    expect(run(in.data(), n, -w, h, depth, ct, out_len) == OFL_E_SHAPE, "negative width is accepted", 0);
    expect(run(in.data(), n, w, h, 3, ct, out_len) == OFL_E_ARG, "bit depth 3 is accepted", 0);
    expect(run(in.data(), n, w, h, depth, 5, out_len) == OFL_E_ARG, "colour type 5 is accepted", 0);
    expect(run(in.data(), n, 1 << 30, 1 << 30, depth, ct, out_len) == OFL_E_SHAPE, "a 2^60-pixel header is accepted", 0);
    expect(ofl_png_unfilter(nullptr, n, w, h, depth, ct, nullptr, out_len) == OFL_E_NULL, "NULL buffers are accepted", 0);

    // 5. palette indices beyond the palette: the unfiltered bytes of a greyscale image read as indices into a 2-entry palette
    if (ct == 0 && depth == 8 && !raw.empty()) {
        bool beyond = false;
        for (uint8_t v : raw) beyond = beyond || v >= 2;
        expect(run_grey(raw, w, h, 8, 3, palette, 2, (int64_t)w * h) == (beyond ? OFL_E_ARG : OFL_OK), "palette range check", 0);
    }
    if (failures) return 1;
    printf("png_unfilter_check: ok (%lld bytes, %d x %d, depth %d, colour type %d)\n", (long long)n, w, h, depth, ct);
    return 0;
}
