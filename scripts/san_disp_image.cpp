// Sanitizer driver of the host disparity images (sd_disp_image_host, csrc/host_disp_image.cpp) over the odd sizes: a stand-alone program,
// no GPU, nothing loaded into Python.
//   g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -ffp-contract=off -Iinclude scripts/san_disp_image.cpp \
//       semantic_depth_amd/csrc/host_disp_image.cpp semantic_depth_amd/csrc/host_seg_eval.cpp -o scripts/san_disp_image && scripts/san_disp_image
// Every output buffer is allocated at its exact size, so a write past an image or a flag array is an AddressSanitizer report; the program
// also checks the statuses, the flags and that a frame gives the same bytes alone and inside its batch.  Exit status 0 and "ok" = clean.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "semdepth.h"

static uint32_t rng_state = 12345u;
static float rnd() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return (float)(rng_state >> 8) / 16777216.0f;
}

static int run(int B, int h, int w, int oh, int ow, int cmap, int mode) {
    const size_t n = (size_t)h * w, n2 = (size_t)oh * ow;
    std::vector<float> disp((size_t)B * n), mult((size_t)B);
    for (auto& v : disp) v = rnd() * 0.1f - 0.01f;
    for (int b = 0; b < B; ++b) mult[(size_t)b] = b % 2 ? 3800.0f : 1.0f;
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    if (mode == 1) disp[n / 2] = nan, disp[0] = inf, disp[n - 1] = -inf;          // non-finite pixels in frame 0
    if (mode == 2)
        for (size_t i = 0; i < n; ++i) disp[i] = nan;                              // an all-NaN frame 0
    if (mode == 3)
        for (size_t i = 0; i < n; ++i) disp[i] = 0.25f;                            // a constant frame 0
    if (mode == 4) disp[0] = 3.0e38f, disp[n - 1] = -3.0e38f;                      // hi - lo beyond the float32 range
    std::vector<uint8_t> out((size_t)B * n2 * 3), one(n2 * 3);
    std::vector<int32_t> flags((size_t)B), flag1(1);
    if (sd_disp_image_host(disp.data(), mult.data(), B, h, w, oh, ow, cmap, out.data(), flags.data()) != SD_OK) return 1;
    if (flags[0] != (mode == 1 || mode == 2 ? 1 : 0)) return 2;
    for (int b = 1; b < B; ++b)
        if (flags[(size_t)b] != 0) return 3;
    for (int b = 0; b < B; ++b) {
        if (sd_disp_image_host(disp.data() + (size_t)b * n, mult.data() + b, 1, h, w, oh, ow, cmap, one.data(), flag1.data()) != SD_OK) return 4;
        if (std::memcmp(one.data(), out.data() + (size_t)b * n2 * 3, n2 * 3) != 0 || flag1[0] != flags[(size_t)b]) return 5;
    }
    if (mode == 2 || mode == 3) {                                                  // entry 0 of the map everywhere
        uint8_t rgb[768];
        if (sd_disp_colormap(cmap, rgb) != SD_OK) return 6;
        for (size_t i = 0; i < n2; ++i)
            if (out[3 * i] != rgb[2] || out[3 * i + 1] != rgb[1] || out[3 * i + 2] != rgb[0]) return 7;
    }
    return 0;
}

int main() {
    static const int sizes[][4] = {{8, 16, 20, 40}, {8, 16, 8, 16}, {16, 32, 5, 7},  {7, 13, 9, 11},  {3, 5, 1, 1},   {1, 1, 1, 1},
                                   {1, 1, 7, 3},    {5, 3, 5, 9},   {9, 5, 2, 5},    {64, 33, 2, 33}, {1, 97, 3, 11}, {31, 1, 1, 1}};
    int runs = 0;
    for (const auto& s : sizes)
        for (int cmap = 0; cmap < 2; ++cmap)
            for (int mode = 0; mode < 5; ++mode)
                for (int B = 1; B <= 3; B += 2) {
                    const int r = run(B, s[0], s[1], s[2], s[3], cmap, mode);
                    if (r) {
                        std::printf("FAILED %d: B=%d %dx%d -> %dx%d cmap=%d mode=%d\n", r, B, s[0], s[1], s[2], s[3], cmap, mode);
                        return 1;
                    }
                    ++runs;
                }
    // the refusals: nothing is written
    uint8_t px[3];
    int32_t flag;
    const float one = 1.0f;
    size_t bytes = 0;
    if (sd_disp_image_host(&one, nullptr, 1, 1, 1, 1, 1, 2, px, &flag) != SD_ERR_INVALID) return 2;
    if (sd_disp_image_host(&one, nullptr, 1, 0, 1, 1, 1, 0, px, &flag) != SD_ERR_INVALID) return 2;
    if (sd_disp_image_host(&one, nullptr, 1, 1, 1, 1, 16385, 0, px, &flag) != SD_ERR_INVALID) return 2;
    if (sd_disp_image_host(nullptr, nullptr, 1, 1, 1, 1, 1, 0, px, &flag) != SD_ERR_INVALID) return 2;
    if (sd_disp_image_workspace(1, 66, 1, 2, 1, &bytes) != SD_ERR_INVALID || sd_disp_image_workspace(1, 64, 1, 2, 1, &bytes) != SD_OK) return 2;
    if (sd_disp_colormap(-1, px) != SD_ERR_INVALID) return 2;
    std::printf("ok: %d runs\n", runs);
    return 0;
}
