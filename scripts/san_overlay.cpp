// Sanitizer driver of the host measurement lines (sd_overlay_segments_host, sd_overlay_draw_host; csrc/host_overlay.cpp) over crafted frames
// in the manner of tests/overlay_cases.py: a stand-alone program, no GPU, nothing loaded into Python.
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined -Iinclude scripts/san_overlay.cpp semantic_depth_amd/csrc/host_overlay.cpp \
//       -fsanitize=address,undefined -o scripts/san_overlay && scripts/san_overlay
// (host_overlay.cpp includes the HIP runtime's header for its __host__ __device__ rule, hence hipcc; only host code runs.)  The segment
// array is allocated at exactly 4 D + 2 entries and every image at its exact size, so a write past either is an AddressSanitizer report; the
// program also checks the statuses, the flags, that rows above clip_top stay untouched and that refused calls write nothing.
// Exit status 0 and "ok" = clean.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "semdepth.h"

static uint32_t rng_state = 2463534242u;
static double rnd() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return (double)(rng_state >> 8) / 16777216.0;
}

static const int NET_H = 128, NET_W = 256;

// the 3D point that lands near output pixel (fx * w, fy * h) at depth zn
static void point_at(const sd_camera& c, int h, int w, double fx, double fy, double zn, double* out) {
    const double xn = (fx * w + 0.5) * NET_W / w - 0.5, yn = (fy * h + 0.5) * NET_H / h - 0.5;
    out[0] = (xn - c.cx) * zn / c.f;
    out[1] = (c.cy - yn) * zn / c.f;
    out[2] = -zn;
}
static void to_f(const double* p, float* q) {
    for (int k = 0; k < 3; ++k) q[k] = (float)p[k];
}

static int run(int h, int w, int D, int fence, int thickness, int profile_thickness, int clip_top, int mode) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    sd_camera cam{NET_W / 2 + rnd() * 6 - 3, NET_H / 2 + rnd() * 4 - 2, 60.0 + rnd() * 20, 0.22, 3800.0};
    sd_rw_result rec{};
    sd_f2f_result f2{};
    double p[3];
    rec.found = 1;
    point_at(cam, h, w, mode == 1 ? -0.3 : 0.2, mode == 1 ? -0.2 : 0.6, 10.0, p);
    to_f(p, rec.left_pt);
    point_at(cam, h, w, 0.8, mode == 2 ? 0.2 : 0.6, 10.0, p);
    to_f(p, rec.right_pt);
    f2.ok = 1;
    point_at(cam, h, w, 0.1, 0.9, 10.0, f2.left_pt);
    point_at(cam, h, w, mode == 3 ? 40000.0 / w : 1.4, 0.3, 10.0, f2.right_pt);
    int want_flag = mode == 3 && fence ? 1 : 0;
    if (mode == 4) rec.right_pt[2] = 1.0f, want_flag |= 1;       // Z >= 0
    if (mode == 5) rec.left_pt[0] = (float)nan, want_flag |= 1;  // a NaN coordinate
    if (mode == 6) rec.found = 0;
    std::vector<sd_rw_depth_result> prof((size_t)D);
    std::vector<sd_f2f_depth_result> fprof((size_t)D);
    for (int i = 0; i < D; ++i) {
        const double d = D > 1 ? 5.0 + 35.0 * (mode % 2 ? D - 1 - i : i) / (D - 1) : 12.0, t = (d - 5.0) / 35.0;
        const double half = 0.45 * (1.0 - t) + 0.02, y = 0.95 - 0.6 * t;
        prof[(size_t)i] = sd_rw_depth_result{};
        fprof[(size_t)i] = sd_f2f_depth_result{};
        prof[(size_t)i].found = !(D >= 3 && i == D / 2);         // a hole in the middle
        point_at(cam, h, w, 0.5 - half, y, d, p);
        to_f(p, prof[(size_t)i].left_pt);
        point_at(cam, h, w, 0.5 + half, y, d, p);
        to_f(p, prof[(size_t)i].right_pt);
        fprof[(size_t)i].ok = !(D >= 3 && i == 1);
        point_at(cam, h, w, 0.5 - half - 0.04, y, d, fprof[(size_t)i].left_pt);
        point_at(cam, h, w, 0.5 + half + 0.04, y, d, fprof[(size_t)i].right_pt);
    }
    if (D >= 2 && mode == 4) prof[0].left_pt[2] = 1.0f;
    sd_overlay_style st{{0, 0, 255}, {0, 255, 0}, {0, 255, 255}, {0, 0, 0}, thickness, profile_thickness, clip_top};
    std::vector<sd_overlay_segment> segs((size_t)(4 * D + 2));
    int n = -1;
    int32_t flag = -1;
    if (sd_overlay_segments_host(&rec, fence ? &f2 : nullptr, D ? prof.data() : nullptr, fence && D ? fprof.data() : nullptr, D, &cam, NET_H, NET_W, h, w,
                                 &st, segs.data(), &n, &flag) != SD_OK)
        return 1;
    if (n < 0 || n > 4 * D + 2 || flag != want_flag) return 2;
    std::vector<uint8_t> img((size_t)h * w * 3), before;
    for (auto& v : img) v = (uint8_t)(rnd() * 256);
    before = img;
    std::vector<sd_overlay_segment> exact(segs.begin(), segs.begin() + n);      // exactly n entries: a read past them is a report too
    if (sd_overlay_draw_host(img.data(), h, w, exact.data(), n, clip_top) != SD_OK) return 3;
    if (std::memcmp(img.data(), before.data(), (size_t)clip_top * w * 3) != 0) return 4;
    if (n > 0 && mode == 0 && clip_top < h / 2 && img == before) return 5;
    return 0;
}

int main() {
    static const int sizes[][2] = {{16, 64}, {37, 130}, {120, 700}, {1, 1}, {3, 500}, {257, 5}};
    static const int depths[] = {0, 1, 7, 256};
    int runs = 0;
    for (const auto& s : sizes)
        for (int D : depths)
            for (int mode = 0; mode < 7; ++mode)
                for (int fence = 0; fence < 2; ++fence)
                    for (int thick = 0; thick < 3; ++thick) {
                        const int t = thick == 0 ? 1 : thick == 1 ? 3 : 32;
                        const int clip = thick == 1 ? 0 : s[0] / 2;
                        const int r = run(s[0], s[1], D, fence, t, thick == 2 ? 32 : 1, clip, mode);
                        if (r) {
                            std::printf("FAILED %d: %dx%d D=%d mode=%d fence=%d thickness=%d\n", r, s[0], s[1], D, mode, fence, t);
                            return 1;
                        }
                        ++runs;
                    }
    // the refusals: nothing is written
    sd_camera cam{128.0, 64.0, 70.0, 0.22, 1.0};
    sd_rw_result rec{};
    sd_overlay_style st{{0, 0, 255}, {0, 255, 0}, {0, 255, 255}, {0, 0, 0}, 3, 1, 0};
    sd_overlay_segment seg{1, 2, 3, 4, {5, 6, 7}, 8}, kept = seg;
    int n = -7;
    int32_t flag = -7;
    sd_overlay_style bad = st;
    bad.thickness = 33;
    sd_camera nancam = cam;
    nancam.f = std::numeric_limits<double>::quiet_NaN();
    if (sd_overlay_segments_host(&rec, nullptr, nullptr, nullptr, 1, &cam, NET_H, NET_W, 8, 8, &st, &seg, &n, &flag) != SD_ERR_INVALID) return 2;
    if (sd_overlay_segments_host(&rec, nullptr, nullptr, nullptr, 257, &cam, NET_H, NET_W, 8, 8, &st, &seg, &n, &flag) != SD_ERR_INVALID) return 2;
    if (sd_overlay_segments_host(&rec, nullptr, nullptr, nullptr, 0, &cam, NET_H, NET_W, 8, 16385, &st, &seg, &n, &flag) != SD_ERR_INVALID) return 2;
    if (sd_overlay_segments_host(&rec, nullptr, nullptr, nullptr, 0, &cam, NET_H, NET_W, 8, 8, &bad, &seg, &n, &flag) != SD_ERR_INVALID) return 2;
    if (sd_overlay_segments_host(&rec, nullptr, nullptr, nullptr, 0, &nancam, NET_H, NET_W, 8, 8, &st, &seg, &n, &flag) != SD_ERR_INVALID) return 2;
    if (n != -7 || flag != -7 || std::memcmp(&seg, &kept, sizeof seg) != 0) return 3;
    uint8_t px[3] = {9, 9, 9};
    seg.thickness = 33;
    if (sd_overlay_draw_host(px, 1, 1, &seg, 1, 0) != SD_ERR_INVALID) return 4;
    seg.thickness = 1;
    if (sd_overlay_draw_host(px, 1, 1, &seg, 1, 2) != SD_ERR_INVALID || sd_overlay_draw_host(px, 1, 1, nullptr, 1, 0) != SD_ERR_INVALID) return 4;
    if (px[0] != 9 || px[1] != 9 || px[2] != 9) return 5;
    std::printf("ok: %d runs\n", runs);
    return 0;
}
