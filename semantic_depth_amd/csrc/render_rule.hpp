// The rule of the rendered clouds (sd_render_rw / sd_render_rw_host; contract: include/semdepth.h), stated ONCE for the kernels of
// render_gpu.hip and the host function of host_render.cpp: which rows a frame has, which of them are drawn, where the camera puts a row,
// which pixels it covers and which row a pixel shows.  Both sides call these functions, so they agree on every byte; what differs is only
// who walks the rows (one loop on the host, one lane per row and an integer atomic minimum per pixel on the device).  The rows are those of
// ply_format.hpp -- the cloud, then the road-width line from its own line_point -- so the picture shows what the frame's _rw.ply holds.
#pragma once
#include "../../include/semdepth.h"
#include "ply_format.hpp"

namespace sdrender {

using sdply::kBlockRows;
using sdply::kLineRows;

constexpr int kMaxExtent = SD_RENDER_MAX_EXTENT, kMaxPoint = SD_RENDER_MAX_POINT;
constexpr uint64_t kEmptyKey = ~0ull;      // above every key: the float bits of a key are at most those of +inf
constexpr int kGroup = 4;                  // pixels one lane of the resolve kernel owns: twelve bytes, three words

SDPLY_HD bool finite(double v) { return (sdply::dbits(v) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull; }
SDPLY_HD bool finite3(const double* p) { return finite(p[0]) && finite(p[1]) && finite(p[2]); }

SDPLY_HD bool valid_camera(const sd_render_camera& c) {
    for (int i = 0; i < 12; ++i)
        if (!finite(c.ext[i])) return false;
    if (!finite(c.fx) || !finite(c.fy) || !finite(c.cx) || !finite(c.cy) || !finite(c.z_near) || !(c.z_near > 0.0)) return false;
    return c.width >= 1 && c.width <= kMaxExtent && c.height >= 1 && c.height <= kMaxExtent && c.point_size >= 1 && c.point_size <= kMaxPoint;
}

// the frame's rows; a count outside 0..cap leaves it without any (flag 1, background only).  The end points of a found record are not
// range-tested here: a line row that is not finite is skipped like any other row.
SDPLY_HD sdply::Frame make_frame(const float* xyz, const uint8_t* rgb, int n, int cap, const float* left, const float* right, int found) {
    sdply::Frame f = sdply::make_frame(xyz, rgb, n, cap, left, right, found);
    f.bad = n < 0 || n > cap;
    if (f.bad) f.rows = 0;
    return f;
}

// where the camera puts a world point: false = not drawn; else the pixel of its centre and the depth half of its key
struct Hit {
    int px, py;
    uint32_t zbits;
};
SDPLY_HD bool project(const sd_render_camera& c, const double* p, Hit* h) {
#pragma clang fp contract(off)
    const double* e = c.ext;
    const double X = ((e[0] * p[0] + e[1] * p[1]) + e[2] * p[2]) + e[3];
    const double Y = ((e[4] * p[0] + e[5] * p[1]) + e[6] * p[2]) + e[7];
    const double Z = ((e[8] * p[0] + e[9] * p[1]) + e[10] * p[2]) + e[11];
    if (!(Z >= c.z_near)) return false;
    const double xz = X / Z, yz = Y / Z;
    const double u = c.fx * xz + c.cx;
    const double v = c.fy * yz + c.cy;
    const double s = (double)c.point_size;
    if (!(-s <= u && u < (double)c.width + s && -s <= v && v < (double)c.height + s)) return false;      // a NaN fails; before any cast
    h->px = (int)__builtin_floor(u);
    h->py = (int)__builtin_floor(v);
    const float zf = (float)Z;
    __builtin_memcpy(&h->zbits, &zf, 4);
    return true;
}
SDPLY_HD uint64_t make_key(uint32_t zbits, uint32_t row) { return ((uint64_t)zbits << 32) | row; }

// the square of a hit, clipped to the image: columns x0..x1, rows y0..y1 (empty when x0 > x1 or y0 > y1)
struct Box {
    int x0, x1, y0, y1;
};
SDPLY_HD Box splat_box(const sd_render_camera& c, const Hit& h) {
    const int s = c.point_size, lo = (s - 1) / 2, hi = s / 2;
    Box b;
    b.x0 = h.px - lo < 0 ? 0 : h.px - lo;
    b.x1 = h.px + hi > c.width - 1 ? c.width - 1 : h.px + hi;
    b.y0 = h.py - lo < 0 ? 0 : h.py - lo;
    b.y1 = h.py + hi > c.height - 1 ? c.height - 1 : h.py + hi;
    return b;
}

// the three bytes of a pixel whose smallest key is `key`, in BGR
SDPLY_HD void resolve(const sd_render_camera& c, uint64_t key, const uint8_t* rgb, int n, uint8_t* out) {
    if (key == kEmptyKey) {
        for (int j = 0; j < 3; ++j) out[j] = c.background[j];
        return;
    }
    const uint32_t row = (uint32_t)key;
    if (row < (uint32_t)n) {
        const uint8_t* q = rgb + 3 * (size_t)row;
        out[0] = q[2];
        out[1] = q[1];
        out[2] = q[0];
        return;
    }
    out[0] = 0;              // the line's 250 0 0
    out[1] = 0;
    out[2] = 250;
}

// ---- workspace of the device route (render_gpu.hip)
inline size_t key_count(int B, const sd_render_camera& cam) { return (size_t)B * (size_t)cam.height * (size_t)cam.width; }
struct Layout : sdarena::Walker {
    size_t px, nb, B;
    Layout(int B_, int cap, const sd_render_camera& cam) : px(key_count(B_, cam)), nb((size_t)B_ * sdply::blocks_per_frame(cap)), B((size_t)B_) {}
    size_t keys = take(px * 8, 16);      // u64 [B][height][width], 16-byte aligned (with the workspace): the depth keys, cleared two at a time
    size_t bmin = take(nb * 8, 8);       // f64 [B][blocks_per_frame(cap)], 8: per 256-row block its minimum z
    size_t zmin = take(B * 8, 8);        // f64 [B], 8: the frame's minimum z
    size_t slack = end();                // 64 bytes of historical slack: nothing reads or writes them
    size_t total = end_with_slack(64);
};

}  // namespace sdrender
