// The measurement lines of the result images (sd_overlay_draw / sd_overlay_segments_host / sd_overlay_draw_host; contract:
// include/semdepth.h), stated ONCE for the kernels of overlay_gpu.hip and the host functions of host_overlay.cpp: how a 3D end point becomes
// a position in 1/256 pixel of the output image, which slot of a frame holds which segment, and the pixel box outside which a segment paints
// nothing.  Which pixel a segment paints is sdtext::hit of text_draw.hpp, unchanged.  Both sides call these functions, so they agree on every
// pixel; what differs is only who walks the slots and the pixels.
//
// hit()'s integers under the caps here (extents <= 16384, |coordinate| <= 32768 px, thickness <= 32): an end point is |q| <= 2^15 * 2^8 =
// 2^23, a pixel centre < 2^14 * 2^8 = 2^22, so |w| = |P - A| < 2^23 + 2^22 < 2^24 and |d| = |B - A| <= 2^24 per axis.  w.d and w x d are sums
// of two products below 2^48: below 2^49 < 2^50.  |w|^2, |P - B|^2 and |d|^2 are below 2^49 as well, r^2 = (128 * 32)^2 = 2^24; all of these
// fit an int64.  r^2 |d|^2 < 2^73 and (w x d)^2 < 2^98 do not: hit() forms both as 128-bit products.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/semdepth.h"
#include "text_draw.hpp"

#if defined(__HIPCC__)
#define SDOVL_HD __host__ __device__ inline
#else
#define SDOVL_HD inline
#endif

namespace sdoverlay {

constexpr int kMaxDepths = SD_PROFILE_MAX_DEPTHS, kMaxSegs = SD_OVERLAY_MAX_SEGS, kMaxThickness = SD_OVERLAY_MAX_THICKNESS, kMaxExtent = 16384;
constexpr int kMaxQ = SD_OVERLAY_MAX_COORD * 256;      // the largest |coordinate| of a segment, in 1/256 pixel
constexpr double kMaxCoord = (double)SD_OVERLAY_MAX_COORD;
constexpr double kFloatMax = 3.4028234663852886e38;
static_assert(kMaxThickness == sdtext::kMaxThickness && kMaxExtent == sdtext::kMaxExtent, "hit()'s caps");

SDOVL_HD int slots_of(int D) { return 4 * D + 2; }

// the camera as the Q matrix holds it (np.float32([...]), semantic_depth.py:691-694) and the scale of the output image
struct View {
    double cx, cy, f, sx, sy;
};
SDOVL_HD bool finite_f32(double v) { return fabs(v) <= kFloatMax; }      // (a NaN fails)
SDOVL_HD bool camera_ok(const sd_camera& c) { return finite_f32(c.cx) && finite_f32(c.cy) && finite_f32(c.f); }
SDOVL_HD View make_view(double cx_f32, double cy_f32, double f_f32, int net_h, int net_w, int dst_h, int dst_w) {
    return View{cx_f32, cy_f32, f_f32, (double)dst_w / (double)net_w, (double)dst_h / (double)net_h};
}
SDOVL_HD View make_view(const sd_camera& c, int net_h, int net_w, int dst_h, int dst_w) {
    return make_view((double)(float)c.cx, (double)(float)c.cy, (double)(float)c.f, net_h, net_w, dst_h, dst_w);
}
SDOVL_HD bool sizes_ok(int net_h, int net_w, int dst_h, int dst_w) {
    return net_h >= 1 && net_w >= 1 && dst_h >= 1 && dst_w >= 1 && net_h <= kMaxExtent && net_w <= kMaxExtent && dst_h <= kMaxExtent &&
           dst_w <= kMaxExtent;
}
SDOVL_HD bool style_ok(const sd_overlay_style& s, int dst_h) {
    return s.thickness >= 1 && s.thickness <= kMaxThickness && s.profile_thickness >= 1 && s.profile_thickness <= kMaxThickness &&
           s.clip_top >= 0 && s.clip_top <= dst_h;
}

// an end point: absent (its record was not found / not ok), projected, or present but dropped by the projection
enum : int32_t { kAbsent = 0, kOk = 1, kDropped = 2 };
struct Pt {
    int32_t x, y, state;
};
SDOVL_HD Pt absent() { return Pt{0, 0, kAbsent}; }

SDOVL_HD Pt project(const View& v, double X, double Y, double Z) {
#pragma clang fp contract(off)
    Pt p{0, 0, kDropped};
    const double zn = -Z;
    if (!(zn > 0.0)) return p;
    const double s = v.f / zn;
    const double xn = v.cx + X * s;
    const double yn = v.cy - Y * s;
    const double xo = (xn + 0.5) * v.sx - 0.5;
    const double yo = (yn + 0.5) * v.sy - 0.5;
    if (!(fabs(xo) <= kMaxCoord) || !(fabs(yo) <= kMaxCoord)) return p;
    p.x = (int32_t)floor(xo * 256.0 + 0.5);
    p.y = (int32_t)floor(yo * 256.0 + 0.5);
    p.state = kOk;
    return p;
}
SDOVL_HD Pt project(const View& v, const float* pt) { return project(v, (double)pt[0], (double)pt[1], (double)pt[2]); }
SDOVL_HD Pt project(const View& v, const double* pt) { return project(v, pt[0], pt[1], pt[2]); }

// the four end points of profile entry i: the road's left and right end, the fences' left and right intersection
struct EntryPts {
    Pt rl, rr, fl, fr;
};
SDOVL_HD EntryPts entry_points(const View& v, const sd_rw_depth_result* rw, const sd_f2f_depth_result* f2f) {
    EntryPts e{absent(), absent(), absent(), absent()};
    if (rw->found != 0) {
        e.rl = project(v, rw->left_pt);
        e.rr = project(v, rw->right_pt);
    }
    if (f2f && f2f->ok != 0) {
        e.fl = project(v, f2f->left_pt);
        e.fr = project(v, f2f->right_pt);
    }
    return e;
}

// the segment a -> b of a slot: kAbsent (no such segment), kOk (seg is filled) or kDropped (it exists and is skipped: the frame's flag)
SDOVL_HD int32_t join(const Pt& a, const Pt& b, const uint8_t* bgr, int thickness, sd_overlay_segment* seg) {
    if (a.state == kAbsent || b.state == kAbsent) return kAbsent;
    if (a.state != kOk || b.state != kOk) return kDropped;
    seg->ax = a.x;
    seg->ay = a.y;
    seg->bx = b.x;
    seg->by = b.y;
    seg->bgr[0] = bgr[0];
    seg->bgr[1] = bgr[1];
    seg->bgr[2] = bgr[2];
    seg->thickness = (uint8_t)thickness;
    return kOk;
}
// the slots of profile entry i, given its points and those of entry i + 1 (absent() behind the last entry): group 0 the left edge, 1 the
// right edge, 2 the road rung, 3 the fence rung -- slot g * D + i
SDOVL_HD int32_t entry_slot(int group, const EntryPts& e, const EntryPts& next, const sd_overlay_style& st, sd_overlay_segment* seg) {
    switch (group) {
    case 0: return join(e.rl, next.rl, st.edge_bgr, st.profile_thickness, seg);
    case 1: return join(e.rr, next.rr, st.edge_bgr, st.profile_thickness, seg);
    case 2: return join(e.rl, e.rr, st.rw_bgr, st.profile_thickness, seg);
    default: return join(e.fl, e.fr, st.f2f_bgr, st.profile_thickness, seg);
    }
}
// slots 4 D and 4 D + 1: the record's road-width line and the fence record's line
SDOVL_HD int32_t record_slot(const View& v, const sd_rw_result& rec, const sd_overlay_style& st, sd_overlay_segment* seg) {
    if (rec.found == 0) return kAbsent;
    return join(project(v, rec.left_pt), project(v, rec.right_pt), st.rw_bgr, st.thickness, seg);
}
SDOVL_HD int32_t fence_slot(const View& v, const sd_f2f_result* f2f, const sd_overlay_style& st, sd_overlay_segment* seg) {
    if (!f2f || f2f->ok == 0) return kAbsent;
    return join(project(v, f2f->left_pt), project(v, f2f->right_pt), st.f2f_bgr, st.thickness, seg);
}

SDOVL_HD sdtext::Seg seg_of(const sd_overlay_segment& s) { return sdtext::Seg{s.ax, s.ay, s.bx, s.by}; }
SDOVL_HD bool segment_ok(const sd_overlay_segment& s) {
    return s.thickness >= 1 && s.thickness <= kMaxThickness && s.ax >= -kMaxQ && s.ax <= kMaxQ && s.ay >= -kMaxQ && s.ay <= kMaxQ &&
           s.bx >= -kMaxQ && s.bx <= kMaxQ && s.by >= -kMaxQ && s.by <= kMaxQ;
}
// the pixels [x0, x1] x [y0, y1] outside which the segment paints nothing: its bounding box widened by the radius (a pixel outside it is
// farther than the radius from the segment), clipped to rows clip_top .. h - 1 and columns 0 .. w - 1; false when that is empty
SDOVL_HD bool seg_box(const sd_overlay_segment& s, int h, int w, int clip_top, int32_t* box) {
    const int r = (int)s.thickness * 128;
    const int x0 = sdtext::ceil256((s.ax < s.bx ? s.ax : s.bx) - r), x1 = sdtext::floor256((s.ax > s.bx ? s.ax : s.bx) + r);
    const int y0 = sdtext::ceil256((s.ay < s.by ? s.ay : s.by) - r), y1 = sdtext::floor256((s.ay > s.by ? s.ay : s.by) + r);
    box[0] = x0 < 0 ? 0 : x0;
    box[1] = y0 < clip_top ? clip_top : y0;
    box[2] = x1 > w - 1 ? w - 1 : x1;
    box[3] = y1 > h - 1 ? h - 1 : y1;
    return box[0] <= box[2] && box[1] <= box[3];
}

// ---- workspace of the device route (overlay_gpu.hip)
// a frame's camera as the host stages it: cx, cy, f rounded to float32 and promoted
struct CamDev {
    double cx, cy, f, pad;
};
// what overlay_setup_kernel leaves per frame for overlay_raster_kernel: the union of the boxes of the frame's valid slots (empty: x0 > x1)
struct FrameHead {
    int32_t box[4];
};
// ... and per slot: the segment, whether it paints at all (a valid segment with a non-empty box) and that box
struct Slot {
    sd_overlay_segment seg;
    int32_t valid;
    int32_t box[4];      // x0, y0, x1, y1, clipped to rows clip_top .. h - 1 of the frame
};
static_assert(sizeof(CamDev) == 32 && sizeof(FrameHead) == 16 && sizeof(Slot) == 40, "overlay workspace layout");
struct Layout : sdarena::Walker {
    size_t B, nslots;
    Layout(int B_, int D) : B((size_t)B_), nslots((size_t)B_ * slots_of(D)) {}
    size_t cams = take(B * sizeof(CamDev), 16);           // CamDev [B], 16-byte aligned: the caller's upload
    size_t heads = take(B * sizeof(FrameHead), 16);       // FrameHead [B], 16
    size_t slots = take(nslots * sizeof(Slot), 16);       // Slot [B][slots_of(D)], 16
    size_t total = end();
};

}  // namespace sdoverlay
