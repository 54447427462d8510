// device route of the measurement lines (overlay_gpu.hip): launcher and workspace layout, used by capi.cpp
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/semdepth.h"
#include "overlay_rule.hpp"

namespace sd {

// a frame's camera as the host stages it: cx, cy, f rounded to float32 and promoted
struct OverlayCamDev {
    double cx, cy, f, pad;
};
// what overlay_setup_kernel leaves per frame for overlay_raster_kernel: the union of the boxes of the frame's valid slots (empty: x0 > x1)
struct OverlayFrameHead {
    int32_t box[4];
};
// ... and per slot: the segment, whether it paints at all (a valid segment with a non-empty box) and that box
struct OverlaySlot {
    sd_overlay_segment seg;
    int32_t valid;
    int32_t box[4];      // x0, y0, x1, y1, clipped to rows clip_top .. h - 1 of the frame
};
static_assert(sizeof(OverlayCamDev) == 32 && sizeof(OverlayFrameHead) == 16 && sizeof(OverlaySlot) == 40, "overlay workspace layout");

// [B] cameras, [B] heads, [B][4 D + 2] slots; every section starts 16-byte aligned
inline size_t overlay_workspace_bytes(int B, int D) {
    return (size_t)B * (sizeof(OverlayCamDev) + sizeof(OverlayFrameHead)) + (size_t)B * sdoverlay::slots_of(D) * sizeof(OverlaySlot);
}

constexpr int kOverlayTileW = 64, kOverlayTileH = 16;      // the pixel tile of one 256-lane workgroup: lane -> column lane % 64, rows lane / 64 + 4 k

struct OverlayArgs {
    uint8_t* dst;                              // u8 [B,h,w,3]
    const sd_rw_result* records;               // [B]
    const sd_f2f_result* f2f;                  // [B] or null
    const sd_rw_depth_result* rw_profile;      // [B][D] or null when D == 0
    const sd_f2f_depth_result* f2f_profile;    // [B][D] or null
    int32_t* flags;                            // [B]
    OverlayCamDev* cams;                       // workspace
    OverlayFrameHead* heads;
    OverlaySlot* slots;
    sd_overlay_style style;
    int B, D, h, w, net_h, net_w, tiles_x;
};
// lays the workspace sections out in `a`
void overlay_layout(OverlayArgs& a, uint8_t* workspace);
// the caller has checked every argument, laid the workspace out and enqueued the upload of a.cams on s.  Two launches on s.
hipError_t launch_overlay_draw(OverlayArgs a, hipStream_t s);

}  // namespace sd
