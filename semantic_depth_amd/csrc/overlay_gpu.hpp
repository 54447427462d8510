// device route of the measurement lines (overlay_gpu.hip): launcher and workspace layout, used by capi.cpp
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/semdepth.h"
#include "overlay_rule.hpp"

namespace sd {

// workspace: sdoverlay::Layout and its records (overlay_rule.hpp)
using OverlayCamDev = sdoverlay::CamDev;
using OverlayFrameHead = sdoverlay::FrameHead;
using OverlaySlot = sdoverlay::Slot;

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
