// device text route (text_gpu.hip): launcher and workspace layout, used by capi.cpp
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/semdepth.h"
#include "text_draw.hpp"

namespace sd {

// workspace: sdtext::Layout and its records (text_draw.hpp)
using TextExtra = sdtext::Extra;
using TextFrameWs = sdtext::FrameWs;

constexpr int kTextTileW = 64, kTextTileH = 16;      // the pixel tile of one 256-lane workgroup: lane -> column lane % 64, rows lane / 64 + 4 k

// dst u8 [B,h,w,3], records [B], depth[0 .. dlen): the sequence layout drawn in place.  The caller has checked B, the extents, dlen, the
// pointers and the workspace.  Two launches on s, no synchronisation.
hipError_t launch_text_draw_rw(uint8_t* dst, int B, int h, int w, const sd_rw_result* records, const uint8_t* depth, int dlen, uint8_t* workspace,
                               hipStream_t s);

}  // namespace sd
