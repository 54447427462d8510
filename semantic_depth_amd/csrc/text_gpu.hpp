// device text route (text_gpu.hip): launcher and workspace layout, used by capi.cpp
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/semdepth.h"
#include "text_draw.hpp"

namespace sd {

// what text_layout_kernel leaves per frame for text_raster_kernel: the items, and per item its pixel box and the pen position of every character
struct TextExtra {
    int32_t box[4];                              // x0, y0, x1, y1, clipped to the frame; empty when x0 > x1 or y0 > y1
    uint16_t pen[sdtext::kMaxBytes + 2];         // pen[c] = the advances of the characters before c, pen[len] = the item's
};
struct TextFrameWs {
    int32_t n, pad[3];
    sd_text_item it[sdtext::kMaxItems];
    TextExtra ex[sdtext::kMaxItems];
};
inline size_t text_workspace_bytes(int B) { return (size_t)B * sizeof(TextFrameWs); }

constexpr int kTextTileW = 64, kTextTileH = 16;      // the pixel tile of one 256-lane workgroup: lane -> column lane % 64, rows lane / 64 + 4 k

// dst u8 [B,h,w,3], records [B], depth[0 .. dlen): the sequence layout drawn in place.  The caller has checked B, the extents, dlen, the
// pointers and the workspace.  Two launches on s, no synchronisation.
hipError_t launch_text_draw_rw(uint8_t* dst, int B, int h, int w, const sd_rw_result* records, const uint8_t* depth, int dlen, uint8_t* workspace,
                               hipStream_t s);

}  // namespace sd
