// device half of the split JPEG route (jpeg_gpu.hip): launcher and workspace layout, used by capi.cpp
#pragma once
#include <hip/hip_runtime.h>

#include "jpeg_common.hpp"

namespace sd {

// the workspace holds frame after frame, component after component, each padded u8 plane at a 256-byte boundary
inline size_t jpeg_plane_slot(const sd_jpeg_frame_desc& d, int c) { return ((size_t)d.blocks_w[c] * d.blocks_h[c] * 64 + 255) / 256 * 256; }
inline size_t jpeg_workspace_bytes(const sd_jpeg_frame_desc* descs, int B) {
    size_t n = 0;
    for (int b = 0; b < B; ++b)
        for (int c = 0; c < descs[b].ncomp; ++c) n += jpeg_plane_slot(descs[b], c);
    return n;
}

// every descriptor must have passed sdjpeg::desc_ok and the buffers must hold what the descriptors imply (capi.cpp checks both)
hipError_t launch_jpeg_reconstruct(const int16_t* coef, size_t frame_stride_elems, const sd_jpeg_frame_desc* descs, int B, uint8_t* bgr,
                                   size_t bgr_frame_stride, uint8_t* workspace, hipStream_t s);

}  // namespace sd
