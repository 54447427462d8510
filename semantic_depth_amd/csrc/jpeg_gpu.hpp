// device half of the split JPEG route (jpeg_gpu.hip): launcher and workspace layout, used by capi.cpp
#pragma once
#include <hip/hip_runtime.h>

#include "jpeg_common.hpp"

namespace sd {

// workspace: sdjpeg::take_planes / sdjpeg::workspace_bytes (jpeg_common.hpp)

// every descriptor must have passed sdjpeg::desc_ok and the buffers must hold what the descriptors imply (capi.cpp checks both)
hipError_t launch_jpeg_reconstruct(const int16_t* coef, size_t frame_stride_elems, const sd_jpeg_frame_desc* descs, int B, uint8_t* bgr,
                                   size_t bgr_frame_stride, uint8_t* workspace, hipStream_t s);

}  // namespace sd
