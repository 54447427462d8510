// device PNG route (png_gpu.hip): launcher and workspace layout, used by capi.cpp
#pragma once
#include <hip/hip_runtime.h>

#include "png_deflate.hpp"

namespace sd {

// workspace: sdpng::Layout (png_deflate.hpp)
constexpr size_t kPngSlot = sdpng::kSlot;

// frames u8 [B,h,w,3] BGR at frame_stride -> one zlib stream per frame at streams + b * stream_stride, sizes[b] = its bytes.  The caller
// has checked the extents (1..16384), stream_stride >= sdpng::stream_bound and the workspace size.  Three launches on s, no synchronisation.
hipError_t launch_png_encode(const uint8_t* frames, size_t frame_stride, int B, int h, int w, uint8_t* streams, size_t stream_stride,
                             uint64_t* sizes, uint8_t* workspace, hipStream_t s);

}  // namespace sd
