// device JPEG encoder (jpeg_enc_gpu.hip): launcher and workspace layout, used by capi.cpp
#pragma once
#include <hip/hip_runtime.h>

#include "jpeg_enc.hpp"

namespace sd {

// workspace: sdjenc::Layout (jpeg_enc.hpp)

// frames u8 [B,h,w,3] BGR at frame_stride -> one JFIF file per frame at streams + b * stream_stride, sizes[b] = its bytes, flags[b] = 1
// (and size 0) when it would pass stream_stride.  The caller has checked the extents (1..16384), the quality (1..100), stream_stride >=
// sdjenc::kHeaderLen and the workspace size.  Three launches on s, no synchronisation.
hipError_t launch_jpeg_encode(const uint8_t* frames, size_t frame_stride, int B, int h, int w, int quality, uint8_t* streams,
                              size_t stream_stride, uint64_t* sizes, int32_t* flags, uint8_t* workspace, hipStream_t s);

}  // namespace sd
