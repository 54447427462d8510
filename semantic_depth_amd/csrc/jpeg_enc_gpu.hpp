// device JPEG encoder (jpeg_enc_gpu.hip): launcher and workspace layout, used by capi.cpp
#pragma once
#include <hip/hip_runtime.h>

#include "jpeg_enc.hpp"

namespace sd {

// workspace of B frames of r MCU rows each: [B * r] u64 offsets of the rows inside their frame's file, then [B * r] u32 row sizes.  No
// coded byte passes through it: the rows are coded twice, once for their sizes and once into place.
inline size_t jpeg_enc_workspace_bytes(int B, int h) {
    const size_t n = (size_t)B * (size_t)sdjenc::mcu_rows(h);
    return (n * (sizeof(uint64_t) + sizeof(uint32_t)) + 15) & ~(size_t)15;
}

// frames u8 [B,h,w,3] BGR at frame_stride -> one JFIF file per frame at streams + b * stream_stride, sizes[b] = its bytes, flags[b] = 1
// (and size 0) when it would pass stream_stride.  The caller has checked the extents (1..16384), the quality (1..100), stream_stride >=
// sdjenc::kHeaderLen and the workspace size.  Three launches on s, no synchronisation.
hipError_t launch_jpeg_encode(const uint8_t* frames, size_t frame_stride, int B, int h, int w, int quality, uint8_t* streams,
                              size_t stream_stride, uint64_t* sizes, int32_t* flags, uint8_t* workspace, hipStream_t s);

}  // namespace sd
