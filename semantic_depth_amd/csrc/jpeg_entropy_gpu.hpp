// device JPEG entropy decoder (jpeg_entropy_gpu.hip): launcher and workspace layout, used by capi.cpp
#pragma once
#include <hip/hip_runtime.h>

#include "jpeg_entropy.hpp"

namespace sd {

// workspace of B frames: [B] sd_jpeg_entropy_frame, [B * 8] sd_jpeg_huff_table, [B * interval_stride] sd_jpeg_interval, each part
// rounded up to 16 bytes
inline size_t jpeg_entropy_part(size_t bytes) { return (bytes + 15) & ~(size_t)15; }
inline size_t jpeg_entropy_workspace_bytes(int B, size_t interval_stride) {
    return jpeg_entropy_part((size_t)B * sizeof(sd_jpeg_entropy_frame)) + jpeg_entropy_part((size_t)B * sdjent::kTables * sizeof(sd_jpeg_huff_table)) +
           jpeg_entropy_part((size_t)B * interval_stride * sizeof(sd_jpeg_interval));
}

// The caller has run sdjent::args_ok() and checked the alignments and the workspace size.  Uploads the records, the tables and the
// frames' ranges from the host arrays into the workspace (three asynchronous copies on s), clears the eligible frames' coefficients
// and status words with one kernel and decodes with another.  No synchronisation.
hipError_t launch_jpeg_entropy_decode(const uint8_t* bytes, size_t byte_stride, const sd_jpeg_frame_desc* descs_host,
                                      const sd_jpeg_entropy_frame* frames_host, const sd_jpeg_interval* intervals_host, size_t interval_stride,
                                      const sd_jpeg_huff_table* tables_host, int B, int16_t* coef, size_t coef_stride_elems, int32_t* status,
                                      uint8_t* workspace, hipStream_t s);

}  // namespace sd
