// device JPEG entropy decoder (jpeg_entropy_gpu.hip): launcher and workspace layout, used by capi.cpp
#pragma once
#include <hip/hip_runtime.h>

#include "jpeg_entropy.hpp"

namespace sd {

// workspace: sdjent::Layout (jpeg_entropy.hpp)

// The caller has run sdjent::args_ok() and checked the alignments and the workspace size.  Uploads the records, the tables and the
// frames' ranges from the host arrays into the workspace (three asynchronous copies on s), clears the eligible frames' coefficients
// and status words with one kernel and decodes with another.  No synchronisation.
hipError_t launch_jpeg_entropy_decode(const uint8_t* bytes, size_t byte_stride, const sd_jpeg_frame_desc* descs_host,
                                      const sd_jpeg_entropy_frame* frames_host, const sd_jpeg_interval* intervals_host, size_t interval_stride,
                                      const sd_jpeg_huff_table* tables_host, int B, int16_t* coef, size_t coef_stride_elems, int32_t* status,
                                      uint8_t* workspace, hipStream_t s);

}  // namespace sd
