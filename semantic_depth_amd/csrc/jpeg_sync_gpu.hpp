// device JPEG sync decoder (jpeg_sync_gpu.hip): launcher and workspace layout, used by capi.cpp
#pragma once
#include <hip/hip_runtime.h>

#include "jpeg_sync.hpp"

namespace sd {

// workspace: sdjsync::Layout (jpeg_sync.hpp)

// The caller has run sdjsync::args_ok(), checked the alignments and that the workspace holds max_pieces = the largest n_pieces of the
// eligible frames.  Uploads the records, the tables and the ranges (three asynchronous copies on s) and enqueues the six kernels.  No
// synchronisation.
hipError_t launch_jpeg_sync_decode(const uint8_t* bytes, size_t byte_stride, const sd_jpeg_sync_frame* frames_host, const sd_jpeg_sync_interval* intervals_host,
                                   size_t interval_stride, const sd_jpeg_huff_table* tables_host, int B, int subseq_bytes, size_t max_pieces, int16_t* coef,
                                   size_t coef_stride_elems, int32_t* status, uint8_t* workspace, hipStream_t s);

}  // namespace sd
