// device JPEG sync decoder (jpeg_sync_gpu.hip): launcher and workspace layout, used by capi.cpp
#pragma once
#include <hip/hip_runtime.h>

#include "jpeg_sync.hpp"

namespace sd {

// workspace of B frames of at most P pieces (P rounded up to whole workgroups of sdjsync::kGroup): [B] sd_jpeg_sync_frame,
// [B * 8] sd_jpeg_huff_table, [B * interval_stride] sd_jpeg_sync_interval, [B * P] records, [B * P / kGroup] workgroup end records,
// [B * P] unit ordinals, each part rounded up to 16 bytes
inline size_t jpeg_sync_part(size_t bytes) { return (bytes + 15) & ~(size_t)15; }
inline size_t jpeg_sync_piece_stride(size_t max_pieces) {
    const size_t g = sdjsync::kGroup;
    return (max_pieces < 1 ? 1 : (max_pieces + g - 1) / g) * g;
}
inline size_t jpeg_sync_workspace_bytes(int B, size_t interval_stride, size_t max_pieces) {
    const size_t P = jpeg_sync_piece_stride(max_pieces);
    return jpeg_sync_part((size_t)B * sizeof(sd_jpeg_sync_frame)) + jpeg_sync_part((size_t)B * sdjsync::kTables * sizeof(sd_jpeg_huff_table)) +
           jpeg_sync_part((size_t)B * interval_stride * sizeof(sd_jpeg_sync_interval)) + jpeg_sync_part((size_t)B * P * sizeof(sdjsync::Rec)) +
           jpeg_sync_part((size_t)B * (P / sdjsync::kGroup) * sizeof(sdjsync::Rec)) + jpeg_sync_part((size_t)B * P * sizeof(uint32_t));
}

// The caller has run sdjsync::args_ok(), checked the alignments and that the workspace holds max_pieces = the largest n_pieces of the
// eligible frames.  Uploads the records, the tables and the ranges (three asynchronous copies on s) and enqueues the six kernels.  No
// synchronisation.
hipError_t launch_jpeg_sync_decode(const uint8_t* bytes, size_t byte_stride, const sd_jpeg_sync_frame* frames_host, const sd_jpeg_sync_interval* intervals_host,
                                   size_t interval_stride, const sd_jpeg_huff_table* tables_host, int B, int subseq_bytes, size_t max_pieces, int16_t* coef,
                                   size_t coef_stride_elems, int32_t* status, uint8_t* workspace, hipStream_t s);

}  // namespace sd
