// Launch interfaces of seg_eval_gpu.hip (the test mode's input stage and its confusion matrix on the device; contract: include/semdepth.h,
// rule: pil_resample.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include "pil_resample.hpp"

namespace sd {

// workspace: sdpil::Layout (pil_resample.hpp), 16-byte aligned; the caller has
// copied the four tables to their places (`wx`: the host copy of the x windows, which sizes the tiles) in stream order before this.  Two launches (one when dst_h == src_h).
hipError_t launch_pil_resample_u8(const uint8_t* src, int B, int src_h, int src_w, int pixel_stride, int channels, int reverse, uint8_t* dst,
                                  int dst_h, int dst_w, const sdpil::Windows& wx, uint8_t* workspace, hipStream_t s);

struct SegTable {
    uint8_t v[256];
};
// counts: int64 [B][sdpil::kCells], added to with 64-bit vector atomics
hipError_t launch_seg_confusion(const uint8_t* pred, const uint8_t* labels, int B, int height, int width, const SegTable& table, int64_t* counts,
                                hipStream_t s);

}  // namespace sd
