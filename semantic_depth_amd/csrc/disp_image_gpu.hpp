// Launch interface of disp_image_gpu.hip (the disparity images on the device; contract: include/semdepth.h, rule: disp_image_rule.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include "disp_image_rule.hpp"

namespace sd {

// disp f32 [B,h,w] -> dst u8 [B,out_h,out_w,3] BGR, flags i32 [B].  workspace: sddisp::Layout(...).total bytes, 16-byte aligned; the caller
// has copied the frames' multipliers to its `mult` part (has_mult) and, when the sizes differ, the four window tables of the resample to
// their places in its `pil` part (`wx`: the host copy of the x windows), in stream order before this.  Five launches, seven when the sizes
// differ (six when only the widths do); no synchronisation, no allocation.
hipError_t launch_disp_image(const float* disp, int B, int h, int w, int out_h, int out_w, int cmap, int has_mult, uint8_t* dst, int32_t* flags,
                             const sdpil::Windows& wx, uint8_t* workspace, hipStream_t s);

}  // namespace sd
