// rendered clouds on the device (render_gpu.hip): launcher and workspace layout, used by capi.cpp
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/semdepth.h"
#include "render_rule.hpp"

namespace sd {

// workspace: sdrender::Layout (render_rule.hpp)

// xyz f32 [B,cap,3], rgb u8 [B,cap,3], n i32 [B], records [B] -> dst u8 [B,height,width,3] BGR, flags i32 [B].  The caller has checked B, cap,
// the camera, the pointers and the workspace.  Five launches on s, no synchronisation.
hipError_t launch_render_rw(const float* xyz, const uint8_t* rgb, const int32_t* n, int B, int cap, const sd_rw_result* records,
                            const sd_render_camera& cam, uint8_t* dst, int32_t* flags, uint8_t* workspace, hipStream_t s);

}  // namespace sd
