// Launch interfaces of rw_profile.hip (the depth profile on the device; contract: include/semdepth.h, arithmetic: rw_profile.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include "rw_profile.hpp"

namespace sd {

// workspace: sdrwp::Layout (rw_profile.hpp), 16-byte aligned; the caller copies the D sorted windows to its `windows` part in stream order before this.
hipError_t launch_rw_profile(const float* xyz, const int32_t* n, int B, int cap, int D, void* workspace, sd_rw_depth_result* results, hipStream_t s);

struct F2fDepths {
    double d[SD_PROFILE_MAX_DEPTHS];
};
hipError_t launch_f2f_profile(const sd_rw_result* road, const sd_f2f_result* fence, int B, const F2fDepths& depths, int D,
                              sd_f2f_depth_result* results, hipStream_t s);

}  // namespace sd
