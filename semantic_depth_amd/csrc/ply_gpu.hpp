// device PLY route (ply_gpu.hip): launcher and workspace layout, used by capi.cpp
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/semdepth.h"
#include "ply_format.hpp"

namespace sd {

// workspace: sdply::Layout (ply_format.hpp)
inline size_t ply_text_bound(int B, int cap) { return (size_t)B * sdply::frame_bound(cap); }

// xyz f32 [B,cap,3], rgb u8 [B,cap,3], n i32 [B], records [B] -> the packed files in text[0 .. offsets[B]), offsets u64 [B+1], flags i32 [B].
// The caller has checked B, cap, the pointers and the workspace.  Five launches on s, no synchronisation.
hipError_t launch_ply_format(const float* xyz, const uint8_t* rgb, const int32_t* n, int B, int cap, const sd_rw_result* records, uint8_t* text,
                             size_t capacity, uint64_t* offsets, int32_t* flags, uint8_t* workspace, hipStream_t s);

}  // namespace sd
