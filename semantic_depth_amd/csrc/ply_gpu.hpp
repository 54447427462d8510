// device PLY route (ply_gpu.hip): launcher and workspace layout, used by capi.cpp
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/semdepth.h"
#include "ply_format.hpp"

namespace sd {

// workspace of B frames of nb = blocks_per_frame(cap) row blocks each: per block its minimum z (f64), its offset inside the frame's rows
// (u64), its bytes, its kept rows and its range verdict (u32 each); per frame the minimum z (f64) and where its rows begin in the text (u64)
inline size_t ply_workspace_bytes(int B, int cap) {
    const size_t nb = (size_t)B * sdply::blocks_per_frame(cap);
    return nb * (2 * sizeof(uint64_t) + 3 * sizeof(uint32_t)) + (size_t)B * 2 * sizeof(uint64_t) + 64;
}
inline size_t ply_text_bound(int B, int cap) { return (size_t)B * sdply::frame_bound(cap); }

// xyz f32 [B,cap,3], rgb u8 [B,cap,3], n i32 [B], records [B] -> the packed files in text[0 .. offsets[B]), offsets u64 [B+1], flags i32 [B].
// The caller has checked B, cap, the pointers and the workspace.  Five launches on s, no synchronisation.
hipError_t launch_ply_format(const float* xyz, const uint8_t* rgb, const int32_t* n, int B, int cap, const sd_rw_result* records, uint8_t* text,
                             size_t capacity, uint64_t* offsets, int32_t* flags, uint8_t* workspace, hipStream_t s);

}  // namespace sd
