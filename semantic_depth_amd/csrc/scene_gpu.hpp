// device scene PLY route (scene_gpu.hip): launcher and workspace layout, used by capi.cpp
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/semdepth.h"
#include "scene_format.hpp"

namespace sd {

// what sd_scene_format was given (device pointers; the fence group, f2f and the boxes nullable)
struct SceneBatch {
    const float *road_xyz, *left_xyz, *right_xyz;
    const uint8_t *road_rgb, *left_rgb, *right_rgb;
    const int32_t* n_road;
    int B, cap_road, cap_fence;
    const sd_rw_result* records;
    const sd_f2f_result* f2f;
    const sd_plane_box *road_boxes, *fence_boxes;
    uint32_t mask, lattice_cap;
};

// workspace: sdscene::Layout (scene_format.hpp)
inline size_t scene_text_bound(int B, int cap_road, int cap_fence, uint32_t lattice_cap, uint32_t mask) {
    return (size_t)B * ((size_t)sdply::kHeaderCap + (size_t)sdscene::rows_bound(cap_road, cap_fence, lattice_cap, mask) * sdply::kRowCap);
}

// The caller has checked the counts, the pointers, their alignment and the workspace.  Six launches on s, no synchronisation.
hipError_t launch_scene_format(const SceneBatch& in, uint8_t* text, size_t capacity, uint64_t* offsets, int32_t* flags, uint8_t* workspace,
                               hipStream_t s);

}  // namespace sd
