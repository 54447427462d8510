// device PNG scanline reconstruction (png_in_gpu.hip): launcher, argument check and workspace layout, used by capi.cpp
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/semdepth.h"
#include "png_unfilter.hpp"

namespace sd {

// workspace: sdpngin::Layout (png_unfilter.hpp)

// bytes of frame_stride a frame of `channels` needs: its rows, rounded up to the 16-byte pieces the lanes load
inline size_t png_in_rows_bytes(int height, int width, int channels) {
    return (((size_t)height * (1 + (size_t)width * channels)) + 15) & ~(size_t)15;
}

// every index the kernel forms follows from these checks; *why names the first that fails
inline bool png_in_args_ok(size_t frame_stride, const sd_png_frame_desc* descs, int B, int height, int width, size_t out_stride, const char** why) {
    *why = "";
    if (height < 1 || width < 1 || height > sdpngin::kMaxExtent || width > sdpngin::kMaxExtent) { *why = "height and width must be 1..16384"; return false; }
    if (B < 1 || B > 65535) { *why = "B must be 1..65535"; return false; }
    if (frame_stride & 15) { *why = "frame_stride must be a multiple of 16"; return false; }
    if (out_stride < (size_t)height * width * 3) { *why = "a frame is larger than out_stride"; return false; }
    for (int b = 0; b < B; ++b) {
        const sd_png_frame_desc& d = descs[b];
        if (d.height != height || d.width != width) { *why = "a descriptor has another size"; return false; }
        if (d.channels < 1 || d.channels != sdpngin::channels_of(d.color_type)) { *why = "a descriptor's channels are not its colour type's"; return false; }
        if (d.palette_entries < 0 || d.palette_entries > 256 || (d.color_type != 3 && d.palette_entries != 0)) { *why = "a descriptor's palette count is out of range"; return false; }
        if (png_in_rows_bytes(height, width, d.channels) > frame_stride) { *why = "a frame's rows are longer than frame_stride"; return false; }
    }
    return true;
}

// The caller has run png_in_args_ok and checked the alignments and the workspace size.  Uploads the descriptors into the workspace with
// one asynchronous copy on s and launches one workgroup per frame: `waves` is sdpngin::kWaves (the shipped form) or 1 (the bands of a
// frame walked serially by one wave: the degenerate case of the same kernel).  No synchronisation.
hipError_t launch_png_reconstruct(const uint8_t* rows, size_t frame_stride, const sd_png_frame_desc* descs_host, int B, int height, int width,
                                  uint8_t* out, size_t out_stride, int32_t* status, uint8_t* workspace, int waves, hipStream_t s);

}  // namespace sd
