// PNG scanline reconstruction, stated ONCE for the host and the device (PNG spec §9, filter types 0-4): the five predictors, the channel
// map of a colour type to OpenCV's 3-channel BGR, and the schedule constants of png_in_gpu.hip that the tests read.  Plain integer
// functions, no state: png_in_gpu.hip runs them per lane, tests/png_in_cases.py restates them in Python.
#pragma once
#include <stdint.h>

#include "../../include/semdepth.h"
#include "arena.hpp"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SDPNGIN_HD __host__ __device__ inline
#else
#define SDPNGIN_HD inline
#endif

namespace sdpngin {

constexpr int kMaxExtent = 16384;        // rows / columns of a frame the device route takes
constexpr int kBandRows = 64;            // rows of one band: one row per lane of a wave
constexpr int kWaves = 16;               // waves of the shipped workgroup: bands in flight per frame
constexpr int kPassRows = 1024;          // = kBandRows * kWaves: rows one pass of the shipped workgroup covers
constexpr int kPhase = 32;               // pixel steps between two workgroup barriers
constexpr int kLag = 3;                  // phases wave j runs behind wave j - 1 ((kLag - 1) * kPhase >= kBandRows: see png_in_gpu.hip)
constexpr int kRing = 128;               // pixels of the LDS ring between two neighbouring bands
static_assert(kPassRows == kBandRows * kWaves, "pass rows");
static_assert((kLag - 1) * kPhase >= kBandRows, "a band's last row must be a whole phase ahead of the band below");
static_assert(kRing >= (kLag + 1) * kPhase && (kRing & (kRing - 1)) == 0, "ring");

// channels (= bytes per pixel at 8 bits) of a colour type, 0 for one this reader does not take
SDPNGIN_HD int channels_of(int ctype) { return ctype == 0 ? 1 : ctype == 2 ? 3 : ctype == 3 ? 1 : ctype == 4 ? 2 : ctype == 6 ? 4 : 0; }

SDPNGIN_HD int iabs(int v) { return v < 0 ? -v : v; }

// a: the byte bpp to the left, b: the byte above, c: the byte above-left (0 outside the frame); signed integers throughout
SDPNGIN_HD int paeth(int a, int b, int c) {
    const int p = a + b - c, pa = iabs(p - a), pb = iabs(p - b), pc = iabs(p - c);
    return pa <= pb && pa <= pc ? a : (pb <= pc ? b : c);
}

SDPNGIN_HD int predictor(int ft, int a, int b, int c) {
    return ft == 0 ? 0 : ft == 1 ? a : ft == 2 ? b : ft == 3 ? ((a + b) >> 1) : paeth(a, b, c);      // (a + b is at most 510: ints)
}

// one filtered byte s -> the reconstructed byte
SDPNGIN_HD int unfilter_byte(int ft, int s, int a, int b, int c) { return (s + predictor(ft, a, b, c)) & 255; }

// One pixel, its `channels` bytes packed little-endian in a word (byte k = channel k), from the packed neighbours.
template <int CH>
SDPNGIN_HD uint32_t unfilter_pixel(int ft, uint32_t s, uint32_t a, uint32_t b, uint32_t c) {
    uint32_t o = 0;
#pragma unroll
    for (int k = 0; k < CH; ++k)
        o |= (uint32_t)unfilter_byte(ft, (s >> (8 * k)) & 255, (a >> (8 * k)) & 255, (b >> (8 * k)) & 255, (c >> (8 * k)) & 255) << (8 * k);
    return o;
}

// packed pixel -> B | G << 8 | R << 16 as cv2.IMREAD_COLOR gives it: gray (0) and gray + alpha (4) replicated, RGB (2) and RGBA (6)
// reversed with the alpha dropped.  Colour type 3 gives the replicated INDEX; the palette lookup is the caller's.
SDPNGIN_HD uint32_t to_bgr(int ctype, uint32_t px) {
    if (ctype == 2 || ctype == 6) return ((px >> 16) & 255) | (px & 0xFF00) | ((px & 255) << 16);
    return (px & 255) * 0x010101u;
}

// ---- workspace of the device route (png_in_gpu.hip)
struct Layout : sdarena::Walker {
    explicit Layout(int B) : descs(take((size_t)B * sizeof(sd_png_frame_desc), 16)) {}
    size_t descs;                // sd_png_frame_desc [B], 16-byte aligned: the launcher's upload
    size_t total = end(16);
};

}  // namespace sdpngin
