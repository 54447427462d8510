// What the host JPEG reader (host_jpeg.cpp) and the device reconstruction (jpeg_gpu.hip) share, so that the two routes cannot drift:
// the ISLOW inverse DCT as ONE function compiled for both sides, and the geometry / consistency rules of sd_jpeg_frame_desc.
// Plain C++17: host_jpeg.cpp is also built with g++ alone (scripts/fuzz_decoders.cpp).
#pragma once
#include "../../include/semdepth.h"

#include <cstddef>
#include <cstdint>

#include "arena.hpp"

#if defined(__HIPCC__)
#define SD_JPEG_HD __host__ __device__
#else
#define SD_JPEG_HD
#endif
// the device pass keeps a block in registers: both passes fully unrolled there; the host build is left to its compiler as before
#if defined(__HIP_DEVICE_COMPILE__)
#define SD_JPEG_UNROLL _Pragma("unroll")
#else
#define SD_JPEG_UNROLL
#endif

namespace sdjpeg {

// jidctint.c (libjpeg 6b / libjpeg-turbo, DCTSIZE 8): accurate integer inverse DCT on dequantised coefficients, output
// level-shifted by +128 and range-limited to 0..255.  The sums are formed in int64_t on both sides: a crafted stream may carry
// dequantised coefficients up to 32767 * 65535, far outside what 32-bit sums hold, and the two routes must agree on it too.
SD_JPEG_HD inline int32_t descale(int64_t x, int n) { return (int32_t)((x + ((int64_t)1 << (n - 1))) >> n); }
SD_JPEG_HD inline uint8_t clamp_shift(int32_t v) { v += 128; return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }
SD_JPEG_HD static void idct_islow(const int32_t* in, uint8_t* out, int stride) {
    constexpr int CB = 13, P1 = 2;
    const int32_t F0_298631336 = 2446, F0_390180644 = 3196, F0_541196100 = 4433, F0_765366865 = 6270, F0_899976223 = 7373,
                  F1_175875602 = 9633, F1_501321110 = 12299, F1_847759065 = 15137, F1_961570560 = 16069, F2_053119869 = 16819,
                  F2_562915447 = 20995, F3_072711026 = 25172;
    int32_t ws[64];
    SD_JPEG_UNROLL
    for (int c = 0; c < 8; ++c) {
        const int32_t* ip = in + c;
        int32_t* wp = ws + c;
        if (!(ip[8] | ip[16] | ip[24] | ip[32] | ip[40] | ip[48] | ip[56])) {
            const int32_t dc = (int32_t)((uint32_t)ip[0] << P1);      // (the product modulo 2^32 without signed overflow: a crafted DC may exceed 2^29)
            for (int r = 0; r < 8; ++r) wp[8 * r] = dc;
            continue;
        }
        int64_t z2 = ip[16], z3 = ip[48];
        int64_t z1 = (z2 + z3) * F0_541196100;
        int64_t tmp2 = z1 + z3 * (-F1_847759065);
        int64_t tmp3 = z1 + z2 * F0_765366865;
        z2 = ip[0]; z3 = ip[32];
        int64_t tmp0 = (z2 + z3) * (1 << CB);
        int64_t tmp1 = (z2 - z3) * (1 << CB);
        const int64_t tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
        tmp0 = ip[56]; tmp1 = ip[40]; tmp2 = ip[24]; tmp3 = ip[8];
        z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
        int64_t z4 = tmp1 + tmp3;
        const int64_t z5 = (z3 + z4) * F1_175875602;
        tmp0 *= F0_298631336; tmp1 *= F2_053119869; tmp2 *= F3_072711026; tmp3 *= F1_501321110;
        z1 *= -F0_899976223; z2 *= -F2_562915447; z3 *= -F1_961570560; z4 *= -F0_390180644;
        z3 += z5; z4 += z5;
        tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
        wp[0] = descale(tmp10 + tmp3, CB - P1);  wp[56] = descale(tmp10 - tmp3, CB - P1);
        wp[8] = descale(tmp11 + tmp2, CB - P1);  wp[48] = descale(tmp11 - tmp2, CB - P1);
        wp[16] = descale(tmp12 + tmp1, CB - P1); wp[40] = descale(tmp12 - tmp1, CB - P1);
        wp[24] = descale(tmp13 + tmp0, CB - P1); wp[32] = descale(tmp13 - tmp0, CB - P1);
    }
    SD_JPEG_UNROLL
    for (int r = 0; r < 8; ++r) {
        const int32_t* wp = ws + 8 * r;
        uint8_t* o = out + (size_t)r * stride;
        if (!(wp[1] | wp[2] | wp[3] | wp[4] | wp[5] | wp[6] | wp[7])) {
            const uint8_t dc = clamp_shift(descale(wp[0], P1 + 3));
            for (int c = 0; c < 8; ++c) o[c] = dc;
            continue;
        }
        int64_t z2 = wp[2], z3 = wp[6];
        int64_t z1 = (z2 + z3) * F0_541196100;
        int64_t tmp2 = z1 + z3 * (-F1_847759065);
        int64_t tmp3 = z1 + z2 * F0_765366865;
        int64_t tmp0 = ((int64_t)wp[0] + wp[4]) * (1 << CB);
        int64_t tmp1 = ((int64_t)wp[0] - wp[4]) * (1 << CB);
        const int64_t tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
        tmp0 = wp[7]; tmp1 = wp[5]; tmp2 = wp[3]; tmp3 = wp[1];
        z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
        int64_t z4 = tmp1 + tmp3;
        const int64_t z5 = (z3 + z4) * F1_175875602;
        tmp0 *= F0_298631336; tmp1 *= F2_053119869; tmp2 *= F3_072711026; tmp3 *= F1_501321110;
        z1 *= -F0_899976223; z2 *= -F2_562915447; z3 *= -F1_961570560; z4 *= -F0_390180644;
        z3 += z5; z4 += z5;
        tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
        constexpr int S = CB + P1 + 3;
        o[0] = clamp_shift(descale(tmp10 + tmp3, S)); o[7] = clamp_shift(descale(tmp10 - tmp3, S));
        o[1] = clamp_shift(descale(tmp11 + tmp2, S)); o[6] = clamp_shift(descale(tmp11 - tmp2, S));
        o[2] = clamp_shift(descale(tmp12 + tmp1, S)); o[5] = clamp_shift(descale(tmp12 - tmp1, S));
        o[3] = clamp_shift(descale(tmp13 + tmp0, S)); o[4] = clamp_shift(descale(tmp13 - tmp0, S));
    }
}

// 8x8 blocks per row / column of component i's padded plane (a whole number of MCUs), as the decoder lays its planes out
inline int blocks_w(int W, int hmax, int h) { return (W + 8 * hmax - 1) / (8 * hmax) * h; }
inline int blocks_h(int H, int vmax, int v) { return (H + 8 * vmax - 1) / (8 * vmax) * v; }

// int16 elements of a frame's coefficient buffer
inline size_t desc_coef_elems(const sd_jpeg_frame_desc& d) {
    size_t n = 0;
    for (int i = 0; i < d.ncomp; ++i) n += (size_t)d.blocks_w[i] * d.blocks_h[i] * 64;
    return n;
}
// bytes of a frame's padded u8 component planes
inline size_t desc_plane_bytes(const sd_jpeg_frame_desc& d) { return desc_coef_elems(d); }

// a descriptor the decoder could have written: the sizes, samplings and offsets follow from height, width, ncomp, hmax, vmax alone, so a
// consistent descriptor bounds every index the reconstruction forms
inline bool desc_ok(const sd_jpeg_frame_desc& d) {
    if (d.height <= 0 || d.width <= 0 || d.height > 65535 || d.width > 65535 || (size_t)d.height * (size_t)d.width > ((size_t)1 << 28)) return false;
    if (d.ncomp != 1 && d.ncomp != 3) return false;
    if (d.orientation < 1 || d.orientation > 8 || d.adobe_transform < -1 || d.adobe_transform > 255) return false;
    if (d.ncomp == 1 ? !(d.hmax == 1 && d.vmax == 1)
                     : !((d.hmax == 1 && d.vmax == 1) || (d.hmax == 2 && d.vmax == 1) || (d.hmax == 2 && d.vmax == 2)))
        return false;
    int64_t off = 0;
    for (int i = 0; i < d.ncomp; ++i) {
        const int h = i ? 1 : d.hmax, v = i ? 1 : d.vmax;
        if (d.blocks_w[i] != blocks_w(d.width, d.hmax, h) || d.blocks_h[i] != blocks_h(d.height, d.vmax, v) || d.coef_offset[i] != off) return false;
        off += (int64_t)d.blocks_w[i] * d.blocks_h[i] * 64;
    }
    return true;
}

// ---- workspace of the device half (jpeg_gpu.hip): frame after frame, component after component, each padded u8 plane
// [blocks_h * 8][blocks_w * 8] at a 256-byte boundary.  One walk serves the size query and the launcher: plane[c] of the next frame
inline void take_planes(sdarena::Walker& w, const sd_jpeg_frame_desc& d, size_t plane[3]) {
    for (int c = 0; c < d.ncomp; ++c) plane[c] = w.take((size_t)d.blocks_w[c] * d.blocks_h[c] * 64, 256);
}
inline size_t workspace_bytes(const sd_jpeg_frame_desc* descs, int B) {
    sdarena::Walker w;
    size_t plane[3];
    for (int b = 0; b < B; ++b) take_planes(w, descs[b], plane);
    return w.end(256);
}

}  // namespace sdjpeg
