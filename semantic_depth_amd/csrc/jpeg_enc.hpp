// The coder of the result video's frames (sd_jpeg_encode_bgr / sd_jpeg_encode_bgr_host; stream format: include/semdepth.h), stated ONCE for
// the kernels of jpeg_enc_gpu.hip and the host function of host_jpeg_enc.cpp: the colour rule, the chroma box, the two passes of the integer
// forward DCT, the quantiser, the Huffman symbols of one block, the file header and the bound on a frame's bytes.  Both sides call these
// functions and all of it is integer arithmetic, so they agree on every bit; what differs is only who walks the blocks (one loop on the host,
// one workgroup per MCU row on the device).
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include <stddef.h>
#include <stdint.h>

#include "arena.hpp"

#if defined(__HIPCC__)
#define SDJENC_HD __host__ __device__ inline
#else
#define SDJENC_HD inline
#endif

namespace sdjenc {

constexpr int kMaxExtent = 16384;
constexpr int kHeaderLen = 613;      // SOI 2, APP0 18, DQT 134, SOF0 19, DHT 420, DRI 6, SOS 14
// A block's worst case: a DC symbol of at most 11 bits with 11 extra bits (category <= 11) and 63 AC symbols of at most 16 bits with 10
// extra bits each (category <= 10; no ZRL and no EOB then): 22 + 63 * 26 = 1660 bits, counted as 208 bytes.
constexpr int kBlockBitsMax = 22 + 63 * 26;
constexpr int kBlockBytesMax = 208;
static_assert(kBlockBitsMax <= 8 * kBlockBytesMax, "block bound");

SDJENC_HD int mcus_w(int w) { return (w + 15) >> 4; }
SDJENC_HD int mcu_rows(int h) { return (h + 15) >> 4; }
// one restart interval (an MCU row: 6 blocks per MCU), every byte stuffed, the padding inside the last byte, and its RSTm / EOI marker
SDJENC_HD size_t row_bound(int w) { return 2 * (size_t)kBlockBytesMax * 6 * (size_t)mcus_w(w) + 2; }
// capacity bound of a frame's file for any content
SDJENC_HD size_t stream_bound(int h, int w) { return (size_t)kHeaderLen + (size_t)mcu_rows(h) * row_bound(w); }

// ---- tables: the zigzag scan, the ITU T.81 Annex K quantisation tables (in zigzag order) and typical Huffman tables (BITS, HUFFVAL, and the
// canonical code and size of every symbol derived from them; size 0 = no such symbol) ----
constexpr uint8_t kZigzag[64] = {
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5,
    12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
    58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63,
};
constexpr uint8_t kInvZigzag[64] = {
    0, 1, 5, 6, 14, 15, 27, 28, 2, 4, 7, 13, 16, 26, 29, 42,
    3, 8, 12, 17, 25, 30, 41, 43, 9, 11, 18, 24, 31, 40, 44, 53,
    10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60,
    21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63,
};
constexpr uint8_t kBaseLumaZz[64] = {
    16, 11, 12, 14, 12, 10, 16, 14, 13, 14, 18, 17, 16, 19, 24, 40,
    26, 24, 22, 22, 24, 49, 35, 37, 29, 40, 58, 51, 61, 60, 57, 51,
    56, 55, 64, 72, 92, 78, 64, 68, 87, 69, 55, 56, 80, 109, 81, 87,
    95, 98, 103, 104, 103, 62, 77, 113, 121, 112, 100, 120, 92, 101, 103, 99,
};
constexpr uint8_t kBaseChromaZz[64] = {
    17, 18, 18, 24, 21, 24, 47, 26, 26, 47, 99, 66, 56, 66, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
};
constexpr uint8_t kBitsDcLuma[16] = {
    0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0,
};
constexpr uint8_t kValsDcLuma[12] = {
    0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11,
};
constexpr uint16_t kCodeDcLuma[12] = {
    0, 2, 3, 4, 5, 6, 14, 30, 62, 126, 254, 510,
};
constexpr uint8_t kSizeDcLuma[12] = {
    2, 3, 3, 3, 3, 3, 4, 5, 6, 7, 8, 9,
};
constexpr uint8_t kBitsAcLuma[16] = {
    0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125,
};
constexpr uint8_t kValsAcLuma[162] = {
    1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113,
    20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21, 82, 209, 240, 36, 51, 98, 114,
    130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55,
    56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89,
    90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 131,
    132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163,
    164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195,
    196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 225, 226,
    227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250,
};
constexpr uint16_t kCodeAcLuma[256] = {
    10, 0, 1, 4, 11, 26, 120, 248, 1014, 65410, 65411, 0, 0, 0, 0, 0,
    0, 12, 27, 121, 502, 2038, 65412, 65413, 65414, 65415, 65416, 0, 0, 0, 0, 0,
    0, 28, 249, 1015, 4084, 65417, 65418, 65419, 65420, 65421, 65422, 0, 0, 0, 0, 0,
    0, 58, 503, 4085, 65423, 65424, 65425, 65426, 65427, 65428, 65429, 0, 0, 0, 0, 0,
    0, 59, 1016, 65430, 65431, 65432, 65433, 65434, 65435, 65436, 65437, 0, 0, 0, 0, 0,
    0, 122, 2039, 65438, 65439, 65440, 65441, 65442, 65443, 65444, 65445, 0, 0, 0, 0, 0,
    0, 123, 4086, 65446, 65447, 65448, 65449, 65450, 65451, 65452, 65453, 0, 0, 0, 0, 0,
    0, 250, 4087, 65454, 65455, 65456, 65457, 65458, 65459, 65460, 65461, 0, 0, 0, 0, 0,
    0, 504, 32704, 65462, 65463, 65464, 65465, 65466, 65467, 65468, 65469, 0, 0, 0, 0, 0,
    0, 505, 65470, 65471, 65472, 65473, 65474, 65475, 65476, 65477, 65478, 0, 0, 0, 0, 0,
    0, 506, 65479, 65480, 65481, 65482, 65483, 65484, 65485, 65486, 65487, 0, 0, 0, 0, 0,
    0, 1017, 65488, 65489, 65490, 65491, 65492, 65493, 65494, 65495, 65496, 0, 0, 0, 0, 0,
    0, 1018, 65497, 65498, 65499, 65500, 65501, 65502, 65503, 65504, 65505, 0, 0, 0, 0, 0,
    0, 2040, 65506, 65507, 65508, 65509, 65510, 65511, 65512, 65513, 65514, 0, 0, 0, 0, 0,
    0, 65515, 65516, 65517, 65518, 65519, 65520, 65521, 65522, 65523, 65524, 0, 0, 0, 0, 0,
    2041, 65525, 65526, 65527, 65528, 65529, 65530, 65531, 65532, 65533, 65534, 0, 0, 0, 0, 0,
};
constexpr uint8_t kSizeAcLuma[256] = {
    4, 2, 2, 3, 4, 5, 7, 8, 10, 16, 16, 0, 0, 0, 0, 0,
    0, 4, 5, 7, 9, 11, 16, 16, 16, 16, 16, 0, 0, 0, 0, 0,
    0, 5, 8, 10, 12, 16, 16, 16, 16, 16, 16, 0, 0, 0, 0, 0,
    0, 6, 9, 12, 16, 16, 16, 16, 16, 16, 16, 0, 0, 0, 0, 0,
    0, 6, 10, 16, 16, 16, 16, 16, 16, 16, 16, 0, 0, 0, 0, 0,
    0, 7, 11, 16, 16, 16, 16, 16, 16, 16, 16, 0, 0, 0, 0, 0,
    0, 7, 12, 16, 16, 16, 16, 16, 16, 16, 16, 0, 0, 0, 0, 0,
    0, 8, 12, 16, 16, 16, 16, 16, 16, 16, 16, 0, 0, 0, 0, 0,
    0, 9, 15, 16, 16, 16, 16, 16, 16, 16, 16, 0, 0, 0, 0, 0,
    0, 9, 16, 16, 16, 16, 16, 16, 16, 16, 16, 0, 0, 0, 0, 0,
    0, 9, 16, 16, 16, 16, 16, 16, 16, 16, 16, 0, 0, 0, 0, 0,
    0, 10, 16, 16, 16, 16, 16, 16, 16, 16, 16, 0, 0, 0, 0, 0,
    0, 10, 16, 16, 16, 16, 16, 16, 16, 16, 16, 0, 0, 0, 0, 0,
    0, 11, 16, 16, 16, 16, 16, 16, 16, 16, 16, 0, 0, 0, 0, 0,
    0, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 0, 0, 0, 0, 0,
    11, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 0, 0, 0, 0, 0,
};
constexpr uint8_t kBitsDcChroma[16] = {
    0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0,
};
constexpr uint8_t kValsDcChroma[12] = {
    0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11,
};
constexpr uint16_t kCodeDcChroma[12] = {
    0, 1, 2, 6, 14, 30, 62, 126, 254, 510, 1022, 2046,
};
constexpr uint8_t kSizeDcChroma[12] = {
    2, 2, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11,
};
constexpr uint8_t kBitsAcChroma[16] = {
    0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119,
};
constexpr uint8_t kValsAcChroma[162] = {
    0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34,
    50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35, 51, 82, 240, 21, 98, 114, 209,
    10, 22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54,
    55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88,
    89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122,
    130, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154,
    162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186,
    194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218,
    226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250,
};
constexpr uint16_t kCodeAcChroma[256] = {
    0, 1, 4, 10, 24, 25, 56, 120, 500, 1014, 4084, 0, 0, 0, 0, 0,
    0, 11, 57, 246, 501, 2038, 4085, 65416, 65417, 65418, 65419, 0, 0, 0, 0, 0,
    0, 26, 247, 1015, 4086, 32706, 65420, 65421, 65422, 65423, 65424, 0, 0, 0, 0, 0,
    0, 27, 248, 1016, 4087, 65425, 65426, 65427, 65428, 65429, 65430, 0, 0, 0, 0, 0,
    0, 58, 502, 65431, 65432, 65433, 65434, 65435, 65436, 65437, 65438, 0, 0, 0, 0, 0,
    0, 59, 1017, 65439, 65440, 65441, 65442, 65443, 65444, 65445, 65446, 0, 0, 0, 0, 0,
    0, 121, 2039, 65447, 65448, 65449, 65450, 65451, 65452, 65453, 65454, 0, 0, 0, 0, 0,
    0, 122, 2040, 65455, 65456, 65457, 65458, 65459, 65460, 65461, 65462, 0, 0, 0, 0, 0,
    0, 249, 65463, 65464, 65465, 65466, 65467, 65468, 65469, 65470, 65471, 0, 0, 0, 0, 0,
    0, 503, 65472, 65473, 65474, 65475, 65476, 65477, 65478, 65479, 65480, 0, 0, 0, 0, 0,
    0, 504, 65481, 65482, 65483, 65484, 65485, 65486, 65487, 65488, 65489, 0, 0, 0, 0, 0,
    0, 505, 65490, 65491, 65492, 65493, 65494, 65495, 65496, 65497, 65498, 0, 0, 0, 0, 0,
    0, 506, 65499, 65500, 65501, 65502, 65503, 65504, 65505, 65506, 65507, 0, 0, 0, 0, 0,
    0, 2041, 65508, 65509, 65510, 65511, 65512, 65513, 65514, 65515, 65516, 0, 0, 0, 0, 0,
    0, 16352, 65517, 65518, 65519, 65520, 65521, 65522, 65523, 65524, 65525, 0, 0, 0, 0, 0,
    1018, 32707, 65526, 65527, 65528, 65529, 65530, 65531, 65532, 65533, 65534, 0, 0, 0, 0, 0,
};
constexpr uint8_t kSizeAcChroma[256] = {
    2, 2, 3, 4, 5, 5, 6, 7, 9, 10, 12, 0, 0, 0, 0, 0,
    0, 4, 6, 8, 9, 11, 12, 16, 16, 16, 16, 0, 0, 0, 0, 0,
    0, 5, 8, 10, 12, 15, 16, 16, 16, 16, 16, 0, 0, 0, 0, 0,
    0, 5, 8, 10, 12, 16, 16, 16, 16, 16, 16, 0, 0, 0, 0, 0,
    0, 6, 9, 16, 16, 16, 16, 16, 16, 16, 16, 0, 0, 0, 0, 0,
    0, 6, 10, 16, 16, 16, 16, 16, 16, 16, 16, 0, 0, 0, 0, 0,
    0, 7, 11, 16, 16, 16, 16, 16, 16, 16, 16, 0, 0, 0, 0, 0,
    0, 7, 11, 16, 16, 16, 16, 16, 16, 16, 16, 0, 0, 0, 0, 0,
    0, 8, 16, 16, 16, 16, 16, 16, 16, 16, 16, 0, 0, 0, 0, 0,
    0, 9, 16, 16, 16, 16, 16, 16, 16, 16, 16, 0, 0, 0, 0, 0,
    0, 9, 16, 16, 16, 16, 16, 16, 16, 16, 16, 0, 0, 0, 0, 0,
    0, 9, 16, 16, 16, 16, 16, 16, 16, 16, 16, 0, 0, 0, 0, 0,
    0, 9, 16, 16, 16, 16, 16, 16, 16, 16, 16, 0, 0, 0, 0, 0,
    0, 11, 16, 16, 16, 16, 16, 16, 16, 16, 16, 0, 0, 0, 0, 0,
    0, 14, 16, 16, 16, 16, 16, 16, 16, 16, 16, 0, 0, 0, 0, 0,
    10, 15, 16, 16, 16, 16, 16, 16, 16, 16, 16, 0, 0, 0, 0, 0,
};

// ---- colour: BGR u8 -> Y Cb Cr u8, 16-bit fixed point ----
SDJENC_HD int ycc_y(int b, int g, int r) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }
SDJENC_HD int ycc_cb(int b, int g, int r) { return (-11059 * r - 21709 * g + 32768 * b + 8421375) >> 16; }
SDJENC_HD int ycc_cr(int b, int g, int r) { return (32768 * r - 27439 * g - 5329 * b + 8421375) >> 16; }
SDJENC_HD int box4(int a, int b, int c, int d) { return (a + b + c + d + 2) >> 2; }

// ---- forward DCT: the separable 13-bit-constant integer form (Loeffler, Ligtenberg and Moschytz's 12-multiply flow graph).  The row
// pass leaves its outputs scaled by 4 * sqrt(8), the column pass takes 2 of those bits back: the 64 results are the orthonormal DCT's
// coefficients times 8. ----
constexpr int kC0_298 = 2446, kC0_390 = 3196, kC0_541 = 4433, kC0_765 = 6270, kC0_899 = 7373, kC1_175 = 9633;
constexpr int kC1_501 = 12299, kC1_847 = 15137, kC1_961 = 16069, kC2_053 = 16819, kC2_562 = 20995, kC3_072 = 25172;
SDJENC_HD int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }
// v[0..8) in place
template <bool kRowPass>
SDJENC_HD void fdct8(int* v) {
    const int s07 = v[0] + v[7], d07 = v[0] - v[7], s16 = v[1] + v[6], d16 = v[1] - v[6];
    const int s25 = v[2] + v[5], d25 = v[2] - v[5], s34 = v[3] + v[4], d34 = v[3] - v[4];
    const int e0 = s07 + s34, e3 = s07 - s34, e1 = s16 + s25, e2 = s16 - s25;
    constexpr int down = kRowPass ? 13 - 2 : 13 + 2;
    if (kRowPass) {
        v[0] = (e0 + e1) * 4;
        v[4] = (e0 - e1) * 4;
    } else {
        v[0] = descale(e0 + e1, 2);
        v[4] = descale(e0 - e1, 2);
    }
    const int ze = (e2 + e3) * kC0_541;
    v[2] = descale(ze + e3 * kC0_765, down);
    v[6] = descale(ze - e2 * kC1_847, down);
    const int z1 = (d34 + d07) * -kC0_899, z2 = (d25 + d16) * -kC2_562;
    const int z5 = (d34 + d16 + d25 + d07) * kC1_175;
    const int z3 = (d34 + d16) * -kC1_961 + z5, z4 = (d25 + d07) * -kC0_390 + z5;
    v[7] = descale(d34 * kC0_298 + z1 + z3, down);
    v[5] = descale(d25 * kC2_053 + z2 + z4, down);
    v[3] = descale(d16 * kC3_072 + z2 + z3, down);
    v[1] = descale(d07 * kC1_501 + z1 + z4, down);
}

// ---- quantisation ----
// entry of the table for `quality` 1..100 from the Annex K entry `base` (the IJG rule)
SDJENC_HD int quant_entry(int base, int quality) {
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    const int t = (base * s + 50) / 100;
    return t < 1 ? 1 : (t > 255 ? 255 : t);
}
// c = 8 * the coefficient, d = 8 * the table entry: half away from zero
SDJENC_HD int quantise(int c, int d) {
    const int a = c < 0 ? -c : c;
    const int q = (a + (d >> 1)) / d;
    return c < 0 ? -q : q;
}

// ---- entropy coding of one block ----
SDJENC_HD int category(int a) { return a ? 32 - __builtin_clz((unsigned)a) : 0; }
// Sink: void put(uint32_t bits, int nbits), most significant bit first, nbits <= 27.  zz: the block's quantised coefficients in zigzag
// order; diff: zz[0] minus the predictor.
template <class Sink>
SDJENC_HD void encode_block(const int16_t* zz, int diff, bool chroma, Sink& s) {
    const uint16_t* dcc = chroma ? kCodeDcChroma : kCodeDcLuma;
    const uint8_t* dcs = chroma ? kSizeDcChroma : kSizeDcLuma;
    const uint16_t* acc = chroma ? kCodeAcChroma : kCodeAcLuma;
    const uint8_t* acs = chroma ? kSizeAcChroma : kSizeAcLuma;
    {
        int cat = category(diff < 0 ? -diff : diff);
        if (cat > 11) cat = 11;                                     // (never: |diff| <= 2040)
        const uint32_t extra = (uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << cat) - 1);
        s.put(((uint32_t)dcc[cat] << cat) | extra, dcs[cat] + cat);
    }
    int run = 0;
    for (int k = 1; k < 64; ++k) {
        const int v = zz[k];
        if (v == 0) { ++run; continue; }
        for (; run > 15; run -= 16) s.put(acc[0xF0], acs[0xF0]);    // ZRL
        const int cat = category(v < 0 ? -v : v);
        const int sym = (run << 4) | cat;
        const uint32_t extra = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << cat) - 1);
        s.put(((uint32_t)acc[sym] << cat) | extra, acs[sym] + cat);
        run = 0;
    }
    if (run) s.put(acc[0], acs[0]);                                 // EOB, omitted when coefficient 63 is non-zero
}
struct CountSink {
    uint32_t bits;
    SDJENC_HD void put(uint32_t, int n) { bits += (uint32_t)n; }
};

// ---- the file header, kHeaderLen bytes; div[c][k] = 8 * the quantiser of class c (0 luminance, 1 chrominance) at zigzag position k ----
SDJENC_HD void make_header(uint8_t* p, uint16_t (*div)[64], int h, int w, int quality) {
    int n = 0;
    auto u8 = [&](int v) { p[n++] = (uint8_t)v; };
    auto u16 = [&](int v) { u8(v >> 8); u8(v); };
    u16(0xFFD8);
    u16(0xFFE0); u16(16); u8('J'); u8('F'); u8('I'); u8('F'); u8(0); u16(0x0101); u8(0); u16(1); u16(1); u8(0); u8(0);
    u16(0xFFDB); u16(2 + 2 * 65);
    for (int c = 0; c < 2; ++c) {
        u8(c);
        for (int k = 0; k < 64; ++k) {
            const int q = quant_entry(c ? kBaseChromaZz[k] : kBaseLumaZz[k], quality);
            div[c][k] = (uint16_t)(8 * q);
            u8(q);
        }
    }
    u16(0xFFC0); u16(17); u8(8); u16(h); u16(w); u8(3);
    u8(1); u8(0x22); u8(0);
    u8(2); u8(0x11); u8(1);
    u8(3); u8(0x11); u8(1);
    u16(0xFFC4); u16(2 + 2 * (17 + 12) + 2 * (17 + 162));
    u8(0x00); for (int i = 0; i < 16; ++i) u8(kBitsDcLuma[i]);   for (int i = 0; i < 12; ++i) u8(kValsDcLuma[i]);
    u8(0x10); for (int i = 0; i < 16; ++i) u8(kBitsAcLuma[i]);   for (int i = 0; i < 162; ++i) u8(kValsAcLuma[i]);
    u8(0x01); for (int i = 0; i < 16; ++i) u8(kBitsDcChroma[i]); for (int i = 0; i < 12; ++i) u8(kValsDcChroma[i]);
    u8(0x11); for (int i = 0; i < 16; ++i) u8(kBitsAcChroma[i]); for (int i = 0; i < 162; ++i) u8(kValsAcChroma[i]);
    u16(0xFFDD); u16(4); u16(mcus_w(w));
    u16(0xFFDA); u16(12); u8(3); u8(1); u8(0x00); u8(2); u8(0x11); u8(3); u8(0x11); u8(0); u8(63); u8(0);
}

// ---- workspace of the device route (jpeg_enc_gpu.hip).  No coded byte passes through it: the rows are coded twice, once for their sizes
// and once into place.
struct Layout : sdarena::Walker {
    size_t n;                        // MCU rows of all frames
    Layout(int B, int h) : n((size_t)B * (size_t)mcu_rows(h)) {}
    size_t offsets = take(n * 8, 16);      // u64 [n], 16-byte aligned (with the workspace): a row's offset inside its frame's file
    size_t rowsize = take(n * 4, 4);       // u32 [n], 4: its bytes
    size_t total = end(16);
};

}  // namespace sdjenc
