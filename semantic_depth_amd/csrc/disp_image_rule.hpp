// The disparity image of a frame, stated once for host and device (contract: include/semdepth.h).
//
// semantic_depth.py:681-683 is scipy.misc.imresize(disp, [h, w]) followed by plt.imsave(name, img, cmap='gray'): imresize byte-scales the
// float map over its own range (bytescale), resamples the bytes with Pillow's bilinear filter (pil_resample.hpp), and imsave normalises the
// resized bytes over THEIR range before it looks the colour up.  Per frame b of a float32 [B, H, W] map, mult[b] the disparity multiplier:
//   v      = d * mult[b]                                                   (float32)
//   lo, hi = minimum, maximum of the finite v of the frame; cs = hi - lo (float32); cs == 0 or no finite v: cs = 1 (no finite v: lo = 0)
//   scale  = (float)(255.0 / (double)cs)
//   byte   = (int)(clip((v - lo) * scale, 0, 255) + 0.5f), the difference and the product each rounded to float32 (never one fma: the two
//            files that include this for arithmetic are compiled with -ffp-contract=off); a non-finite v gives 0 and flags the frame.  A
//            product that is not a number (hi - lo beyond the float32 range: inf * 0) gives 0 as well.
//   resize = Pillow's bilinear resample of the byte image, one channel; equal sizes: the bytes themselves
//   idx    = hi8 == lo8 ? 0 : min(255, 256 * (p - lo8) / (hi8 - lo8))      (integers, floor; lo8, hi8 the range of the RESIZED frame)
//            -- matplotlib's float32 Normalize followed by int(x * 256) with 256 -> 255, for every (p, lo8, hi8)
//   pixel  = table[cmap][idx], stored B, G, R
// The minimum and maximum are taken on an order-preserving 32-bit key of the float, so that integer atomics can combine the workgroups of
// a frame in any order; the host twin goes through the same keys.
// The two tables are matplotlib's (colormaps[name](np.arange(256), bytes=True)), taken as data: gray is trunc(i / 255 * 255) in double,
// which is one below i at 24 places.
#pragma once
#include <cstddef>
#include <cstdint>

#include "pil_resample.hpp"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SDDISP_HD __host__ __device__ inline
#else
#define SDDISP_HD inline
#endif

namespace sddisp {

constexpr int kMaps = 2;                       // SD_CMAP_GRAY, SD_CMAP_PLASMA
constexpr uint32_t kKeyNone = 0xFFFFFFFFu;     // the minimum cell before any finite value (the key of no finite float); the maximum cell starts at 0

SDDISP_HD uint32_t f32_bits(float v) { return __builtin_bit_cast(uint32_t, v); }
SDDISP_HD float bits_f32(uint32_t u) { return __builtin_bit_cast(float, u); }
SDDISP_HD bool finite_f32(float v) { return (f32_bits(v) & 0x7F800000u) != 0x7F800000u; }

// unsigned order of the keys = numeric order of the floats (-0 sorts below +0; both give the same bytes)
SDDISP_HD uint32_t key_of(float v) {
    const uint32_t u = f32_bits(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
SDDISP_HD float value_of(uint32_t k) { return bits_f32((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

struct Range {
    float lo, scale;
};
// steps 2: the frame's range from its two cells (kmin > kmax: no finite value was seen)
SDDISP_HD Range make_range(uint32_t kmin, uint32_t kmax) {
    Range r;
    if (kmin > kmax) {
        r.lo = 0.0f;
        r.scale = 255.0f;
        return r;
    }
    r.lo = value_of(kmin);
    float cs = value_of(kmax) - r.lo;
    if (cs == 0.0f) cs = 1.0f;
    r.scale = (float)(255.0 / (double)cs);
    return r;
}

// step 1
SDDISP_HD float scaled(float d, float mult) { return d * mult; }

// step 3 for a finite v
SDDISP_HD uint8_t byte_of(float v, Range r) {
    const float diff = v - r.lo;
    float t = diff * r.scale;
    if (!(t > 0.0f)) t = 0.0f;          // (also a product that is not a number)
    if (t > 255.0f) t = 255.0f;
    return (uint8_t)(int)(t + 0.5f);
}

// step 5
SDDISP_HD int index_of(int p, int lo8, int hi8) {
    if (hi8 <= lo8 || p <= lo8) return 0;
    const int i = 256 * (p - lo8) / (hi8 - lo8);
    return i > 255 ? 255 : i;
}

constexpr uint8_t kGray[256] = {
    0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31,
    32, 32, 34, 35, 36, 36, 38, 39, 40, 40, 42, 43, 44, 44, 46, 47, 48, 48, 50, 51, 52, 52, 54, 55, 56, 56, 58, 59, 60, 60, 62, 63,
    64, 65, 65, 67, 68, 69, 70, 71, 72, 73, 73, 75, 76, 77, 78, 79, 80, 81, 81, 83, 84, 85, 86, 87, 88, 89, 89, 91, 92, 93, 94, 95,
    96, 97, 97, 99, 100, 101, 102, 103, 104, 105, 105, 107, 108, 109, 110, 111, 112, 113, 113, 115, 116, 117, 118, 119, 120, 121, 121, 123, 124, 125, 126, 127,
    128, 129, 130, 131, 131, 133, 134, 135, 136, 137, 138, 139, 140, 141, 142, 143, 144, 145, 146, 147, 147, 149, 150, 151, 152, 153, 154, 155, 156, 157, 158, 159,
    160, 161, 162, 163, 163, 165, 166, 167, 168, 169, 170, 171, 172, 173, 174, 175, 176, 177, 178, 179, 179, 181, 182, 183, 184, 185, 186, 187, 188, 189, 190, 191,
    192, 193, 194, 195, 195, 197, 198, 199, 200, 201, 202, 203, 204, 205, 206, 207, 208, 209, 210, 211, 211, 213, 214, 215, 216, 217, 218, 219, 220, 221, 222, 223,
    224, 225, 226, 227, 227, 229, 230, 231, 232, 233, 234, 235, 236, 237, 238, 239, 240, 241, 242, 243, 243, 245, 246, 247, 248, 249, 250, 251, 252, 253, 254, 255,
};

constexpr uint8_t kPlasma[768] = {      // R, G, B per entry
    12, 7, 134, 16, 7, 135, 19, 6, 137, 21, 6, 138, 24, 6, 139, 27, 6, 140, 29, 6, 141, 31, 5, 142, 33, 5, 143, 35, 5, 144, 37, 5, 145, 39, 5, 146, 41, 5, 147, 43, 5, 148, 45, 4, 148, 47, 4, 149,
    49, 4, 150, 51, 4, 151, 52, 4, 152, 54, 4, 152, 56, 4, 153, 58, 4, 154, 59, 3, 154, 61, 3, 155, 63, 3, 156, 64, 3, 156, 66, 3, 157, 68, 3, 158, 69, 3, 158, 71, 2, 159, 73, 2, 159, 74, 2, 160,
    76, 2, 161, 78, 2, 161, 79, 2, 162, 81, 1, 162, 82, 1, 163, 84, 1, 163, 86, 1, 163, 87, 1, 164, 89, 1, 164, 90, 0, 165, 92, 0, 165, 94, 0, 165, 95, 0, 166, 97, 0, 166, 98, 0, 166, 100, 0, 167,
    101, 0, 167, 103, 0, 167, 104, 0, 167, 106, 0, 167, 108, 0, 168, 109, 0, 168, 111, 0, 168, 112, 0, 168, 114, 0, 168, 115, 0, 168, 117, 0, 168, 118, 1, 168, 120, 1, 168, 121, 1, 168, 123, 2, 168, 124, 2, 167,
    126, 3, 167, 127, 3, 167, 129, 4, 167, 130, 4, 167, 132, 5, 166, 133, 6, 166, 134, 7, 166, 136, 7, 165, 137, 8, 165, 139, 9, 164, 140, 10, 164, 142, 12, 164, 143, 13, 163, 144, 14, 163, 146, 15, 162, 147, 16, 161,
    149, 17, 161, 150, 18, 160, 151, 19, 160, 153, 20, 159, 154, 21, 158, 155, 23, 158, 157, 24, 157, 158, 25, 156, 159, 26, 155, 160, 27, 155, 162, 28, 154, 163, 29, 153, 164, 30, 152, 165, 31, 151, 167, 33, 151, 168, 34, 150,
    169, 35, 149, 170, 36, 148, 172, 37, 147, 173, 38, 146, 174, 39, 145, 175, 40, 144, 176, 42, 143, 177, 43, 143, 178, 44, 142, 180, 45, 141, 181, 46, 140, 182, 47, 139, 183, 48, 138, 184, 50, 137, 185, 51, 136, 186, 52, 135,
    187, 53, 134, 188, 54, 133, 189, 55, 132, 190, 56, 131, 191, 57, 130, 192, 59, 129, 193, 60, 128, 194, 61, 128, 195, 62, 127, 196, 63, 126, 197, 64, 125, 198, 65, 124, 199, 66, 123, 200, 68, 122, 201, 69, 121, 202, 70, 120,
    203, 71, 119, 204, 72, 118, 205, 73, 117, 206, 74, 117, 207, 75, 116, 208, 77, 115, 209, 78, 114, 209, 79, 113, 210, 80, 112, 211, 81, 111, 212, 82, 110, 213, 83, 109, 214, 85, 109, 215, 86, 108, 215, 87, 107, 216, 88, 106,
    217, 89, 105, 218, 90, 104, 219, 91, 103, 220, 93, 102, 220, 94, 102, 221, 95, 101, 222, 96, 100, 223, 97, 99, 223, 98, 98, 224, 100, 97, 225, 101, 96, 226, 102, 96, 227, 103, 95, 227, 104, 94, 228, 106, 93, 229, 107, 92,
    229, 108, 91, 230, 109, 90, 231, 110, 90, 232, 112, 89, 232, 113, 88, 233, 114, 87, 234, 115, 86, 234, 116, 85, 235, 118, 84, 236, 119, 84, 236, 120, 83, 237, 121, 82, 237, 123, 81, 238, 124, 80, 239, 125, 79, 239, 126, 78,
    240, 128, 77, 240, 129, 77, 241, 130, 76, 242, 132, 75, 242, 133, 74, 243, 134, 73, 243, 135, 72, 244, 137, 71, 244, 138, 71, 245, 139, 70, 245, 141, 69, 246, 142, 68, 246, 143, 67, 246, 145, 66, 247, 146, 65, 247, 147, 65,
    248, 149, 64, 248, 150, 63, 248, 152, 62, 249, 153, 61, 249, 154, 60, 250, 156, 59, 250, 157, 58, 250, 159, 58, 250, 160, 57, 251, 162, 56, 251, 163, 55, 251, 164, 54, 252, 166, 53, 252, 167, 53, 252, 169, 52, 252, 170, 51,
    252, 172, 50, 252, 173, 49, 253, 175, 49, 253, 176, 48, 253, 178, 47, 253, 179, 46, 253, 181, 45, 253, 182, 45, 253, 184, 44, 253, 185, 43, 253, 187, 43, 253, 188, 42, 253, 190, 41, 253, 192, 41, 253, 193, 40, 253, 195, 40,
    253, 196, 39, 253, 198, 38, 252, 199, 38, 252, 201, 38, 252, 203, 37, 252, 204, 37, 252, 206, 37, 251, 208, 36, 251, 209, 36, 251, 211, 36, 250, 213, 36, 250, 214, 36, 250, 216, 36, 249, 217, 36, 249, 219, 36, 248, 221, 36,
    248, 223, 36, 247, 224, 36, 247, 226, 37, 246, 228, 37, 246, 229, 37, 245, 231, 38, 245, 233, 38, 244, 234, 38, 243, 236, 38, 243, 238, 38, 242, 240, 38, 242, 241, 38, 241, 243, 38, 240, 245, 37, 240, 246, 35, 239, 248, 33,
};

// step 6: entry idx of a map as the three bytes of a stored pixel packed B | G << 8 | R << 16
SDDISP_HD uint32_t bgr_of(int cmap, int idx) {
    if (cmap == 0) return (uint32_t)kGray[idx] * 0x010101u;
    return (uint32_t)kPlasma[3 * idx + 2] | (uint32_t)kPlasma[3 * idx + 1] << 8 | (uint32_t)kPlasma[3 * idx] << 16;
}

inline bool valid_map(int cmap) { return cmap >= 0 && cmap < kMaps; }
inline bool valid_sizes(int h, int w, int out_h, int out_w) { return sdpil::axis_ok(h, out_h) && sdpil::axis_ok(w, out_w); }
inline bool resized(int h, int w, int out_h, int out_w) { return h != out_h || w != out_w; }

// ---- workspace of the device route (disp_image_gpu.hip); every part 16-byte aligned
struct Layout : sdarena::Walker {
    size_t B, px, out_px, pil_bytes;      // (out_px, pil_bytes: 0 when the sizes do not differ; the two parts are then empty, at `total`)
    Layout(int B_, int h, int w, int out_h, int out_w)
        : B((size_t)B_), px((size_t)h * w), out_px(sddisp::resized(h, w, out_h, out_w) ? (size_t)out_h * out_w : 0),
          pil_bytes(out_px ? sdpil::workspace_bytes(B_, h, w, out_h, out_w, 1) : 0) {}
    size_t cells = take(B * 4 * sizeof(uint32_t), 16);      // u32 [B][4]: key min, key max, lo8, hi8
    size_t mult = take(B * sizeof(float), 16);              // f32 [B]
    size_t bytes = take(B * px, 16);                        // u8 [B][h][w]
    size_t resized = take(B * out_px, 16);                  // u8 [B][out_h][out_w]
    size_t pil = take(pil_bytes, 16);                       // the resample's own workspace, sdpil::Layout(..., channels = 1)
    size_t total = end(16);
};

}  // namespace sddisp
