// Device half of the split JPEG route (sd_jpeg_reconstruct_bgr): the host Huffman-decodes a frame to quantised coefficients
// (sd_jpeg_decode_coefficients) and everything behind that -- integer arithmetic on independent 8x8 blocks and pixels -- runs here,
// restating host_jpeg.cpp's back half integer for integer:
//   jpeg_idct_kernel    dequantise + jidctint ISLOW (jpeg_common.hpp's idct_islow, THE function the host runs: int64 sums, the same
//                       zero-column / zero-row shortcuts) -> u8 padded component planes in the caller's workspace
//   jpeg_colour_kernel  per OUTPUT pixel: EXIF position -> stored position, h2v1 / h2v2 fancy chroma filter (edge columns, cw == 1,
//                       replicated edge rows) or the 1x1 copy, jdcolor's 16-bit fixed-point YCbCr -> RGB (or Adobe RGB pass-through, or
//                       gray replication), BGR store
// The descriptors of up to JPEG_GROUP frames travel as kernel arguments (no host buffer outlives the call, no copy to wait for), so a
// batch of 32 frames is four launches of each kernel.
//
// Thread mapping.  IDCT: one lane per 8x8 block.  A lane reads its block's 128 contiguous bytes as eight 16-byte loads (neighbouring
// lanes are 128 bytes apart: every line fetched is used whole) and stores eight 8-byte row pieces that are contiguous across the lanes
// of a block row.  Colour: one lane per output pixel, consecutive lanes consecutive pixels, so the BGR stores of a wave cover one
// contiguous 192-byte span; for the unrotated orientations the plane reads are contiguous too, for the transposing ones (5..8) the
// READS stride through the planes (caches absorb that better than strided stores would).
// The stage moves about 9 bytes per pixel.  What bounds it has not been measured: 32 frames of 2048 x 1024 take 0.61 ms, about 0.8 TB/s of
// useful traffic and well below the HBM rate (the IDCT kernel holds a block in 146 VGPRs at 3 waves per SIMD, the colour kernel stores
// single bytes).  That is 8 - 156 ms of host Huffman decoding away from mattering, so the simple, provably equal form stays.
#include <hip/hip_runtime.h>

#include "jpeg_gpu.hpp"

namespace sd {
namespace {

constexpr int JPEG_GROUP = 8;

struct JpegFrameDev {
    int H, W, ncomp, hmax, vmax, orientation, transform, pad;
    int bw[3], bh[3];
    unsigned long long coef_off[3];      // int16 elements from the frame's first coefficient
    unsigned long long plane_off[3];     // bytes from the workspace base
    uint16_t qt[3][64];
};
struct JpegGroupArgs {
    JpegFrameDev f[JPEG_GROUP];
};
static_assert(sizeof(JpegGroupArgs) <= 4000, "the frame group must fit the kernel-argument segment");

__global__ __launch_bounds__(128) void jpeg_idct_kernel(const JpegGroupArgs g, const int16_t* __restrict__ coef, size_t frame_stride_elems,
                                                        uint8_t* __restrict__ ws) {
    const JpegFrameDev& f = g.f[blockIdx.z];
    const int c = blockIdx.y;
    if (c >= f.ncomp) return;
    const int bw = f.bw[c];
    const int b = blockIdx.x * 128 + threadIdx.x;
    if (b >= bw * f.bh[c]) return;
    const int by = b / bw, bx = b - by * bw;
    const uint4* src = reinterpret_cast<const uint4*>(coef + blockIdx.z * frame_stride_elems + f.coef_off[c] + (size_t)b * 64);
    int32_t in[64];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const uint4 v = src[r];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            in[8 * r + 2 * j] = (int32_t)(int16_t)(w[j] & 0xffffu) * (int32_t)f.qt[c][8 * r + 2 * j];
            in[8 * r + 2 * j + 1] = (int32_t)(int16_t)(w[j] >> 16) * (int32_t)f.qt[c][8 * r + 2 * j + 1];
        }
    }
    uint8_t px[64];
    sdjpeg::idct_islow(in, px, 8);
    const size_t pw = (size_t)bw * 8;
    uint8_t* dst = ws + f.plane_off[c] + (size_t)by * 8 * pw + (size_t)bx * 8;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        uint2 o;
        o.x = px[8 * r] | (px[8 * r + 1] << 8) | (px[8 * r + 2] << 16) | ((uint32_t)px[8 * r + 3] << 24);
        o.y = px[8 * r + 4] | (px[8 * r + 5] << 8) | (px[8 * r + 6] << 16) | ((uint32_t)px[8 * r + 7] << 24);
        *reinterpret_cast<uint2*>(dst + r * pw) = o;
    }
}

// jdsample.c's fancy upsampling of one chroma plane, evaluated at luma position (x, y): host_jpeg.cpp's Decoder::upsample per pixel.
// cw x chh is the real chroma extent; x < W <= hmax * cw and y < H <= vmax * chh.  With cw == 1 the two special columns x == 0 and
// x == 2 cw - 1 are all there is, and they are the host's cw == 1 formulas.
__device__ inline int chroma_at(const uint8_t* __restrict__ P, size_t pw, int cw, int chh, int hmax, int vmax, int x, int y) {
    if (hmax == 1) return P[(size_t)y * pw + x];
    const int i = x >> 1;
    if (vmax == 1) {                                    // h2v1_fancy_upsample
        const uint8_t* in = P + (size_t)y * pw;
        if (x == 0) return in[0];
        if (x == 2 * cw - 1) return in[cw - 1];
        return (x & 1) ? (in[i] * 3 + in[i + 1] + 2) >> 2 : (in[i] * 3 + in[i - 1] + 1) >> 2;
    }
    // h2v2_fancy_upsample: output row y is nearer to chroma row (y >> 1) - 1 when even, + 1 when odd; beyond the real extent the edge row
    const int cy = y >> 1;
    int yn = (y & 1) ? cy + 1 : cy - 1;
    yn = yn < 0 ? 0 : (yn > chh - 1 ? chh - 1 : yn);
    const uint8_t* in0 = P + (size_t)cy * pw;
    const uint8_t* in1 = P + (size_t)yn * pw;
    const int s = in0[i] * 3 + in1[i];
    if (x == 0) return (s * 4 + 8) >> 4;
    if (x == 2 * cw - 1) return (s * 4 + 7) >> 4;
    if (x & 1) return (s * 3 + (in0[i + 1] * 3 + in1[i + 1]) + 7) >> 4;
    return (s * 3 + (in0[i - 1] * 3 + in1[i - 1]) + 8) >> 4;
}

__device__ inline uint8_t clamp_u8(int v) { return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

__global__ __launch_bounds__(256) void jpeg_colour_kernel(const JpegGroupArgs g, const uint8_t* __restrict__ ws, uint8_t* __restrict__ bgr,
                                                          size_t bgr_frame_stride) {
    const JpegFrameDev& f = g.f[blockIdx.z];
    const int H = f.H, W = f.W, orientation = f.orientation;
    const int OW = orientation >= 5 ? H : W;
    const size_t npix = (size_t)H * W;
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= npix) return;
    const int oy = (int)(p / (unsigned)OW), ox = (int)(p - (size_t)oy * OW);
    int sx, sy;
    switch (orientation) {                              // OpenCV's ExifTransform, as host_jpeg.cpp's emit_bgr inverts it
        case 1: sx = ox; sy = oy; break;
        case 2: sx = W - 1 - ox; sy = oy; break;
        case 3: sx = W - 1 - ox; sy = H - 1 - oy; break;
        case 4: sx = ox; sy = H - 1 - oy; break;
        case 5: sx = oy; sy = ox; break;
        case 6: sx = oy; sy = H - 1 - ox; break;
        case 7: sx = W - 1 - oy; sy = H - 1 - ox; break;
        default: sx = W - 1 - oy; sy = ox; break;       // 8
    }
    const int Y = ws[f.plane_off[0] + (size_t)sy * ((size_t)f.bw[0] * 8) + sx];
    uint8_t* o = bgr + blockIdx.z * bgr_frame_stride + p * 3;
    if (f.ncomp == 1) {
        o[0] = o[1] = o[2] = (uint8_t)Y;
        return;
    }
    const int cw = (W + f.hmax - 1) / f.hmax, chh = (H + f.vmax - 1) / f.vmax;
    const int cb = chroma_at(ws + f.plane_off[1], (size_t)f.bw[1] * 8, cw, chh, f.hmax, f.vmax, sx, sy);
    const int cr = chroma_at(ws + f.plane_off[2], (size_t)f.bw[2] * 8, cw, chh, f.hmax, f.vmax, sx, sy);
    if (f.transform == 0) {                             // Adobe marker: the three components ARE R, G, B
        o[0] = (uint8_t)cr; o[1] = (uint8_t)cb; o[2] = (uint8_t)Y;
        return;
    }
    // jdcolor.c build_ycc_rgb_table, SCALEBITS 16: the table entries of the host, computed (arithmetic shifts of signed values, as there)
    const int xb = cb - 128, xr = cr - 128;
    o[2] = clamp_u8(Y + ((91881 * xr + 32768) >> 16));                          // FIX(1.40200)
    o[1] = clamp_u8(Y + ((-22554 * xb + 32768 + -46802 * xr) >> 16));           // FIX(0.34414), FIX(0.71414), ONE_HALF
    o[0] = clamp_u8(Y + ((116130 * xb + 32768) >> 16));                         // FIX(1.77200)
}

}  // namespace

hipError_t launch_jpeg_reconstruct(const int16_t* coef, size_t frame_stride_elems, const sd_jpeg_frame_desc* descs, int B, uint8_t* bgr,
                                   size_t bgr_frame_stride, uint8_t* workspace, hipStream_t s) {
    sdarena::Walker ws_walk;
    for (int b0 = 0; b0 < B; b0 += JPEG_GROUP) {
        const int nb = B - b0 < JPEG_GROUP ? B - b0 : JPEG_GROUP;
        JpegGroupArgs g{};
        size_t max_blocks = 0, max_pix = 0;
        for (int k = 0; k < nb; ++k) {
            const sd_jpeg_frame_desc& d = descs[b0 + k];
            JpegFrameDev& f = g.f[k];
            f.H = d.height; f.W = d.width; f.ncomp = d.ncomp; f.hmax = d.hmax; f.vmax = d.vmax;
            f.orientation = d.orientation; f.transform = d.adobe_transform;
            size_t plane[3];
            sdjpeg::take_planes(ws_walk, d, plane);
            for (int c = 0; c < d.ncomp; ++c) {
                f.bw[c] = d.blocks_w[c]; f.bh[c] = d.blocks_h[c];
                f.coef_off[c] = (unsigned long long)d.coef_offset[c];
                f.plane_off[c] = plane[c];
                for (int q = 0; q < 64; ++q) f.qt[c][q] = d.qt[c][q];
                const size_t blocks = (size_t)d.blocks_w[c] * d.blocks_h[c];
                max_blocks = blocks > max_blocks ? blocks : max_blocks;
            }
            const size_t pix = (size_t)d.height * d.width;
            max_pix = pix > max_pix ? pix : max_pix;
        }
        const dim3 g1((unsigned)((max_blocks + 127) / 128), 3, (unsigned)nb);
        hipLaunchKernelGGL(jpeg_idct_kernel, g1, dim3(128), 0, s, g, coef + (size_t)b0 * frame_stride_elems, frame_stride_elems, workspace);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        const dim3 g2((unsigned)((max_pix + 255) / 256), 1, (unsigned)nb);
        hipLaunchKernelGGL(jpeg_colour_kernel, g2, dim3(256), 0, s, g, workspace, bgr + (size_t)b0 * bgr_frame_stride, bgr_frame_stride);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace sd
