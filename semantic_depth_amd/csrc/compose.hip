// Output stage of the sequence tool (semantic_depth_cityscapes_sequence.py:303-336, :463-485): the per-frame result image.
// For B network-size BGR frames, their road / fence masks and their road-width records, one pass writes
//   1. the segmentation overlay -- PIL's Image.paste(colour, mask=alpha) of the road colour, then of the fence colour, on masked
//      pixels: t = dst*(255-a) + src*a + 128, out = ((t >> 8) + t) >> 8 (libImaging/Paste.c BLEND), unmasked pixels unchanged --
//   2. cubic-resized to the original frame size exactly like sd_resize_cubic_u8 (same host tap tables, A = -0.75, int32 sums,
//      (sum + 2^21) >> 22) -- the overlay is evaluated per source tap, so the network-size overlay never goes to memory --
//   3. with the grey banner cv2.rectangle((0,0), (w, int(0.25*h)), (156,157,159), -1) on frames whose record has found != 0
//      (the flag is read here, on the device: no host synchronisation between the road chain and this launch).
// A thread writes 4 consecutive output pixels (12 bytes, one dwordx3 store when the 4 are in range and the buffer is 4-byte
// aligned); the 16 x 4 source taps per pixel are byte loads served by L1 / L2 (a 512 x 1024 source frame is 1.5 MB + 1 MB of masks).
#include "kernels.hpp"

namespace sd {

namespace {

__device__ __forceinline__ int pil_blend(int dst, int src, int a) {
    const int t = dst * (255 - a) + src * a + 128;
    return ((t >> 8) + t) >> 8;
}

}  // namespace

__global__ __launch_bounds__(256) void compose_result_frames_kernel(ComposeArgs p) {
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    const long npx = (long)p.B * p.dh * p.dw;
    const long p0 = g * 4;
    if (p0 >= npx) return;
    uint8_t px[12];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const long i = p0 + q;
        if (i >= npx) { px[3 * q] = px[3 * q + 1] = px[3 * q + 2] = 0; continue; }
        const int x = (int)(i % p.dw);
        const long r = i / p.dw;
        const int y = (int)(r % p.dh);
        const int b = (int)(r / p.dh);
        if (y <= p.banner_y1 && p.records[b].found != 0) {
            px[3 * q] = p.banner[0]; px[3 * q + 1] = p.banner[1]; px[3 * q + 2] = p.banner[2];
            continue;
        }
        const size_t fo = (size_t)b * p.sh * p.sw;
        const uint8_t* s = p.frames + fo * 3;
        const uint8_t* mr = p.road + fo;
        const uint8_t* mf = p.fence + fo;
        int acc0 = 0, acc1 = 0, acc2 = 0;
#pragma unroll
        for (int ky = 0; ky < 4; ++ky) {
            const size_t row = (size_t)p.yi[y * 4 + ky] * p.sw;
            int h0 = 0, h1 = 0, h2 = 0;
#pragma unroll
            for (int kx = 0; kx < 4; ++kx) {
                const size_t o = row + p.xi[x * 4 + kx];
                int c0 = s[o * 3], c1 = s[o * 3 + 1], c2 = s[o * 3 + 2];
                if (mr[o]) { c0 = pil_blend(c0, p.road_c[0], p.alpha); c1 = pil_blend(c1, p.road_c[1], p.alpha); c2 = pil_blend(c2, p.road_c[2], p.alpha); }
                if (mf[o]) { c0 = pil_blend(c0, p.fence_c[0], p.alpha); c1 = pil_blend(c1, p.fence_c[1], p.alpha); c2 = pil_blend(c2, p.fence_c[2], p.alpha); }
                const int a = p.xa[x * 4 + kx];
                h0 += c0 * a; h1 += c1 * a; h2 += c2 * a;
            }
            const int w = p.ya[y * 4 + ky];
            acc0 += h0 * w; acc1 += h1 * w; acc2 += h2 * w;
        }
        const int v0 = (acc0 + (1 << 21)) >> 22, v1 = (acc1 + (1 << 21)) >> 22, v2 = (acc2 + (1 << 21)) >> 22;
        px[3 * q] = (uint8_t)(v0 < 0 ? 0 : (v0 > 255 ? 255 : v0));
        px[3 * q + 1] = (uint8_t)(v1 < 0 ? 0 : (v1 > 255 ? 255 : v1));
        px[3 * q + 2] = (uint8_t)(v2 < 0 ? 0 : (v2 > 255 ? 255 : v2));
    }
    uint8_t* d = p.dst + p0 * 3;
    if (p.aligned && p0 + 4 <= npx) {
        uint32_t w[3];
#pragma unroll
        for (int k = 0; k < 3; ++k)
            w[k] = (uint32_t)px[4 * k] | ((uint32_t)px[4 * k + 1] << 8) | ((uint32_t)px[4 * k + 2] << 16) | ((uint32_t)px[4 * k + 3] << 24);
        uint32_t* d32 = reinterpret_cast<uint32_t*>(d);
        d32[0] = w[0]; d32[1] = w[1]; d32[2] = w[2];
    } else {
        const int n = (int)((npx - p0) < 4 ? (npx - p0) : 4);
        for (int k = 0; k < 3 * n; ++k) d[k] = px[k];
    }
}

hipError_t launch_compose_result_frames(const ComposeArgs& a, hipStream_t s) {
    const long groups = ((long)a.B * a.dh * a.dw + 3) / 4;
    hipLaunchKernelGGL(compose_result_frames_kernel, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace sd
