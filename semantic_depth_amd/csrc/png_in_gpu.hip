// PNG scanline reconstruction on the device (the split PNG route, FrameFeeder(png="device")): filtered rows as zlib leaves them ->
// u8 [B,h,w,3] BGR, the bytes of sd_png_decode_bgr.  The arithmetic is png_unfilter.hpp; this file is the schedule.
//
// A byte needs its left neighbour a, the byte above b and the byte above-left c, so row y can run one pixel behind row y - 1.  Lane l
// of a wave owns row y0 + l of a 64-row BAND; at step t it reconstructs pixel x = t - l.  It keeps its own last pixel (a, <= 4 channels
// packed in one register) and last step's b (c), and takes b from the lane above with one cross-lane move (DPP wave_shr:1) per step:
// what lane l - 1 produced at step t - 1 is pixel t - l of the row above.  A band takes w + 63 steps.
//
// The bands of a frame are pipelined across the NW waves of ONE workgroup (one workgroup per frame).  Wave j runs band j
// kLag * kPhase = 96 steps behind wave j - 1; lane 63 of wave j - 1 leaves its pixels in an LDS ring of kRing = 128 pixels and lane 0
// of wave j reads them.  The waves keep in step with workgroup barriers only, one every kPhase = 32 steps: pixel x of a band's last row
// is written at that wave's step x + 63 and read (one step ahead of its use) at the next wave's step x - 1, i.e. at the writer's step
// x + 95 -- always in a later phase, since (kLag - 1) * kPhase >= 64; the slot is written again 128 steps later, after the phase
// of its read.  A frame with more than 64 * NW rows takes several passes; the last row of a pass is carried in a whole-row LDS buffer
// (one word per pixel, 64 KiB at the extent cap).  Nothing is handed between workgroups, there are no flags, spin-waits or atomics,
// and every LDS word that is read was written earlier in the same launch: the bytes cannot depend on scheduling.  NW = 1 is the
// degenerate case -- the bands walked serially, each one's last row carried in the row buffer.
//
// Memory: a lane reads its row as aligned 16-byte pieces, two present and the third in flight (loaded >= 4 steps before its first
// byte is used); it writes its BGR bytes as aligned 16-byte pieces, with single words in the first and last piece of a row and single
// bytes only at the unaligned head and tail.
// Lanes of a wave touch different rows, so neither side coalesces; the recurrence, not the bandwidth, bounds this kernel.
#include "png_in_gpu.hpp"

#include <stdint.h>

namespace sd {

namespace {

using namespace sdpngin;

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// value of `v` in the lane above; lane 0 keeps `first`
__device__ __forceinline__ uint32_t from_lane_above(uint32_t first, uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)first, (int)v, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
}

// the aligned 16-byte piece at q; a piece at or past the frame's stride (only ever requested ahead of a row's end, never used) is
// read from the frame's last piece instead.  The guard is on the ADDRESS, so nothing waits for the loaded value before its first use.
__device__ __forceinline__ u32x4 load_piece(const uint8_t* q, const uint8_t* end) {
    return *reinterpret_cast<const u32x4*>(q < end ? q : end - 16);
}

template <int NW, int CH>
__device__ __forceinline__ int reconstruct_frame(const uint8_t* __restrict__ rows, size_t frame_stride, int ctype, int pal_n, int h, int w,
                                                 uint8_t* __restrict__ out, uint32_t* pal, uint32_t* ring, uint32_t* carry) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const size_t row_len = 1 + (size_t)w * CH;
    const uint8_t* const rows_end = rows + frame_stride;
    // wave wv reads the row above its band from `src` and leaves its last row in `dst` (ring slots are x & 127, the row buffer is x)
    const uint32_t* const src = wv == 0 ? carry : ring + (wv - 1) * kRing;
    const int src_mask = wv == 0 ? 0x7FFF : kRing - 1;
    uint32_t* const dst = wv == NW - 1 ? carry : ring + wv * kRing;
    const int dst_mask = wv == NW - 1 ? 0x7FFF : kRing - 1;
    int flagged = 0;

    for (int pass0 = 0; pass0 < h; pass0 += kBandRows * NW) {
        const int bands = min(NW, (h - pass0 + kBandRows - 1) / kBandRows);        // bands of this pass that hold rows
        const int steps = (bands - 1) * kLag * kPhase + w + kBandRows - 1;
        const int y0 = pass0 + wv * kBandRows, y = y0 + lane;
        const bool row_ok = y < h;
        // the lane's row: filter byte, input pieces, output cursor
        int ft = 0;
        u32x4 p0 = {0u, 0u, 0u, 0u}, p1 = p0, p2 = p0;
        const uint8_t* next_piece = rows;
        int ip = 0;                                  // byte offset of the next pixel in p0
        uint8_t* optr = out;
        uint64_t oacc = 0;
        int on = 0;                                  // bytes waiting in oacc
        u32x4 q = {0u, 0u, 0u, 0u};                  // the aligned 16-byte output piece being filled
        int qmask = 0;                               // its words that are set
        if (row_ok) {
            const uint8_t* r = rows + (size_t)y * row_len;
            ft = r[0];
            const uintptr_t a0 = reinterpret_cast<uintptr_t>(r + 1);
            const uint8_t* q = reinterpret_cast<const uint8_t*>(a0 & ~(uintptr_t)15);
            ip = (int)(a0 & 15);
            p0 = load_piece(q, rows_end);
            p1 = load_piece(q + 16, rows_end);
            p2 = load_piece(q + 32, rows_end);
            next_piece = q + 48;
            optr = out + (size_t)y * w * 3;
        }
        uint32_t prev = 0, bprev = 0, above = 0;     // my last pixel; last step's b; lane 0: the pixel above this step's
        const bool has_above = y0 > 0;

        for (int g0 = 0; g0 < steps; g0 += kPhase) {
            const int t0 = g0 - wv * kLag * kPhase;                                  // (wave-uniform)
            if (wv < bands && t0 >= 0 && t0 < w + kBandRows - 1) {
                if (t0 == 0 && lane == 0 && has_above) above = src[0];
#pragma unroll 1
                for (int i = 0; i < kPhase; ++i) {
                    const int t = t0 + i, x = t - lane;
                    const uint32_t up = from_lane_above(above, prev);
                    if (lane == 0 && has_above && t + 1 < w) above = src[(t + 1) & src_mask];      // one step ahead of its use
                    if (row_ok && x >= 0 && x < w) {
                        const int d = ip >> 2;
                        const uint32_t lo = d == 0 ? p0.x : d == 1 ? p0.y : d == 2 ? p0.z : p0.w;
                        const uint32_t hi = d == 0 ? p0.y : d == 1 ? p0.z : d == 2 ? p0.w : p1.x;
                        const uint32_t s = (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * (ip & 3)));
                        const uint32_t b = y > 0 ? up : 0u;
                        const uint32_t a = x > 0 ? prev : 0u, c = x > 0 ? bprev : 0u;
                        const uint32_t o = unfilter_pixel<CH>(ft, s, a, b, c);
                        prev = o;
                        bprev = b;
                        if (lane == kBandRows - 1) dst[x & dst_mask] = o;
                        ip += CH;
                        if (ip >= 16) {                                              // p2 was requested >= 4 steps ago
                            ip -= 16;
                            p0 = p1;
                            p1 = p2;
                            p2 = load_piece(next_piece, rows_end);
                            next_piece += 16;
                        }
                        uint32_t bgr;
                        if (ctype == 3) {
                            uint32_t k = o & 255u;
                            if ((int)k >= pal_n) { flagged = 1; k = 0; }             // the guarded lookup: entry 0, nothing out of bounds
                            bgr = pal[k];
                        } else {
                            bgr = to_bgr(ctype, o);
                        }
                        oacc |= (uint64_t)bgr << (8 * on);
                        on += 3;
                        if (reinterpret_cast<uintptr_t>(optr) & 3) {                 // the unaligned head of a row: single bytes
                            while (on > 0 && (reinterpret_cast<uintptr_t>(optr) & 3)) {
                                *optr++ = (uint8_t)oacc;
                                oacc >>= 8;
                                --on;
                            }
                        }
                        if (on >= 4) {                                               // an aligned word joins the 16-byte piece
                            const uint32_t v = (uint32_t)oacc;
                            const int k = (int)((reinterpret_cast<uintptr_t>(optr) >> 2) & 3);
                            q.x = k == 0 ? v : q.x;
                            q.y = k == 1 ? v : q.y;
                            q.z = k == 2 ? v : q.z;
                            q.w = k == 3 ? v : q.w;
                            qmask |= 1 << k;
                            optr += 4;
                            oacc >>= 32;
                            on -= 4;
                        }
                        const bool last = x == w - 1;
                        if (qmask >= 8 || (last && qmask)) {                         // the piece is complete, or the row ends inside it
                            uint8_t* piece = reinterpret_cast<uint8_t*>(reinterpret_cast<uintptr_t>(optr - 4) & ~(uintptr_t)15);
                            if (qmask == 15) {
                                *reinterpret_cast<u32x4*>(piece) = q;
                            } else {                                                 // a row's first or last piece: its words one by one
                                if (qmask & 1) *reinterpret_cast<uint32_t*>(piece) = q.x;
                                if (qmask & 2) *reinterpret_cast<uint32_t*>(piece + 4) = q.y;
                                if (qmask & 4) *reinterpret_cast<uint32_t*>(piece + 8) = q.z;
                                if (qmask & 8) *reinterpret_cast<uint32_t*>(piece + 12) = q.w;
                            }
                            qmask = 0;
                        }
                        if (last) {                                                  // the tail: at most 3 bytes
                            while (on > 0) {
                                *optr++ = (uint8_t)oacc;
                                oacc >>= 8;
                                --on;
                            }
                        }
                    }
                }
            }
            __syncthreads();
        }
    }
    return flagged;
}

template <int NW>
__global__ __launch_bounds__(64 * NW) void png_reconstruct_kernel(const uint8_t* __restrict__ rows, size_t frame_stride,
                                                                  const sd_png_frame_desc* __restrict__ descs, int h, int w,
                                                                  uint8_t* __restrict__ out, size_t out_stride, int32_t* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    uint32_t* pal = lds;                         // [256] B | G << 8 | R << 16, zero past the palette
    uint32_t* ring = lds + 256;                  // [NW][kRing]
    uint32_t* carry = ring + NW * kRing;         // [w]
    const int b = blockIdx.x;
    const sd_png_frame_desc* d = descs + b;
    const int ch = d->channels, ctype = d->color_type, pal_n = d->palette_entries;
    for (int i = threadIdx.x; i < 256; i += 64 * NW)
        pal[i] = i < pal_n ? ((uint32_t)d->palette[i][2] | ((uint32_t)d->palette[i][1] << 8) | ((uint32_t)d->palette[i][0] << 16)) : 0u;
    __syncthreads();
    const uint8_t* fr = rows + (size_t)b * frame_stride;
    uint8_t* fo = out + (size_t)b * out_stride;
    int flagged;
    if (ch == 1) flagged = reconstruct_frame<NW, 1>(fr, frame_stride, ctype, pal_n, h, w, fo, pal, ring, carry);
    else if (ch == 2) flagged = reconstruct_frame<NW, 2>(fr, frame_stride, ctype, pal_n, h, w, fo, pal, ring, carry);
    else if (ch == 3) flagged = reconstruct_frame<NW, 3>(fr, frame_stride, ctype, pal_n, h, w, fo, pal, ring, carry);
    else flagged = reconstruct_frame<NW, 4>(fr, frame_stride, ctype, pal_n, h, w, fo, pal, ring, carry);
    const int any = __syncthreads_or(flagged);
    if (threadIdx.x == 0) status[b] = any ? 1 : 0;       // every word is written by the call: no clearing pass
}

template <int NW>
hipError_t launch(const uint8_t* rows, size_t frame_stride, const sd_png_frame_desc* descs, int B, int h, int w, uint8_t* out, size_t out_stride,
                  int32_t* status, hipStream_t s) {
    const size_t lds = (256 + (size_t)NW * kRing + (((size_t)w + 3) & ~(size_t)3)) * sizeof(uint32_t);
    static bool attr = false;
    if (!attr) {
        const size_t cap = (256 + (size_t)NW * kRing + kMaxExtent) * sizeof(uint32_t);
        hipError_t e = hipFuncSetAttribute((const void*)png_reconstruct_kernel<NW>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)cap);
        if (e != hipSuccess) return e;
        attr = true;
    }
    hipLaunchKernelGGL((png_reconstruct_kernel<NW>), dim3(B), dim3(64 * NW), lds, s, rows, frame_stride, descs, h, w, out, out_stride, status);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_png_reconstruct(const uint8_t* rows, size_t frame_stride, const sd_png_frame_desc* descs_host, int B, int height, int width,
                                  uint8_t* out, size_t out_stride, int32_t* status, uint8_t* workspace, int waves, hipStream_t s) {
    sd_png_frame_desc* descs = reinterpret_cast<sd_png_frame_desc*>(workspace + sdpngin::Layout(B).descs);
    hipError_t e = hipMemcpyAsync(descs, descs_host, (size_t)B * sizeof(sd_png_frame_desc), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return e;
    return waves == 1 ? launch<1>(rows, frame_stride, descs, B, height, width, out, out_stride, status, s)
                      : launch<kWaves>(rows, frame_stride, descs, B, height, width, out, out_stride, status, s);
}

}  // namespace sd
