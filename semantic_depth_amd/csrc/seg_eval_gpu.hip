// The segmentation score's per-pixel work on gfx950 (sd_resize_pil_bilinear_u8 / sd_seg_confusion; HBM bound, integer only, no MFMA):
// Pillow's bilinear resample of B uint8 frames and the 3 x 3 confusion counts of prediction against resampled labels.  The arithmetic is
// pil_resample.hpp's (shared with the host twins of host_seg_eval.cpp); this file only walks the pixels.
//
// Resample: two launches through a uint8 intermediate [B][src_h][pitch] in the workspace (pitch = dst_w * C rounded up to a dword).
//   pil_h_kernel: a workgroup takes 64 neighbouring output columns of up to 32 source rows.  The source span those 64 windows cover
//     (they overlap: a 3.125 x downscale reads 207 pixels for 64 outputs) comes from global memory ONCE, as aligned dwords into LDS; the
//     lanes then read their taps as LDS bytes.  Pixel stride, channel count and channel order are applied here, so the label image is
//     read straight from channel 0 of a [H, W, 3] frame and a BGR frame leaves as RGB.
//   pil_v_kernel: a lane takes four neighbouring bytes of an output row: one dword load per tap row, one dword store.
// Confusion: a lane classifies four pixels per step (one dword of predictions, one of labels; single bytes when a frame is not dword
// sized / aligned), the wave counts every cell with a ballot and a population count, the workgroup adds its waves' counts in LDS and sends
// the non-zero ones of the ten cells to global memory with 64-bit atomic adds.  Integer adds: the order does not matter.
#include "seg_eval_gpu.hpp"

#include <algorithm>

namespace sd {

using namespace sdpil;

namespace {
constexpr int kThreads = 256;
constexpr int kTileX = 64;                 // output columns per workgroup: the lanes of a wave share a source row
constexpr int kMaxRows = 32;               // source rows per workgroup
constexpr size_t kLdsBudget = 48 * 1024;   // dynamic LDS of pil_h_kernel (the span of the largest factor: 8.4 KB per row)
constexpr int kWave = 64;                  // gfx950
constexpr int kMaxBlocksPerFrame = 64;     // seg_confusion_kernel: workgroups per frame (each ends in at most ten atomics)
}  // namespace

// grid (column tiles, row groups, B).  src: B frames of src_h x src_w pixels, `ps` bytes apart; total = B * src_h * src_w * ps bytes.
// out rows are `out_pitch` bytes apart, frames `out_frame`.
template <int C>
__global__ __launch_bounds__(kThreads) void pil_h_kernel(const uint8_t* __restrict__ src, long long total, int src_h, int src_w, int ps, int reverse,
                                                         int rows_per_block, int span_dwords, const int32_t* __restrict__ xb,
                                                         const int32_t* __restrict__ xk, int dst_w, uint8_t* __restrict__ out, size_t out_pitch,
                                                         size_t out_frame) {
    extern __shared__ uint32_t s_span[];   // [rows_per_block][span_dwords]
    const int tid = threadIdx.x, b = blockIdx.z;
    const int d0 = blockIdx.x * kTileX, d1 = min(d0 + kTileX, dst_w);
    const int y0 = blockIdx.y * rows_per_block, rows = min(rows_per_block, src_h - y0);
    // xmin and xmin + n do not decrease with d: the tile's span is [first window's start, last window's end)
    const int p0 = xb[2 * d0], p1 = xb[2 * (d1 - 1)] + xb[2 * (d1 - 1) + 1];
    const int span_bytes = (p1 - p0) * ps;
    for (int r = 0; r < rows; ++r) {
        const long long off0 = ((long long)b * src_h + (y0 + r)) * src_w * ps + (long long)p0 * ps;
        const int shift = (int)((reinterpret_cast<uintptr_t>(src) + (uintptr_t)off0) & 3);
        const int ndw = (shift + span_bytes + 3) >> 2;          // <= span_dwords (the host sized it from the same windows)
        for (int t = tid; t < ndw; t += kThreads) {
            const long long o = off0 - shift + 4ll * t;         // the aligned dword's offset from src; its ends may lie outside the frames
            uint32_t v = 0;
            if (o >= 0 && o + 4 <= total) {
                v = *reinterpret_cast<const uint32_t*>(src + o);
            } else {
                for (int j = 0; j < 4; ++j)
                    if (o + j >= 0 && o + j < total) v |= (uint32_t)src[o + j] << (8 * j);
            }
            s_span[r * span_dwords + t] = v;
        }
    }
    __syncthreads();
    const int items = rows * kTileX;
    for (int it = tid; it < items; it += kThreads) {
        const int r = it / kTileX, d = d0 + it % kTileX;
        if (d >= d1) continue;
        const long long off0 = ((long long)b * src_h + (y0 + r)) * src_w * ps + (long long)p0 * ps;
        const int shift = (int)((reinterpret_cast<uintptr_t>(src) + (uintptr_t)off0) & 3);
        const int xmin = xb[2 * d], n = xb[2 * d + 1];
        const uint8_t* row = reinterpret_cast<const uint8_t*>(s_span + r * span_dwords) + shift + (xmin - p0) * ps;
        int32_t acc[C];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = kHalf;
        for (int i = 0; i < n; ++i) {
            const int32_t k = xk[(size_t)i * dst_w + d];
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] += k * (int32_t)row[i * ps + (reverse ? C - 1 - c : c)];
        }
        uint8_t* o = out + (size_t)b * out_frame + (size_t)(y0 + r) * out_pitch + (size_t)d * C;
#pragma unroll
        for (int c = 0; c < C; ++c) o[c] = clip_u8(acc[c]);
    }
}

// grid (ceil(dst_h * quads / 256), B); quads = dwords of an output row (row_bytes = dst_w * C rounded up).  mid rows are dword pitched; the
// bytes of a row's last dword beyond row_bytes are never stored.
__global__ __launch_bounds__(kThreads) void pil_v_kernel(const uint8_t* __restrict__ mid, size_t mid_pitch, size_t mid_frame,
                                                         const int32_t* __restrict__ yb, const int32_t* __restrict__ yk, int dst_h, int row_bytes,
                                                         int quads, uint8_t* __restrict__ dst, int dword_stores) {
    const long long g = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (g >= (long long)dst_h * quads) return;
    const int y = (int)(g / quads), q = (int)(g % quads), b = blockIdx.y;
    const int ymin = yb[2 * y], n = yb[2 * y + 1];
    const uint8_t* col = mid + (size_t)b * mid_frame + (size_t)ymin * mid_pitch + (size_t)q * 4;
    int32_t acc[4] = {kHalf, kHalf, kHalf, kHalf};
    for (int i = 0; i < n; ++i) {
        const int32_t k = yk[(size_t)i * dst_h + y];
        const uint32_t v = *reinterpret_cast<const uint32_t*>(col + (size_t)i * mid_pitch);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] += k * (int32_t)((v >> (8 * j)) & 0xff);
    }
    uint8_t* o = dst + ((size_t)b * dst_h + y) * row_bytes + (size_t)q * 4;
    if (dword_stores) {          // row_bytes is a multiple of 4 and dst is dword aligned
        *reinterpret_cast<uint32_t*>(o) = (uint32_t)clip_u8(acc[0]) | (uint32_t)clip_u8(acc[1]) << 8 | (uint32_t)clip_u8(acc[2]) << 16 |
                                          (uint32_t)clip_u8(acc[3]) << 24;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (q * 4 + j < row_bytes) o[j] = clip_u8(acc[j]);
    }
}

hipError_t launch_pil_resample_u8(const uint8_t* src, int B, int src_h, int src_w, int pixel_stride, int channels, int reverse, uint8_t* dst,
                                  int dst_h, int dst_w, const Windows& wx, uint8_t* workspace, hipStream_t s) {
    const Layout l(B, src_h, src_w, dst_h, dst_w, channels);
    const int32_t* xb = reinterpret_cast<const int32_t*>(workspace + l.x_bounds);
    const int32_t* xk = reinterpret_cast<const int32_t*>(workspace + l.x_k);
    const int32_t* yb = reinterpret_cast<const int32_t*>(workspace + l.y_bounds);
    const int32_t* yk = reinterpret_cast<const int32_t*>(workspace + l.y_k);
    uint8_t* mid = workspace + l.mid;
    const bool vertical = dst_h != src_h;
    const int tiles = (dst_w + kTileX - 1) / kTileX;
    int span_bytes = 0;       // the widest tile's span
    for (int t = 0; t < tiles; ++t) {
        const int d0 = t * kTileX, d1 = std::min(d0 + kTileX, dst_w);
        span_bytes = std::max(span_bytes, (wx.bounds[(size_t)(d1 - 1) * 2] + wx.bounds[(size_t)(d1 - 1) * 2 + 1] - wx.bounds[(size_t)d0 * 2]) * pixel_stride);
    }
    const int span_dwords = (span_bytes + 3 + 3) / 4;          // up to 3 bytes in front of the span in its first aligned dword
    const int rows_per_block = (int)std::max<size_t>(1, std::min<size_t>(kMaxRows, kLdsBudget / ((size_t)span_dwords * 4)));
    if ((size_t)span_dwords * 4 > kLdsBudget) return hipErrorInvalidValue;
    const size_t lds = (size_t)rows_per_block * span_dwords * 4;
    const size_t row_bytes = (size_t)dst_w * channels;
    uint8_t* hout = vertical ? mid : dst;
    const size_t hpitch = vertical ? mid_pitch(dst_w, channels) : row_bytes;
    const size_t hframe = (size_t)src_h * hpitch;
    const long long total = (long long)B * src_h * src_w * pixel_stride;
    const dim3 grid(tiles, (src_h + rows_per_block - 1) / rows_per_block, B);
    if (channels == 3)
        hipLaunchKernelGGL(pil_h_kernel<3>, grid, dim3(kThreads), lds, s, src, total, src_h, src_w, pixel_stride, reverse, rows_per_block, span_dwords, xb,
                           xk, dst_w, hout, hpitch, hframe);
    else
        hipLaunchKernelGGL(pil_h_kernel<1>, grid, dim3(kThreads), lds, s, src, total, src_h, src_w, pixel_stride, reverse, rows_per_block, span_dwords, xb,
                           xk, dst_w, hout, hpitch, hframe);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !vertical) return e;
    const int quads = (int)((row_bytes + 3) / 4);
    const long long threads = (long long)dst_h * quads;
    const int dword_stores = (row_bytes % 4 == 0 && (reinterpret_cast<uintptr_t>(dst) & 3) == 0) ? 1 : 0;
    hipLaunchKernelGGL(pil_v_kernel, dim3((unsigned)((threads + kThreads - 1) / kThreads), B), dim3(kThreads), 0, s, mid, hpitch, hframe, yb, yk, dst_h,
                       (int)row_bytes, quads, dst, dword_stores);
    return hipGetLastError();
}

// grid (workgroups per frame, B).  V = 4: n is a multiple of 4 and both arrays are dword aligned; V = 1: any n.
template <int V>
__global__ __launch_bounds__(kThreads) void seg_confusion_kernel(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ labels, long long n,
                                                                 SegTable table, unsigned long long* __restrict__ counts) {
    __shared__ uint8_t s_tab[256];
    __shared__ uint32_t s_cnt[kThreads / kWave][kCells];
    const int tid = threadIdx.x, wave = tid / kWave, lane = tid % kWave, b = blockIdx.y;
    s_tab[tid] = table.v[tid];
    __syncthreads();
    const uint8_t* p = pred + (size_t)b * n;
    const uint8_t* l = labels + (size_t)b * n;
    const long long units = n / V;
    uint32_t cnt[kCells];      // the same in every lane of a wave (at most 2^28 pixels per frame: 32 bits hold a wave's share)
#pragma unroll
    for (int c = 0; c < kCells; ++c) cnt[c] = 0;
    // the loop bound is the wave's: every lane stays in the loop for the ballots, lanes beyond the frame vote for no cell
    for (long long u0 = ((long long)blockIdx.x * (kThreads / kWave) + wave) * kWave; u0 < units; u0 += (long long)gridDim.x * kThreads) {
        const long long u = u0 + lane;
        const bool valid = u < units;
        uint32_t pv = 0, lv = 0;
        if (valid) {
            if (V == 4) {
                pv = reinterpret_cast<const uint32_t*>(p)[u];
                lv = reinterpret_cast<const uint32_t*>(l)[u];
            } else {
                pv = p[u];
                lv = l[u];
            }
        }
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const int cell = valid ? seg_cell(s_tab[(lv >> (8 * j)) & 0xff], (int)((pv >> (8 * j)) & 0xff)) : -1;
#pragma unroll
            for (int c = 0; c < kCells; ++c) cnt[c] += (uint32_t)__popcll(__ballot(cell == c));
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < kCells; ++c) s_cnt[wave][c] = cnt[c];
    }
    __syncthreads();
    if (tid < kCells) {
        unsigned long long sum = 0;
        for (int w = 0; w < kThreads / kWave; ++w) sum += s_cnt[w][tid];
        if (sum) atomicAdd(&counts[(size_t)b * kCells + tid], sum);
    }
}

hipError_t launch_seg_confusion(const uint8_t* pred, const uint8_t* labels, int B, int height, int width, const SegTable& table, int64_t* counts,
                                hipStream_t s) {
    const long long n = (long long)height * width;
    const bool vec = n % 4 == 0 && ((reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(labels)) & 3) == 0;
    const long long units = vec ? n / 4 : n;
    const unsigned blocks = (unsigned)std::min<long long>(kMaxBlocksPerFrame, (units + kThreads - 1) / kThreads);
    unsigned long long* c = reinterpret_cast<unsigned long long*>(counts);
    if (vec)
        hipLaunchKernelGGL(seg_confusion_kernel<4>, dim3(blocks, B), dim3(kThreads), 0, s, pred, labels, n, table, c);
    else
        hipLaunchKernelGGL(seg_confusion_kernel<1>, dim3(blocks, B), dim3(kThreads), 0, s, pred, labels, n, table, c);
    return hipGetLastError();
}

}  // namespace sd
