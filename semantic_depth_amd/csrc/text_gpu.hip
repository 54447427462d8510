// Device half of the result images' banner text (sd_text_draw_rw): the sd_rw_result records of B frames in device memory -> the strokes of
// the sequence tool's text, painted in place into the composed images (contract: include/semdepth.h; font, number format, layout and raster
// rule: text_draw.hpp, which sd_text_draw_host runs too, so both paint the same pixels).  Two launches, no host synchronisation, no atomics:
//   text_layout_kernel   one workgroup per frame: lane 0 reads the record, formats the numbers and writes the frame's items to the workspace;
//                        lane i then writes item i's pen prefix sums and its clipped pixel box
//   text_raster_kernel   grid = (64 x 16 pixel tiles of the largest box an item of this layout can have, items, frames); a workgroup whose
//                        tile lies outside its item's actual box, or whose columns no character reaches, exits at once.  The others find
//                        the characters whose advance box, widened by the stroke radius, meets their columns (one ballot), expand those
//                        glyphs' segments to 1/256-pixel integers in LDS, eight characters at a time, and every lane tests its four pixels
//                        against them -- a segment's widened bounding box first, the exact rule inside it -- until all four are painted.
//                        Only painted pixels are stored.
// The items of a frame share one colour (text_draw.hpp: sequence_items), so the item dimension of the grid cannot change what list order gives.
#include "text_gpu.hpp"

#include <algorithm>

namespace sd {
namespace {

using namespace sdtext;

constexpr int kThreads = 256;
constexpr int kBatchChars = kThreads / kMaxSegs;      // characters whose segments one LDS fill holds

struct TextArgs {
    uint8_t* dst;
    const sd_rw_result* records;
    TextFrameWs* ws;
    int B, h, w, dlen, tiles_x;
    uint64_t depth[3];      // the caller's depth string, byte i in bits 8 (i % 8) of word i / 8 (read with constant indices only: no private copy)
};

__global__ __launch_bounds__(64) void text_layout_kernel(TextArgs a) {
    __shared__ uint8_t depth[kMaxDepthBytes + 1];
    TextFrameWs& f = a.ws[blockIdx.x];
    if (threadIdx.x <= kMaxDepthBytes) {
        const uint64_t word = threadIdx.x < 8 ? a.depth[0] : threadIdx.x < 16 ? a.depth[1] : a.depth[2];
        depth[threadIdx.x] = (uint8_t)(word >> (8 * (threadIdx.x & 7)));
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        f.n = sequence_items(a.records[blockIdx.x], depth, a.dlen, a.h, a.w, f.it);
        f.pad[0] = f.pad[1] = f.pad[2] = 0;
    }
    __syncthreads();
    const int i = (int)threadIdx.x;
    if (i >= f.n) return;
    const sd_text_item& it = f.it[i];
    TextExtra& ex = f.ex[i];
    int pen = 0;
    for (int c = 0; c < it.len; ++c) {
        ex.pen[c] = (uint16_t)pen;
        pen += glyph_of(it.text[c]).adv;
    }
    ex.pen[it.len] = (uint16_t)pen;
    item_box(it, pen, a.h, a.w, ex.box);
}

__global__ __launch_bounds__(kThreads) void text_raster_kernel(TextArgs a) {
    __shared__ Seg segs[kThreads];
    __shared__ int reach[2];
    const TextFrameWs& f = a.ws[blockIdx.z];
    const int item = (int)blockIdx.y;
    if (item >= f.n) return;
    const sd_text_item& it = f.it[item];
    const TextExtra& ex = f.ex[item];
    const int tx = (int)blockIdx.x % a.tiles_x, ty = (int)blockIdx.x / a.tiles_x;
    const int X0 = ex.box[0] + tx * kTextTileW, Y0 = ex.box[1] + ty * kTextTileH;
    if (X0 > ex.box[2] || Y0 > ex.box[3]) return;
    const int X1 = min(X0 + kTextTileW - 1, ex.box[2]), Y1 = min(Y0 + kTextTileH - 1, ex.box[3]);
    const int len = it.len, r = it.thickness * 128, scale = it.scale_q8, ox = it.org_x * 256;
    const int t = (int)threadIdx.x;

    // the characters in reach of columns X0..X1: pen positions grow with the index, so they are one run first..last
    if (t < 64) {
        const bool in = t < len && ox + (int)ex.pen[t + 1] * scale + r >= X0 * 256 && ox + (int)ex.pen[t] * scale - r <= X1 * 256;
        const unsigned long long m = __ballot(in);
        if (t == 0) {
            reach[0] = m ? __ffsll(m) - 1 : 0;
            reach[1] = m ? 63 - __clzll(m) : -1;
        }
    }
    __syncthreads();
    const int first = reach[0], last = reach[1];
    if (last < first) return;

    const int px = X0 + (t & 63), py0 = Y0 + (t >> 6);
    const bool live = px <= X1;
    const int pxq = px * 256;
    unsigned painted = 0, all = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (live && py0 + 4 * k <= Y1) all |= 1u << k;

    for (int c0 = first; c0 <= last; c0 += kBatchChars) {
        // segment j of character c0 + slot goes behind the segments of the characters before it in this fill
        const int slot = t / kMaxSegs, j = t % kMaxSegs;
        int base = 0, total = 0;
#pragma unroll
        for (int i = 0; i < kBatchChars; ++i) {
            const int n = c0 + i <= last ? (int)glyph_of(it.text[c0 + i]).n : 0;
            base += i < slot ? n : 0;
            total += n;
        }
        if (c0 + slot <= last) {
            const Glyph g = glyph_of(it.text[c0 + slot]);
            if (j < g.n) segs[base + j] = seg_at(it, ex.pen[c0 + slot], g.first + j);
        }
        __syncthreads();
        if (painted != all) {
            for (int s = 0; s < total; ++s) {
                const Seg sg = segs[s];
                if (pxq < min(sg.ax, sg.bx) - r || pxq > max(sg.ax, sg.bx) + r) continue;      // outside the widened box: farther than r
                const int ylo = min(sg.ay, sg.by) - r, yhi = max(sg.ay, sg.by) + r;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int py = py0 + 4 * k;
                    if ((all & ~painted) >> k & 1u)
                        if (py * 256 >= ylo && py * 256 <= yhi && hit(sg, px, py, r)) painted |= 1u << k;
                }
                if (painted == all) break;
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (painted >> k & 1u) {      // (painted is a subset of all: px <= X1 < w, py <= Y1 < h)
            uint8_t* d = a.dst + (((size_t)blockIdx.z * a.h + (py0 + 4 * k)) * a.w + px) * 3;
            d[0] = it.bgr[0];
            d[1] = it.bgr[1];
            d[2] = it.bgr[2];
        }
}

}  // namespace

hipError_t launch_text_draw_rw(uint8_t* dst, int B, int h, int w, const sd_rw_result* records, const uint8_t* depth, int dlen, uint8_t* workspace,
                               hipStream_t s) {
    TextArgs a{};
    a.dst = dst;
    a.records = records;
    a.ws = reinterpret_cast<TextFrameWs*>(workspace + sdtext::Layout(B).frames);
    a.B = B;
    a.h = h;
    a.w = w;
    a.dlen = dlen;
    for (int i = 0; i < dlen; ++i) a.depth[i / 8] |= (uint64_t)depth[i] << (8 * (i % 8));
    // the largest box of an item of this layout: 64 characters of advance 24 at the larger scale, the stroke radius on both sides, one
    // pixel for the rounding of either edge; never more than the frame
    const int r = kSeqThickness * 128;
    const int bw = std::min(w, (kMaxBytes * kMaxAdvance * kSeqScaleBigQ8 + 2 * r) / 256 + 2);
    const int bh = std::min(h, ((kAscent + kDescent) * kSeqScaleBigQ8 + 2 * r) / 256 + 2);
    a.tiles_x = (bw + kTextTileW - 1) / kTextTileW;
    const int tiles_y = (bh + kTextTileH - 1) / kTextTileH;
    hipLaunchKernelGGL(text_layout_kernel, dim3((unsigned)B), dim3(64), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(text_raster_kernel, dim3((unsigned)(a.tiles_x * tiles_y), kMaxItems, (unsigned)B), dim3(kThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace sd
