// Device half of the result video (sd_jpeg_encode_bgr): u8 [B,h,w,3] BGR frames in device memory -> one complete baseline JFIF file per
// frame (4:2:0, the Annex K tables, one restart interval per MCU row; format: include/semdepth.h).  Three launches, no host synchronisation:
//   jpeg_row_kernel<false>   one workgroup per MCU row: codes the row and keeps only its byte count
//   jpeg_layout_kernel       one workgroup per frame: exclusive scan of the row sizes, the capacity flag, sizes[b], the header
//   jpeg_row_kernel<true>    the same code again, now storing the row at its place in the file (a flagged frame is skipped)
// A row is coded twice because its place depends on every row above it; in exchange no coded byte goes through a workspace (two words
// per row do) and a stream_stride below the bound costs nothing.  The workgroup walks its row in strips of 8 MCUs: colour and the chroma
// box into LDS, the row and column passes of the DCT with one lane per 8 samples, the quantiser, then one lane per block for the Huffman
// symbols (exact bit lengths, a scan, deposits into an LDS bit buffer), a second scan over the FF bytes for the stuffing, and a coalesced
// store.  Between strips travel the DC predictors, the bits of the unfinished byte and the row's byte count.
// Every coding decision is a function of jpeg_enc.hpp, which sd_jpeg_encode_bgr_host runs too: the files are the same bytes.
#include "jpeg_enc_gpu.hpp"

namespace sd {
namespace {

using namespace sdjenc;

constexpr int kThreads = 256;
constexpr int kStripMcus = 8;
constexpr int kStripBlocks = 6 * kStripMcus;                              // 48
constexpr int kRowPad = 9, kBlockPad = 8 * kRowPad;                       // a block's 8 x 8 ints with 9-word rows: both passes conflict-free
constexpr int kStripBitsMax = 7 + kStripBlocks * kBlockBitsMax;           // the carried bits and every block at its worst
constexpr int kBitWords = (kStripBitsMax + 31) / 32 + 2;
constexpr int kStripBytesMax = (kStripBitsMax + 7) / 8;
constexpr int kStuffedMax = (2 * kStripBytesMax + 15) & ~15;

struct EncArgs {
    const uint8_t* frames;
    size_t frame_stride;
    int h, w, mw, mh;
    uint8_t* streams;
    size_t stream_stride;
    uint64_t* sizes;
    int32_t* flags;
    uint64_t* offsets;
    uint32_t* rowsize;
    uint16_t div[2][64];
    uint8_t header[kHeaderLen];
};

// most significant bit first into zeroed LDS words; a lane's symbols are consecutive bits, whole words leave its accumulator through an
// atomic OR (the first and the last word of a block are shared with the neighbours)
struct LdsSink {
    uint32_t* words;
    uint32_t word;
    uint64_t acc;
    int nacc;
    __device__ LdsSink(uint32_t* w, uint32_t bit) : words(w), word(bit >> 5), acc(0), nacc((int)(bit & 31)) {}
    __device__ void put(uint32_t v, int n) {
        acc = (acc << n) | v;
        nacc += n;
        if (nacc >= 32) {
            nacc -= 32;
            atomicOr(&words[word++], (uint32_t)(acc >> nacc));
            acc &= (1ull << nacc) - 1;
        }
    }
    __device__ void flush() {
        if (nacc > 0 && acc) atomicOr(&words[word], (uint32_t)(acc << (32 - nacc)));
    }
};

__device__ __forceinline__ uint32_t stream_byte(const uint32_t* words, uint32_t i) { return (words[i >> 2] >> (24 - 8 * (i & 3))) & 0xFFu; }

template <bool kWrite>
__global__ __launch_bounds__(kThreads) void jpeg_row_kernel(EncArgs a) {
    __shared__ int work[kStripBlocks * kBlockPad];
    __shared__ uint8_t cfull[2][16][16 * kStripMcus];
    __shared__ __attribute__((aligned(16))) int16_t coef[kStripBlocks][64];
    __shared__ uint32_t bitbuf[kBitWords];
    __shared__ __attribute__((aligned(16))) uint8_t stuffed[kWrite ? kStuffedMax : 16];
    __shared__ uint32_t nbits[kStripBlocks];
    __shared__ uint32_t nff[kThreads];
    __shared__ int pred[3];
    __shared__ uint32_t carry_byte, carry_n, row_pos;

    const int t = threadIdx.x;
    const int my = blockIdx.x;
    const uint32_t b = blockIdx.y;
    if (kWrite && a.flags[b]) return;
    const uint8_t* frame = a.frames + (size_t)b * a.frame_stride;
    const size_t row_id = (size_t)b * a.mh + my;
    uint8_t* dst = kWrite ? a.streams + (size_t)b * a.stream_stride + a.offsets[row_id] : nullptr;

    if (t == 0) { pred[0] = pred[1] = pred[2] = 0; carry_byte = 0; carry_n = 0; row_pos = 0; }

    for (int m0 = 0; m0 < a.mw; m0 += kStripMcus) {
        const int nm = a.mw - m0 < kStripMcus ? a.mw - m0 : kStripMcus;
        const int nblk = 6 * nm, sw = 16 * nm;
        __syncthreads();                                       // the last strip's buffers are free, its carries are visible
        for (int i = t; i < kBitWords; i += kThreads) bitbuf[i] = i == 0 ? carry_byte << 24 : 0u;

        // 1. colour: the strip's 16 x 16nm pixels, the frame's last column and row replicated; Y into its blocks, Cb and Cr at full size
        for (int i = t; i < 16 * sw; i += kThreads) {
            const int ly = i / sw, lx = i - ly * sw;
            const int sy = my * 16 + ly < a.h ? my * 16 + ly : a.h - 1, sx = m0 * 16 + lx < a.w ? m0 * 16 + lx : a.w - 1;
            const uint8_t* p = frame + ((size_t)sy * a.w + sx) * 3;
            const int cb = p[0], cg = p[1], cr = p[2];
            const int blk = (lx >> 4) * 6 + ((ly >> 3) << 1) + ((lx >> 3) & 1);
            work[blk * kBlockPad + (ly & 7) * kRowPad + (lx & 7)] = ycc_y(cb, cg, cr) - 128;
            cfull[0][ly][lx] = (uint8_t)ycc_cb(cb, cg, cr);
            cfull[1][ly][lx] = (uint8_t)ycc_cr(cb, cg, cr);
        }
        __syncthreads();
        // 2. the chroma box
        for (int i = t; i < 2 * 64 * nm; i += kThreads) {
            const int c = i / (64 * nm), j = i - c * 64 * nm, py = j / (8 * nm), px = j - py * 8 * nm;
            const int v = box4(cfull[c][2 * py][2 * px], cfull[c][2 * py][2 * px + 1], cfull[c][2 * py + 1][2 * px], cfull[c][2 * py + 1][2 * px + 1]);
            work[((px >> 3) * 6 + 4 + c) * kBlockPad + py * kRowPad + (px & 7)] = v - 128;
        }
        __syncthreads();
        // 3. row pass: one lane per row of a block
        for (int i = t; i < 8 * nblk; i += kThreads) {
            int* r = work + (i >> 3) * kBlockPad + (i & 7) * kRowPad;
            int v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = r[k];
            fdct8<true>(v);
#pragma unroll
            for (int k = 0; k < 8; ++k) r[k] = v[k];
        }
        __syncthreads();
        // 4. column pass and the quantiser: one lane per column of a block, the results in zigzag order
        for (int i = t; i < 8 * nblk; i += kThreads) {
            const int blk = i >> 3, x = i & 7;
            const int* c = work + blk * kBlockPad + x;
            const int chroma = blk % 6 >= 4;
            int v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = c[k * kRowPad];
            fdct8<false>(v);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int z = kInvZigzag[k * 8 + x];
                coef[blk][z] = (int16_t)quantise(v[k], a.div[chroma][z]);
            }
        }
        __syncthreads();
        // 5. one lane per block, in the order of the interleaved scan: the DC difference and the block's exact bit count
        int diff = 0;
        const int k6 = t % 6, comp = k6 < 4 ? 0 : k6 - 3;
        if (t < nblk) {
            int p;
            if (comp == 0) p = k6 > 0 ? coef[t - 1][0] : (t > 0 ? coef[t - 3][0] : pred[0]);
            else p = t >= 6 ? coef[t - 6][0] : pred[comp];
            diff = coef[t][0] - p;
            CountSink cs{0};
            encode_block(coef[t], diff, comp != 0, cs);
            nbits[t] = cs.bits;
        }
        __syncthreads();
        uint32_t total = carry_n;
        for (int u = 0; u < nblk; ++u) total += nbits[u];
        if (t < nblk) {
            uint32_t bit = carry_n;
            for (int u = 0; u < t; ++u) bit += nbits[u];
            LdsSink sink(bitbuf, bit);
            encode_block(coef[t], diff, comp != 0, sink);
            sink.flush();
        }
        const bool last = m0 + kStripMcus >= a.mw;
        __syncthreads();
        if (t == 0) {
            pred[0] = coef[nblk - 3][0];
            pred[1] = coef[nblk - 2][0];
            pred[2] = coef[nblk - 1][0];
            if (last && (total & 7)) {                         // the interval ends: 1-bits up to the byte boundary
                const uint32_t pad = 8 - (total & 7);
                bitbuf[total >> 5] |= ((1u << pad) - 1) << (32 - (total & 31) - pad);
            }
        }
        if (last) total = (total + 7) & ~7u;
        __syncthreads();
        // 6. byte stuffing: each lane counts the FF bytes of its piece, a scan places the pieces
        const uint32_t nbytes = total >> 3;
        const uint32_t seg = (nbytes + kThreads - 1) / kThreads;
        const uint32_t lo = (uint32_t)t * seg < nbytes ? (uint32_t)t * seg : nbytes, hi = lo + seg < nbytes ? lo + seg : nbytes;
        uint32_t mine = 0;
        for (uint32_t i = lo; i < hi; ++i) mine += stream_byte(bitbuf, i) == 0xFFu;
        nff[t] = mine;
        __syncthreads();
        uint32_t before = 0, all = 0;
#pragma unroll 8
        for (int u = 0; u < kThreads; ++u) {
            const uint32_t v = nff[u];
            before += u < t ? v : 0u;
            all += v;
        }
        const uint32_t pos = row_pos;
        if (kWrite) {
            uint32_t o = lo + before;
            for (uint32_t i = lo; i < hi; ++i) {
                const uint32_t v = stream_byte(bitbuf, i);
                stuffed[o++] = (uint8_t)v;
                if (v == 0xFFu) stuffed[o++] = 0;
            }
        }
        const uint32_t carry = (total & 7) ? stream_byte(bitbuf, nbytes) : 0u;
        __syncthreads();
        if (kWrite)
            for (uint32_t i = t; i < nbytes + all; i += kThreads) dst[pos + i] = stuffed[i];
        if (t == 0) {
            carry_byte = carry;
            carry_n = total & 7;
            row_pos = pos + nbytes + all;
        }
    }
    __syncthreads();
    if (t == 0) {
        const uint32_t pos = row_pos;
        if (kWrite) {
            dst[pos] = 0xFF;
            dst[pos + 1] = my + 1 < a.mh ? (uint8_t)(0xD0 + (my & 7)) : (uint8_t)0xD9;
        } else {
            a.rowsize[row_id] = pos + 2;
        }
    }
}

// one workgroup per frame: where each row goes, whether the file fits, its size and its header
__global__ __launch_bounds__(kThreads) void jpeg_layout_kernel(EncArgs a) {
    __shared__ int fits;
    const int t = threadIdx.x;
    const uint32_t b = blockIdx.x;
    if (t == 0) {
        uint64_t off = kHeaderLen;
        for (int r = 0; r < a.mh; ++r) {
            const size_t id = (size_t)b * a.mh + r;
            a.offsets[id] = off;
            off += a.rowsize[id];
        }
        fits = off <= (uint64_t)a.stream_stride;
        a.sizes[b] = fits ? off : 0;
        a.flags[b] = fits ? 0 : 1;
    }
    __syncthreads();
    if (!fits) return;
    uint8_t* stream = a.streams + (size_t)b * a.stream_stride;
    for (int i = t; i < kHeaderLen; i += kThreads) stream[i] = a.header[i];
}

}  // namespace

hipError_t launch_jpeg_encode(const uint8_t* frames, size_t frame_stride, int B, int h, int w, int quality, uint8_t* streams,
                              size_t stream_stride, uint64_t* sizes, int32_t* flags, uint8_t* workspace, hipStream_t s) {
    EncArgs a{};
    a.frames = frames; a.frame_stride = frame_stride; a.h = h; a.w = w; a.mw = mcus_w(w); a.mh = mcu_rows(h);
    a.streams = streams; a.stream_stride = stream_stride; a.sizes = sizes; a.flags = flags;
    const Layout l(B, h);
    a.offsets = reinterpret_cast<uint64_t*>(workspace + l.offsets);
    a.rowsize = reinterpret_cast<uint32_t*>(workspace + l.rowsize);
    make_header(a.header, a.div, h, w, quality);
    const dim3 grid((unsigned)a.mh, (unsigned)B);
    hipLaunchKernelGGL(jpeg_row_kernel<false>, grid, dim3(kThreads), 0, s, a);
    hipLaunchKernelGGL(jpeg_layout_kernel, dim3((unsigned)B), dim3(kThreads), 0, s, a);
    hipLaunchKernelGGL(jpeg_row_kernel<true>, grid, dim3(kThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace sd
