// Device half of the result-image writer (sd_png_encode_bgr): u8 [B,h,w,3] BGR frames in device memory -> one complete zlib stream per
// frame (Paeth rows, distance-1 run matches, one dynamic-Huffman block per independent 32 KiB chunk; format: include/semdepth.h), so that
// the host only wraps PNG chunks around it.  Three launches, no host synchronisation:
//   png_chunk_kernel    one workgroup per chunk: filtered bytes -> LDS, Adler partials, run boundaries, token histogram, the codes (the
//                       construction of png_deflate.hpp on one lane, the sort of the used symbols on all), bit offsets, packing in LDS,
//                       coalesced store into the chunk's workspace slot
//   png_layout_kernel   one workgroup per frame: exclusive scan of the chunk sizes, the combined Adler-32, header, trailer, sizes[b]
//   png_gather_kernel   one workgroup per chunk: the slot copied to its place in the frame's stream
// Every coding decision is a function of png_deflate.hpp, which sd_png_encode_zlib_host runs too: the streams are the same bytes.
#include "png_gpu.hpp"

namespace sd {
namespace {

using namespace sdpng;

constexpr int kThreads = 256;
constexpr int kSeg = kChunk / kThreads;                       // bytes of a chunk one thread walks: 128
constexpr int kOutWords = (kChunk + kChunkSlack) / 4;
static_assert(kSeg == 128, "the LDS skew below assumes 128-byte segments");

// a thread walks its 128-byte segment byte by byte: one word of skew per segment puts the 64 lanes of a wave on 64 different banks
__device__ __forceinline__ int skew(int i) { return i + ((i >> 7) << 2); }

struct LdsSink {
    uint32_t* words;
    uint32_t bit;
    __device__ void put(uint32_t v, int n) {
        if (!n) return;
        const uint64_t x = (uint64_t)v << (bit & 31);
        words[bit >> 5] |= (uint32_t)x;
        if (x >> 32) words[(bit >> 5) + 1] |= (uint32_t)(x >> 32);
        bit += (uint32_t)n;
    }
};

struct PngArgs {
    const uint8_t* frames;
    size_t frame_stride;
    int h, w;
    uint32_t nchunks;
    uint8_t* streams;
    size_t stream_stride;
    uint64_t* sizes;
    uint8_t* slots;
    uint64_t* offsets;
    uint32_t *csize, *adler_a, *adler_b;
};

// the tokens of bytes [lo, hi) of the chunk, in order: f(position, token, byte value).  s = start of the run that holds byte lo,
// next = first run boundary at or behind hi (the chunk's length when there is none)
template <class F>
__device__ __forceinline__ void walk_tokens(const uint8_t* d, int lo, int hi, int s, int next, F&& f) {
    int i = lo;
    while (i < hi) {
        const uint8_t v = d[skew(i)];
        int e = i + 1;
        while (e < hi && d[skew(e)] == v) ++e;
        const int stop = e;
        if (e == hi) e = next;
        const uint32_t n = (uint32_t)(e - s);
        for (uint32_t p = (uint32_t)(i - s); i < stop; ++i, ++p) {
            const int tok = run_token(n, p);
            if (tok) f(i, tok, v);
        }
        s = e;
    }
}

__global__ __launch_bounds__(kThreads) void png_chunk_kernel(PngArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t d[kChunk + 4 * kThreads];
    __shared__ uint32_t out[kOutWords];
    __shared__ uint32_t hist[288];
    __shared__ HuffScratch sc;
    __shared__ ChunkCodes cc;
    __shared__ int first_b[kThreads], last_b[kThreads];
    __shared__ uint32_t tbits[kThreads];
    __shared__ uint32_t sh_a, sh_b, sh_n, sh_dynamic;

    const int t = threadIdx.x;
    const uint32_t c = blockIdx.x, b = blockIdx.y;
    const uint32_t rowlen = 1 + 3 * (uint32_t)a.w;
    const uint32_t total = (uint32_t)filtered_len(a.h, a.w);              // h (1 + 3 w) <= 16384 * 49153 < 2^32
    const uint32_t g0 = c * (uint32_t)kChunk;
    const int len = (int)(total - g0 < (uint32_t)kChunk ? total - g0 : (uint32_t)kChunk);
    const uint8_t* frame = a.frames + (size_t)b * a.frame_stride;
    const size_t chunk_id = (size_t)b * a.nchunks + c;
    uint8_t* slot = a.slots + chunk_id * kPngSlot;

    for (int i = t; i < 288; i += kThreads) hist[i] = 0;
    for (int i = t; i < kOutWords; i += kThreads) out[i] = 0;
    if (t == 0) { sh_a = 0; sh_b = 0; sh_n = 0; }

    // 1. filtered bytes: four consecutive bytes per lane and step (coalesced reads of the frame, one LDS word store), Adler partials
    uint32_t sa = 0, sb = 0;
    for (int i0 = 4 * t; i0 < kChunk; i0 += 4 * kThreads) {
        uint32_t word = 0;
        if (i0 < len) {
            const uint32_t g = g0 + (uint32_t)i0;
            uint32_t y = g / rowlen, k = g - y * rowlen;
            for (int j = 0; j < 4 && i0 + j < len; ++j) {
                const uint32_t v = filtered_byte(frame, a.w, y, k);
                word |= v << (8 * j);
                sa += v;
                sb += (uint32_t)(len - (i0 + j)) * v;
                if (++k == rowlen) { k = 0; ++y; }
            }
        }
        *reinterpret_cast<uint32_t*>(&d[skew(i0)]) = word;
    }
    __syncthreads();
    atomicAdd(&sh_a, sa % kAdlerMod);                 // per lane at most 128 * 255 * 32768 < 2^32; 256 residues < 2^24
    atomicAdd(&sh_b, sb % kAdlerMod);

    // 2. run boundaries of this lane's segment (byte i starts a run when it differs from byte i - 1)
    const int lo = t * kSeg < len ? t * kSeg : len, hi = (t + 1) * kSeg < len ? (t + 1) * kSeg : len;
    {
        int fb = 0x7fffffff, lb = -1;
        uint8_t prev = lo > 0 && lo < len ? d[skew(lo - 1)] : 0;
        for (int i = lo; i < hi; ++i) {
            const uint8_t v = d[skew(i)];
            if (i == 0 || v != prev) { if (lb < 0) fb = i; lb = i; }
            prev = v;
        }
        first_b[t] = fb;
        last_b[t] = lb;
    }
    __syncthreads();
    int run_start = lo, next = len;
    if (lo < hi) {
        if (first_b[t] != lo)
            for (int u = t - 1; u >= 0; --u)
                if (last_b[u] >= 0) { run_start = last_b[u]; break; }
        for (int u = t + 1; u < kThreads; ++u)
            if (first_b[u] != 0x7fffffff) { next = first_b[u]; break; }
    }

    // 3. token histogram
    walk_tokens(d, lo, hi, run_start, next, [&](int, int tok, uint8_t v) {
        int eb, ev;
        atomicAdd(&hist[tok == 1 ? (int)v : length_symbol(tok, &eb, &ev)], 1u);
    });
    if (t == 0) hist[kEob] = 1;
    __syncthreads();

    // 4. the used symbols in ascending (count, symbol) order: the keys are distinct, so a key's rank is its place
    for (int s = t; s < kLitSyms; s += kThreads) {
        const uint32_t f = hist[s];
        if (!f) continue;
        const uint32_t key = (f << 9) | (uint32_t)s;
        int rank = 0;
        for (int u = 0; u < kLitSyms; ++u) {
            const uint32_t fu = hist[u];
            rank += fu && ((fu << 9) | (uint32_t)u) < key;
        }
        sc.key[rank] = key;
        atomicAdd(&sh_n, 1u);
    }
    __syncthreads();

    // 5. one lane builds both codes and writes the block header
    if (t == 0) {
        build_chunk_codes(hist, (int)sh_n, sc, cc);
        const bool dyn = chunk_is_dynamic(cc, (uint32_t)len);
        sh_dynamic = dyn;
        if (dyn) {
            LdsSink sink{out, 0};
            write_block_header(sink, cc);
        }
        a.csize[chunk_id] = chunk_coded_bytes(cc, (uint32_t)len);
        a.adler_a[chunk_id] = sh_a % kAdlerMod;
        a.adler_b[chunk_id] = sh_b % kAdlerMod;
    }
    __syncthreads();

    if (!sh_dynamic) {                                // stored: 00 LEN NLEN bytes, then the empty stored block 00 00 00 FF FF
        if (t == 0) slot[0] = 0;
        else if (t < 5) slot[t] = (uint8_t)((t < 3 ? len : ~len) >> (8 * ((t - 1) & 1)));
        else if (t < 10) slot[len + t] = t < 8 ? 0 : 0xFF;
        for (int i = t; i < len; i += kThreads) slot[5 + i] = d[skew(i)];
        return;
    }

    // 6. bit offsets of the segments
    uint32_t mine = 0;
    walk_tokens(d, lo, hi, run_start, next, [&](int, int tok, uint8_t v) {
        int nb;
        token_bits(cc, tok, v, &nb);
        mine += (uint32_t)nb;
    });
    tbits[t] = mine;
    __syncthreads();
    uint32_t bit = cc.header_bits;
    for (int u = 0; u < t; ++u) bit += tbits[u];

    // 7. packing: a lane's tokens are consecutive bits; whole words leave its accumulator through an LDS atomic OR (the first and the
    // last word of a segment are shared with the neighbours)
    {
        uint64_t acc = 0;
        uint32_t word = bit >> 5;
        int nacc = (int)(bit & 31);
        walk_tokens(d, lo, hi, run_start, next, [&](int, int tok, uint8_t v) {
            int nb;
            const uint32_t bits = token_bits(cc, tok, v, &nb);
            acc |= (uint64_t)bits << nacc;
            nacc += nb;
            if (nacc >= 32) {
                atomicOr(&out[word++], (uint32_t)acc);
                acc >>= 32;
                nacc -= 32;
            }
        });
        if (nacc > 0 && (uint32_t)acc) atomicOr(&out[word], (uint32_t)acc);
    }
    const uint32_t end_bits = cc.header_bits + cc.body_bits;
    const uint32_t nbytes = (end_bits + 3 + 7) / 8 + 4;
    if (t == 0) {                                     // end of block, then the empty stored block: 000, padding, 00 00 FF FF
        const uint32_t eb = end_bits - cc.ll[kEob];
        const uint64_t x = (uint64_t)cc.llcode[kEob] << (eb & 31);
        atomicOr(&out[eb >> 5], (uint32_t)x);
        if (x >> 32) atomicOr(&out[(eb >> 5) + 1], (uint32_t)(x >> 32));
        for (uint32_t p = nbytes - 2; p < nbytes; ++p) atomicOr(&out[p >> 2], 0xFFu << (8 * (p & 3)));
    }
    __syncthreads();
    uint32_t* dst = reinterpret_cast<uint32_t*>(slot);
    for (uint32_t i = t; i < (nbytes + 3) / 4; i += kThreads) dst[i] = out[i];
}

// one workgroup per frame: where each chunk goes, and everything of the stream that is not a chunk
__global__ __launch_bounds__(kThreads) void png_layout_kernel(PngArgs a) {
    __shared__ uint32_t s_size[kThreads], s_a[kThreads], s_b[kThreads];
    __shared__ uint64_t s_off[kThreads];
    __shared__ uint64_t carry_off;
    __shared__ uint32_t carry_a, carry_b;
    const int t = threadIdx.x;
    const uint32_t b = blockIdx.x;
    const uint32_t total = (uint32_t)filtered_len(a.h, a.w);
    uint8_t* stream = a.streams + (size_t)b * a.stream_stride;
    if (t == 0) { carry_off = 2; carry_a = 1; carry_b = 0; }
    for (uint32_t c0 = 0; c0 < a.nchunks; c0 += kThreads) {
        const uint32_t c = c0 + t;
        const size_t id = (size_t)b * a.nchunks + c;
        __syncthreads();
        if (c < a.nchunks) { s_size[t] = a.csize[id]; s_a[t] = a.adler_a[id]; s_b[t] = a.adler_b[id]; }
        __syncthreads();
        if (t == 0) {
            uint64_t off = carry_off;
            uint32_t ca = carry_a, cb = carry_b;
            const uint32_t m = a.nchunks - c0 < (uint32_t)kThreads ? a.nchunks - c0 : (uint32_t)kThreads;
            for (uint32_t u = 0; u < m; ++u) {
                const uint32_t g0 = (c0 + u) * (uint32_t)kChunk;
                const uint32_t len = total - g0 < (uint32_t)kChunk ? total - g0 : (uint32_t)kChunk;
                s_off[u] = off;
                off += s_size[u];
                adler_append(ca, cb, len, s_a[u], s_b[u]);
            }
            carry_off = off; carry_a = ca; carry_b = cb;
        }
        __syncthreads();
        if (c < a.nchunks) a.offsets[id] = s_off[t];
    }
    __syncthreads();
    if (t == 0) {
        const uint64_t off = carry_off;
        const uint32_t adler = (carry_b << 16) | carry_a;
        stream[0] = 0x78;
        stream[1] = 0x01;
        stream[off] = 1; stream[off + 1] = 0; stream[off + 2] = 0; stream[off + 3] = 0xFF; stream[off + 4] = 0xFF;      // the final, empty stored block
        stream[off + 5] = (uint8_t)(adler >> 24); stream[off + 6] = (uint8_t)(adler >> 16);
        stream[off + 7] = (uint8_t)(adler >> 8); stream[off + 8] = (uint8_t)adler;
        a.sizes[b] = off + 9;
    }
}

// one workgroup per chunk: slot -> stream.  The destination offset is any byte; words are stored where the destination is aligned.
__global__ __launch_bounds__(kThreads) void png_gather_kernel(PngArgs a) {
    const size_t id = (size_t)blockIdx.y * a.nchunks + blockIdx.x;
    const uint8_t* src = a.slots + id * kPngSlot;
    uint8_t* dst = a.streams + (size_t)blockIdx.y * a.stream_stride + a.offsets[id];
    const uint32_t n = a.csize[id];
    const uint32_t head = (uint32_t)((4 - (reinterpret_cast<uintptr_t>(dst) & 3)) & 3);
    const uint32_t h = head < n ? head : n;
    const uint32_t words = (n - h) / 4;
    if (threadIdx.x < h) dst[threadIdx.x] = src[threadIdx.x];
    for (uint32_t i = threadIdx.x; i < words; i += kThreads) {
        const uint8_t* s = src + h + 4 * (size_t)i;
        const uint32_t v = (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16) | ((uint32_t)s[3] << 24);
        *reinterpret_cast<uint32_t*>(dst + h + 4 * (size_t)i) = v;
    }
    const uint32_t done = h + 4 * words;
    if (threadIdx.x < n - done) dst[done + threadIdx.x] = src[done + threadIdx.x];
}

}  // namespace

hipError_t launch_png_encode(const uint8_t* frames, size_t frame_stride, int B, int h, int w, uint8_t* streams, size_t stream_stride,
                             uint64_t* sizes, uint8_t* workspace, hipStream_t s) {
    const size_t nch = sdpng::num_chunks(h, w);
    PngArgs a{};
    a.frames = frames; a.frame_stride = frame_stride; a.h = h; a.w = w; a.nchunks = (uint32_t)nch;
    a.streams = streams; a.stream_stride = stream_stride; a.sizes = sizes;
    const sdpng::Layout l(B, h, w);
    a.slots = workspace + l.slots;
    a.offsets = reinterpret_cast<uint64_t*>(workspace + l.offsets);
    a.csize = reinterpret_cast<uint32_t*>(workspace + l.csize);
    a.adler_a = reinterpret_cast<uint32_t*>(workspace + l.adler_a);
    a.adler_b = reinterpret_cast<uint32_t*>(workspace + l.adler_b);
    hipLaunchKernelGGL(png_chunk_kernel, dim3((unsigned)nch, (unsigned)B), dim3(kThreads), 0, s, a);
    hipLaunchKernelGGL(png_layout_kernel, dim3((unsigned)B), dim3(kThreads), 0, s, a);
    hipLaunchKernelGGL(png_gather_kernel, dim3((unsigned)nch, (unsigned)B), dim3(kThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace sd
