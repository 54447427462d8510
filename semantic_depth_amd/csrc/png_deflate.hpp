// The coder of the device PNG route (sd_png_encode_bgr / sd_png_encode_zlib_host; stream format: include/semdepth.h), stated ONCE for
// the kernels of png_gpu.hip and the host function of host_png.cpp: the Paeth residual of one filtered byte, the token a byte of a run
// becomes, the length symbols, histogram -> length-limited Huffman code lengths, canonical codes and the dynamic-block header.  Both sides
// call these functions, so they agree on every tie and every bit; what differs is only who walks the bytes (one loop on the host, one
// workgroup per chunk on the device).
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include <stddef.h>
#include <stdint.h>

#include "arena.hpp"

#if defined(__HIPCC__)
#define SDPNG_HD __host__ __device__ inline
#else
#define SDPNG_HD inline
#endif

namespace sdpng {

constexpr int kChunk = 32768;        // C: filtered bytes per independently coded chunk
constexpr int kChunkSlack = 16;      // a coded chunk never exceeds len + 16 bytes
constexpr int kLitSyms = 286, kClSyms = 19, kLitBits = 15, kClBits = 7, kEob = 256;
constexpr int kMaxExtent = 16384;
constexpr uint32_t kAdlerMod = 65521;

SDPNG_HD size_t filtered_len(int h, int w) { return (size_t)h * (1 + 3 * (size_t)w); }
SDPNG_HD size_t num_chunks(int h, int w) { return (filtered_len(h, w) + kChunk - 1) / kChunk; }
// capacity bound of a frame's stream: 2 + sum(len_c + 16) + 16
SDPNG_HD size_t stream_bound(int h, int w) { return 2 + filtered_len(h, w) + (size_t)kChunkSlack * num_chunks(h, w) + 16; }

// byte k (0 = the filter type, 1 + 3x + ch = channel ch of RGB pixel x) of filtered row y of a u8 [h,w,3] BGR frame: filter 4 (Paeth),
// bpp 3, pixels outside the image are 0
SDPNG_HD uint8_t filtered_byte(const uint8_t* frame, int w, uint32_t y, uint32_t k) {
    if (k == 0) return 4;
    const uint32_t j = k - 1, x = j / 3, ch = j - 3 * x;
    const uint8_t* p = frame + ((size_t)y * w + x) * 3 + (2 - ch);
    const ptrdiff_t up = (ptrdiff_t)w * 3;
    const int cur = p[0], a = x ? p[-3] : 0, b = y ? p[-up] : 0, c = (x && y) ? p[-up - 3] : 0;
    const int pp = a + b - c;
    const int pa = pp > a ? pp - a : a - pp, pb = pp > b ? pp - b : b - pp, pc = pp > c ? pp - c : c - pp;
    const int pr = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
    return (uint8_t)(cur - pr);
}

// what byte p (0-based) of a maximal run of n equal bytes inside a chunk becomes: 0 = covered by a match, 1 = a literal, L >= 3 = the
// start of a distance-1 match of length L.  n >= 4: one literal, matches of 258 over the other n - 1 bytes, a last match of 3..257 or
// 1..2 literals.
SDPNG_HD int run_token(uint32_t n, uint32_t p) {
    if (n < 4 || p == 0) return 1;
    const uint32_t q = p - 1, m = q / 258, off = q - m * 258, rest = (n - 1) - m * 258;
    const uint32_t piece = rest < 258 ? rest : 258;
    if (piece < 3) return 1;
    return off == 0 ? (int)piece : 0;
}

// DEFLATE length symbol of a match length 3..258, its number of extra bits and their value
SDPNG_HD int length_symbol(int L, int* extra_bits, int* extra_val) {
    if (L == 258) { *extra_bits = 0; *extra_val = 0; return 285; }
    const int v = L - 3;
    if (v < 4) { *extra_bits = 0; *extra_val = 0; return 257 + v; }
    int k = 2;
    while ((v >> (k + 1)) != 0) ++k;                 // floor(log2 v), v in 4..254
    const int eb = k - 2;
    *extra_bits = eb;
    *extra_val = v & ((1 << eb) - 1);
    return 261 + 4 * eb + ((v >> eb) & 3);
}
SDPNG_HD int symbol_extra_bits(int sym) { return (sym < 265 || sym == 285) ? 0 : (sym - 261) >> 2; }

// working storage of the code construction (LDS on the device, the stack on the host)
struct HuffScratch {
    uint32_t key[288];        // (count << 9 | symbol) of the used symbols, ascending
    uint32_t iw[288];         // weights of the internal nodes in creation order
    uint16_t parent[576];
    uint8_t depth[576];
    uint32_t num_codes[16];
    uint32_t next_code[16];
    uint32_t clfreq[kClSyms];
};

// the used symbols of freq[0..nsym) as ascending keys (insertion sort: the keys are distinct, so every correct sort gives this order)
SDPNG_HD int sort_keys(const uint32_t* freq, int nsym, uint32_t* key) {
    int n = 0;
    for (int s = 0; s < nsym; ++s) {
        if (!freq[s]) continue;
        const uint32_t k = (freq[s] << 9) | (uint32_t)s;
        int i = n++;
        for (; i > 0 && key[i - 1] > k; --i) key[i] = key[i - 1];
        key[i] = k;
    }
    return n;
}

// code lengths (at most maxbits, Kraft sum exactly 1) from sc.key[0..n): Huffman's tree by the two-queue method (a leaf before an internal
// node of equal weight), depths clamped to maxbits, the excess repaired on the per-length counts (drop one code of maxbits, split the
// longest shorter one, until the sum fits), lengths handed out longest first to the rarest symbol.  One used symbol gets length 1 beside
// a second, unused code of length 1 (a complete tree every inflater takes).
SDPNG_HD void lengths_from_sorted(HuffScratch& sc, int n, int nsym, int maxbits, uint8_t* lens) {
    for (int s = 0; s < nsym; ++s) lens[s] = 0;
    if (n <= 0) return;
    if (n == 1) {
        const int s = (int)(sc.key[0] & 511);
        lens[s] = 1;
        lens[s == 0 ? 1 : 0] = 1;
        return;
    }
    int li = 0, ii = 0, ni = 0;
    for (int k = 0; k < n - 1; ++k) {
        uint32_t sum = 0;
        for (int t = 0; t < 2; ++t) {
            if (li < n && (ii >= ni || (sc.key[li] >> 9) <= sc.iw[ii])) {
                sum += sc.key[li] >> 9;
                sc.parent[li++] = (uint16_t)(n + ni);
            } else {
                sum += sc.iw[ii];
                sc.parent[n + ii] = (uint16_t)(n + ni);
                ++ii;
            }
        }
        sc.iw[ni++] = sum;
    }
    for (int i = 0; i <= maxbits; ++i) sc.num_codes[i] = 0;
    sc.depth[2 * n - 2] = 0;
    for (int k = 2 * n - 3; k >= 0; --k) {
        const int d = sc.depth[sc.parent[k]] + 1;
        sc.depth[k] = (uint8_t)d;
        if (k < n) sc.num_codes[d < maxbits ? d : maxbits]++;
    }
    uint32_t total = 0;
    for (int i = maxbits; i > 0; --i) total += sc.num_codes[i] << (maxbits - i);
    while (total != (1u << maxbits)) {
        sc.num_codes[maxbits]--;
        for (int i = maxbits - 1; i > 0; --i)
            if (sc.num_codes[i]) { sc.num_codes[i]--; sc.num_codes[i + 1] += 2; break; }
        total--;
    }
    int idx = 0;
    for (int len = maxbits; len > 0; --len)
        for (uint32_t c = 0; c < sc.num_codes[len]; ++c) lens[sc.key[idx++] & 511] = (uint8_t)len;
}

// canonical codes of lens[0..nsym), each stored bit-reversed (DEFLATE packs Huffman codes most significant bit first into a stream that
// fills bytes from the least significant bit)
SDPNG_HD void canonical_codes(HuffScratch& sc, const uint8_t* lens, int nsym, int maxbits, uint16_t* codes) {
    for (int i = 0; i <= maxbits; ++i) sc.num_codes[i] = 0;
    for (int s = 0; s < nsym; ++s) sc.num_codes[lens[s]]++;
    sc.num_codes[0] = 0;
    uint32_t code = 0;
    for (int b = 1; b <= maxbits; ++b) {
        code = (code + sc.num_codes[b - 1]) << 1;
        sc.next_code[b] = code;
    }
    for (int s = 0; s < nsym; ++s) {
        const int len = lens[s];
        uint32_t r = 0;
        if (len) {
            uint32_t c = sc.next_code[len]++;
            for (int i = 0; i < len; ++i) { r = (r << 1) | (c & 1); c >>= 1; }
        }
        codes[s] = (uint16_t)r;
    }
}

// the two codes of one chunk and the sizes that follow from its histogram
struct ChunkCodes {
    uint8_t ll[288];          // literal/length code lengths
    uint16_t llcode[288];
    uint8_t cl[kClSyms];      // code-length code lengths
    uint16_t clcode[kClSyms];
    int32_t hlit;             // literal/length lengths sent (257..286)
    uint32_t header_bits;     // BFINAL .. the last distance code length
    uint32_t body_bits;       // every token and the end-of-block symbol
};

// from the chunk's token histogram hist[0..286) (hist[256] = 1) and its used symbols sorted in sc.key[0..n): lengths, codes, sizes.
// The header sends plain code lengths (no repeat codes), all 19 code-length-code lengths, and the distance codes 0 and 1 at length 1.
SDPNG_HD void build_chunk_codes(const uint32_t* hist, int n, HuffScratch& sc, ChunkCodes& cc) {
    lengths_from_sorted(sc, n, kLitSyms, kLitBits, cc.ll);
    canonical_codes(sc, cc.ll, kLitSyms, kLitBits, cc.llcode);
    int hlit = kLitSyms;
    while (hlit > 257 && cc.ll[hlit - 1] == 0) --hlit;
    cc.hlit = hlit;
    for (int i = 0; i < kClSyms; ++i) sc.clfreq[i] = 0;
    for (int i = 0; i < hlit; ++i) sc.clfreq[cc.ll[i]]++;
    sc.clfreq[1] += 2;
    const int ncl = sort_keys(sc.clfreq, kClSyms, sc.key);
    lengths_from_sorted(sc, ncl, kClSyms, kClBits, cc.cl);
    canonical_codes(sc, cc.cl, kClSyms, kClBits, cc.clcode);
    uint32_t hb = 3 + 5 + 5 + 4 + 3 * kClSyms + 2 * cc.cl[1];
    for (int i = 0; i < hlit; ++i) hb += cc.cl[cc.ll[i]];
    cc.header_bits = hb;
    uint32_t bb = 0;
    for (int s = 0; s < kLitSyms; ++s) bb += hist[s] * (uint32_t)(cc.ll[s] + symbol_extra_bits(s) + (s > kEob ? 1 : 0));
    cc.body_bits = bb;
}

// the chunk is a dynamic block when that block is smaller than the stored form's len + 5 bytes
SDPNG_HD bool chunk_is_dynamic(const ChunkCodes& cc, uint32_t len) { return (cc.header_bits + cc.body_bits + 7) / 8 < len + 5; }
// bytes of a coded chunk with its alignment (an empty stored block)
SDPNG_HD uint32_t chunk_coded_bytes(const ChunkCodes& cc, uint32_t len) {
    return chunk_is_dynamic(cc, len) ? (cc.header_bits + cc.body_bits + 3 + 7) / 8 + 4 : len + 10;
}

// Sink: void put(uint32_t bits, int nbits), least significant bit first
template <class Sink>
SDPNG_HD void write_block_header(Sink& s, const ChunkCodes& cc) {
    const uint8_t order[kClSyms] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    s.put(0, 1);                                // BFINAL 0
    s.put(2, 2);                                // BTYPE 10
    s.put((uint32_t)(cc.hlit - 257), 5);
    s.put(1, 5);                                // HDIST - 1: two distance codes
    s.put(kClSyms - 4, 4);
    for (int i = 0; i < kClSyms; ++i) s.put(cc.cl[order[i]], 3);
    for (int i = 0; i < cc.hlit; ++i) s.put(cc.clcode[cc.ll[i]], cc.cl[cc.ll[i]]);
    s.put(cc.clcode[1], cc.cl[1]);
    s.put(cc.clcode[1], cc.cl[1]);
}

// bits and bit count of one token: a literal, or a match (length symbol, extra bits, distance code 0 = one zero bit)
SDPNG_HD uint32_t token_bits(const ChunkCodes& cc, int tok, uint8_t value, int* nbits) {
    if (tok == 1) { *nbits = cc.ll[value]; return cc.llcode[value]; }
    int eb, ev;
    const int sym = length_symbol(tok, &eb, &ev);
    *nbits = cc.ll[sym] + eb + 1;
    return (uint32_t)cc.llcode[sym] | ((uint32_t)ev << cc.ll[sym]);
}

// Adler-32 over chunks: (a, b) after a chunk of len bytes with sum(d) = A and sum((len - i) d_i) = Bsum, both already mod 65521
SDPNG_HD void adler_append(uint32_t& a, uint32_t& b, uint32_t len, uint32_t A, uint32_t Bsum) {
    b = (uint32_t)((b + (uint64_t)(len % kAdlerMod) * a + Bsum) % kAdlerMod);
    a = (a + A) % kAdlerMod;
}

// ---- workspace of the device route (png_gpu.hip)
constexpr size_t kSlot = kChunk + kChunkSlack;
struct Layout : sdarena::Walker {
    size_t n;                        // chunks of all frames
    Layout(int B, int h, int w) : n((size_t)B * num_chunks(h, w)) {}
    size_t slots = take(n * kSlot, 16);    // u8 [n][kSlot], 16-byte aligned: the coded chunks
    size_t offsets = take(n * 8, 8);       // u64 [n], 8: a chunk's offset inside its frame's stream
    size_t csize = take(n * 4, 4);         // u32 [n], 4: its coded size
    size_t adler_a = take(n * 4, 4);       // u32 [n], 4: its two Adler partials
    size_t adler_b = take(n * 4, 4);       // u32 [n], 4
    size_t slack = end();                  // 64 bytes of historical slack: nothing reads or writes them
    size_t total = end_with_slack(64);
};

}  // namespace sdpng
