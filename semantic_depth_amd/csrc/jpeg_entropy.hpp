// The entropy decoder of ONE restart interval of a sequential, interleaved Huffman JPEG scan, as ONE function compiled for both sides
// (jpeg_entropy_gpu.hip runs it one lane per interval, host_jpeg_entropy.cpp in a plain loop), and the argument checks both entry
// points make before they run it.  It takes the decisions of host_jpeg.cpp's block_store(): the same symbols, the same extend(), the
// DC predictors from 0, the same four refusals.  Plain C++17 without hipcc (scripts/fuzz_jpeg_entropy.cpp builds it with g++).
//
// Bounds, by construction: the reader fetches bytes of [begin, end) only and supplies zero bits past end (host_jpeg.cpp's BitReader does
// that at a marker); every store goes to a block index below the component's block count, which frame_ok() ties to the descriptor; every
// table index is bounded by table_ok() or by the width of the bit field that forms it.  Each index below says what bounds it.
#pragma once
#include "jpeg_common.hpp"

namespace sdjent {

constexpr int kTables = SD_JPEG_ENTROPY_TABLES;      // per frame: slots 0..3 the DC tables Td, slots 4..7 the AC tables 4 + Ta
enum Refusal : int { kOk = 0, kBadSymbol = 1, kBadDcCategory = 2, kBadPredictor = 3, kRunPast63 = 4 };

constexpr uint8_t kZigzag[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48,
                                 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// MSB-first bit reader over the bytes [pos, end) of `base` with the byte stuffing resolved on refill: FF 00 is the data byte FF; an FF
// followed by anything else, or by `end`, is a marker -- zero bits from there on, like the host's BitReader.  64-bit buffer, refilled
// when fewer than 33 bits are left, so a 16-bit peek and a 15-bit get are always served.
struct BitReader {
    const uint8_t* base;
    uint32_t pos, end;
    uint64_t acc = 0;
    int n = 0;
    bool hit = false;
#if defined(__HIP_DEVICE_COMPILE__)
    // the device fetches the aligned dword that holds byte i (i < end <= the frame's byte stride; base and the stride are multiples of
    // 16, which sd_jpeg_entropy_decode checks, so the dword lies inside the frame's bytes) and keeps it until the walk leaves it
    uint32_t word = 0, word_at = 0xffffffffu;
    SD_JPEG_HD inline uint32_t byte_at(uint32_t i) {
        if ((i >> 2) != word_at) { word_at = i >> 2; word = reinterpret_cast<const uint32_t*>(base)[word_at]; }
        return (word >> ((i & 3) * 8)) & 0xffu;
    }
#else
    SD_JPEG_HD inline uint32_t byte_at(uint32_t i) { return base[i]; }       // i < end: the callers below test it first
#endif
    SD_JPEG_HD BitReader(const uint8_t* b, uint32_t begin, uint32_t e) : base(b), pos(begin), end(e) {}
    SD_JPEG_HD inline void fill() {
        while (n <= 56) {
            uint32_t b = 0;
            if (!hit && pos < end) {
                b = byte_at(pos);                                              // pos < end
                if (b == 0xFFu) {
                    if (pos + 1 < end && byte_at(pos + 1) == 0) pos += 2;      // pos + 1 < end
                    else { hit = true; b = 0; }
                } else ++pos;
            }
            acc |= (uint64_t)b << (56 - n);
            n += 8;
        }
    }
    SD_JPEG_HD inline int peek(int k) { if (n < 33) fill(); return (int)(acc >> (64 - k)); }      // 1 <= k <= 16
    SD_JPEG_HD inline void skip(int k) { acc <<= k; n -= k; }                                      // k <= 16 <= n after a peek
    SD_JPEG_HD inline int get(int k) { if (!k) return 0; const int v = peek(k); skip(k); return v; }
};

SD_JPEG_HD inline int extend(int v, int t) { return v < (1 << (t - 1)) ? v - (1 << t) + 1 : v; }

// one Huffman symbol, or -1: host_jpeg.cpp's decode_sym() on the table's decodable form
SD_JPEG_HD inline int decode_sym(BitReader& br, const sd_jpeg_huff_table& h) {
    const int look = br.peek(9);                               // 9 bits: look < 512 = the entries of look[]
    const uint32_t e = h.look[look];
    if (e) { br.skip((int)(e >> 8)); return (int)(e & 0xff); } // table_ok(): 1 <= length <= 9
    const int code = br.peek(16);
    for (int l = 10; l <= 16; ++l) {                           // l indexes mincode / maxcode / valptr [17]
        const int c = code >> (16 - l);
        if (h.maxcode[l] >= 0 && c <= h.maxcode[l] && c >= h.mincode[l]) {
            br.skip(l);
            return h.vals[h.valptr[l] + c - h.mincode[l]];     // table_ok(): 0 <= valptr[l] and valptr[l] + maxcode[l] - mincode[l] <= 255
        }
    }
    return -1;
}

// Decodes restart interval `index` of the frame `fr` describes: the MCUs index * DRI .. of the scan (fewer in the last interval; an
// interval may begin and end inside an MCU row), from the bytes [begin, end) of `bytes`, into the frame's coefficient buffer `coef`
// laid out as sd_jpeg_decode_coefficients lays it out.  The buffer holds zeros where this interval's blocks go (the callers clear it);
// only non-zero coefficients are stored.  Returns kOk or the refusal; the caller flags the frame.
// The caller has checked frame_ok(fr, desc), index < fr.n_intervals, begin <= end, table_ok() of every table the frame names.
SD_JPEG_HD inline int decode_interval(const uint8_t* bytes, uint32_t begin, uint32_t end, const sd_jpeg_entropy_frame& fr,
                                      const sd_jpeg_huff_table* tables, int index, int16_t* coef) {
    BitReader br(bytes, begin, end);
    const int ncomp = fr.ncomp;                                // frame_ok(): 1 or 3
    const int64_t total = (int64_t)fr.mcus_x * fr.mcus_y;
    const int64_t first = (int64_t)index * fr.restart_interval;       // index < n_intervals = ceil(total / DRI): first < total
    const int64_t count = total - first < fr.restart_interval ? total - first : fr.restart_interval;
    int pred[3] = {0, 0, 0};
    int mx = (int)(first % fr.mcus_x), my = (int)(first / fr.mcus_x);         // my < mcus_y since first < total
    for (int64_t m = 0; m < count; ++m) {
        int64_t comp_off = 0;
        for (int c = 0; c < ncomp; ++c) {                      // c < 3: the extent of comp_h / comp_v / comp_dc / comp_ac
            const int ch = fr.comp_h[c], cv = fr.comp_v[c];    // frame_ok(): 1 or 2
            const int bw = fr.mcus_x * ch, bh = fr.mcus_y * cv;        // frame_ok(): the descriptor's blocks_w / blocks_h
            const sd_jpeg_huff_table& hd = tables[fr.comp_dc[c]];      // frame_ok(): 0..3
            const sd_jpeg_huff_table& ha = tables[4 + fr.comp_ac[c]];  // frame_ok(): 0..3, so the slot is 4..7 < kTables
            for (int v = 0; v < cv; ++v)
                for (int h = 0; h < ch; ++h) {
                    // bx < bw and by < bh because mx < mcus_x, h < ch, my < mcus_y, v < cv: the block lies inside the component, and
                    // comp_off + (by * bw + bx) * 64 + 63 < the descriptor's coef_elems, which the caller holds below the stride
                    const int bx = mx * ch + h, by = my * cv + v;
                    int16_t* blk = coef + comp_off + ((int64_t)by * bw + bx) * 64;
                    const int t = decode_sym(br, hd);
                    if (t < 0) return kBadSymbol;
                    if (t > 15) return kBadDcCategory;
                    pred[c] += t ? extend(br.get(t), t) : 0;
                    if (pred[c] < -32767 || pred[c] > 32767) return kBadPredictor;
                    if (pred[c]) blk[0] = (int16_t)pred[c];
                    for (int k = 1; k < 64;) {
                        const int rs = decode_sym(br, ha);
                        if (rs < 0) return kBadSymbol;
                        const int r = rs >> 4, s = rs & 15;
                        if (!s) { if (r == 15) { k += 16; continue; } break; }
                        k += r;
                        if (k > 63) return kRunPast63;
                        const int val = extend(br.get(s), s);
                        if (val) blk[kZigzag[k]] = (int16_t)val;       // k <= 63; kZigzag[] < 64: inside the block
                        ++k;
                    }
                }
            comp_off += (int64_t)bw * bh * 64;
        }
        if (++mx == fr.mcus_x) { mx = 0; ++my; }
    }
    return kOk;
}

// ---- the checks of sd_jpeg_entropy_decode / sd_jpeg_entropy_decode_host: nothing runs unless all of them hold ----

// a table Huff::build() could have produced, as far as the decoder's indices go
inline bool table_ok(const sd_jpeg_huff_table& t) {
    for (int i = 0; i < 512; ++i) {
        const int len = t.look[i] >> 8;
        if (t.look[i] && (len < 1 || len > 9)) return false;
    }
    for (int l = 1; l <= 16; ++l) {
        if (t.maxcode[l] < 0) continue;
        if (t.mincode[l] < 0 || t.mincode[l] > t.maxcode[l] || t.maxcode[l] >= (1 << l)) return false;
        if (t.valptr[l] < 0 || (int64_t)t.valptr[l] + t.maxcode[l] - t.mincode[l] > 255) return false;
    }
    return true;
}

// the record of an eligible frame agrees with its descriptor: the scan geometry is the descriptor's, so every block the decoder
// addresses exists in the descriptor's layout
inline bool frame_ok(const sd_jpeg_entropy_frame& fr, const sd_jpeg_frame_desc& d) {
    if (!sdjpeg::desc_ok(d) || fr.ncomp != d.ncomp) return false;
    if (fr.mcus_x != (d.width + 8 * d.hmax - 1) / (8 * d.hmax) || fr.mcus_y != (d.height + 8 * d.vmax - 1) / (8 * d.vmax)) return false;
    for (int i = 0; i < d.ncomp; ++i) {
        if (fr.comp_h[i] != (i ? 1 : d.hmax) || fr.comp_v[i] != (i ? 1 : d.vmax)) return false;
        if (fr.comp_dc[i] < 0 || fr.comp_dc[i] > 3 || fr.comp_ac[i] < 0 || fr.comp_ac[i] > 3) return false;
    }
    const int64_t total = (int64_t)fr.mcus_x * fr.mcus_y;
    if (fr.restart_interval < 1 || fr.restart_interval > 65535) return false;
    if (fr.n_intervals != (total + fr.restart_interval - 1) / fr.restart_interval) return false;
    return true;
}

// all of a call's arguments; `why` names the first violation
inline bool args_ok(size_t byte_stride, const sd_jpeg_frame_desc* descs, const sd_jpeg_entropy_frame* frames, const sd_jpeg_interval* intervals,
                    size_t interval_stride, const sd_jpeg_huff_table* tables, int B, size_t coef_stride_bytes, const char** why) {
    for (int b = 0; b < B; ++b) {
        const sd_jpeg_entropy_frame& fr = frames[b];
        if (!fr.eligible) continue;
        if (!frame_ok(fr, descs[b])) { *why = "a frame record disagrees with its descriptor"; return false; }
        if (sdjpeg::desc_coef_elems(descs[b]) * sizeof(int16_t) > coef_stride_bytes) { *why = "a frame has more coefficients than the coefficient stride"; return false; }
        if ((size_t)fr.n_intervals > interval_stride) { *why = "a frame has more intervals than interval_stride"; return false; }
        for (int i = 0; i < fr.n_intervals; ++i) {
            const sd_jpeg_interval& iv = intervals[(size_t)b * interval_stride + i];
            if (iv.begin > iv.end || iv.end > byte_stride) { *why = "an interval range leaves its frame's byte stride"; return false; }
        }
        for (int i = 0; i < fr.ncomp; ++i)
            if (!table_ok(tables[(size_t)b * kTables + fr.comp_dc[i]]) || !table_ok(tables[(size_t)b * kTables + 4 + fr.comp_ac[i]])) {
                *why = "a Huffman table is not in decodable form";
                return false;
            }
    }
    return true;
}

// ---- workspace of the device route (jpeg_entropy_gpu.hip): the launcher's three uploads, every part 16-byte aligned
struct Layout : sdarena::Walker {
    size_t B, stride;
    Layout(int B_, size_t interval_stride) : B((size_t)B_), stride(interval_stride) {}
    size_t frames = take(B * sizeof(sd_jpeg_entropy_frame), 16);
    size_t tables = take(B * kTables * sizeof(sd_jpeg_huff_table), 16);       // [B][kTables]
    size_t intervals = take(B * stride * sizeof(sd_jpeg_interval), 16);       // [B][interval_stride]
    size_t total = end(16);
};

}  // namespace sdjent
