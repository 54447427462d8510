// Self-synchronising decoding of a sequential, interleaved Huffman JPEG scan in short pieces, as ONE statement compiled for both sides
// (jpeg_sync_gpu.hip runs it a lane per piece, host_jpeg_sync.cpp runs the same lanes in a loop), and the argument checks both entry
// points make before they run it.  Plain C++17 without hipcc (scripts/fuzz_jpeg_sync.cpp builds it with g++).
//
// The decoder's state at a bit position is (p, u, k): bit position in the frame's CLEAN stream (stuffing resolved, RST markers dropped:
// the plan writes it), data unit inside the MCU, zigzag index (0: a DC symbol comes next).  step() advances it by one TOKEN (a Huffman
// code and its extra bits, at most 31 bits) and is the only place that reads bits; a token belongs to the piece in which it begins.
// step() never stops: where the true decoder refuses (the four refusals of sdjent::decode_interval) it reports the anomaly and carries
// on by a fixed rule, because a speculative lane in a wrong state meets anomalies the stream does not have and must live through them
// to fall into step.  The write pass turns an anomaly inside the interval's units into the frame's refusal.
//
// Passes (the lanes of each pass touch disjoint records, so their order inside a pass does not matter and the CPU loop predicts the GPU):
//   speculative   lane i decodes piece i from (u 0, k 0) -- the TRUE state for an interval's first piece -- and records the end state and
//                 the units completed; then, round by round inside its workgroup of kGroup pieces and inside its interval, it decodes
//                 the next piece from the state it holds, writes that piece's record and stops where the state it found there was
//                 already its own.  After the rounds a piece's record comes from the lowest lane that reached it.
//   across        lane g (workgroup g >= 1 whose first piece does not begin an interval) starts from the end record workgroup g - 1
//                 had after the speculative pass and walks workgroup g's pieces the same way.
//   placement     exclusive scan of the unit counts: a piece's first unit ordinal inside its interval.
//   write         lane i decodes piece i from the record of piece i - 1 (or the true start), stores the coefficients and DC DIFFERENCES
//                 of units below the interval's count, and verifies that it ends in the record of piece i.
//   DC            segmented inclusive scan of the differences per (interval, component) in decode order.
// Every equality the write pass checks, chained from the interval's true start, is the induction step of "this is the sequential
// decode"; so status 0 implies the sequential result whatever the speculative passes recorded.
//
// Bounds, by construction: the reader fetches bytes below the interval's end only (zero bits past it, as the host's BitReader supplies
// at a marker) and the end lies inside the frame's byte stride (args_ok()); a store goes to the block of a unit ordinal below the
// interval's unit count, which is a block of the descriptor's layout (frame_ok()); table indices as in jpeg_entropy.hpp; record
// indices are piece indices below the frame's n_pieces, which args_ok() holds below the record capacity.
#pragma once
#include "jpeg_entropy.hpp"
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

// step(), run_piece() and the lanes' entry points are inlined into the kernels, so that the reader and the state live in registers there
#if defined(__HIPCC__)
#define SD_SYNC_FN __host__ __device__ __forceinline__
#else
#define SD_SYNC_FN inline
#endif

namespace sdjsync {

using sdjent::kTables;
constexpr int kNotSynchronised = SD_JPEG_SYNC_NOT_SYNCHRONISED, kBitsRanOut = SD_JPEG_SYNC_BITS_RAN_OUT;
constexpr int kGroup = SD_JPEG_SYNC_GROUP;

// MSB-first reader over the clean stream: bytes below `end` only, zero bytes from there on.  bit() is the position of the next bit.
struct Reader {
    const uint8_t* base;
    uint32_t pos, end;            // pos counts the zero bytes supplied past end as well
    uint64_t acc = 0;
    int n = 0;
#if defined(__HIP_DEVICE_COMPILE__)
    // the device fetches the aligned 8 bytes that hold byte i (i < end <= the frame's byte stride; base and the stride are multiples of
    // 16, which sd_jpeg_sync_decode checks) and keeps them until the walk leaves them.  (Aligned 16-byte pieces were tried first: picking
    // one of four kept dwords by the byte index became an indexed access and put the reader into scratch; a shift of one 64-bit word
    // does not.)
    uint64_t word = 0;
    uint32_t word_at = 0xffffffffu;
    SD_SYNC_FN uint32_t byte_at(uint32_t i) {
        if ((i >> 3) != word_at) { word_at = i >> 3; word = reinterpret_cast<const uint64_t*>(base)[word_at]; }
        return (uint32_t)(word >> ((i & 7) * 8)) & 0xffu;
    }
#else
    SD_SYNC_FN uint32_t byte_at(uint32_t i) { return base[i]; }       // i < end
#endif
    // starts at bit position p (p <= 8 * end + 64, see step())
    SD_SYNC_FN Reader(const uint8_t* b, uint32_t p, uint32_t e) : base(b), pos(p >> 3), end(e) {
        fill();
        skip((int)(p & 7));
    }
    SD_SYNC_FN void fill() {
        while (n <= 56) {
            const uint32_t b = pos < end ? byte_at(pos) : 0u;
            ++pos;
            acc |= (uint64_t)b << (56 - n);
            n += 8;
        }
    }
    SD_SYNC_FN int peek(int k) { if (n < 33) fill(); return (int)(acc >> (64 - k)); }      // 1 <= k <= 16
    SD_SYNC_FN void skip(int k) { acc <<= k; n -= k; }                                      // k <= 16 <= n after a peek
    SD_SYNC_FN int get(int k) { if (!k) return 0; const int v = peek(k); skip(k); return v; }
    SD_SYNC_FN uint32_t bit() const { return pos * 8u - (uint32_t)n; }
};

struct State {
    uint32_t p;
    int u, k;                     // u < units per MCU, k 0..63
};
SD_JPEG_HD inline bool same(const State& a, const State& b) { return a.p == b.p && a.u == b.u && a.k == b.k; }

// a piece's record: its end state and the data units completed by the tokens that begin in it
struct Rec {
    uint32_t p, uk, n, pad;       // uk = u << 8 | k
};
SD_JPEG_HD inline Rec pack(const State& s, uint32_t n) { return Rec{s.p, (uint32_t)s.u << 8 | (uint32_t)s.k, n, 0u}; }
SD_JPEG_HD inline State unpack(const Rec& r) { return State{r.p, (int)(r.uk >> 8), (int)(r.uk & 255u)}; }

SD_JPEG_HD inline int luma_units(const sd_jpeg_sync_frame& fr) { return fr.comp_h[0] * fr.comp_v[0]; }                 // frame_ok(): 1, 2 or 4
SD_JPEG_HD inline int units_per_mcu(const sd_jpeg_sync_frame& fr) { return fr.ncomp == 1 ? 1 : luma_units(fr) + 2; }   // <= 6
SD_JPEG_HD inline int unit_comp(const sd_jpeg_sync_frame& fr, int u) {                                                 // u < units per MCU: 0..ncomp-1
    const int l = luma_units(fr);
    return u < l ? 0 : 1 + u - l;
}

// one Huffman symbol, or -1: sdjent::decode_sym() on this file's reader
SD_SYNC_FN int decode_sym(Reader& br, const sd_jpeg_huff_table& h) {
    const uint32_t e = h.look[br.peek(9)];                     // 9 bits: below the 512 entries of look[]
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

// One token from state s.  The sink hears coefficient(zigzag index, value), unit_done() and anomaly(code).  THE CARRY-ON RULE, one for
// both sides (which frames get flagged depends on it): an unassigned code skips 16 bits and keeps (u, k); a DC category above 15 counts
// as category 0; a run past coefficient 63 takes its extra bits and closes the block.  Every call consumes at least one bit.
template <class Sink>
SD_SYNC_FN void step(Reader& br, const sd_jpeg_sync_frame& fr, const sd_jpeg_huff_table* tables, State& s, Sink& sink) {
    const int c = unit_comp(fr, s.u);                                  // c < 3: the extent of comp_dc / comp_ac
    bool done = false;
    if (s.k == 0) {
        int t = decode_sym(br, tables[fr.comp_dc[c]]);         // frame_ok(): slot 0..3
        if (t < 0) { sink.anomaly(sdjent::kBadSymbol); br.skip(16); s.p = br.bit(); return; }
        if (t > 15) { sink.anomaly(sdjent::kBadDcCategory); t = 0; }
        sink.coefficient(0, t ? sdjent::extend(br.get(t), t) : 0);
        s.k = 1;
    } else {
        const int rs = decode_sym(br, tables[4 + fr.comp_ac[c]]);      // slot 4..7 < kTables
        if (rs < 0) { sink.anomaly(sdjent::kBadSymbol); br.skip(16); s.p = br.bit(); return; }
        const int r = rs >> 4, sz = rs & 15;
        if (!sz) {
            if (r == 15) { s.k += 16; done = s.k > 63; }               // (a ZRL that leaves the block ends it, as block_store()'s loop does)
            else done = true;
        } else {
            s.k += r;
            const int v = sdjent::extend(br.get(sz), sz);
            if (s.k > 63) { sink.anomaly(sdjent::kRunPast63); done = true; }
            else { sink.coefficient(s.k, v); done = ++s.k > 63; }
        }
    }
    if (done) {
        s.k = 0;
        if (++s.u == units_per_mcu(fr)) s.u = 0;
        sink.unit_done();
    }
    s.p = br.bit();
}

// every token that begins before bit `end_bit` (a piece's end), from state s; reads bytes below iv_end.  s.p <= end_bit + 30 going in
// (a record's position, or a piece's begin) and coming out.  Bounded: each step() moves p by at least one bit.
template <class Sink>
SD_SYNC_FN void run_piece(const uint8_t* bytes, uint32_t iv_end, uint32_t end_bit, const sd_jpeg_sync_frame& fr,
                                 const sd_jpeg_huff_table* tables, State& s, Sink& sink) {
    if (s.p >= end_bit) return;
    Reader br(bytes, s.p, iv_end);
    while (s.p < end_bit) step(br, fr, tables, s, sink);
}

// the speculative passes only count
struct CountSink {
    uint32_t units = 0;
    SD_JPEG_HD inline void coefficient(int, int) {}
    SD_JPEG_HD inline void anomaly(int) {}
    SD_JPEG_HD inline void unit_done() { ++units; }
};

// int16 offset of the block of unit ordinal q of the interval that begins at MCU `first_mcu`.  The caller holds q below the interval's unit
// count, so the MCU is below mcus_x * mcus_y and the block lies inside its component (as in sdjent::decode_interval).
SD_JPEG_HD inline int64_t unit_block(const sd_jpeg_sync_frame& fr, int64_t first_mcu, int64_t q) {
    const int upm = units_per_mcu(fr), l = luma_units(fr);
    const int64_t m = first_mcu + q / upm;
    const int u = (int)(q % upm);
    const int64_t mx = m % fr.mcus_x, my = m / fr.mcus_x, mcus = (int64_t)fr.mcus_x * fr.mcus_y;
    if (u < l) {
        const int ch = fr.comp_h[0], cv = fr.comp_v[0];
        return ((my * cv + u / ch) * ((int64_t)fr.mcus_x * ch) + mx * ch + u % ch) * 64;
    }
    return (mcus * l + (u - l) * mcus + my * fr.mcus_x + mx) * 64;
}

// the write pass's sink: stores into the cleared coefficients while the unit ordinal is below the interval's count, and keeps the first
// anomaly met there
struct WriteSink {
    const sd_jpeg_sync_frame& fr;
    int16_t* coef;
    int64_t first_mcu, q, limit;
    int16_t* blk = nullptr;
    int refusal = 0;
    uint32_t units = 0;
    SD_JPEG_HD WriteSink(const sd_jpeg_sync_frame& f, int16_t* c, int64_t first, int64_t q0, int64_t lim) : fr(f), coef(c), first_mcu(first), q(q0), limit(lim) { place(); }
    SD_JPEG_HD inline void place() { blk = q < limit ? coef + unit_block(fr, first_mcu, q) : nullptr; }
    SD_JPEG_HD inline void coefficient(int k, int v) { if (blk && v) blk[sdjent::kZigzag[k]] = (int16_t)v; }     // k <= 63; |v| <= 32767
    SD_JPEG_HD inline void anomaly(int code) { if (blk && !refusal) refusal = code; }
    SD_JPEG_HD inline void unit_done() { ++units; ++q; place(); }
};

// ---- where a piece lies ----
struct Piece {
    uint32_t iv;                  // its interval
    uint32_t begin_bit, end_bit;  // of the piece
    uint32_t iv_end;              // byte
    uint32_t iv_first, iv_last;   // the interval's first and last piece
};
SD_JPEG_HD inline uint32_t piece_end_bit(const sd_jpeg_sync_interval& v, uint32_t piece, uint32_t S) {
    const uint64_t e = (uint64_t)v.begin + (uint64_t)(piece - v.first_piece + 1) * S;
    return (uint32_t)(e < v.end ? e : v.end) * 8u;
}
// piece < n_pieces; ivs[0].first_piece is 0 and first_piece grows strictly (args_ok()), so the search ends on the piece's interval
SD_SYNC_FN Piece locate(const sd_jpeg_sync_interval* ivs, int n_iv, uint32_t n_pieces, uint32_t piece, uint32_t S) {
    int lo = 0, hi = n_iv - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (ivs[mid].first_piece <= piece) lo = mid; else hi = mid - 1;
    }
    const sd_jpeg_sync_interval v = ivs[lo];
    Piece pc;
    pc.iv = (uint32_t)lo;
    const uint64_t b = (uint64_t)v.begin + (uint64_t)(piece - v.first_piece) * S;
    pc.begin_bit = (uint32_t)(b < v.end ? b : v.end) * 8u;
    pc.end_bit = piece_end_bit(v, piece, S);
    pc.iv_end = v.end;
    pc.iv_first = v.first_piece;
    pc.iv_last = (lo + 1 < n_iv ? ivs[lo + 1].first_piece : n_pieces) - 1;
    return pc;
}

SD_JPEG_HD inline int64_t interval_mcus(const sd_jpeg_sync_frame& fr, uint32_t iv) {
    const int64_t total = (int64_t)fr.mcus_x * fr.mcus_y, first = (int64_t)iv * fr.restart_interval;
    return total - first < fr.restart_interval ? total - first : fr.restart_interval;
}

// ---- the lanes of the passes, as the kernels and the host loop call them ----

// speculative pass, round 0
SD_SYNC_FN Rec spec_first(const uint8_t* bytes, const sd_jpeg_sync_frame& fr, const sd_jpeg_huff_table* tables, const Piece& pc, State& s) {
    s = State{pc.begin_bit, 0, 0};
    CountSink sink;
    run_piece(bytes, pc.iv_end, pc.end_bit, fr, tables, s, sink);
    return pack(s, sink.units);
}
// one further piece (of the same interval) from the state the lane holds; *stop: the record it found there already held that state
SD_SYNC_FN Rec walk_on(const uint8_t* bytes, const sd_jpeg_sync_frame& fr, const sd_jpeg_huff_table* tables, const sd_jpeg_sync_interval& v,
                              uint32_t piece, uint32_t S, State& s, const Rec& found, bool* stop) {
    CountSink sink;
    run_piece(bytes, v.end, piece_end_bit(v, piece, S), fr, tables, s, sink);
    *stop = same(s, unpack(found));
    return pack(s, sink.units);
}

// write pass: piece `piece` from `start`, its first unit ordinal q0; returns 0 or the lane's code for the frame
SD_SYNC_FN int write_piece(const uint8_t* bytes, const sd_jpeg_sync_frame& fr, const sd_jpeg_huff_table* tables, const Piece& pc, uint32_t piece,
                                  State s, int64_t q0, const Rec& own, int16_t* coef) {
    const int64_t limit = interval_mcus(fr, pc.iv) * units_per_mcu(fr);
    WriteSink sink(fr, coef, (int64_t)pc.iv * fr.restart_interval, q0, limit);
    run_piece(bytes, pc.iv_end, pc.end_bit, fr, tables, s, sink);
    if (sink.refusal) return sink.refusal;
    if (!same(s, unpack(own)) || sink.units != own.n) return kNotSynchronised;
    if (piece == pc.iv_last && sink.q < limit) return kBitsRanOut;
    return 0;
}

// DC pass: component c's blocks in decode order.  j < mcus * h * v: the int16 offset of block j and whether it begins an interval.
SD_JPEG_HD inline int64_t dc_blocks(const sd_jpeg_sync_frame& fr, int c) { return (int64_t)fr.mcus_x * fr.mcus_y * fr.comp_h[c] * fr.comp_v[c]; }
SD_JPEG_HD inline int64_t dc_block(const sd_jpeg_sync_frame& fr, int c, int64_t j, bool* head) {
    const int per = fr.comp_h[c] * fr.comp_v[c];
    const int64_t m = j / per;
    const int r = (int)(j % per);
    *head = r == 0 && m % fr.restart_interval == 0;
    const int l = luma_units(fr);
    return unit_block(fr, 0, m * units_per_mcu(fr) + (c ? l + c - 1 : r));
}

// ---- the checks of sd_jpeg_sync_decode / sd_jpeg_sync_decode_host: nothing runs unless all of them hold ----

inline bool subseq_ok(int S) { return S >= 32 && S <= 1024 && (S & (S - 1)) == 0; }
constexpr size_t kMaxBytes = (size_t)1 << 28;         // bit positions and unit counts stay inside 32 bits

inline bool frame_ok(const sd_jpeg_sync_frame& fr, const sd_jpeg_frame_desc& d) {
    if (!sdjpeg::desc_ok(d) || fr.ncomp != d.ncomp) return false;
    if (fr.mcus_x != (d.width + 8 * d.hmax - 1) / (8 * d.hmax) || fr.mcus_y != (d.height + 8 * d.vmax - 1) / (8 * d.vmax)) return false;
    for (int i = 0; i < d.ncomp; ++i) {
        if (fr.comp_h[i] != (i ? 1 : d.hmax) || fr.comp_v[i] != (i ? 1 : d.vmax)) return false;
        if (fr.comp_dc[i] < 0 || fr.comp_dc[i] > 3 || fr.comp_ac[i] < 0 || fr.comp_ac[i] > 3) return false;
    }
    const int64_t total = (int64_t)fr.mcus_x * fr.mcus_y;
    if (fr.restart_interval < 1) return false;
    if (fr.n_intervals != (total + fr.restart_interval - 1) / fr.restart_interval) return false;
    return true;
}

inline uint32_t interval_pieces(uint32_t begin, uint32_t end, uint32_t S) { return end > begin ? (end - begin + S - 1) / S : 1u; }

// all of a call's arguments; `why` names the first violation
inline bool args_ok(size_t byte_stride, const sd_jpeg_frame_desc* descs, const sd_jpeg_sync_frame* frames, const sd_jpeg_sync_interval* intervals,
                    size_t interval_stride, const sd_jpeg_huff_table* tables, int B, int S, size_t coef_stride_bytes, const char** why) {
    if (!subseq_ok(S)) { *why = "subseq_bytes is no power of two from 32 to 1024"; return false; }
    if (byte_stride >= kMaxBytes) { *why = "byte_stride of 256 MiB or more"; return false; }
    for (int b = 0; b < B; ++b) {
        const sd_jpeg_sync_frame& fr = frames[b];
        if (!fr.eligible) continue;
        if (!frame_ok(fr, descs[b])) { *why = "a frame record disagrees with its descriptor"; return false; }
        if (fr.subseq_bytes != (uint32_t)S) { *why = "a frame was planned with another subseq_bytes"; return false; }
        if (sdjpeg::desc_coef_elems(descs[b]) * sizeof(int16_t) > coef_stride_bytes) { *why = "a frame has more coefficients than the coefficient stride"; return false; }
        if ((size_t)fr.n_intervals > interval_stride) { *why = "a frame has more intervals than interval_stride"; return false; }
        if (fr.clean_bytes > byte_stride) { *why = "a frame's clean stream leaves its byte stride"; return false; }
        uint64_t piece = 0;
        for (int i = 0; i < fr.n_intervals; ++i) {
            const sd_jpeg_sync_interval& iv = intervals[(size_t)b * interval_stride + i];
            if (iv.begin > iv.end || iv.end > fr.clean_bytes) { *why = "an interval range leaves its frame's clean stream"; return false; }
            if (iv.first_piece != piece) { *why = "an interval's first piece does not follow from the ranges"; return false; }
            piece += interval_pieces(iv.begin, iv.end, (uint32_t)S);
        }
        if (piece != fr.n_pieces) { *why = "a frame's piece count does not follow from the ranges"; return false; }
        for (int i = 0; i < fr.ncomp; ++i)
            if (!sdjent::table_ok(tables[(size_t)b * kTables + fr.comp_dc[i]]) || !sdjent::table_ok(tables[(size_t)b * kTables + 4 + fr.comp_ac[i]])) {
                *why = "a Huffman table is not in decodable form";
                return false;
            }
    }
    return true;
}

// ---- workspace of the device route (jpeg_sync_gpu.hip) for frames of at most P pieces, P = max_pieces rounded up to whole workgroups of
// kGroup (at least one); every part 16-byte aligned
inline size_t piece_stride(size_t max_pieces) {
    const size_t g = kGroup;
    return (max_pieces < 1 ? 1 : (max_pieces + g - 1) / g) * g;
}
struct Layout : sdarena::Walker {
    size_t B, stride, P;
    Layout(int B_, size_t interval_stride, size_t max_pieces) : B((size_t)B_), stride(interval_stride), P(piece_stride(max_pieces)) {}
    size_t frames = take(B * sizeof(sd_jpeg_sync_frame), 16);                     // the launcher's three uploads
    size_t tables = take(B * kTables * sizeof(sd_jpeg_huff_table), 16);           // [B][kTables]
    size_t intervals = take(B * stride * sizeof(sd_jpeg_sync_interval), 16);      // [B][interval_stride]
    size_t rec = take(B * P * sizeof(Rec), 16);                                   // Rec [B][P]: the pieces' records
    size_t group_end = take(B * (P / kGroup) * sizeof(Rec), 16);                  // Rec [B][P / kGroup]: the workgroups' end records
    size_t before = take(B * P * sizeof(uint32_t), 16);                           // u32 [B][P]: the unit ordinals
    size_t total = end(16);
};

}  // namespace sdjsync
