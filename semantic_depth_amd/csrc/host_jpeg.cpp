// Host-side baseline JPEG reader of the input stage: the frames of the reference's own example are JPEGs
// (assets/images/test_munich/test_3.jpg, read by cv2.imread at semantic_depth.py:105).  cv2.imread decodes with libjpeg(-turbo) at its
// default settings and then applies the EXIF orientation; this file restates that path for baseline / extended-sequential Huffman JPEGs
// and progressive Huffman JPEGs (SOF0 / SOF1 / SOF2 -- test_3.jpg is progressive --, 8-bit, 1 or 3 components, sampling 1x1, 2x1,
// 2x2 for the chroma: what cameras and OpenCV itself write):
//   * entropy decoding per ITU T.81 (Huffman, byte stuffing, restart intervals, interleaved and single-component scans)
//   * inverse DCT = libjpeg's jidctint.c "ISLOW" integer transform (CONST_BITS 13, PASS1_BITS 2), the default dct_method
//   * chroma upsampling = libjpeg's "fancy" triangle filters (h2v1_fancy_upsample / h2v2_fancy_upsample), the default
//   * YCbCr -> RGB = jdcolor.c's 16-bit fixed-point tables
//   * EXIF orientation 1..8 as OpenCV's ExifTransform applies it (cv2.imread without IMREAD_IGNORE_ORIENTATION)
// Output: u8 [height, width, 3] BGR.  Pinned in tests/test_frame_io.py against Pillow (libjpeg-turbo, same defaults) bit for bit.
// Arithmetic-coded, lossless, 12-bit, CMYK and other sampling ratios are refused with SD_ERR_INVALID.
#include "../../include/semdepth.h"
#include "jpeg_common.hpp"

#include <cstdint>
#include <cstring>
#include <vector>

namespace {

const uint8_t kZigzag[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct Huff {
    bool present = false;
    uint8_t bits[17] = {0};
    uint8_t vals[256] = {0};
    // canonical decoding tables (T.81 F.2.2.3)
    int mincode[17], maxcode[18], valptr[17];
    uint16_t look[512];      // 9-bit lookahead: (length << 8) | symbol, 0 = longer than 9 bits
    // false when the code-length counts do not form a prefix code (libjpeg's JERR_BAD_HUFF_TABLE: more codes of length l than 2^l
    // leaves free) -- an over-subscribed table would index look[] past its 512 entries
    bool build() {
        int code = 0, k = 0;
        for (int l = 1; l <= 16; ++l) {
            valptr[l] = k;
            mincode[l] = code;
            code += bits[l];
            k += bits[l];
            if (code > (1 << l) || k > 256) { present = false; return false; }
            maxcode[l] = bits[l] ? code - 1 : -1;
            code <<= 1;
        }
        maxcode[17] = 0x7fffffff;
        std::memset(look, 0, sizeof(look));
        code = 0; k = 0;
        for (int l = 1; l <= 9; ++l) {
            for (int i = 0; i < bits[l]; ++i, ++k, ++code) {
                const int first = code << (9 - l), n = 1 << (9 - l);
                if (first + n > 512) { present = false; return false; }
                for (int j = 0; j < n; ++j) look[first + j] = (uint16_t)((l << 8) | vals[k]);
            }
            code <<= 1;
        }
        return true;
    }
};

struct Comp {
    int id = 0, h = 1, v = 1, tq = 0, td = 0, ta = 0;
    int bw = 0, bh = 0;            // blocks per row / column of the padded plane
    int pw = 0, ph = 0;            // padded plane size in samples
    int dw = 0, dh = 0;            // downsampled (real) size in samples
    int pred = 0;
    std::vector<uint8_t> plane;
    std::vector<int16_t> coef;     // progressive: quantised coefficients of every block (natural order), accumulated over the scans
    int16_t* cf = nullptr;         // where the scans accumulate: coef.data(), or this component's part of the caller's buffer (coefficient route)
};

struct BitReader {
    const uint8_t* p; const uint8_t* end;
    uint32_t acc = 0; int n = 0;
    bool hit_marker = false;
    void reset() { acc = 0; n = 0; hit_marker = false; }
    inline void fill() {
        while (n <= 24) {
            int b = 0;
            if (!hit_marker && p < end) {
                b = *p;
                if (b == 0xFF) {
                    if (p + 1 < end && p[1] == 0x00) { p += 2; }
                    else { hit_marker = true; b = 0; }          // a marker: feed zeros, leave p on the 0xFF
                } else ++p;
            }
            acc |= (uint32_t)b << (24 - n);
            n += 8;
        }
    }
    inline int peek(int k) { if (n < k) fill(); return (int)(acc >> (32 - k)); }
    inline void skip(int k) { acc <<= k; n -= k; }
    inline int get(int k) { if (!k) return 0; const int v = peek(k); skip(k); return v; }
};

inline int extend(int v, int t) { return v < (1 << (t - 1)) ? v - (1 << t) + 1 : v; }

inline int decode_sym(BitReader& br, const Huff& h) {
    const int look = br.peek(9);
    const uint16_t e = h.look[look];
    if (e) { br.skip(e >> 8); return e & 0xff; }
    int code = br.peek(16);
    for (int l = 10; l <= 16; ++l) {
        const int c = code >> (16 - l);
        if (h.maxcode[l] >= 0 && c <= h.maxcode[l] && c >= h.mincode[l]) { br.skip(l); return h.vals[h.valptr[l] + c - h.mincode[l]]; }
    }
    return -1;
}

using sdjpeg::idct_islow;       // jpeg_common.hpp: the one inverse DCT of the host and the device route

inline uint16_t rd16(const uint8_t* p) { return (uint16_t)((p[0] << 8) | p[1]); }

// EXIF orientation (TIFF tag 0x0112) of an APP1 "Exif\0\0" segment; 1 when absent / unreadable
int exif_orientation(const uint8_t* seg, size_t n) {
    if (n < 14 || std::memcmp(seg, "Exif\0\0", 6) != 0) return 1;
    const uint8_t* t = seg + 6;
    const size_t tn = n - 6;
    bool le;
    if (t[0] == 'I' && t[1] == 'I') le = true; else if (t[0] == 'M' && t[1] == 'M') le = false; else return 1;
    auto r16 = [&](size_t o) -> uint32_t { return o + 2 > tn ? 0u : (le ? (uint32_t)(t[o] | (t[o + 1] << 8)) : (uint32_t)((t[o] << 8) | t[o + 1])); };
    auto r32 = [&](size_t o) -> uint32_t {
        if (o + 4 > tn) return 0u;
        return le ? (uint32_t)(t[o] | (t[o + 1] << 8) | (t[o + 2] << 16) | ((uint32_t)t[o + 3] << 24))
                  : (uint32_t)(((uint32_t)t[o] << 24) | (t[o + 1] << 16) | (t[o + 2] << 8) | t[o + 3]);
    };
    if (r16(2) != 42) return 1;
    const size_t ifd = r32(4);
    const uint32_t cnt = r16(ifd);
    for (uint32_t i = 0; i < cnt; ++i) {
        const size_t e = ifd + 2 + 12 * (size_t)i;
        if (e + 12 > tn) break;
        if (r16(e) == 0x0112) {
            const uint32_t v = r16(e + 8);
            return (v >= 1 && v <= 8) ? (int)v : 1;
        }
    }
    return 1;
}

struct Decoder {
    const uint8_t* f; size_t len;
    int W = 0, H = 0, ncomp = 0, hmax = 1, vmax = 1, restart = 0, orientation = 1, adobe_transform = -1;
    bool sof = false, progressive = false;
    uint16_t qt[4][64] = {};
    bool qt_ok[4] = {false, false, false, false};
    Huff dc[4], ac[4];
    Comp comp[3];

    sd_status header_only(int* h_out, int* w_out) { const sd_status st = parse(false); if (st == SD_OK) dims(h_out, w_out); return st; }
    void dims(int* h_out, int* w_out) const {
        const bool swap = orientation >= 5;
        if (h_out) *h_out = swap ? W : H;
        if (w_out) *w_out = swap ? H : W;
    }

    size_t cap_bytes = 0;                                  // capacity of the caller's output buffer (checked at the frame header)
    // coefficient route (sd_jpeg_decode_coefficients): the blocks' quantised coefficients go to the caller's buffer, no plane exists
    int16_t* coef_ext = nullptr;
    bool allocated = false;
    uint16_t qt_used[3][64] = {};                          // the table each component's coefficients are to be multiplied by
    bool scanned[3] = {false, false, false};               // sequential file: a scan has covered the component
    const uint8_t* sos = nullptr; size_t sos_len = 0, sos_data = 0;      // the first SOS: its header, and the file offset of its entropy data

    void geometry() {
        for (int i = 0; i < ncomp; ++i) {
            Comp& c = comp[i];
            c.bw = sdjpeg::blocks_w(W, hmax, c.h); c.bh = sdjpeg::blocks_h(H, vmax, c.v);
            c.pw = c.bw * 8; c.ph = c.bh * 8;
            c.dw = (W * c.h + hmax - 1) / hmax; c.dh = (H * c.v + vmax - 1) / vmax;
        }
    }
    size_t coef_elems() const {
        size_t n = 0;
        for (int i = 0; i < ncomp; ++i) n += (size_t)comp[i].bw * comp[i].bh * 64;
        return n;
    }
    void fill_desc(sd_jpeg_frame_desc* d) const {
        std::memset(d, 0, sizeof(*d));
        d->height = H; d->width = W; d->ncomp = ncomp; d->hmax = hmax; d->vmax = vmax;
        d->orientation = orientation; d->adobe_transform = adobe_transform;
        int64_t off = 0;
        for (int i = 0; i < ncomp; ++i) {
            d->blocks_w[i] = comp[i].bw; d->blocks_h[i] = comp[i].bh; d->coef_offset[i] = off;
            off += (int64_t)comp[i].bw * comp[i].bh * 64;
            std::memcpy(d->qt[i], qt_used[i], sizeof(qt_used[i]));
        }
    }
    sd_status parse(bool decode) {
        if (len < 4 || f[0] != 0xFF || f[1] != 0xD8) return SD_ERR_INVALID;
        size_t p = 2;
        while (p + 4 <= len) {
            if (f[p] != 0xFF) return SD_ERR_INVALID;
            while (p < len && f[p] == 0xFF) ++p;             // fill bytes
            if (p >= len) return SD_ERR_INVALID;
            const int m = f[p++];
            if (m == 0xD9) break;                            // EOI
            if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;
            if (p + 2 > len) return SD_ERR_INVALID;
            const size_t n = rd16(f + p);
            if (n < 2 || p + n > len) return SD_ERR_INVALID;
            const uint8_t* s = f + p + 2;
            const size_t sn = n - 2;
            if (m == 0xDB) {                                 // DQT
                size_t o = 0;
                while (o < sn) {
                    const int pq = s[o] >> 4, tq = s[o] & 15;
                    ++o;
                    if (tq > 3 || o + (pq ? 128 : 64) > sn) return SD_ERR_INVALID;
                    for (int i = 0; i < 64; ++i) { qt[tq][kZigzag[i]] = pq ? rd16(s + o + 2 * i) : s[o + i]; }
                    o += pq ? 128 : 64;
                    qt_ok[tq] = true;
                }
            } else if (m == 0xC4) {                          // DHT
                size_t o = 0;
                while (o + 17 <= sn) {
                    const int tc = s[o] >> 4, th = s[o] & 15;
                    if (tc > 1 || th > 3) return SD_ERR_INVALID;
                    Huff& h = tc ? ac[th] : dc[th];
                    int total = 0;
                    h.bits[0] = 0;
                    for (int i = 1; i <= 16; ++i) { h.bits[i] = s[o + i]; total += s[o + i]; }
                    o += 17;
                    if (total > 256 || o + total > sn) return SD_ERR_INVALID;
                    std::memcpy(h.vals, s + o, (size_t)total);
                    o += total;
                    h.present = true;
                    if (!h.build()) return SD_ERR_INVALID;
                }
            } else if (m == 0xC0 || m == 0xC1 || m == 0xC2) {     // SOF0 / SOF1 / SOF2: baseline / extended sequential / progressive, Huffman
                if (sof) return SD_ERR_INVALID;                  // one frame header per file: a second one would re-shape planes already allocated
                progressive = m == 0xC2;
                hmax = vmax = 1;
                if (sn < 6 || s[0] != 8) return SD_ERR_INVALID;
                H = rd16(s + 1); W = rd16(s + 3); ncomp = s[5];
                if (H <= 0 || W <= 0 || (ncomp != 1 && ncomp != 3) || sn < 6 + 3 * (size_t)ncomp) return SD_ERR_INVALID;
                if ((size_t)H * (size_t)W > ((size_t)1 << 28)) return SD_ERR_INVALID;      // (256 Mpixel: refuse absurd headers before allocating planes)
                if (decode && !coef_ext && cap_bytes < (size_t)H * W * 3) return SD_ERR_INVALID;       // the caller's buffer bounds what a header can make us allocate
                for (int i = 0; i < ncomp; ++i) {
                    comp[i].id = s[6 + 3 * i]; comp[i].h = s[7 + 3 * i] >> 4; comp[i].v = s[7 + 3 * i] & 15; comp[i].tq = s[8 + 3 * i];
                    if (comp[i].h < 1 || comp[i].v < 1 || comp[i].tq > 3) return SD_ERR_INVALID;
                    hmax = comp[i].h > hmax ? comp[i].h : hmax; vmax = comp[i].v > vmax ? comp[i].v : vmax;
                }
                if (ncomp == 1) { comp[0].h = comp[0].v = 1; hmax = vmax = 1; }
                else {
                    // luma at the full rate, both chroma planes at 1x1 of (1x1 | 2x1 | 2x2): what the fancy upsamplers cover
                    if (comp[0].h != hmax || comp[0].v != vmax || comp[1].h != 1 || comp[1].v != 1 || comp[2].h != 1 || comp[2].v != 1) return SD_ERR_INVALID;
                    if (!((hmax == 1 && vmax == 1) || (hmax == 2 && vmax == 1) || (hmax == 2 && vmax == 2))) return SD_ERR_INVALID;
                }
                geometry();
                if (decode && coef_ext && cap_bytes < coef_elems() * sizeof(int16_t)) return SD_ERR_INVALID;      // (the same bound on the coefficient route)
                sof = true;
                if (!decode) { /* keep scanning for APP1 only until SOS */ }
            } else if (m >= 0xC3 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC) {
                return SD_ERR_INVALID;                       // lossless / differential / arithmetic
            } else if (m == 0xDD) {                          // DRI
                if (sn < 2) return SD_ERR_INVALID;
                restart = rd16(s);
            } else if (m == 0xE1) {                          // APP1: EXIF
                const int o = exif_orientation(s, sn);
                if (o != 1) orientation = o;
            } else if (m == 0xEE) {                          // APP14 Adobe: colour transform flag
                if (sn >= 12 && std::memcmp(s, "Adobe", 5) == 0) adobe_transform = s[11];
            } else if (m == 0xDA) {                          // SOS
                if (!sof) return SD_ERR_INVALID;
                sos = s; sos_len = sn; sos_data = p + n;         // (the entropy plan reads the scan header from here)
                if (!decode) return SD_OK;
                size_t next = 0;
                const sd_status st = scan(s, sn, p + n, next);
                if (st != SD_OK) return st;
                p = next;
                continue;
            }
            p += n;
        }
        return sof ? SD_OK : SD_ERR_INVALID;
    }

    void alloc_planes() {
        if (allocated) return;
        allocated = true;
        if (coef_ext) {                                    // no plane: every block of the padded planes starts as zeros in the caller's buffer
            size_t off = 0;
            for (int i = 0; i < ncomp; ++i) { comp[i].cf = coef_ext + off; off += (size_t)comp[i].bw * comp[i].bh * 64; }
            std::memset(coef_ext, 0, off * sizeof(int16_t));
            return;
        }
        for (int i = 0; i < ncomp; ++i) {
            Comp& c = comp[i];
            c.plane.assign((size_t)c.pw * c.ph, 0);
            if (progressive) { c.coef.assign((size_t)c.bw * c.bh * 64, 0); c.cf = c.coef.data(); }
        }
    }

    // ---- progressive scans (T.81 annex G; libjpeg jdphuff.c): coefficients accumulate in Comp::coef, the inverse DCT runs at the end
    int eobrun = 0;
    bool prog_dc(BitReader& br, Comp& c, int bx, int by, int Ah, int Al) {
        int16_t* blk = (bx < c.bw && by < c.bh) ? &c.cf[((size_t)by * c.bw + bx) * 64] : nullptr;
        if (Ah == 0) {
            const Huff& hd = dc[c.td];
            if (!hd.present) return false;
            const int t = decode_sym(br, hd);
            if (t < 0 || t > 15) return false;
            c.pred += t ? extend(br.get(t), t) : 0;
            if (c.pred < -32767 || c.pred > 32767) return false;      // (a valid 8-bit stream stays within 11 bits)
            if (blk) blk[0] = (int16_t)(c.pred * (1 << Al));
        } else if (br.get(1)) {
            if (blk) blk[0] = (int16_t)(blk[0] | (1 << Al));
        }
        return true;
    }
    bool prog_ac(BitReader& br, Comp& c, int bx, int by, int Ss, int Se, int Ah, int Al) {
        if (bx >= c.bw || by >= c.bh) return false;
        int16_t* blk = &c.cf[((size_t)by * c.bw + bx) * 64];
        const Huff& ha = ac[c.ta];
        if (!ha.present) return false;
        if (Ah == 0) {
            if (eobrun > 0) { --eobrun; return true; }
            for (int k = Ss; k <= Se; ++k) {
                const int rs = decode_sym(br, ha);
                if (rs < 0) return false;
                const int r = rs >> 4, s2 = rs & 15;
                if (s2) {
                    k += r;
                    if (k > 63) return false;
                    blk[kZigzag[k]] = (int16_t)(extend(br.get(s2), s2) * (1 << Al));
                } else {
                    if (r != 15) { eobrun = (1 << r) - 1; if (r) eobrun += br.get(r); break; }
                    k += 15;
                }
            }
            return true;
        }
        const int p1 = 1 << Al, m1 = -(1 << Al);
        int k = Ss;
        if (eobrun == 0) {
            for (; k <= Se; ++k) {
                const int rs = decode_sym(br, ha);
                if (rs < 0) return false;
                int r = rs >> 4, s2 = rs & 15;
                if (s2) {
                    s2 = br.get(1) ? p1 : m1;               // (the size of a newly non-zero coefficient is always 1)
                } else if (r != 15) {
                    eobrun = 1 << r;
                    if (r) eobrun += br.get(r);
                    break;                                  // EOBr: the rest of this block only refines
                }
                do {                                        // skip r still-zero coefficients, refining the non-zero ones passed
                    int16_t& cf = blk[kZigzag[k]];
                    if (cf != 0) {
                        if (br.get(1) && (cf & p1) == 0) cf = (int16_t)(cf + (cf >= 0 ? p1 : m1));
                    } else if (--r < 0) break;
                    ++k;
                } while (k <= Se);
                if (s2 && k <= 63) blk[kZigzag[k]] = (int16_t)s2;
            }
        }
        if (eobrun > 0) {
            for (; k <= Se; ++k) {
                int16_t& cf = blk[kZigzag[k]];
                if (cf != 0 && br.get(1) && (cf & p1) == 0) cf = (int16_t)(cf + (cf >= 0 ? p1 : m1));
            }
            --eobrun;
        }
        return true;
    }
    // dequantise + inverse DCT of every block of component i from its coefficients (the end of a progressive file; the whole of
    // sd_jpeg_reconstruct_bgr_host's first stage)
    void idct_component(int i, const int16_t* cf, const uint16_t* q) {
        int32_t tmp[64];
        Comp& c = comp[i];
        for (int by = 0; by < c.bh; ++by)
            for (int bx = 0; bx < c.bw; ++bx) {
                const int16_t* blk = &cf[((size_t)by * c.bw + bx) * 64];
                for (int k = 0; k < 64; ++k) tmp[k] = (int32_t)blk[k] * (int32_t)q[k];
                idct_islow(tmp, c.plane.data() + (size_t)by * 8 * c.pw + (size_t)bx * 8, c.pw);
            }
    }
    void prog_finish() {
        for (int i = 0; i < ncomp; ++i) idct_component(i, comp[i].cf, qt[comp[i].tq]);
    }

    // coefficient route of a sequential file: block() with the transform taken out -- the same symbols, the same DC predictor, the same
    // refusals; the block's 64 quantised coefficients REPLACE what an earlier scan of the component left there, as the transform would
    bool block_store(BitReader& br, Comp& c, int bx, int by) {
        const Huff& hd = dc[c.td];
        const Huff& ha = ac[c.ta];
        if (!hd.present || !ha.present || !qt_ok[c.tq]) return false;
        int16_t coef[64];
        std::memset(coef, 0, sizeof(coef));
        const int t = decode_sym(br, hd);
        if (t < 0 || t > 15) return false;
        const int diff = t ? extend(br.get(t), t) : 0;
        c.pred += diff;
        if (c.pred < -32767 || c.pred > 32767) return false;
        coef[0] = (int16_t)c.pred;
        for (int k = 1; k < 64;) {
            const int rs = decode_sym(br, ha);
            if (rs < 0) return false;
            const int r = rs >> 4, s = rs & 15;
            if (!s) { if (r == 15) { k += 16; continue; } break; }
            k += r;
            if (k > 63) return false;
            coef[kZigzag[k]] = (int16_t)extend(br.get(s), s);
            ++k;
        }
        if (bx < c.bw && by < c.bh) std::memcpy(&c.cf[((size_t)by * c.bw + bx) * 64], coef, sizeof(coef));
        return true;
    }

    bool block(BitReader& br, Comp& c, int bx, int by) {
        const Huff& hd = dc[c.td];
        const Huff& ha = ac[c.ta];
        if (!hd.present || !ha.present || !qt_ok[c.tq]) return false;
        int32_t coef[64];
        std::memset(coef, 0, sizeof(coef));
        const int t = decode_sym(br, hd);
        if (t < 0 || t > 15) return false;
        const int diff = t ? extend(br.get(t), t) : 0;
        c.pred += diff;
        if (c.pred < -32767 || c.pred > 32767) return false;          // (keeps pred * qt inside int32 on crafted streams)
        coef[0] = c.pred * (int32_t)qt[c.tq][0];
        for (int k = 1; k < 64;) {
            const int rs = decode_sym(br, ha);
            if (rs < 0) return false;
            const int r = rs >> 4, s = rs & 15;
            if (!s) { if (r == 15) { k += 16; continue; } break; }
            k += r;
            if (k > 63) return false;
            const int z = kZigzag[k];
            coef[z] = extend(br.get(s), s) * (int32_t)qt[c.tq][z];
            ++k;
        }
        if (bx < c.bw && by < c.bh) idct_islow(coef, c.plane.data() + (size_t)by * 8 * c.pw + (size_t)bx * 8, c.pw);
        return true;
    }

    sd_status scan(const uint8_t* s, size_t sn, size_t data_off, size_t& next) {
        if (sn < 1) return SD_ERR_INVALID;
        const int ns = s[0];
        if (ns < 1 || ns > ncomp || sn < 1 + 2 * (size_t)ns + 3) return SD_ERR_INVALID;
        Comp* sc[3];
        for (int i = 0; i < ns; ++i) {
            Comp* c = nullptr;
            for (int j = 0; j < ncomp; ++j) if (comp[j].id == s[1 + 2 * i]) c = &comp[j];
            if (!c) return SD_ERR_INVALID;
            c->td = s[2 + 2 * i] >> 4; c->ta = s[2 + 2 * i] & 15;
            if (c->td > 3 || c->ta > 3) return SD_ERR_INVALID;
            sc[i] = c;
        }
        alloc_planes();
        // a sequential scan multiplies by the tables in force while it is decoded; the coefficient route hands that table on
        if (coef_ext && !progressive)
            for (int i = 0; i < ns; ++i) { std::memcpy(qt_used[sc[i] - comp], qt[sc[i]->tq], sizeof(qt_used[0])); scanned[sc[i] - comp] = true; }
        const int Ss = s[1 + 2 * ns], Se = s[2 + 2 * ns], Ah = s[3 + 2 * ns] >> 4, Al = s[3 + 2 * ns] & 15;
        if (progressive && (Ss > Se || Se > 63 || (Ss == 0 && Se != 0) || (Ss > 0 && ns != 1) || Al > 13)) return SD_ERR_INVALID;
        eobrun = 0;
        BitReader br{f + data_off, f + len};
        for (int i = 0; i < ns; ++i) sc[i]->pred = 0;
        int mcus_x, mcus_y;
        if (ns == 1) { mcus_x = (sc[0]->dw + 7) / 8; mcus_y = (sc[0]->dh + 7) / 8; }       // non-interleaved: MCU = one block of the real extent
        else { mcus_x = (W + 8 * hmax - 1) / (8 * hmax); mcus_y = (H + 8 * vmax - 1) / (8 * vmax); }
        int rst_left = restart, rst_next = 0;
        for (int my = 0; my < mcus_y; ++my)
            for (int mx = 0; mx < mcus_x; ++mx) {
                if (restart && rst_left == 0) {
                    // byte-align, expect RSTn
                    br.reset();
                    const uint8_t* q = br.p;
                    while (q + 1 < br.end && !(q[0] == 0xFF && q[1] >= 0xD0 && q[1] <= 0xD7)) ++q;
                    if (q + 1 >= br.end || (q[1] & 7) != rst_next) return SD_ERR_INVALID;
                    br.p = q + 2;
                    rst_next = (rst_next + 1) & 7;
                    rst_left = restart;
                    eobrun = 0;
                    for (int i = 0; i < ns; ++i) sc[i]->pred = 0;
                }
                auto one = [&](Comp& c, int bx, int by) {
                    if (!progressive) return coef_ext ? block_store(br, c, bx, by) : block(br, c, bx, by);
                    return Ss == 0 ? prog_dc(br, c, bx, by, Ah, Al) : prog_ac(br, c, bx, by, Ss, Se, Ah, Al);
                };
                if (ns == 1) {
                    if (!one(*sc[0], mx, my)) return SD_ERR_INVALID;
                } else {
                    for (int i = 0; i < ns; ++i)
                        for (int v = 0; v < sc[i]->v; ++v)
                            for (int h = 0; h < sc[i]->h; ++h)
                                if (!one(*sc[i], mx * sc[i]->h + h, my * sc[i]->v + v)) return SD_ERR_INVALID;
                }
                if (restart) --rst_left;
            }
        // the next marker
        const uint8_t* q = br.p;
        while (q + 1 < br.end && !(q[0] == 0xFF && q[1] != 0x00 && !(q[1] >= 0xD0 && q[1] <= 0xD7) && q[1] != 0xFF)) ++q;
        next = (size_t)(q - f);
        return SD_OK;
    }

    // libjpeg's fancy upsampling of one chroma plane to luma resolution (jdsample.c)
    void upsample(const Comp& c, std::vector<uint8_t>& full) const {
        full.assign((size_t)W * H, 0);
        const int cw = c.dw, chh = c.dh;
        if (hmax == 1 && vmax == 1) {
            for (int y = 0; y < H; ++y) std::memcpy(&full[(size_t)y * W], &c.plane[(size_t)y * c.pw], (size_t)W);
            return;
        }
        if (hmax == 2 && vmax == 1) {           // h2v1_fancy_upsample
            for (int y = 0; y < H; ++y) {
                const uint8_t* in = &c.plane[(size_t)y * c.pw];
                uint8_t* o = &full[(size_t)y * W];
                auto put = [&](int x, int v) { if (x < W) o[x] = (uint8_t)v; };
                if (cw == 1) { put(0, in[0]); put(1, in[0]); continue; }
                put(0, in[0]);
                put(1, (in[0] * 3 + in[1] + 2) >> 2);
                for (int i = 1; i < cw - 1; ++i) {
                    const int iv = in[i] * 3;
                    put(2 * i, (iv + in[i - 1] + 1) >> 2);
                    put(2 * i + 1, (iv + in[i + 1] + 2) >> 2);
                }
                put(2 * (cw - 1), (in[cw - 1] * 3 + in[cw - 2] + 1) >> 2);
                put(2 * (cw - 1) + 1, in[cw - 1]);
            }
            return;
        }
        // h2v2_fancy_upsample: output rows 2y (nearer to chroma row y-1) and 2y+1 (nearer to row y+1); the rows beyond the real
        // chroma extent are the replicated edge rows (jdmainct.c context rows)
        std::vector<int> sum((size_t)cw);
        for (int oy = 0; oy < H; ++oy) {
            const int y = oy >> 1;
            int yn = (oy & 1) ? y + 1 : y - 1;
            yn = yn < 0 ? 0 : (yn > chh - 1 ? chh - 1 : yn);
            const uint8_t* in0 = &c.plane[(size_t)y * c.pw];
            const uint8_t* in1 = &c.plane[(size_t)yn * c.pw];
            for (int i = 0; i < cw; ++i) sum[i] = in0[i] * 3 + in1[i];
            uint8_t* o = &full[(size_t)oy * W];
            auto put = [&](int x, int v) { if (x < W) o[x] = (uint8_t)v; };
            if (cw == 1) { put(0, (sum[0] * 4 + 8) >> 4); put(1, (sum[0] * 4 + 7) >> 4); continue; }
            put(0, (sum[0] * 4 + 8) >> 4);
            put(1, (sum[0] * 3 + sum[1] + 7) >> 4);
            for (int i = 1; i < cw - 1; ++i) {
                put(2 * i, (sum[i] * 3 + sum[i - 1] + 8) >> 4);
                put(2 * i + 1, (sum[i] * 3 + sum[i + 1] + 7) >> 4);
            }
            put(2 * (cw - 1), (sum[cw - 1] * 3 + sum[cw - 2] + 8) >> 4);
            put(2 * (cw - 1) + 1, (sum[cw - 1] * 4 + 7) >> 4);
        }
    }

    sd_status decode(uint8_t* out, size_t cap) {
        cap_bytes = cap;
        const sd_status st = parse(true);
        if (st != SD_OK) return st;
        for (int i = 0; i < ncomp; ++i) if (comp[i].plane.empty()) return SD_ERR_INVALID;
        if (cap < (size_t)W * H * 3) return SD_ERR_INVALID;
        if (progressive) {
            for (int i = 0; i < ncomp; ++i) if (!qt_ok[comp[i].tq] || comp[i].coef.empty()) return SD_ERR_INVALID;
            prog_finish();
        }
        return emit_bgr(out);
    }

    sd_status decode_coefficients(int16_t* out, size_t cap, sd_jpeg_frame_desc* desc) {
        coef_ext = out;
        cap_bytes = cap;
        const sd_status st = parse(true);
        if (st != SD_OK) return st;
        if (!allocated) return SD_ERR_INVALID;                        // no scan
        if (progressive)
            for (int i = 0; i < ncomp; ++i) {
                if (!qt_ok[comp[i].tq]) return SD_ERR_INVALID;
                std::memcpy(qt_used[i], qt[comp[i].tq], sizeof(qt_used[i]));     // a progressive file is dequantised at its end
            }
        // A sequential file need not scan every component (non-interleaved scans, the file cut between two of them).  The one-call decoder
        // never transforms a block of such a component, so its plane keeps the initial sample 0 -- not the 128 that zero coefficients
        // transform to.  DC = -1024 under a table of ones is the block that transforms to exactly 0 everywhere: the DC-only shortcuts give
        // descale(-1024 * 4, 5) = -128, and the level shift makes that 0.  Progressive files transform every block on both routes.
        if (!progressive)
            for (int i = 0; i < ncomp; ++i) {
                if (scanned[i]) continue;
                for (int k = 0; k < 64; ++k) qt_used[i][k] = 1;
                const size_t nblk = (size_t)comp[i].bw * comp[i].bh;
                for (size_t b = 0; b < nblk; ++b) comp[i].cf[b * 64] = -1024;
            }
        fill_desc(desc);
        return SD_OK;
    }

    // The plan of the entropy route (sd_jpeg_entropy_plan): the header parse above up to the first SOS, the scan header as scan() reads
    // it, and a byte walk over the scan data that accepts nothing but stuffed FFs, the expected RSTk and the closing EOI.  Wherever
    // scan()'s marker hunting could matter the file is left to scan(): eligible stays 0.
    sd_status plan(sd_jpeg_frame_desc* desc, sd_jpeg_entropy_frame* fr, sd_jpeg_huff_table* tables, sd_jpeg_interval* iv, size_t iv_cap) {
        std::memset(desc, 0, sizeof(*desc));
        std::memset(fr, 0, sizeof(*fr));
        std::memset(tables, 0, sizeof(*tables) * SD_JPEG_ENTROPY_TABLES);
        if (parse(false) != SD_OK || !sos || progressive || restart <= 0) return SD_OK;
        if (sos_len < 1) return SD_OK;                                 // (an empty SOS segment may end at the file's end: nothing to read)
        const int ns = sos[0];
        if (ns != ncomp || sos_len < 1 + 2 * (size_t)ns + 3) return SD_OK;
        for (int i = 0; i < ncomp; ++i) {
            // the scan names the components in the frame header's order, and no two components share an id (scan() resolves ids by search)
            if (sos[1 + 2 * i] != comp[i].id) return SD_OK;
            for (int j = 0; j < i; ++j) if (comp[j].id == comp[i].id) return SD_OK;
            comp[i].td = sos[2 + 2 * i] >> 4; comp[i].ta = sos[2 + 2 * i] & 15;
            if (comp[i].td > 3 || comp[i].ta > 3) return SD_OK;
            if (!dc[comp[i].td].present || !ac[comp[i].ta].present || !qt_ok[comp[i].tq]) return SD_OK;      // (block_store() refuses these)
        }
        const int mcus_x = (W + 8 * hmax - 1) / (8 * hmax), mcus_y = (H + 8 * vmax - 1) / (8 * vmax);
        const int64_t total = (int64_t)mcus_x * mcus_y, n_iv = (total + restart - 1) / restart;
        // the walk: memchr finds the FFs, everything between them is data
        size_t pos = sos_data, begin = sos_data;
        int64_t count = 0;
        bool closed = false;
        while (pos < len) {
            const uint8_t* q = static_cast<const uint8_t*>(std::memchr(f + pos, 0xFF, len - pos));
            if (!q) break;
            const size_t at = (size_t)(q - f);
            if (at + 1 >= len) break;
            const int m = f[at + 1];
            if (m == 0x00) { pos = at + 2; continue; }
            const bool last = count + 1 == n_iv;
            if (!last && m == 0xD0 + (int)(count & 7)) {
                if ((size_t)count < iv_cap) { iv[count].begin = (uint32_t)(begin - sos_data); iv[count].end = (uint32_t)(at - sos_data); }
                ++count;
                begin = pos = at + 2;
                continue;
            }
            if (last && m == 0xD9 && at + 2 == len) {
                if ((size_t)count < iv_cap) { iv[count].begin = (uint32_t)(begin - sos_data); iv[count].end = (uint32_t)(at - sos_data); }
                ++count;
                fr->scan_begin = (uint32_t)sos_data; fr->scan_end = (uint32_t)at;
                closed = true;
            }
            break;
        }
        if (!closed) return SD_OK;
        for (int i = 0; i < ncomp; ++i) std::memcpy(qt_used[i], qt[comp[i].tq], sizeof(qt_used[i]));
        fill_desc(desc);
        fr->ncomp = ncomp; fr->mcus_x = mcus_x; fr->mcus_y = mcus_y; fr->restart_interval = restart; fr->n_intervals = (int32_t)n_iv;
        for (int i = 0; i < ncomp; ++i) {
            fr->comp_h[i] = comp[i].h; fr->comp_v[i] = comp[i].v; fr->comp_dc[i] = comp[i].td; fr->comp_ac[i] = comp[i].ta;
            for (int k = 0; k < 2; ++k) {
                const Huff& h = k ? ac[comp[i].ta] : dc[comp[i].td];
                sd_jpeg_huff_table& t = tables[k ? 4 + comp[i].ta : comp[i].td];
                std::memcpy(t.look, h.look, sizeof(t.look));
                std::memcpy(t.vals, h.vals, sizeof(t.vals));
                for (int l = 1; l <= 16; ++l) { t.mincode[l] = h.mincode[l]; t.maxcode[l] = h.maxcode[l]; t.valptr[l] = h.valptr[l]; }
                t.maxcode[17] = h.maxcode[17];
            }
        }
        if ((size_t)n_iv > iv_cap) return SD_ERR_INVALID;            // (eligible stays 0; n_intervals says what the file needs)
        fr->eligible = 1;
        return SD_OK;
    }

    // The plan of the sync route (sd_jpeg_sync_plan): plan()'s rule with DRI = 0 admitted -- such a scan is one interval of all its
    // MCUs -- and the same byte walk, which here also writes the CLEAN stream: the data between the FFs copied, FF 00 as FF, the RSTk
    // dropped.  S is the piece length the piece indices are counted with.
    sd_status plan_sync(int S, sd_jpeg_frame_desc* desc, sd_jpeg_sync_frame* fr, sd_jpeg_huff_table* tables, sd_jpeg_sync_interval* iv, size_t iv_cap,
                        uint8_t* clean, size_t clean_cap) {
        std::memset(desc, 0, sizeof(*desc));
        std::memset(fr, 0, sizeof(*fr));
        std::memset(tables, 0, sizeof(*tables) * SD_JPEG_ENTROPY_TABLES);
        if (parse(false) != SD_OK || !sos || progressive || restart < 0) return SD_OK;
        if (sos_len < 1) return SD_OK;
        const int ns = sos[0];
        if (ns != ncomp || sos_len < 1 + 2 * (size_t)ns + 3) return SD_OK;
        for (int i = 0; i < ncomp; ++i) {
            if (sos[1 + 2 * i] != comp[i].id) return SD_OK;
            for (int j = 0; j < i; ++j) if (comp[j].id == comp[i].id) return SD_OK;
            comp[i].td = sos[2 + 2 * i] >> 4; comp[i].ta = sos[2 + 2 * i] & 15;
            if (comp[i].td > 3 || comp[i].ta > 3) return SD_OK;
            if (!dc[comp[i].td].present || !ac[comp[i].ta].present || !qt_ok[comp[i].tq]) return SD_OK;
        }
        const int mcus_x = (W + 8 * hmax - 1) / (8 * hmax), mcus_y = (H + 8 * vmax - 1) / (8 * vmax);
        const int64_t total = (int64_t)mcus_x * mcus_y;
        if (total < 1 || total > 0x7fffffff) return SD_OK;
        const int64_t per = restart ? restart : total, n_iv = (total + per - 1) / per;
        size_t pos = sos_data, from = sos_data;      // from: the first byte not yet copied
        size_t out = 0, begin_out = 0;               // clean bytes so far; where the open interval began
        uint64_t piece = 0;
        int64_t count = 0;
        bool closed = false;
        auto copy = [&](size_t upto) {               // the data bytes [from, upto)
            if (clean && out + (upto - from) <= clean_cap) std::memcpy(clean + out, f + from, upto - from);
            out += upto - from;
        };
        auto close = [&]() {
            if ((size_t)count < iv_cap) { iv[count].begin = (uint32_t)begin_out; iv[count].end = (uint32_t)out; iv[count].first_piece = (uint32_t)piece; iv[count].reserved = 0; }
            piece += out > begin_out ? (out - begin_out + (size_t)S - 1) / (size_t)S : 1;
            ++count;
            begin_out = out;
        };
        while (pos < len) {
            const uint8_t* q = static_cast<const uint8_t*>(std::memchr(f + pos, 0xFF, len - pos));
            if (!q) break;
            const size_t at = (size_t)(q - f);
            if (at + 1 >= len) break;
            const int m = f[at + 1];
            if (m == 0x00) { copy(at + 1); from = pos = at + 2; continue; }      // the FF is data, its 00 is not
            const bool last = count + 1 == n_iv;
            if (!last && m == 0xD0 + (int)(count & 7)) {
                copy(at);
                close();
                from = pos = at + 2;
                continue;
            }
            if (last && m == 0xD9 && at + 2 == len) {
                copy(at);
                close();
                fr->scan_begin = (uint32_t)sos_data; fr->scan_end = (uint32_t)at;
                closed = true;
            }
            break;
        }
        if (!closed) return SD_OK;
        for (int i = 0; i < ncomp; ++i) std::memcpy(qt_used[i], qt[comp[i].tq], sizeof(qt_used[i]));
        fill_desc(desc);
        fr->ncomp = ncomp; fr->mcus_x = mcus_x; fr->mcus_y = mcus_y; fr->restart_interval = (int32_t)per; fr->n_intervals = (int32_t)n_iv;
        fr->clean_bytes = (uint32_t)out; fr->subseq_bytes = (uint32_t)S; fr->n_pieces = (uint32_t)piece;
        for (int i = 0; i < ncomp; ++i) {
            fr->comp_h[i] = comp[i].h; fr->comp_v[i] = comp[i].v; fr->comp_dc[i] = comp[i].td; fr->comp_ac[i] = comp[i].ta;
            for (int k = 0; k < 2; ++k) {
                const Huff& h = k ? ac[comp[i].ta] : dc[comp[i].td];
                sd_jpeg_huff_table& t = tables[k ? 4 + comp[i].ta : comp[i].td];
                std::memcpy(t.look, h.look, sizeof(t.look));
                std::memcpy(t.vals, h.vals, sizeof(t.vals));
                for (int l = 1; l <= 16; ++l) { t.mincode[l] = h.mincode[l]; t.maxcode[l] = h.maxcode[l]; t.valptr[l] = h.valptr[l]; }
                t.maxcode[17] = h.maxcode[17];
            }
        }
        if ((size_t)n_iv > iv_cap || (clean && out > clean_cap)) return SD_ERR_INVALID;       // (eligible stays 0; the record says what the file needs)
        fr->eligible = 1;
        return SD_OK;
    }

    // the back half from a coefficient buffer: the planes of a descriptor's geometry, every block transformed, then emit_bgr
    sd_status reconstruct(const int16_t* coef, const sd_jpeg_frame_desc& d, uint8_t* out, size_t cap) {
        if (!sdjpeg::desc_ok(d) || cap < (size_t)d.height * d.width * 3) return SD_ERR_INVALID;
        H = d.height; W = d.width; ncomp = d.ncomp; hmax = d.hmax; vmax = d.vmax; orientation = d.orientation; adobe_transform = d.adobe_transform;
        for (int i = 0; i < ncomp; ++i) { comp[i].h = i ? 1 : hmax; comp[i].v = i ? 1 : vmax; }
        geometry();
        for (int i = 0; i < ncomp; ++i) {
            comp[i].plane.assign((size_t)comp[i].pw * comp[i].ph, 0);
            idct_component(i, coef + d.coef_offset[i], d.qt[i]);
        }
        return emit_bgr(out);
    }

    // planes -> BGR: fancy chroma upsampling, YCbCr -> RGB (or the Adobe pass-through, or the gray replication), EXIF orientation
    sd_status emit_bgr(uint8_t* out) {
        std::vector<uint8_t> bgr;
        const bool direct = orientation == 1;
        uint8_t* dst = out;
        if (!direct) { bgr.resize((size_t)W * H * 3); dst = bgr.data(); }
        if (ncomp == 1) {
            for (int y = 0; y < H; ++y) {
                const uint8_t* in = &comp[0].plane[(size_t)y * comp[0].pw];
                uint8_t* o = dst + (size_t)y * W * 3;
                for (int x = 0; x < W; ++x) o[3 * x] = o[3 * x + 1] = o[3 * x + 2] = in[x];
            }
        } else {
            std::vector<uint8_t> cb, cr;
            upsample(comp[1], cb);
            upsample(comp[2], cr);
            // jdcolor.c build_ycc_rgb_table: SCALEBITS 16
            int crr[256], cbb[256];
            int32_t crg[256], cbg[256];
            for (int i = 0; i < 256; ++i) {
                const int x = i - 128;
                crr[i] = (int)((91881 * (int64_t)x + 32768) >> 16);       // FIX(1.40200)
                cbb[i] = (int)((116130 * (int64_t)x + 32768) >> 16);      // FIX(1.77200)
                crg[i] = -46802 * x;                                      // FIX(0.71414)
                cbg[i] = -22554 * x + 32768;                              // FIX(0.34414) + ONE_HALF
            }
            auto cl = [](int v) { return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); };
            const bool rgb_direct = adobe_transform == 0;                 // Adobe marker: the three components ARE R, G, B
            for (int y = 0; y < H; ++y) {
                const uint8_t* yy = &comp[0].plane[(size_t)y * comp[0].pw];
                const uint8_t* b = &cb[(size_t)y * W];
                const uint8_t* r = &cr[(size_t)y * W];
                uint8_t* o = dst + (size_t)y * W * 3;
                for (int x = 0; x < W; ++x) {
                    if (rgb_direct) { o[3 * x] = r[x]; o[3 * x + 1] = b[x]; o[3 * x + 2] = yy[x]; continue; }
                    const int Y = yy[x];
                    o[3 * x + 2] = cl(Y + crr[r[x]]);
                    o[3 * x + 1] = cl(Y + (int)((cbg[b[x]] + crg[r[x]]) >> 16));
                    o[3 * x] = cl(Y + cbb[b[x]]);
                }
            }
        }
        if (direct) return SD_OK;
        // EXIF orientation, as OpenCV's ExifTransform: 2 flip horizontally, 3 rotate 180, 4 flip vertically, 5 transpose,
        // 6 rotate 90 clockwise, 7 transverse, 8 rotate 90 counter-clockwise
        const int OW = orientation >= 5 ? H : W, OH = orientation >= 5 ? W : H;
        for (int oy = 0; oy < OH; ++oy)
            for (int ox = 0; ox < OW; ++ox) {
                int sx, sy;
                switch (orientation) {
                    case 2: sx = W - 1 - ox; sy = oy; break;
                    case 3: sx = W - 1 - ox; sy = H - 1 - oy; break;
                    case 4: sx = ox; sy = H - 1 - oy; break;
                    case 5: sx = oy; sy = ox; break;
                    case 6: sx = oy; sy = H - 1 - ox; break;
                    case 7: sx = W - 1 - oy; sy = H - 1 - ox; break;
                    default: sx = W - 1 - oy; sy = ox; break;      // 8
                }
                std::memcpy(out + ((size_t)oy * OW + ox) * 3, dst + ((size_t)sy * W + sx) * 3, 3);
            }
        return SD_OK;
    }
};

}  // namespace

extern "C" sd_status sd_jpeg_decode_bgr(const uint8_t* file_host, size_t len, uint8_t* bgr_out_host, size_t out_capacity, int* height_out,
                                        int* width_out) {
    if (!file_host) return SD_ERR_INVALID;
    try {                                                  // (no exception crosses the C ABI: an allocation failure is a refused file)
        Decoder d;
        d.f = file_host; d.len = len;
        if (!bgr_out_host) return d.header_only(height_out, width_out);
        const sd_status st = d.decode(bgr_out_host, out_capacity);
        if (st == SD_OK) d.dims(height_out, width_out);
        return st;
    } catch (...) {
        return SD_ERR_INVALID;
    }
}

extern "C" sd_status sd_jpeg_decode_coefficients(const uint8_t* file_host, size_t len, int16_t* coef_out_host, size_t capacity_bytes,
                                                 sd_jpeg_frame_desc* desc_out) {
    if (!file_host || !desc_out) return SD_ERR_INVALID;
    try {
        Decoder d;
        d.f = file_host; d.len = len;
        if (!coef_out_host) {
            const sd_status st = d.parse(false);
            if (st == SD_OK) {                               // (the tables read so far: final only after the full call)
                for (int i = 0; i < d.ncomp; ++i) std::memcpy(d.qt_used[i], d.qt[d.comp[i].tq], sizeof(d.qt_used[i]));
                d.fill_desc(desc_out);
            }
            return st;
        }
        return d.decode_coefficients(coef_out_host, capacity_bytes, desc_out);
    } catch (...) {
        return SD_ERR_INVALID;
    }
}

extern "C" sd_status sd_jpeg_entropy_plan(const uint8_t* file_host, size_t len, sd_jpeg_frame_desc* desc_out, sd_jpeg_entropy_frame* frame_out,
                                          sd_jpeg_huff_table* tables_out, sd_jpeg_interval* intervals_out, size_t interval_cap) {
    if (frame_out) std::memset(frame_out, 0, sizeof(*frame_out));       // eligible is 0 on every return but the eligible one
    if (!file_host || !desc_out || !frame_out || !tables_out || (!intervals_out && interval_cap) || len >= ((size_t)1 << 31)) return SD_ERR_INVALID;
    if (len < 2 || file_host[0] != 0xFF || file_host[1] != 0xD8) return SD_ERR_FORMAT;
    try {
        Decoder d;
        d.f = file_host; d.len = len;
        return d.plan(desc_out, frame_out, tables_out, intervals_out, interval_cap);
    } catch (...) {
        return SD_ERR_INVALID;
    }
}

extern "C" sd_status sd_jpeg_sync_plan(const uint8_t* file_host, size_t len, int subseq_bytes, sd_jpeg_frame_desc* desc_out, sd_jpeg_sync_frame* frame_out,
                                       sd_jpeg_huff_table* tables_out, sd_jpeg_sync_interval* intervals_out, size_t interval_cap, uint8_t* clean_out,
                                       size_t clean_capacity) {
    if (frame_out) std::memset(frame_out, 0, sizeof(*frame_out));       // eligible is 0 on every return but the eligible one
    if (!file_host || !desc_out || !frame_out || !tables_out || (!intervals_out && interval_cap) || len >= ((size_t)1 << 28)) return SD_ERR_INVALID;
    if (subseq_bytes < 32 || subseq_bytes > 1024 || (subseq_bytes & (subseq_bytes - 1))) return SD_ERR_INVALID;
    if (len < 2 || file_host[0] != 0xFF || file_host[1] != 0xD8) return SD_ERR_FORMAT;
    try {
        Decoder d;
        d.f = file_host; d.len = len;
        return d.plan_sync(subseq_bytes, desc_out, frame_out, tables_out, intervals_out, interval_cap, clean_out, clean_capacity);
    } catch (...) {
        return SD_ERR_INVALID;
    }
}

extern "C" sd_status sd_jpeg_reconstruct_bgr_host(const int16_t* coef_host, const sd_jpeg_frame_desc* desc, uint8_t* bgr_out_host,
                                                  size_t out_capacity) {
    if (!coef_host || !desc || !bgr_out_host) return SD_ERR_INVALID;
    try {
        Decoder d;
        d.f = nullptr; d.len = 0;
        return d.reconstruct(coef_host, *desc, bgr_out_host, out_capacity);
    } catch (...) {
        return SD_ERR_INVALID;
    }
}
