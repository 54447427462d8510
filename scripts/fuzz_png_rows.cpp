// dev tool: fuzz harness of the split PNG route's host side (CPU build under ASan + UBSan; it runs no GPU code and nothing of it goes
// through Python): sd_png_inflate_rows against the existing decoder sd_png_decode_bgr.
//   g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -Iinclude scripts/fuzz_png_rows.cpp \
//       semantic_depth_amd/csrc/host_png.cpp semantic_depth_amd/csrc/host_jpeg.cpp -lz -lpthread -o /tmp/fuzz_png_rows
//   /tmp/fuzz_png_rows 4000 case1.png case2.png ...      (seeds: python -c "import png_in_cases as P; P.dump('/tmp/png_seeds')" from tests/)
// Every iteration mutates a seed and calls both entry points on an exact-size heap copy of the file, with exact-size output buffers, so one
// byte too far on either side is an ASan report.  Two kinds of mutation:
//   A  the FILE bytes: bit flips, random bytes, truncation, a random IHDR field (the decoders do not check CRCs);
//   B  the ROWS: the IDAT stream is inflated, filter bytes (to 0..7) and samples are changed, rows are dropped or added, the PLTE chunk is
//      shortened or removed, and the file is put together again with a fresh zlib stream.
// Required of every mutated file: the descriptor query and sd_png_decode_bgr's size query return the same status; the full calls return
// the same status, except that sd_png_inflate_rows may accept a colour type 3 file that sd_png_decode_bgr refuses when -- and only when --
// the reconstructed rows hold an index beyond the palette; where both accept, sd_png_unfilter_bgr on the rows plus the palette lookup gives
// the decoder's bytes; a capacity one byte short is refused and leaves its buffer untouched.
#include <zlib.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "semdepth.h"

typedef std::vector<uint8_t> Bytes;

static Bytes readf(const char* p) {
    FILE* f = fopen(p, "rb");
    Bytes v;
    if (!f) return v;
    fseek(f, 0, SEEK_END);
    long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    v.resize(n > 0 ? n : 0);
    if (n > 0 && fread(v.data(), 1, n, f) != (size_t)n) v.clear();
    fclose(f);
    return v;
}

static uint32_t be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }
static void put32(Bytes& o, uint32_t v) { o.push_back(v >> 24); o.push_back(v >> 16); o.push_back(v >> 8); o.push_back(v); }
static void chunk(Bytes& o, const char* tag, const uint8_t* d, size_t n) {
    put32(o, (uint32_t)n);
    o.insert(o.end(), tag, tag + 4);
    if (n) o.insert(o.end(), d, d + n);
    put32(o, 0);                                                   // (no decoder here reads the CRC)
}

struct Parts { Bytes ihdr, plte, raw; bool has_plte = false, ok = false; };

static Parts take_apart(const Bytes& f) {
    Parts p;
    if (f.size() < 33 || be32(f.data() + 8) != 13) return p;
    p.ihdr.assign(f.begin() + 16, f.begin() + 29);
    Bytes z;
    for (size_t q = 8; q + 12 <= f.size();) {
        const size_t n = be32(f.data() + q);
        if (q + 12 + n > f.size()) return p;
        if (!memcmp(f.data() + q + 4, "IDAT", 4)) z.insert(z.end(), f.begin() + q + 8, f.begin() + q + 8 + n);
        if (!memcmp(f.data() + q + 4, "PLTE", 4)) { p.plte.assign(f.begin() + q + 8, f.begin() + q + 8 + n); p.has_plte = true; }
        q += 12 + n;
    }
    p.raw.resize((size_t)1 << 22);
    uLongf len = p.raw.size();
    if (uncompress(p.raw.data(), &len, z.data(), z.size()) != Z_OK) return p;
    p.raw.resize(len);
    p.ok = true;
    return p;
}

static Bytes put_together(const Parts& p) {
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
    Bytes o(sig, sig + 8);
    chunk(o, "IHDR", p.ihdr.data(), p.ihdr.size());
    if (p.has_plte) chunk(o, "PLTE", p.plte.data(), p.plte.size());
    Bytes z(compressBound(p.raw.size()));
    uLongf len = z.size();
    compress2(z.data(), &len, p.raw.data(), p.raw.size(), 1);
    chunk(o, "IDAT", z.data(), len);
    chunk(o, "IEND", nullptr, 0);
    return o;
}

#define REQUIRE(c, ...) do { if (!(c)) { printf("FINDING (%s): ", #c); printf(__VA_ARGS__); printf("\n"); return 1; } } while (0)

int main(int argc, char** argv) {
    if (argc < 3) { printf("usage: fuzz_png_rows ITERATIONS seed.png ...\n"); return 2; }
    const int iters = atoi(argv[1]);
    std::mt19937_64 rng(20261020);
    long runs = 0, both_ok = 0, both_refused = 0, palette_exception = 0, skipped_large = 0, short_caps = 0;
    for (int a = 2; a < argc; ++a) {
        const Bytes base = readf(argv[a]);
        if (base.empty()) continue;
        const Parts parts = take_apart(base);
        for (int it = 0; it < iters; ++it) {
            Bytes m;
            if (parts.ok && (rng() & 1)) {                         // B: the rows
                Parts p = parts;
                const int h = (int)be32(p.ihdr.data() + 4);
                const size_t row = h > 0 ? p.raw.size() / h : 0;
                const int n = 1 + rng() % 4;
                for (int k = 0; k < n; ++k) {
                    switch (rng() % 6) {
                        case 0: if (row) p.raw[(rng() % h) * row] = rng() % 8; break;
                        case 1: if (row) p.raw[((rng() % 3 == 0) ? 0 : (rng() % 2 ? h - 1 : rng() % h)) * row] = 5 + rng() % 3; break;
                        case 2: if (!p.raw.empty()) p.raw[rng() % p.raw.size()] = (uint8_t)rng(); break;
                        case 3: if (row && p.raw.size() > row) p.raw.resize(p.raw.size() - (rng() % 2 ? row : 1 + rng() % row)); break;
                        case 4: p.raw.resize(p.raw.size() + 1 + rng() % (row + 1), (uint8_t)(rng() % 5)); break;
                        default:
                            if (p.has_plte) { if (rng() % 3 == 0) p.has_plte = false; else p.plte.resize(rng() % (p.plte.size() + 1)); }
                            else if (rng() % 4 == 0) { p.has_plte = true; p.plte.assign(3 * (rng() % 300), (uint8_t)rng()); }
                    }
                }
                m = put_together(p);
            } else {                                               // A: the file
                m = base;
                const int n = 1 + rng() % 4;
                for (int k = 0; k < n; ++k) {
                    switch (rng() % 5) {
                        case 0: m[rng() % m.size()] ^= (uint8_t)(1u << (rng() % 8)); break;
                        case 1: m[rng() % m.size()] = (uint8_t)rng(); break;
                        case 2: m.resize(rng() % (m.size() + 1)); break;
                        case 3: if (m.size() > 29) { const int f = 16 + rng() % 13; m[f] = (rng() % 2) ? (uint8_t)(rng() % 20) : (uint8_t)rng(); } break;
                        default: if (m.size() > 40) m[33 + rng() % (m.size() - 33)] = (uint8_t)rng();
                    }
                    if (m.empty()) break;
                }
            }
            ++runs;
            uint8_t* file = (uint8_t*)malloc(m.size() ? m.size() : 1);        // exact size: a read past the file is a report
            if (!m.empty()) memcpy(file, m.data(), m.size());
            int h = 0, w = 0;
            sd_png_frame_desc d;
            const sd_status q_dec = sd_png_decode_bgr(file, m.size(), nullptr, 0, &h, &w);
            const sd_status q_inf = sd_png_inflate_rows(file, m.size(), nullptr, 0, &d);
            REQUIRE(q_dec == q_inf, "%s it %d: query %d vs %d", argv[a], it, q_dec, q_inf);
            if (q_dec != SD_OK) { ++both_refused; free(file); continue; }
            REQUIRE(d.height == h && d.width == w && d.channels >= 1 && d.channels <= 4, "%s it %d: descriptor", argv[a], it);
            if ((size_t)h * w > ((size_t)1 << 20)) { ++skipped_large; free(file); continue; }      // (a mutated IHDR: no 4 GiB buffers)
            const size_t raw_len = (size_t)h * (1 + (size_t)w * d.channels), out_len = (size_t)h * w * 3;
            uint8_t* out = (uint8_t*)malloc(out_len);
            uint8_t* rows = (uint8_t*)malloc(raw_len);
            const sd_status s_dec = sd_png_decode_bgr(file, m.size(), out, out_len, nullptr, nullptr);
            const sd_status s_inf = sd_png_inflate_rows(file, m.size(), rows, raw_len, &d);
            if (s_inf == SD_OK) {
                REQUIRE(d.palette_entries >= 0 && d.palette_entries <= 256 && (d.color_type == 3 || d.palette_entries == 0), "%s it %d: palette count", argv[a], it);
                uint8_t* again = (uint8_t*)malloc(out_len);
                REQUIRE(sd_png_unfilter_bgr(rows, h, w, d.channels, again) == SD_OK, "%s it %d: accepted rows are refused by the unfilter", argv[a], it);
                bool over = false;
                if (d.color_type == 3)
                    for (size_t i = 0; i < (size_t)h * w; ++i) {
                        const int k = again[3 * i];
                        if (k >= d.palette_entries) { over = true; continue; }
                        again[3 * i] = d.palette[k][2]; again[3 * i + 1] = d.palette[k][1]; again[3 * i + 2] = d.palette[k][0];
                    }
                if (s_dec == SD_OK) {
                    REQUIRE(!over && !memcmp(out, again, out_len), "%s it %d: accepted by both, other bytes", argv[a], it);
                    ++both_ok;
                } else {
                    REQUIRE(over, "%s it %d: accepted by inflate_rows only, and no index is beyond the palette", argv[a], it);
                    ++palette_exception;
                }
                free(again);
                if (raw_len > 1) {                                 // one byte short: refused, nothing written
                    uint8_t* shortbuf = (uint8_t*)malloc(raw_len - 1);
                    memset(shortbuf, 0xA5, raw_len - 1);
                    REQUIRE(sd_png_inflate_rows(file, m.size(), shortbuf, raw_len - 1, &d) == SD_ERR_INVALID, "%s it %d: short capacity accepted", argv[a], it);
                    for (size_t i = 0; i + 1 < raw_len; ++i) REQUIRE(shortbuf[i] == 0xA5, "%s it %d: short capacity written", argv[a], it);
                    free(shortbuf);
                    ++short_caps;
                }
            } else {
                REQUIRE(s_dec == s_inf, "%s it %d: refused by inflate_rows (%d), decode says %d", argv[a], it, s_inf, s_dec);
                ++both_refused;
            }
            free(rows);
            free(out);
            free(file);
        }
    }
    printf("fuzz_png_rows: %ld mutated files: %ld accepted by both with equal bytes, %ld refused by both, %ld palette-index exceptions, "
           "%ld short-capacity probes, %ld skipped as too large; no finding\n", runs, both_ok, both_refused, palette_exception, short_caps, skipped_large);
    return 0;
}
