// dev tool: fuzz harness of the JPEG sync route's host side (CPU build under ASan + UBSan; it runs no GPU code): the plan
// (sd_jpeg_sync_plan) and the CPU statement of the device decoder (sd_jpeg_sync_decode_host), which runs the passes the kernels run
// (semantic_depth_amd/csrc/jpeg_sync.hpp).  This is the evidence that no input makes those passes read outside a frame's clean stream,
// index a record outside the frame's pieces or write outside a frame's coefficients, and that status 0 means the sequential decode.
//   g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -Iinclude scripts/fuzz_jpeg_sync.cpp \
//       semantic_depth_amd/csrc/host_jpeg.cpp semantic_depth_amd/csrc/host_jpeg_sync.cpp -lpthread -o /tmp/fuzz_jpeg_sync
//   /tmp/fuzz_jpeg_sync 20000 seed1.jpg seed2.jpg ...     (seeds: small sequential JPEG files, with and without restart intervals)
// Two kinds of iteration, from exact-size heap copies so that one byte too far is an ASan report, at a piece length drawn from 32..1024:
//   A  the FILE is mutated (bit flips, random bytes, FF runs, inserted markers, truncation, deletions, insertions -- in the scan and,
//      less often, in the header); when the plan still calls it eligible the CPU statement decodes it and the result is held against
//      sd_jpeg_decode_coefficients: a non-zero status where that decoder refuses the file; where the status is 0 the same descriptor and
//      coefficients.  A file that decoder accepts may be flagged 5 or 6 (not synchronised, bits ran out) and nothing else.
//   B  the PLAN'S OUTPUTS are mutated (record fields, interval ranges and piece indices, table entries, descriptor fields, strides, the
//      piece length); whatever the argument checks still let through is decoded: nothing may crash or touch memory outside the buffers.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "semdepth.h"

static std::vector<uint8_t> readf(const char* p) {
    FILE* f = fopen(p, "rb");
    std::vector<uint8_t> v;
    if (!f) return v;
    fseek(f, 0, SEEK_END);
    long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    v.resize(n);
    if (fread(v.data(), 1, n, f) != (size_t)n) v.clear();
    fclose(f);
    return v;
}

// the first n elements of v as an exact-size copy (n may be 0, v may be empty)
template <class T>
static std::vector<T> head(const std::vector<T>& v, size_t n) {
    std::vector<T> o(n < v.size() ? n : v.size());
    if (!o.empty()) std::memcpy(o.data(), v.data(), o.size() * sizeof(T));
    return o;
}

static size_t coef_elems(const sd_jpeg_frame_desc& d) {
    size_t n = 0;
    for (int i = 0; i < d.ncomp && i < 3; ++i) n += (size_t)d.blocks_w[i] * d.blocks_h[i] * 64;
    return n;
}

static size_t scan_start(const std::vector<uint8_t>& f) {
    size_t p = 2;
    while (p + 4 <= f.size() && f[p] == 0xFF) {
        const size_t n = ((size_t)f[p + 2] << 8) | f[p + 3];
        if (f[p + 1] == 0xDA) return p + 2 + n < f.size() ? p + 2 + n : f.size() - 1;
        p += 2 + n;
    }
    return 2;
}

int main(int argc, char** argv) {
    if (argc < 3) { printf("usage: fuzz_jpeg_sync ITERATIONS seed.jpg ...\n"); return 2; }
    const int iters = atoi(argv[1]);
    std::mt19937_64 rng(20261021);
    long eligible = 0, accepted = 0, flagged5 = 0, flagged6 = 0, refused = 0, plan_runs = 0, plan_passed = 0;
    constexpr size_t kCap = 4096;
    for (int a = 2; a < argc; ++a) {
        const std::vector<uint8_t> base = readf(argv[a]);
        if (base.size() < 4) { printf("cannot read %s\n", argv[a]); return 2; }
        const size_t s0 = scan_start(base);
        for (int it = 0; it < iters; ++it) {
            const bool plan_kind = it & 1;
            const int S = 32 << (rng() % 6);
            std::vector<uint8_t> f = base;
            if (!plan_kind || rng() % 4 == 0) {                                   // A (and a quarter of B starts from a mutated file)
                const int kind = rng() % 8;
                const size_t lo = rng() % 8 ? s0 : 0;                             // mostly the scan, sometimes the header
                auto at = [&]() { return lo + rng() % (f.size() - lo); };
                if (kind == 0) f.resize(2 + rng() % (f.size() - 1));
                else if (kind == 1) { int n = 1 + rng() % 4; for (int i = 0; i < n; ++i) f[at()] ^= (uint8_t)(1u << (rng() % 8)); }
                else if (kind == 2) { int n = 1 + rng() % 8; for (int i = 0; i < n; ++i) f[at()] = (uint8_t)rng(); }
                else if (kind == 3) { size_t p = at(), n = rng() % 16; for (size_t i = p; i < p + n && i < f.size(); ++i) f[i] = 0xff; }
                else if (kind == 4) { const uint8_t m[2] = {0xFF, (uint8_t)(0xD0 + rng() % 10)}; f.insert(f.begin() + at(), m, m + 2); }
                else if (kind == 5) { size_t p = at(), n = 1 + rng() % 40; if (p + n < f.size()) f.erase(f.begin() + p, f.begin() + p + n); }
                else if (kind == 6) { size_t p = at(); f.insert(f.begin() + p, (size_t)(rng() % 32), (uint8_t)(rng() % 3 ? 0 : 0xFF)); }
                else { int n = 1 + rng() % 48; for (int i = 0; i < n; ++i) f[at()] ^= (uint8_t)(1u << (rng() % 8)); }
                if (rng() % 6 == 0 && f.size() > 4) {                             // keep the file closed by EOI: the plan wants it as the last two bytes
                    f[f.size() - 2] = 0xFF; f[f.size() - 1] = 0xD9;
                }
            }
            // exact-size heap copies: one byte too far is a report
            std::vector<uint8_t> file(f.begin(), f.end());
            sd_jpeg_frame_desc desc;
            sd_jpeg_sync_frame fr;
            std::vector<sd_jpeg_huff_table> tables(SD_JPEG_ENTROPY_TABLES);
            const size_t cap = rng() % 16 ? kCap : rng() % 64;                    // sometimes too little room for the ranges
            std::vector<sd_jpeg_sync_interval> iv(cap);
            const size_t room = rng() % 16 ? file.size() : rng() % (file.size() + 1);      // sometimes too little room for the clean stream
            std::vector<uint8_t> clean(room);
            const sd_status ps = sd_jpeg_sync_plan(file.data(), file.size(), S, &desc, &fr, tables.data(), iv.data(), cap, clean.data(), room);
            if (ps != SD_OK || !fr.eligible) continue;
            if (clean.size() < fr.clean_bytes) continue;                          // (no room at all: data() was null, which asks the plan to count only)
            ++eligible;
            iv.resize(fr.n_intervals);
            iv.shrink_to_fit();
            std::vector<uint8_t> scan = head(clean, fr.clean_bytes);
            size_t byte_stride = scan.size(), interval_stride = iv.size(), coef_stride = coef_elems(desc) * 2;
            int piece = S;
            static uint8_t none;                                                  // (an empty clean stream: a pointer the entry point takes, never read)
            if (!plan_kind) {
                std::vector<int16_t> coef(coef_stride / 2, (int16_t)0x5a5a), ref(coef_stride / 2);
                int32_t status = -1;
                const sd_status ds = sd_jpeg_sync_decode_host(scan.empty() ? &none : scan.data(), byte_stride, &desc, &fr, iv.data(), interval_stride, tables.data(), 1, piece,
                                                              coef.data(), coef_stride, &status);
                if (ds != SD_OK) { printf("FAIL: an eligible plan was refused by the argument checks (%s, iteration %d)\n", argv[a], it); return 1; }
                sd_jpeg_frame_desc hd;
                const sd_status hs = sd_jpeg_decode_coefficients(file.data(), file.size(), ref.data(), coef_stride, &hd);
                if (hs == SD_OK) {
                    if (status == 0) {
                        ++accepted;
                        if (std::memcmp(&hd, &desc, sizeof(hd)) != 0 || std::memcmp(coef.data(), ref.data(), coef_stride) != 0) {
                            printf("FAIL: status 0 but differs from sd_jpeg_decode_coefficients (%s, iteration %d, piece %d)\n", argv[a], it, piece);
                            return 1;
                        }
                    } else if (status == SD_JPEG_SYNC_NOT_SYNCHRONISED) ++flagged5;
                    else if (status == SD_JPEG_SYNC_BITS_RAN_OUT) ++flagged6;
                    else { printf("FAIL: refusal %d of a file the host decoder accepts (%s, iteration %d, piece %d)\n", status, argv[a], it, piece); return 1; }
                } else {
                    ++refused;
                    if (status == 0) { printf("FAIL: the host decoder refuses a file the CPU statement accepts (%s, iteration %d)\n", argv[a], it); return 1; }
                }
                continue;
            }
            // B: damage the plan's outputs
            ++plan_runs;
            const int n = 1 + rng() % 3;
            for (int k = 0; k < n; ++k) {
                const int what = rng() % 9;
                auto val = [&]() -> int32_t { const int r = rng() % 6; return r == 0 ? 0 : r == 1 ? -1 : r == 2 ? (int32_t)(rng() % 5) : r == 3 ? (int32_t)(rng() % 70000) : r == 4 ? 0x7fffffff : (int32_t)rng(); };
                if (what == 0) { int32_t* p = &fr.ncomp; p[rng() % 17] = val(); }                         // ncomp .. comp_ac[2]
                else if (what == 1 && !iv.empty()) {
                    sd_jpeg_sync_interval& x = iv[rng() % iv.size()];
                    uint32_t* p = &x.begin;
                    p[rng() % 3] = rng() % 3 ? (uint32_t)(rng() % (scan.size() + 2)) : (uint32_t)rng();   // begin, end, first_piece
                }
                else if (what == 2) { sd_jpeg_huff_table& t = tables[rng() % tables.size()]; for (int i = 0; i < 4; ++i) t.look[rng() % 512] = rng() % 3 ? (uint16_t)(((rng() % 11) << 8) | (rng() & 255)) : (uint16_t)rng(); }
                else if (what == 3) { sd_jpeg_huff_table& t = tables[rng() % tables.size()]; int32_t* p = t.mincode; p[rng() % 52] = rng() % 2 ? (int32_t)(rng() % 66000) - 100 : val(); }   // mincode / maxcode / valptr
                else if (what == 4) { sd_jpeg_huff_table& t = tables[rng() % tables.size()]; for (int i = 0; i < 8; ++i) t.vals[rng() % 256] = (uint8_t)rng(); }
                else if (what == 5) { int32_t* p = &desc.height; p[rng() % 14] = val(); }                 // height .. blocks_h[2]
                else if (what == 6) { desc.coef_offset[rng() % 3] = (int64_t)val(); }
                else if (what == 7) { uint32_t* p = &fr.clean_bytes; p[rng() % 3] = rng() % 2 ? (uint32_t)val() : (uint32_t)(rng() % (scan.size() + 300)); }   // clean_bytes, subseq_bytes, n_pieces
                else { const int r = rng() % 4; if (r == 0) byte_stride = rng() % (scan.size() + 1); else if (r == 1) interval_stride = rng() % (iv.size() + 1); else if (r == 2) coef_stride = (rng() % (coef_stride / 2 + 1)) * 2; else piece = rng() % 2 ? 32 << (rng() % 6) : (int)(rng() % 2100); }
            }
            std::vector<uint8_t> scan2 = head(scan, byte_stride);
            std::vector<int16_t> coef(coef_stride / 2, (int16_t)0x5a5a);
            std::vector<sd_jpeg_sync_interval> iv2 = head(iv, interval_stride);
            int32_t status = -1;
            // (the vectors may be empty: data() of an empty vector may be null, which the entry point refuses)
            const sd_status ds = sd_jpeg_sync_decode_host(scan2.data(), byte_stride, &desc, &fr, iv2.data(), interval_stride, tables.data(), 1, piece, coef.data(),
                                                          coef_stride, &status);
            if (ds == SD_OK) ++plan_passed;
        }
    }
    printf("eligible %ld: file mutations accepted-and-equal %ld, accepted by the host decoder but flagged not-synchronised %ld / bits-ran-out %ld, "
           "refused-by-both %ld; plan mutations %ld, of which the argument checks passed %ld\n",
           eligible, accepted, flagged5, flagged6, refused, plan_runs, plan_passed);
    return 0;
}
