// dev tool: fuzz harness of the JPEG entropy route's host side (CPU build under ASan + UBSan; it runs no GPU code): the plan
// (sd_jpeg_entropy_plan) and the CPU statement of the device decoder (sd_jpeg_entropy_decode_host), which runs the function the kernel
// runs (semantic_depth_amd/csrc/jpeg_entropy.hpp).  This is the evidence that no input makes that function read outside an interval's
// bytes or write outside a frame's coefficients.
//   g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -Iinclude scripts/fuzz_jpeg_entropy.cpp \
//       semantic_depth_amd/csrc/host_jpeg.cpp semantic_depth_amd/csrc/host_jpeg_entropy.cpp -lpthread -o /tmp/fuzz_jpeg_entropy
//   /tmp/fuzz_jpeg_entropy 20000 seed1.jpg seed2.jpg ...     (seeds: small JPEG files with restart intervals)
// Two kinds of iteration, from exact-size heap copies so that one byte too far is an ASan report:
//   A  the FILE is mutated (bit flips, random bytes, FF runs, inserted markers, truncation, a cut right behind a shortened SOS header -- in
//      the scan and, less often, in the header); when the plan still calls it eligible the CPU statement decodes it and the result is held against
//      sd_jpeg_decode_coefficients: the same descriptor and coefficients and status 0 where that decoder accepts the file, a non-zero
//      status where it refuses it.
//   B  the PLAN'S OUTPUTS are mutated (record fields, interval ranges, table entries, descriptor fields, strides); whatever the argument
//      checks still let through is decoded: nothing may crash or touch memory outside the buffers.
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
    if (argc < 3) { printf("usage: fuzz_jpeg_entropy ITERATIONS seed.jpg ...\n"); return 2; }
    const int iters = atoi(argv[1]);
    std::mt19937_64 rng(20261018);
    long eligible = 0, accepted = 0, refused = 0, plan_runs = 0, plan_passed = 0;
    constexpr size_t kCap = 4096;
    for (int a = 2; a < argc; ++a) {
        const std::vector<uint8_t> base = readf(argv[a]);
        if (base.size() < 4) { printf("cannot read %s\n", argv[a]); return 2; }
        const size_t s0 = scan_start(base);
        for (int it = 0; it < iters; ++it) {
            const bool plan_kind = it & 1;
            std::vector<uint8_t> f = base;
            if (!plan_kind || rng() % 4 == 0) {                                   // A (and a quarter of B starts from a mutated file)
                const int kind = rng() % 9;
                const size_t lo = rng() % 8 ? s0 : 0;                             // mostly the scan, sometimes the header
                auto at = [&]() { return lo + rng() % (f.size() - lo); };
                if (kind == 0) f.resize(2 + rng() % (f.size() - 1));
                else if (kind == 1) { int n = 1 + rng() % 4; for (int i = 0; i < n; ++i) f[at()] ^= (uint8_t)(1u << (rng() % 8)); }
                else if (kind == 2) { int n = 1 + rng() % 8; for (int i = 0; i < n; ++i) f[at()] = (uint8_t)rng(); }
                else if (kind == 3) { size_t p = at(), n = rng() % 16; for (size_t i = p; i < p + n && i < f.size(); ++i) f[i] = 0xff; }
                else if (kind == 4) { const uint8_t m[2] = {0xFF, (uint8_t)(0xD0 + rng() % 10)}; f.insert(f.begin() + at(), m, m + 2); }
                else if (kind == 5) { size_t p = at(), n = 1 + rng() % 40; if (p + n < f.size()) f.erase(f.begin() + p, f.begin() + p + n); }
                else if (kind == 6) { size_t p = at(); f.insert(f.begin() + p, (size_t)(rng() % 32), (uint8_t)(rng() % 3 ? 0 : 0xFF)); }
                else if (kind == 8) {                                             // the file cut right behind a SOS header whose length field is shortened
                    size_t q = 2;
                    while (q + 4 <= f.size() && f[q] == 0xFF && f[q + 1] != 0xDA) q += 2 + (((size_t)f[q + 2] << 8) | f[q + 3]);
                    if (q + 4 <= f.size() && f[q + 1] == 0xDA) {
                        const size_t n = 2 + rng() % 12;                          // 2: the payload begins at the end of the buffer
                        f[q + 2] = 0; f[q + 3] = (uint8_t)n;
                        if (q + 2 + n <= f.size()) f.resize(q + 2 + n);
                    }
                }
                else { int n = 1 + rng() % 48; for (int i = 0; i < n; ++i) f[at()] ^= (uint8_t)(1u << (rng() % 8)); }
            }
            // exact-size heap copies: one byte too far is a report
            std::vector<uint8_t> file(f.begin(), f.end());
            sd_jpeg_frame_desc desc;
            sd_jpeg_entropy_frame fr;
            std::vector<sd_jpeg_huff_table> tables(SD_JPEG_ENTROPY_TABLES);
            const size_t cap = rng() % 16 ? kCap : rng() % 64;                    // sometimes too little room for the ranges
            std::vector<sd_jpeg_interval> iv(cap);
            const sd_status ps = sd_jpeg_entropy_plan(file.data(), file.size(), &desc, &fr, tables.data(), iv.data(), cap);
            if (ps != SD_OK || !fr.eligible) continue;
            ++eligible;
            iv.resize(fr.n_intervals);
            iv.shrink_to_fit();
            std::vector<uint8_t> scan(file.begin() + fr.scan_begin, file.begin() + fr.scan_end);
            size_t byte_stride = scan.size(), interval_stride = iv.size(), coef_stride = coef_elems(desc) * 2;
            if (!plan_kind) {
                std::vector<int16_t> coef(coef_stride / 2, (int16_t)0x5a5a), ref(coef_stride / 2);
                int32_t status = -1;
                const sd_status ds = sd_jpeg_entropy_decode_host(scan.data(), byte_stride, &desc, &fr, iv.data(), interval_stride, tables.data(), 1,
                                                                 coef.data(), coef_stride, &status);
                if (ds != SD_OK) { printf("FAIL: an eligible plan was refused by the argument checks (%s, iteration %d)\n", argv[a], it); return 1; }
                sd_jpeg_frame_desc hd;
                const sd_status hs = sd_jpeg_decode_coefficients(file.data(), file.size(), ref.data(), coef_stride, &hd);
                if (hs == SD_OK) {
                    ++accepted;
                    if (status != 0 || std::memcmp(&hd, &desc, sizeof(hd)) != 0 || std::memcmp(coef.data(), ref.data(), coef_stride) != 0) {
                        printf("FAIL: differs from sd_jpeg_decode_coefficients (%s, iteration %d, status %d)\n", argv[a], it, status);
                        return 1;
                    }
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
                const int what = rng() % 8;
                auto val = [&]() -> int32_t { const int r = rng() % 6; return r == 0 ? 0 : r == 1 ? -1 : r == 2 ? (int32_t)(rng() % 5) : r == 3 ? (int32_t)(rng() % 70000) : r == 4 ? 0x7fffffff : (int32_t)rng(); };
                if (what == 0) { int32_t* p = &fr.ncomp; p[rng() % 17] = val(); }                         // ncomp .. comp_ac[2]
                else if (what == 1 && !iv.empty()) { sd_jpeg_interval& x = iv[rng() % iv.size()]; (rng() & 1 ? x.begin : x.end) = rng() % 3 ? (uint32_t)(rng() % (scan.size() + 2)) : (uint32_t)rng(); }
                else if (what == 2) { sd_jpeg_huff_table& t = tables[rng() % tables.size()]; for (int i = 0; i < 4; ++i) t.look[rng() % 512] = rng() % 3 ? (uint16_t)(((rng() % 11) << 8) | (rng() & 255)) : (uint16_t)rng(); }
                else if (what == 3) { sd_jpeg_huff_table& t = tables[rng() % tables.size()]; int32_t* p = t.mincode; p[rng() % 52] = rng() % 2 ? (int32_t)(rng() % 66000) - 100 : val(); }   // mincode / maxcode / valptr
                else if (what == 4) { sd_jpeg_huff_table& t = tables[rng() % tables.size()]; for (int i = 0; i < 8; ++i) t.vals[rng() % 256] = (uint8_t)rng(); }
                else if (what == 5) { int32_t* p = &desc.height; p[rng() % 14] = val(); }                 // height .. blocks_h[2]
                else if (what == 6) { desc.coef_offset[rng() % 3] = (int64_t)val(); }
                else { const int r = rng() % 3; if (r == 0) byte_stride = rng() % (scan.size() + 1); else if (r == 1) interval_stride = rng() % (iv.size() + 1); else coef_stride = (rng() % (coef_stride / 2 + 1)) * 2; }
            }
            std::vector<uint8_t> scan2(scan.begin(), scan.begin() + (byte_stride < scan.size() ? byte_stride : scan.size()));
            std::vector<int16_t> coef(coef_stride / 2, (int16_t)0x5a5a);
            std::vector<sd_jpeg_interval> iv2(iv.begin(), iv.begin() + (interval_stride < iv.size() ? interval_stride : iv.size()));
            int32_t status = -1;
            // (the vectors may be empty: data() of an empty vector may be null, which the entry point refuses)
            const sd_status ds = sd_jpeg_entropy_decode_host(scan2.data(), byte_stride, &desc, &fr, iv2.data(), interval_stride, tables.data(), 1, coef.data(),
                                                             coef_stride, &status);
            if (ds == SD_OK) ++plan_passed;
        }
    }
    printf("eligible %ld: file mutations accepted-and-equal %ld, refused-by-both %ld; plan mutations %ld, of which the argument checks passed %ld\n",
           eligible, accepted, refused, plan_runs, plan_passed);
    return 0;
}
