// Host-side helper of the input stage: PNG scanline reconstruction for the frame reader that replaces
// cv2.imread (semantic_depth.py:105, semantic_depth_cityscapes_sequence.py:123).  The DEFLATE stream is inflated by zlib
// (Python's zlib module, which releases the GIL); what remains per frame is this serial byte recurrence (PNG spec §9,
// filter types 0-4) plus the channel shuffle to OpenCV's 3-channel BGR layout.  On the default route (FrameFeeder(png="host"))
// there is no GPU work: the Paeth/Average predictors are a dependency chain along each row and host cores run it while the GPU
// computes.  The opt-in split route (png="device": sd_png_inflate_rows / sd_inflate_files_png below) leaves only the chunk walk and
// the inflate here and hands the recurrence to png_in_gpu.hip, a row per lane; sd_png_unfilter_bgr stays the yardstick of both.
#include "../../include/semdepth.h"

#include <cstdlib>
#include <cstring>

extern "C" sd_status sd_png_unfilter_bgr(const uint8_t* filtered, int height, int width, int channels, uint8_t* bgr_out) {
    if (!filtered || !bgr_out || height <= 0 || width <= 0 || channels < 1 || channels > 4) return SD_ERR_INVALID;
    const int bpp = channels, stride = width * channels;
    uint8_t* prev = static_cast<uint8_t*>(std::calloc((size_t)stride, 1));
    uint8_t* cur = static_cast<uint8_t*>(std::malloc((size_t)stride));
    if (!prev || !cur) { std::free(prev); std::free(cur); return SD_ERR_INVALID; }
    for (int y = 0; y < height; ++y) {
        const uint8_t* row = filtered + (size_t)y * (stride + 1);
        const int ft = row[0];
        const uint8_t* s = row + 1;
        switch (ft) {
            case 0: std::memcpy(cur, s, (size_t)stride); break;
            case 1:
                for (int i = 0; i < bpp; ++i) cur[i] = s[i];
                for (int i = bpp; i < stride; ++i) cur[i] = (uint8_t)(s[i] + cur[i - bpp]);
                break;
            case 2:
                for (int i = 0; i < stride; ++i) cur[i] = (uint8_t)(s[i] + prev[i]);
                break;
            case 3:
                for (int i = 0; i < bpp; ++i) cur[i] = (uint8_t)(s[i] + (prev[i] >> 1));
                for (int i = bpp; i < stride; ++i) cur[i] = (uint8_t)(s[i] + ((cur[i - bpp] + prev[i]) >> 1));
                break;
            case 4:
                for (int i = 0; i < bpp; ++i) cur[i] = (uint8_t)(s[i] + prev[i]);       // paeth(0, b, 0) = b
                for (int i = bpp; i < stride; ++i) {
                    const int a = cur[i - bpp], b = prev[i], c = prev[i - bpp];
                    const int p = a + b - c, pa = std::abs(p - a), pb = std::abs(p - b), pc = std::abs(p - c);
                    const int pr = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
                    cur[i] = (uint8_t)(s[i] + pr);
                }
                break;
            default: std::free(prev); std::free(cur); return SD_ERR_INVALID;
        }
        uint8_t* o = bgr_out + (size_t)y * width * 3;
        if (channels >= 3) {                      // RGB / RGBA -> BGR (cv2.IMREAD_COLOR drops alpha)
            for (int x = 0; x < width; ++x) { o[3 * x] = cur[bpp * x + 2]; o[3 * x + 1] = cur[bpp * x + 1]; o[3 * x + 2] = cur[bpp * x]; }
        } else {                                  // gray / gray + alpha -> replicated
            for (int x = 0; x < width; ++x) { o[3 * x] = o[3 * x + 1] = o[3 * x + 2] = cur[bpp * x]; }
        }
        uint8_t* t = prev; prev = cur; cur = t;
    }
    std::free(prev); std::free(cur);
    return SD_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Whole-file decode and the batch reader (round 3): one native call per frame -- chunk walk, zlib inflate straight into a
// scratch buffer, scanline reconstruction, BGR shuffle, palette expansion -- and one native call per BATCH that reads and
// decodes a list of files on its own threads.  Nothing of the per-frame work runs under the Python interpreter lock any
// more (the Python-side form joined the IDAT chunks, let zlib.decompress grow its output and copied the frame twice under
// the lock: 64 threads decoded 8.8x, not 64x, what one did).
// ---------------------------------------------------------------------------------------------------------------------
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <thread>
#include <vector>

#include "file_pool.hpp"

namespace {

inline uint32_t be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }
const uint8_t kPngSig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};

struct PngHead { int w = 0, h = 0, depth = 0, ctype = 0, interlace = 0, channels = 0; };

// IHDR of a PNG byte stream; false when it is not a PNG or not one this reader takes (8-bit, non-interlaced)
bool png_head(const uint8_t* f, size_t len, PngHead& hd) {
    if (!f || len < 8 + 25 || std::memcmp(f, kPngSig, 8) != 0) return false;
    if (be32(f + 8) != 13 || std::memcmp(f + 12, "IHDR", 4) != 0) return false;
    hd.w = (int)be32(f + 16); hd.h = (int)be32(f + 20);
    hd.depth = f[24]; hd.ctype = f[25]; hd.interlace = f[28];
    switch (hd.ctype) { case 0: hd.channels = 1; break; case 2: hd.channels = 3; break; case 3: hd.channels = 1; break;
                        case 4: hd.channels = 2; break; case 6: hd.channels = 4; break; default: return false; }
    return hd.depth == 8 && hd.interlace == 0 && hd.w > 0 && hd.h > 0;
}

sd_status png_decode(const uint8_t* f, size_t len, uint8_t* out, size_t out_cap, int* h_out, int* w_out) {
    PngHead hd;
    if (!png_head(f, len, hd)) return SD_ERR_INVALID;
    if (h_out) *h_out = hd.h;
    if (w_out) *w_out = hd.w;
    if (!out) return SD_OK;                                     // (size query)
    if (out_cap < (size_t)hd.h * hd.w * 3) return SD_ERR_INVALID;
    const size_t raw_len = (size_t)hd.h * (1 + (size_t)hd.w * hd.channels);
    std::vector<uint8_t> raw(raw_len);
    z_stream zs;
    std::memset(&zs, 0, sizeof(zs));
    if (inflateInit(&zs) != Z_OK) return SD_ERR_INVALID;
    zs.next_out = raw.data();
    zs.avail_out = (uInt)raw_len;
    const uint8_t* plte = nullptr;
    size_t plte_n = 0;
    bool done = false, ok = true;
    for (size_t p = 8; p + 12 <= len && !done;) {
        const uint32_t n = be32(f + p);
        if (p + 12 + (size_t)n > len) { ok = false; break; }
        const uint8_t* tag = f + p + 4;
        const uint8_t* body = f + p + 8;
        if (!std::memcmp(tag, "IDAT", 4)) {                     // the zlib stream runs through every IDAT chunk in file order
            zs.next_in = const_cast<Bytef*>(body);
            zs.avail_in = n;
            const int r = inflate(&zs, Z_NO_FLUSH);
            if (r != Z_OK && r != Z_STREAM_END) { ok = false; break; }
        } else if (!std::memcmp(tag, "PLTE", 4)) {
            plte = body; plte_n = n / 3;
        } else if (!std::memcmp(tag, "IEND", 4)) {
            done = true;
        }
        p += 12 + (size_t)n;
    }
    const bool full = zs.total_out == raw_len;
    inflateEnd(&zs);
    if (!ok || !full) return SD_ERR_INVALID;
    const sd_status st = sd_png_unfilter_bgr(raw.data(), hd.h, hd.w, hd.channels, out);
    if (st != SD_OK) return st;
    if (hd.ctype == 3) {                                        // palette indices (replicated by the helper) -> BGR palette entries
        if (!plte) return SD_ERR_INVALID;
        const size_t npx = (size_t)hd.h * hd.w;
        for (size_t i = 0; i < npx; ++i) {
            const size_t k = out[3 * i];
            if (k >= plte_n) return SD_ERR_INVALID;
            out[3 * i] = plte[3 * k + 2]; out[3 * i + 1] = plte[3 * k + 1]; out[3 * i + 2] = plte[3 * k];
        }
    }
    return SD_OK;
}

// PNG or baseline JPEG (host_jpeg.cpp), by signature
sd_status image_decode(const uint8_t* f, size_t len, uint8_t* out, size_t out_cap, int* h_out, int* w_out) {
    if (f && len >= 2 && f[0] == 0xFF && f[1] == 0xD8) return sd_jpeg_decode_bgr(f, len, out, out_cap, h_out, w_out);
    try {                                                       // (no exception crosses the C ABI or a worker thread: an allocation failure is a refused file)
        return png_decode(f, len, out, out_cap, h_out, w_out);
    } catch (...) {
        return SD_ERR_INVALID;
    }
}

}  // namespace

extern "C" sd_status sd_png_decode_bgr(const uint8_t* file_host, size_t len, uint8_t* bgr_out_host, size_t out_capacity, int* height_out,
                                       int* width_out) {
    try {
        return png_decode(file_host, len, bgr_out_host, out_capacity, height_out, width_out);
    } catch (...) {
        return SD_ERR_INVALID;
    }
}

extern "C" sd_status sd_image_decode_bgr(const uint8_t* file_host, size_t len, uint8_t* bgr_out_host, size_t out_capacity, int* height_out,
                                         int* width_out) {
    return image_decode(file_host, len, bgr_out_host, out_capacity, height_out, width_out);
}

extern "C" sd_status sd_decode_files_bgr(const char* const* paths, int n, int height, int width, uint8_t* out_host, size_t frame_stride,
                                         int threads, int* status_out) {
    if (!paths || n < 0 || height <= 0 || width <= 0 || !out_host || frame_stride < (size_t)height * width * 3) return SD_ERR_INVALID;
    return sdfiles::for_each_file(paths, n, threads, status_out, true, [&](int i, const std::vector<uint8_t>& file) -> sd_status {
        int h = 0, w = 0;
        sd_status st = image_decode(file.data(), file.size(), nullptr, 0, &h, &w);
        if (st == SD_OK && (h != height || w != width)) st = SD_ERR_INVALID;     // every frame of a batch has the batch's shape
        if (st == SD_OK) st = image_decode(file.data(), file.size(), out_host + (size_t)i * frame_stride, frame_stride, nullptr, nullptr);
        return st;
    });
}

// the same pool for the split JPEG route: file i -> quantised coefficients + descriptor (sd_jpeg_decode_coefficients); a file that is
// not a JPEG is reported as SD_ERR_FORMAT and left to sd_decode_files_bgr
extern "C" sd_status sd_decode_files_jpeg_coef(const char* const* paths, int n, int height, int width, int16_t* coef_out_host,
                                               size_t frame_stride_bytes, sd_jpeg_frame_desc* descs_out, int threads, int* status_out) {
    if (!paths || n < 0 || height <= 0 || width <= 0 || !coef_out_host || !descs_out || (frame_stride_bytes & 1)) return SD_ERR_INVALID;
    return sdfiles::for_each_file(paths, n, threads, status_out, false, [&](int i, const std::vector<uint8_t>& file) -> sd_status {
        if (file.size() < 2 || file[0] != 0xFF || file[1] != 0xD8) return SD_ERR_FORMAT;
        sd_jpeg_frame_desc d;
        sd_status st = sd_jpeg_decode_coefficients(file.data(), file.size(), nullptr, 0, &d);
        if (st == SD_OK && !sdfiles::oriented_size_is(d, height, width)) st = SD_ERR_INVALID;
        if (st == SD_OK)
            st = sd_jpeg_decode_coefficients(file.data(), file.size(), coef_out_host + (size_t)i * (frame_stride_bytes / 2), frame_stride_bytes,
                                             &descs_out[i]);
        return st;
    });
}

// ---------------------------------------------------------------------------------------------------------------------
// The split PNG route (FrameFeeder(png="device")): the host keeps the serial part -- chunk walk and inflate, straight into the
// caller's (pinned) staging -- and png_in_gpu.hip runs the scanline recurrence, the channel map and the palette lookup for the
// whole batch.  The same png_head and the same walk as png_decode above; what png_decode learns from sd_png_unfilter_bgr (a
// filter byte above 4) is checked here with one byte read per row, so the device never sees a row type it cannot name.
// ---------------------------------------------------------------------------------------------------------------------
namespace {

sd_status png_inflate(const uint8_t* f, size_t len, uint8_t* rows, size_t cap, sd_png_frame_desc* desc) {
    PngHead hd;
    if (!png_head(f, len, hd)) return SD_ERR_INVALID;
    if (desc) {
        std::memset(desc, 0, sizeof(*desc));
        desc->height = hd.h; desc->width = hd.w; desc->channels = hd.channels; desc->color_type = hd.ctype;
    }
    if (!rows) return SD_OK;                                    // (descriptor query)
    const size_t row_len = 1 + (size_t)hd.w * hd.channels, raw_len = (size_t)hd.h * row_len;
    if (cap < raw_len || raw_len > 0xFFFFFFFFu) return SD_ERR_INVALID;      // before anything is written
    z_stream zs;
    std::memset(&zs, 0, sizeof(zs));
    if (inflateInit(&zs) != Z_OK) return SD_ERR_INVALID;
    zs.next_out = rows;
    zs.avail_out = (uInt)raw_len;
    const uint8_t* plte = nullptr;
    size_t plte_n = 0;
    bool done = false, ok = true;
    for (size_t p = 8; p + 12 <= len && !done;) {
        const uint32_t n = be32(f + p);
        if (p + 12 + (size_t)n > len) { ok = false; break; }
        const uint8_t* tag = f + p + 4;
        const uint8_t* body = f + p + 8;
        if (!std::memcmp(tag, "IDAT", 4)) {
            zs.next_in = const_cast<Bytef*>(body);
            zs.avail_in = n;
            const int r = inflate(&zs, Z_NO_FLUSH);
            if (r != Z_OK && r != Z_STREAM_END) { ok = false; break; }
        } else if (!std::memcmp(tag, "PLTE", 4)) {
            plte = body; plte_n = n / 3;
        } else if (!std::memcmp(tag, "IEND", 4)) {
            done = true;
        }
        p += 12 + (size_t)n;
    }
    const bool full = zs.total_out == raw_len;
    inflateEnd(&zs);
    if (!ok || !full) return SD_ERR_INVALID;
    for (int y = 0; y < hd.h; ++y)
        if (rows[(size_t)y * row_len] > 4) return SD_ERR_INVALID;
    if (hd.ctype == 3) {
        if (!plte) return SD_ERR_INVALID;
        if (desc) {
            const size_t k = plte_n < 256 ? plte_n : 256;       // (an index is a byte: entries past 255 are never named)
            desc->palette_entries = (int32_t)k;
            std::memcpy(desc->palette, plte, 3 * k);
        }
    }
    return SD_OK;
}

}  // namespace

extern "C" sd_status sd_png_inflate_rows(const uint8_t* file_host, size_t len, uint8_t* rows_out_host, size_t capacity, sd_png_frame_desc* desc_out) {
    try {
        return png_inflate(file_host, len, rows_out_host, capacity, desc_out);
    } catch (...) {
        return SD_ERR_INVALID;
    }
}

extern "C" sd_status sd_inflate_files_png(const char* const* paths, int n, int height, int width, uint8_t* rows_out_host, size_t frame_stride,
                                          sd_png_frame_desc* descs_out, int threads, int* status_out) {
    if (!paths || n < 0 || height <= 0 || width <= 0 || !rows_out_host || !descs_out) return SD_ERR_INVALID;
    return sdfiles::for_each_file(paths, n, threads, status_out, false, [&](int i, const std::vector<uint8_t>& file) -> sd_status {
        if (file.size() < 8 || std::memcmp(file.data(), kPngSig, 8) != 0) return SD_ERR_FORMAT;
        sd_png_frame_desc d;
        sd_status st = png_inflate(file.data(), file.size(), nullptr, 0, &d);
        if (st == SD_OK && (d.height != height || d.width != width)) st = SD_ERR_INVALID;
        if (st == SD_OK) st = png_inflate(file.data(), file.size(), rows_out_host + (size_t)i * frame_stride, frame_stride, &descs_out[i]);
        return st;
    });
}

// ---------------------------------------------------------------------------------------------------------------------
// The writer of the sequence tool's result images (cv2.imwrite at seq:336): BGR -> RGB rows with filter type 0, one zlib
// stream deflated in pieces of a few rows (no whole-frame raw copy), one IDAT per deflate output block, on native threads.
// ---------------------------------------------------------------------------------------------------------------------
namespace {

void put_be32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v; }

bool write_chunk(FILE* fp, const char* tag, const uint8_t* data, uint32_t n) {
    uint8_t hd[8];
    put_be32(hd, n);
    std::memcpy(hd + 4, tag, 4);
    uLong crc = crc32(0L, reinterpret_cast<const Bytef*>(tag), 4);
    if (n) crc = crc32(crc, data, n);
    uint8_t tl[4];
    put_be32(tl, (uint32_t)crc);
    return std::fwrite(hd, 1, 8, fp) == 8 && (n == 0 || std::fwrite(data, 1, n, fp) == n) && std::fwrite(tl, 1, 4, fp) == 4;
}

sd_status png_encode_file(const char* path, const uint8_t* bgr, int h, int w, int level) {
    FILE* fp = std::fopen(path, "wb");
    if (!fp) return SD_ERR_NOTFOUND;
    bool ok = std::fwrite(kPngSig, 1, 8, fp) == 8;
    uint8_t ihdr[13];
    put_be32(ihdr, (uint32_t)w);
    put_be32(ihdr + 4, (uint32_t)h);
    ihdr[8] = 8; ihdr[9] = 2; ihdr[10] = 0; ihdr[11] = 0; ihdr[12] = 0;       // 8-bit RGB, deflate, filter method 0, no interlace
    ok = ok && write_chunk(fp, "IHDR", ihdr, 13);
    z_stream zs;
    std::memset(&zs, 0, sizeof(zs));
    if (ok && deflateInit(&zs, level) != Z_OK) ok = false;
    const size_t row = 1 + (size_t)w * 3;
    const int rows_per_piece = (int)std::max<size_t>(1, (size_t)(256 << 10) / row);
    std::vector<uint8_t> raw, out(256 << 10);
    if (ok) {
        raw.resize(row * (size_t)std::min(rows_per_piece, h));
        for (int y0 = 0; ok && y0 < h; y0 += rows_per_piece) {
            const int ny = std::min(rows_per_piece, h - y0);
            for (int y = 0; y < ny; ++y) {
                uint8_t* r = raw.data() + (size_t)y * row;
                const uint8_t* s = bgr + (size_t)(y0 + y) * w * 3;
                r[0] = 0;
                for (int x = 0; x < w; ++x) { r[1 + 3 * x] = s[3 * x + 2]; r[2 + 3 * x] = s[3 * x + 1]; r[3 + 3 * x] = s[3 * x]; }
            }
            zs.next_in = raw.data();
            zs.avail_in = (uInt)(row * ny);
            const int flush = y0 + ny >= h ? Z_FINISH : Z_NO_FLUSH;
            int r;
            do {
                zs.next_out = out.data();
                zs.avail_out = (uInt)out.size();
                r = deflate(&zs, flush);
                if (r == Z_STREAM_ERROR) { ok = false; break; }
                const uint32_t got = (uint32_t)(out.size() - zs.avail_out);
                if (got && !write_chunk(fp, "IDAT", out.data(), got)) { ok = false; break; }
            } while (zs.avail_out == 0 || (flush == Z_FINISH && r != Z_STREAM_END));
        }
        deflateEnd(&zs);
    }
    ok = ok && write_chunk(fp, "IEND", nullptr, 0);
    ok = (std::fclose(fp) == 0) && ok;
    return ok ? SD_OK : SD_ERR_NOTFOUND;
}

}  // namespace

extern "C" sd_status sd_png_encode_bgr_files(const char* const* paths, int n, int height, int width, const uint8_t* frames_host,
                                             size_t frame_stride, int level, int threads, int* status_out) {
    if (!paths || n < 0 || height <= 0 || width <= 0 || (n > 0 && !frames_host) || frame_stride < (size_t)height * width * 3 || level < 0 ||
        level > 9)
        return SD_ERR_INVALID;
    if (threads <= 0) threads = (int)std::thread::hardware_concurrency();
    threads = threads < 1 ? 1 : (threads > n ? (n > 0 ? n : 1) : threads);
    std::atomic<int> next(0), failed(0);
    auto work = [&]() {
        for (;;) {
            const int i = next.fetch_add(1);
            if (i >= n) break;
            sd_status st = SD_ERR_NOTFOUND;
            try {
                if (paths[i]) st = png_encode_file(paths[i], frames_host + (size_t)i * frame_stride, height, width, level);
            } catch (...) {
                st = SD_ERR_INVALID;
            }
            if (status_out) status_out[i] = st;
            if (st != SD_OK) failed.fetch_add(1);
        }
    };
    std::vector<std::thread> pool;
    try {
        for (int t = 1; t < threads; ++t) pool.emplace_back(work);
    } catch (...) {
    }
    work();
    for (auto& th : pool) th.join();
    return failed.load() ? SD_ERR_INVALID : SD_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// The device route of the result images (png_gpu.hip makes one zlib stream per frame on the GPU): the CPU statement of that
// encoder -- the same functions of png_deflate.hpp, walked by one loop -- and the writer that wraps finished streams in PNG
// chunks on native threads.
// ---------------------------------------------------------------------------------------------------------------------
#include "png_deflate.hpp"

namespace {

struct ByteSink {
    std::vector<uint8_t>& out;
    uint64_t acc = 0;
    int nacc = 0;
    void put(uint32_t v, int n) {
        acc |= (uint64_t)v << nacc;
        nacc += n;
        while (nacc >= 8) { out.push_back((uint8_t)acc); acc >>= 8; nacc -= 8; }
    }
    void align() { if (nacc > 0) { out.push_back((uint8_t)acc); acc = 0; nacc = 0; } }
};

// f(position, token, byte value) for every token of the chunk d[0..len), run by run
template <class F>
void chunk_tokens(const uint8_t* d, uint32_t len, F&& f) {
    for (uint32_t s = 0; s < len;) {
        uint32_t e = s + 1;
        while (e < len && d[e] == d[s]) ++e;
        for (uint32_t p = 0; p < e - s; ++p) {
            const int tok = sdpng::run_token(e - s, p);
            if (tok) f(s + p, tok, d[s]);
        }
        s = e;
    }
}

void encode_zlib(const uint8_t* frame, int h, int w, std::vector<uint8_t>& out) {
    using namespace sdpng;
    const size_t total = filtered_len(h, w), rowlen = 1 + 3 * (size_t)w;
    out.clear();
    out.reserve(stream_bound(h, w));
    out.push_back(0x78);
    out.push_back(0x01);
    std::vector<uint8_t> d(kChunk);
    uint32_t adler_a = 1, adler_b = 0;
    HuffScratch sc;
    ChunkCodes cc;
    for (size_t g0 = 0; g0 < total; g0 += kChunk) {
        const uint32_t len = (uint32_t)std::min<size_t>(kChunk, total - g0);
        uint32_t y = (uint32_t)(g0 / rowlen), k = (uint32_t)(g0 - (size_t)y * rowlen);
        uint64_t sa = 0, sb = 0;
        for (uint32_t i = 0; i < len; ++i) {
            d[i] = filtered_byte(frame, w, y, k);
            sa += d[i];
            sb += (uint64_t)(len - i) * d[i];
            if (++k == rowlen) { k = 0; ++y; }
        }
        adler_append(adler_a, adler_b, len, (uint32_t)(sa % kAdlerMod), (uint32_t)(sb % kAdlerMod));
        uint32_t hist[kLitSyms] = {0};
        chunk_tokens(d.data(), len, [&](uint32_t, int tok, uint8_t v) {
            int eb, ev;
            hist[tok == 1 ? (int)v : length_symbol(tok, &eb, &ev)]++;
        });
        hist[kEob] = 1;
        const int n = sort_keys(hist, kLitSyms, sc.key);
        build_chunk_codes(hist, n, sc, cc);
        const size_t before = out.size();
        if (chunk_is_dynamic(cc, len)) {
            ByteSink sink{out};
            write_block_header(sink, cc);
            chunk_tokens(d.data(), len, [&](uint32_t, int tok, uint8_t v) {
                int nb;
                const uint32_t bits = token_bits(cc, tok, v, &nb);
                sink.put(bits, nb);
            });
            sink.put(cc.llcode[kEob], cc.ll[kEob]);
            sink.put(0, 3);                              // the empty stored block: BFINAL 0, BTYPE 00, padding, LEN 0, NLEN FFFF
            sink.align();
        } else {
            const uint8_t head[5] = {0, (uint8_t)len, (uint8_t)(len >> 8), (uint8_t)~len, (uint8_t)(~len >> 8)};
            out.insert(out.end(), head, head + 5);
            out.insert(out.end(), d.begin(), d.begin() + len);
            out.push_back(0);
        }
        const uint8_t sync[4] = {0, 0, 0xFF, 0xFF};
        out.insert(out.end(), sync, sync + 4);
        if (out.size() - before != chunk_coded_bytes(cc, len)) throw 0;       // (the size the device lays the stream out with)
    }
    const uint32_t adler = (adler_b << 16) | adler_a;
    const uint8_t tail[9] = {1, 0, 0, 0xFF, 0xFF, (uint8_t)(adler >> 24), (uint8_t)(adler >> 16), (uint8_t)(adler >> 8), (uint8_t)adler};
    out.insert(out.end(), tail, tail + 9);
}

sd_status png_stream_file(const char* path, int h, int w, const uint8_t* stream, size_t size) {
    FILE* fp = std::fopen(path, "wb");
    if (!fp) return SD_ERR_NOTFOUND;
    bool ok = std::fwrite(kPngSig, 1, 8, fp) == 8;
    uint8_t ihdr[13];
    put_be32(ihdr, (uint32_t)w);
    put_be32(ihdr + 4, (uint32_t)h);
    ihdr[8] = 8; ihdr[9] = 2; ihdr[10] = 0; ihdr[11] = 0; ihdr[12] = 0;
    ok = ok && write_chunk(fp, "IHDR", ihdr, 13);
    const size_t piece = (size_t)1 << 20;                                      // one IDAT per MiB of the stream
    for (size_t p = 0; ok && p < size; p += piece) ok = write_chunk(fp, "IDAT", stream + p, (uint32_t)std::min(piece, size - p));
    ok = ok && write_chunk(fp, "IEND", nullptr, 0);
    ok = (std::fclose(fp) == 0) && ok;
    return ok ? SD_OK : SD_ERR_NOTFOUND;
}

}  // namespace

extern "C" sd_status sd_png_encode_zlib_host(const uint8_t* frame_host, int height, int width, uint8_t* out_host, size_t cap, size_t* size_out) {
    if (!frame_host || !out_host || !size_out || height < 1 || width < 1 || height > sdpng::kMaxExtent || width > sdpng::kMaxExtent)
        return SD_ERR_INVALID;
    try {
        std::vector<uint8_t> out;
        encode_zlib(frame_host, height, width, out);
        if (out.size() > cap) return SD_ERR_INVALID;
        std::memcpy(out_host, out.data(), out.size());
        *size_out = out.size();
        return SD_OK;
    } catch (...) {
        return SD_ERR_INVALID;
    }
}

extern "C" sd_status sd_png_write_streams_files(const char* const* paths, int n, int height, int width, const uint8_t* streams_host,
                                                size_t stream_stride, const uint64_t* sizes_host, int threads, int* status_out) {
    if (!paths || n < 0 || height <= 0 || width <= 0 || (n > 0 && (!streams_host || !sizes_host))) return SD_ERR_INVALID;
    for (int i = 0; i < n; ++i)
        if (sizes_host[i] > stream_stride) return SD_ERR_INVALID;
    if (threads <= 0) threads = (int)std::thread::hardware_concurrency();
    threads = threads < 1 ? 1 : (threads > n ? (n > 0 ? n : 1) : threads);
    std::atomic<int> next(0), failed(0);
    auto work = [&]() {
        for (;;) {
            const int i = next.fetch_add(1);
            if (i >= n) break;
            sd_status st = SD_ERR_NOTFOUND;
            try {
                if (paths[i]) st = png_stream_file(paths[i], height, width, streams_host + (size_t)i * stream_stride, (size_t)sizes_host[i]);
            } catch (...) {
                st = SD_ERR_INVALID;
            }
            if (status_out) status_out[i] = st;
            if (st != SD_OK) failed.fetch_add(1);
        }
    };
    std::vector<std::thread> pool;
    try {
        for (int t = 1; t < threads; ++t) pool.emplace_back(work);
    } catch (...) {
    }
    work();
    for (auto& th : pool) th.join();
    return failed.load() ? SD_ERR_INVALID : SD_OK;
}
