// Host side of the result images' banner text: the CPU statement of sd_text_draw_rw (the items of a record as data, and a rasteriser of
// text_draw.hpp's rule for any items) and the font as data.  Every decision -- glyphs, number format, origins, which pixel a stroke
// paints -- is a function of text_draw.hpp, which the kernels of text_gpu.hip run too.  No handle, no GPU.
#include "../../include/semdepth.h"
#include "text_draw.hpp"

#include <algorithm>
#include <cstring>

static_assert(sizeof(sd_text_item) == SD_TEXT_MAX_BYTES + 24, "sd_text_item has no padding");

static bool depth_ok(const char* depth_text, int* len) {
    if (!depth_text) return false;
    const size_t n = strnlen(depth_text, sdtext::kMaxDepthBytes + 1);
    *len = (int)n;
    return n <= (size_t)sdtext::kMaxDepthBytes;
}

extern "C" sd_status sd_text_items_rw_host(const sd_rw_result* record, const char* depth_text, int dst_h, int dst_w, sd_text_item* items_out,
                                           int* n_out) {
    int dlen = 0;
    if (!record || !items_out || !n_out || !depth_ok(depth_text, &dlen) || dst_h < 1 || dst_w < 1 || dst_h > sdtext::kMaxExtent ||
        dst_w > sdtext::kMaxExtent)
        return SD_ERR_INVALID;
    *n_out = sdtext::sequence_items(*record, reinterpret_cast<const uint8_t*>(depth_text), dlen, dst_h, dst_w, items_out);
    return SD_OK;
}

extern "C" sd_status sd_text_draw_host(uint8_t* img_host, int h, int w, const sd_text_item* items, int n) {
    using namespace sdtext;
    if (!img_host || n < 0 || (n > 0 && !items) || h < 1 || w < 1 || h > kMaxExtent || w > kMaxExtent) return SD_ERR_INVALID;
    for (int i = 0; i < n; ++i)
        if (!item_ok(items[i])) return SD_ERR_INVALID;
    for (int i = 0; i < n; ++i) {
        const sd_text_item& it = items[i];
        const int r = it.thickness * 128;
        int pen = 0;
        for (int c = 0; c < it.len; ++c) {
            const Glyph g = glyph_of(it.text[c]);
            for (int j = 0; j < g.n; ++j) {
                const Seg s = seg_at(it, pen, g.first + j);
                // a pixel outside the segment's bounding box widened by r is farther than r from it
                const int x0 = std::max(0, ceil256(std::min(s.ax, s.bx) - r)), x1 = std::min(w - 1, floor256(std::max(s.ax, s.bx) + r));
                const int y0 = std::max(0, ceil256(std::min(s.ay, s.by) - r)), y1 = std::min(h - 1, floor256(std::max(s.ay, s.by) + r));
                for (int y = y0; y <= y1; ++y)
                    for (int x = x0; x <= x1; ++x)
                        if (hit(s, x, y, r)) std::memcpy(img_host + ((size_t)y * w + x) * 3, it.bgr, 3);
            }
            pen += g.adv;
        }
    }
    return SD_OK;
}

extern "C" sd_status sd_text_glyph(int code, int8_t* segs_out, int* n_out, int* advance_out) {
    if (code < 0 || code > 255 || !segs_out || !n_out || !advance_out) return SD_ERR_INVALID;
    const sdtext::Glyph g = sdtext::glyph_of((unsigned)code);
    for (int j = 0; j < g.n; ++j)
        for (int k = 0; k < 4; ++k) segs_out[4 * j + k] = sdtext::kSeg[g.first + j][k];
    *n_out = g.n;
    *advance_out = g.adv;
    return SD_OK;
}
