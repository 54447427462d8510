// Host side of the measurement lines of the result images: the CPU statement of sd_overlay_draw (the valid segments of a frame as data, in
// slot order, and a rasteriser of the paint rule for any segments).  Every decision -- the projection, the slots, the colours, which pixel a
// segment paints -- is a function of overlay_rule.hpp / text_draw.hpp, which the kernels of overlay_gpu.hip run too.  Compiled with
// -ffp-contract=off like the kernels.  No handle, no GPU.
#include "../../include/semdepth.h"
#include "overlay_rule.hpp"

#include <cstring>

static_assert(sizeof(sd_overlay_style) == 24 && sizeof(sd_overlay_segment) == 20, "the overlay structs have no padding");

extern "C" sd_status sd_overlay_segments_host(const sd_rw_result* record, const sd_f2f_result* f2f, const sd_rw_depth_result* rw_profile,
                                              const sd_f2f_depth_result* f2f_profile, int D, const sd_camera* cam, int net_h, int net_w, int dst_h,
                                              int dst_w, const sd_overlay_style* style, sd_overlay_segment* segs_out, int* n_out,
                                              int32_t* flag_out) {
    using namespace sdoverlay;
    if (!record || !cam || !style || !segs_out || !n_out || !flag_out || D < 0 || D > kMaxDepths || (D > 0 && !rw_profile) ||
        !sizes_ok(net_h, net_w, dst_h, dst_w) || !style_ok(*style, dst_h) || !camera_ok(*cam))
        return SD_ERR_INVALID;
    const View v = make_view(*cam, net_h, net_w, dst_h, dst_w);
    int n = 0;
    int32_t flag = 0;
    sd_overlay_segment seg;
    auto take = [&](int32_t state) {
        if (state == kOk) segs_out[n++] = seg;
        if (state == kDropped) flag |= 1;
    };
    for (int group = 0; group < 4; ++group)
        for (int i = 0; i < D; ++i) {
            const EntryPts e = entry_points(v, rw_profile + i, f2f_profile ? f2f_profile + i : nullptr);
            const EntryPts next = i + 1 < D ? entry_points(v, rw_profile + i + 1, f2f_profile ? f2f_profile + i + 1 : nullptr)
                                            : EntryPts{absent(), absent(), absent(), absent()};
            take(entry_slot(group, e, next, *style, &seg));
        }
    take(record_slot(v, *record, *style, &seg));
    take(fence_slot(v, f2f, *style, &seg));
    *n_out = n;
    *flag_out = flag;
    return SD_OK;
}

extern "C" sd_status sd_overlay_draw_host(uint8_t* img_host, int h, int w, const sd_overlay_segment* segs, int n, int clip_top) {
    using namespace sdoverlay;
    if (!img_host || n < 0 || (n > 0 && !segs) || h < 1 || w < 1 || h > kMaxExtent || w > kMaxExtent || clip_top < 0 || clip_top > h)
        return SD_ERR_INVALID;
    for (int i = 0; i < n; ++i)
        if (!segment_ok(segs[i])) return SD_ERR_INVALID;
    for (int i = 0; i < n; ++i) {
        const sd_overlay_segment& s = segs[i];
        int32_t box[4];
        if (!seg_box(s, h, w, clip_top, box)) continue;
        const sdtext::Seg g = seg_of(s);
        const int r = (int)s.thickness * 128;
        for (int y = box[1]; y <= box[3]; ++y)
            for (int x = box[0]; x <= box[2]; ++x)
                if (sdtext::hit(g, x, y, r)) std::memcpy(img_host + ((size_t)y * w + x) * 3, s.bgr, 3);
    }
    return SD_OK;
}
