// Host twins of seg_eval_gpu.hip (sd_resize_pil_bilinear_u8_host / sd_seg_confusion_host; contract: include/semdepth.h): argument checks
// plus plain loops through pil_resample.hpp, the rule the kernels use.  The CPU tests hold these to Pillow and np.bincount, the GPU tests
// hold the kernels to these.  No HIP call is made here.
#include "../../include/semdepth.h"
#include "pil_resample.hpp"

#include <vector>

extern "C" sd_status sd_resize_pil_workspace(int B, int src_h, int src_w, int dst_h, int dst_w, int channels, size_t* bytes_out) {
    if (!bytes_out || B < 1 || B > 65535 || (channels != 1 && channels != 3) || !sdpil::axis_ok(src_h, dst_h) || !sdpil::axis_ok(src_w, dst_w))
        return SD_ERR_INVALID;
    *bytes_out = sdpil::workspace_bytes(B, src_h, src_w, dst_h, dst_w, channels);
    return SD_OK;
}

extern "C" sd_status sd_resize_pil_bilinear_u8_host(const uint8_t* src, int B, int src_h, int src_w, int pixel_stride, int channels, int reverse,
                                                    uint8_t* dst, int dst_h, int dst_w) {
    using namespace sdpil;
    if (!src || !dst || B < 1 || (channels != 1 && channels != 3) || pixel_stride < channels || pixel_stride > 4 || !axis_ok(src_h, dst_h) ||
        !axis_ok(src_w, dst_w))
        return SD_ERR_INVALID;
    Windows wx, wy;
    pil_windows(src_w, dst_w, wx);
    pil_windows(src_h, dst_h, wy);
    const int C = channels;
    std::vector<uint8_t> mid((size_t)src_h * dst_w * C);
    for (int b = 0; b < B; ++b) {
        const uint8_t* s = src + (size_t)b * src_h * src_w * pixel_stride;
        uint8_t* o = dst + (size_t)b * dst_h * dst_w * C;
        for (int y = 0; y < src_h; ++y)
            for (int x = 0; x < dst_w; ++x) {
                const int x0 = wx.bounds[(size_t)x * 2], n = wx.bounds[(size_t)x * 2 + 1];
                for (int c = 0; c < C; ++c) {
                    const int cs = reverse ? C - 1 - c : c;
                    int32_t acc = kHalf;
                    for (int i = 0; i < n; ++i) acc += wx.k[(size_t)i * dst_w + x] * s[((size_t)y * src_w + x0 + i) * pixel_stride + cs];
                    mid[((size_t)y * dst_w + x) * C + c] = clip_u8(acc);
                }
            }
        for (int y = 0; y < dst_h; ++y) {
            const int y0 = wy.bounds[(size_t)y * 2], n = wy.bounds[(size_t)y * 2 + 1];
            for (int j = 0; j < dst_w * C; ++j) {
                int32_t acc = kHalf;
                for (int i = 0; i < n; ++i) acc += wy.k[(size_t)i * dst_h + y] * mid[(size_t)(y0 + i) * dst_w * C + j];
                o[(size_t)y * dst_w * C + j] = clip_u8(acc);
            }
        }
    }
    return SD_OK;
}

extern "C" sd_status sd_seg_confusion_host(const uint8_t* pred, const uint8_t* labels, int B, int height, int width, const uint8_t* table,
                                           int64_t* counts) {
    if (!pred || !labels || !table || !counts || B < 1 || height < 1 || width < 1 || height > sdpil::kMaxExtent || width > sdpil::kMaxExtent)
        return SD_ERR_INVALID;
    for (int i = 0; i < 256; ++i)
        if (table[i] > 2) return SD_ERR_INVALID;
    const size_t n = (size_t)height * width;
    for (int b = 0; b < B; ++b)
        for (size_t i = 0; i < n; ++i) counts[(size_t)b * sdpil::kCells + sdpil::seg_cell(table[labels[b * n + i]], pred[b * n + i])] += 1;
    return SD_OK;
}
