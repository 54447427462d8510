// Host side of the disparity images (sd_disp_image_host / sd_disp_image_workspace / sd_disp_colormap; contract: include/semdepth.h): the CPU
// statement of sd_disp_image -- plain loops through disp_image_rule.hpp, the rule the kernels of disp_image_gpu.hip use, around
// sd_resize_pil_bilinear_u8_host.  Compiled with -ffp-contract=off like the kernels: the byte scaling is a float32 difference and a float32
// product, never one fma.  No handle, no GPU.
#include "../../include/semdepth.h"
#include "disp_image_rule.hpp"

#include <new>
#include <vector>

static_assert(SD_CMAP_GRAY == 0 && SD_CMAP_PLASMA == 1 && sddisp::kMaps == 2, "the maps of disp_image_rule.hpp are the header's");

extern "C" sd_status sd_disp_image_workspace(int B, int h, int w, int out_h, int out_w, size_t* bytes_out) {
    if (!bytes_out || B < 1 || B > 65535 || !sddisp::valid_sizes(h, w, out_h, out_w)) return SD_ERR_INVALID;
    *bytes_out = sddisp::Layout(B, h, w, out_h, out_w).total;
    return SD_OK;
}

extern "C" sd_status sd_disp_colormap(int cmap, uint8_t* rgb_out) {
    if (!rgb_out || !sddisp::valid_map(cmap)) return SD_ERR_INVALID;
    for (int i = 0; i < 256; ++i) {
        const uint32_t c = sddisp::bgr_of(cmap, i);
        rgb_out[3 * i] = (uint8_t)(c >> 16);
        rgb_out[3 * i + 1] = (uint8_t)(c >> 8);
        rgb_out[3 * i + 2] = (uint8_t)c;
    }
    return SD_OK;
}

extern "C" sd_status sd_disp_image_host(const float* disp, const float* mult, int B, int h, int w, int out_h, int out_w, int cmap, uint8_t* out_bgr,
                                        int32_t* flags) {
    using namespace sddisp;
    if (!disp || !out_bgr || !flags || B < 1 || !valid_map(cmap) || !valid_sizes(h, w, out_h, out_w)) return SD_ERR_INVALID;
    const size_t n = (size_t)h * w, n2 = (size_t)out_h * out_w;
    const bool resize = resized(h, w, out_h, out_w);
    std::vector<uint8_t> bytes, big;
    try {
        bytes.resize(n);
        if (resize) big.resize(n2);
    } catch (const std::bad_alloc&) {
        return SD_ERR_INVALID;
    }
    for (int b = 0; b < B; ++b) {
        const float* d = disp + (size_t)b * n;
        const float m = mult ? mult[b] : 1.0f;
        uint32_t kmin = kKeyNone, kmax = 0;
        for (size_t i = 0; i < n; ++i) {
            const float v = scaled(d[i], m);
            if (!finite_f32(v)) continue;
            const uint32_t k = key_of(v);
            kmin = k < kmin ? k : kmin;
            kmax = k > kmax ? k : kmax;
        }
        const Range r = make_range(kmin, kmax);
        int32_t flag = 0;
        for (size_t i = 0; i < n; ++i) {
            const float v = scaled(d[i], m);
            if (finite_f32(v)) {
                bytes[i] = byte_of(v, r);
            } else {
                bytes[i] = 0;
                flag = 1;
            }
        }
        flags[b] = flag;
        const uint8_t* img = bytes.data();
        if (resize) {
            const sd_status st = sd_resize_pil_bilinear_u8_host(bytes.data(), 1, h, w, 1, 1, 0, big.data(), out_h, out_w);
            if (st != SD_OK) return st;
            img = big.data();
        }
        int lo8 = 255, hi8 = 0;
        for (size_t i = 0; i < n2; ++i) {
            lo8 = img[i] < lo8 ? img[i] : lo8;
            hi8 = img[i] > hi8 ? img[i] : hi8;
        }
        uint32_t table[256];
        for (int p = 0; p < 256; ++p) table[p] = bgr_of(cmap, index_of(p, lo8, hi8));
        uint8_t* o = out_bgr + (size_t)b * n2 * 3;
        for (size_t i = 0; i < n2; ++i) {
            const uint32_t c = table[img[i]];
            o[3 * i] = (uint8_t)c;
            o[3 * i + 1] = (uint8_t)(c >> 8);
            o[3 * i + 2] = (uint8_t)(c >> 16);
        }
    }
    return SD_OK;
}
