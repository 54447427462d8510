// Host side of the rendered clouds: the CPU statement of sd_render_rw for one frame -- one plain loop over the rows with a host key buffer.
// Every decision -- the rows, the filter, the projection, the square, the key, the colour -- is a function of render_rule.hpp, which the
// kernels of render_gpu.hip run too.  No handle, no GPU.
#include "../../include/semdepth.h"
#include "render_rule.hpp"

#include <new>
#include <vector>

static_assert(sizeof(sd_render_camera) == 152, "sd_render_camera has no padding");

extern "C" sd_status sd_render_rw_host(const float* xyz_host, const uint8_t* rgb_host, int n, const sd_rw_result* record,
                                       const sd_render_camera* cam, uint8_t* out_host, int32_t* flag_out) {
    using namespace sdrender;
    if (!record || !cam || !out_host || !flag_out || (n > 0 && (!xyz_host || !rgb_host))) return SD_ERR_INVALID;
    if (!valid_camera(*cam)) return SD_ERR_INVALID;
    const size_t pixels = (size_t)cam->height * cam->width;
    std::vector<uint64_t> keys;
    try {
        keys.assign(pixels, kEmptyKey);
    } catch (const std::bad_alloc&) {
        return SD_ERR_INVALID;
    }
    const sdply::Frame f = make_frame(xyz_host, rgb_host, n, n < 0 ? 0 : n, record->left_pt, record->right_pt, record->found);
    *flag_out = f.bad ? 1 : 0;
    double p[3];
    uint8_t c[3];
    // the minimum z of the finite rows
    double zmin = __builtin_huge_val();
    for (int r = 0; r < f.rows; ++r) {
        sdply::row_point(f, r, p, c);
        if (finite3(p)) zmin = p[2] < zmin ? p[2] : zmin;
    }
    // every drawn row lowers the keys of its square
    for (int r = 0; r < f.rows; ++r) {
        sdply::row_point(f, r, p, c);
        if (!finite3(p) || !(p[2] > zmin)) continue;
        Hit h;
        if (!project(*cam, p, &h)) continue;
        const Box box = splat_box(*cam, h);
        const uint64_t key = make_key(h.zbits, (uint32_t)r);
        for (int y = box.y0; y <= box.y1; ++y)
            for (int x = box.x0; x <= box.x1; ++x) {
                uint64_t& k = keys[(size_t)y * cam->width + x];
                k = key < k ? key : k;
            }
    }
    for (size_t i = 0; i < pixels; ++i) resolve(*cam, keys[i], rgb_host, f.n, out_host + 3 * i);
    return SD_OK;
}
