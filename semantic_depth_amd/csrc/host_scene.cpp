// The host statement of the scene PLY route (sd_scene_format): one frame, a single walk over the rows of scene_format.hpp with the coder
// of ply_format.hpp -- the functions the kernels of scene_gpu.hip run, so the files are the same bytes.  No handle, no GPU.
#include "../../include/semdepth.h"
#include "scene_format.hpp"

static_assert(sizeof(sd_plane_box) == 24, "sd_plane_box is 24 bytes");
static_assert(SD_SCENE_ROAD == 1u << sdscene::ROAD && SD_SCENE_ROAD_PLANE == 1u << sdscene::ROAD_PLANE && SD_SCENE_RW_LINE == 1u << sdscene::RW_LINE &&
                  SD_SCENE_FENCE_L == 1u << sdscene::FENCE_L && SD_SCENE_FENCE_R == 1u << sdscene::FENCE_R && SD_SCENE_PLANE_L == 1u << sdscene::PLANE_L &&
                  SD_SCENE_PLANE_R == 1u << sdscene::PLANE_R && SD_SCENE_F2F_LINE == 1u << sdscene::F2F_LINE,
              "include/semdepth.h and scene_format.hpp disagree");

extern "C" sd_status sd_scene_format_host(const float* road_xyz, const uint8_t* road_rgb, int n_road, const float* left_xyz, const uint8_t* left_rgb,
                                          const float* right_xyz, const uint8_t* right_rgb, const sd_rw_result* record, const sd_f2f_result* f2f,
                                          const sd_plane_box* road_box, const sd_plane_box* fence_boxes, uint32_t mask, uint32_t lattice_cap,
                                          uint8_t* out_host, size_t cap, size_t* size_out, int32_t* flag_out) {
    using namespace sdscene;
    using namespace sdply;
    if (n_road < 0 || !record || !size_out || !flag_out || (n_road > 0 && (!road_xyz || !road_rgb)) || (cap > 0 && !out_host) ||
        (left_xyz && !left_rgb) || (right_xyz && !right_rgb) || ((left_xyz || right_xyz) && !f2f) || (mask & ~(uint32_t)SD_SCENE_ALL))
        return SD_ERR_INVALID;
    *size_out = 0;
    *flag_out = 0;
    SceneIn in{};
    in.road_xyz = road_xyz; in.road_rgb = road_rgb; in.left_xyz = left_xyz; in.left_rgb = left_rgb; in.right_xyz = right_xyz; in.right_rgb = right_rgb;
    in.n_road = n_road; in.cap_road = n_road;
    in.cap_fence = 0x7fffffff;                          // (host clouds are as long as their counts say)
    in.rec = record; in.f2f = f2f; in.road_box = road_box; in.fence_box = fence_boxes;
    in.mask = mask; in.lattice_cap = lattice_cap ? lattice_cap : 0xffffffffu;
    SegTable t;
    build_table(in, &t);
    if (t.flag) {
        *flag_out = t.flag;
        return SD_OK;
    }
    const uint32_t rows = t.prefix[kSegs];
    double p[3];
    uint8_t c[3];
    // the minimum z of all rows and the range test
    bool bad = false;
    double zmin = __builtin_huge_val();
    for (uint32_t r = 0; r < rows; ++r) {
        row_point(in, t, r, p, c);
        bad = bad || !in_range(p[0]) || !in_range(p[1]) || !in_range(p[2]);
        zmin = p[2] < zmin ? p[2] : zmin;
    }
    if (bad) {
        *flag_out = 1;
        return SD_OK;
    }
    // the kept rows and their exact length
    uint32_t count = 0;
    size_t body = 0;
    for (uint32_t r = 0; r < rows; ++r) {
        row_point(in, t, r, p, c);
        if (!(p[2] > zmin)) continue;
        ++count;
        body += (size_t)row_len(make_row(p, c));
    }
    const int hdr = header_len(count);
    if ((size_t)hdr + body > cap) {                     // the text would pass the capacity: its size is reported, nothing is written
        *flag_out = 2;
        *size_out = (size_t)hdr + body;
        return SD_OK;
    }
    for (int i = 0; i < hdr; ++i) out_host[i] = header_byte(i, count);
    uint8_t* q = out_host + hdr;
    for (uint32_t r = 0; r < rows; ++r) {
        row_point(in, t, r, p, c);
        if (!(p[2] > zmin)) continue;
        q += put_row(q, make_row(p, c));
    }
    *size_out = (size_t)(q - out_host);
    return SD_OK;
}

extern "C" sd_status sd_scene_lattice_host(const sd_plane_box* box, const double* plane, int axis, uint32_t* n_a, uint32_t* n_b, double* xyz_out,
                                           size_t rows_cap) {
    using namespace sdscene;
    if (!box || !plane || !n_a || !n_b || (axis != 0 && axis != 1)) return SD_ERR_INVALID;
    // the lattice alone, through the same table and row source: as the road plane (axis 1) or as the left fence plane (axis 0)
    sd_rw_result rec{};
    sd_f2f_result f2{};
    sd_plane_box boxes[2] = {*box, *box};
    for (int j = 0; j < 4; ++j) rec.plane[j] = f2.plane_left[j] = plane[j];
    SceneIn in{};
    in.rec = &rec; in.f2f = &f2; in.road_box = box; in.fence_box = boxes;
    in.cap_fence = 0x7fffffff;
    in.lattice_cap = 0xffffffffu;
    in.mask = axis == 1 ? (uint32_t)SD_SCENE_ROAD_PLANE : (uint32_t)SD_SCENE_PLANE_L;
    SegTable t;
    build_table(in, &t);
    if (t.flag) return SD_ERR_INVALID;
    const int k = axis == 1 ? 0 : 1;
    const uint32_t rows = t.prefix[kSegs];
    *n_a = t.na[k];
    *n_b = t.na[k] ? rows / t.na[k] : 0;
    if (!xyz_out) return SD_OK;
    if (rows > rows_cap) return SD_ERR_INVALID;
    uint8_t c[3];
    for (uint32_t r = 0; r < rows; ++r) row_point(in, t, r, xyz_out + 3 * (size_t)r, c);
    return SD_OK;
}
