// The rows of the scene PLY route (sd_scene_format / sd_scene_format_host; contract: include/semdepth.h), stated ONCE for the kernels of
// scene_gpu.hip and the host function of host_scene.cpp.  A file is the concatenation of up to eight segments in the order of
// semantic_depth.py:418-431 -- road cloud, road plane lattice, road-width line, left and right fence cloud, left and right fence plane
// lattice, fence-to-fence line -- behind the minimum-z filter of point_cloud_2_ply.py; digits, rows and header are ply_format.hpp's.
//
// The lattice is pcl.plane_grid under numpy 2 (np.arange(np.float32, np.float32, 0.05) forms its length and its second sample in float32
// and fills a float64 array with start + i * (second - start)), over the sd_plane_box of the cloud that entered the plane fit:
//   count    n_a = max(0, ceil(fl32(fl32(hi_a - lo_a) / fl32(0.05)))); n_b likewise.  (A float64 quotient is wrong on about 28 % of the
//            extents that are an exact multiple of 0.05.)
//   samples  a_0 = (double)lo_a, a_1 = (double)fl32(lo_a + fl32(0.05)), a_i = (double)lo_a + i * d_a with d_a = a_1 - a_0 (a product, then
//            a sum; a_1 equals a_0 + 1 * d_a wherever that difference is exact, and numpy stores a_1 itself)
//   order    row i of the lattice is a = a_{i mod n_a}, b = b_{i div n_a}: meshgrid's default order, a fastest
//   lift     (c_a * a + c_b * b) + C: two products, two sums, each rounded
//   colours  200 200 200 (road plane), 40 70 40 (fence planes)
//   absent   when the box's n == 0 or n_a * n_b == 0
// Everything here is float64 without contraction (the pragma below; the files that include this are compiled with -ffp-contract=off too).
#pragma once
#include "../../include/semdepth.h"
#include "ply_format.hpp"

// the small functions of a row are always inlined: a call would put the caller's arrays and its SceneIn into scratch memory
#define SDSCENE_HD __attribute__((always_inline)) SDPLY_HD

namespace sdscene {

using sdply::in_range;
using sdply::kBlockRows;
using sdply::kLineRows;

constexpr int kSegs = 8;
enum Seg { ROAD = 0, ROAD_PLANE = 1, RW_LINE = 2, FENCE_L = 3, FENCE_R = 4, PLANE_L = 5, PLANE_R = 6, F2F_LINE = 7 };
constexpr uint32_t kMaxRows = 0x7fffffffu - (uint32_t)kBlockRows;      // row indices of a frame stay in an int

// host-known bound of a frame's rows under `mask`: what the device grid is sized from.  Only the selected segments count: the road cloud
// (cap_road), the two fence clouds together (cap_fence), lattice_cap per lattice, 1001 per line -- the _ROAD and _FENCE files have no
// lattice and no line, so their grids are a fraction of the scene file's
SDPLY_HD uint64_t rows_bound(int cap_road, int cap_fence, uint32_t lattice_cap, uint32_t mask) {
    const uint64_t lattices = ((mask >> ROAD_PLANE) & 1u) + ((mask >> PLANE_L) & 1u) + ((mask >> PLANE_R) & 1u);
    const uint64_t lines = ((mask >> RW_LINE) & 1u) + ((mask >> F2F_LINE) & 1u);
    return ((mask >> ROAD) & 1u ? (uint64_t)cap_road : 0) + (mask & ((1u << FENCE_L) | (1u << FENCE_R)) ? (uint64_t)cap_fence : 0) +
           lattices * lattice_cap + lines * kLineRows;
}
SDPLY_HD uint64_t blocks_bound(int cap_road, int cap_fence, uint32_t lattice_cap, uint32_t mask) {
    const uint64_t b = (rows_bound(cap_road, cap_fence, lattice_cap, mask) + kBlockRows - 1) / kBlockRows;
    return b ? b : 1;                                   // (an empty mask still launches one block per frame: every file has a header)
}

// one axis of a lattice: the count and the step.  false: np.arange cannot form a length (a NaN or an unbounded extent) or it is 2^31 or more
SDSCENE_HD bool lattice_axis(float lo, float hi, uint32_t* n, double* d) {
#pragma clang fp contract(off)
    const float ext = hi - lo;
    // the float32 quotient, formed in double and rounded once more: for a division of two float32 values that is the float32 quotient itself
    const double qd = (double)ext / (double)0.05f;
    *n = 0;
    *d = 0.0;
    if (qd != qd || qd >= 3.0e38) return false;
    const float next = lo + 0.05f;
    *d = (double)next - (double)lo;
    if (qd <= 0.0) return true;                        // (an extent of -inf too: no sample)
    const double c = __builtin_ceil((double)(float)qd);
    if (c >= 2147483648.0) return false;
    *n = (uint32_t)c;
    return true;
}
SDSCENE_HD double lattice_sample(float lo, double d, uint32_t i) {
#pragma clang fp contract(off)
    if (i == 0) return (double)lo;
    if (i == 1) return (double)(lo + 0.05f);
    const double step = (double)i * d;
    return (double)lo + step;
}
SDSCENE_HD double lattice_lift(double ca, double a, double cb, double b, double c) {
#pragma clang fp contract(off)
    const double pa = ca * a, pb = cb * b;
    const double s = pa + pb;
    return s + c;
}

// row `row` of create_3Dline_from_3Dpoints on float64 end points: ply_format.hpp's make_line + line_point, from doubles
SDSCENE_HD void line_row(const double* left, const double* right, int row, double* out) {
#pragma clang fp contract(off)
    const double t = (double)(row - 1) * 0.001;
    for (int j = 0; j < 3; ++j) {
        double a = left[j], b = right[j];
        if (j == 1) {
            a += 0.01;
            b += 0.01;
        }
        const double v = b - a;
        if (row == 0) {
            out[j] = a;
        } else {
            const double tv = t * v;
            out[j] = a + tv;
        }
    }
}

// one frame's inputs (host or device pointers; the fence group, the records of the fence chain and the boxes are nullable)
struct SceneIn {
    const float *road_xyz, *left_xyz, *right_xyz;       // f32 [n,3]
    const uint8_t *road_rgb, *left_rgb, *right_rgb;     // u8 [n,3]
    int n_road, cap_road, cap_fence;
    const sd_rw_result* rec;
    const sd_f2f_result* f2f;
    const sd_plane_box* road_box;
    const sd_plane_box* fence_box;                      // [2]: left, right
    uint32_t mask, lattice_cap;                         // lattice_cap 0xffffffff: no cap
};

// the segment table of a frame: a row index finds its segment with at most eight compares
struct SegTable {
    uint32_t count[kSegs];
    uint32_t prefix[kSegs + 1];     // prefix[s] = the first row of segment s, prefix[8] = the rows of the frame
    uint32_t na[3];                 // per lattice (road plane, left, right): samples along a
    int32_t flag;                   // 0; 1: a count outside its capacity, a box np.arange refuses, an end point out of range; 3: a lattice above lattice_cap
    uint32_t pad[3];
    double da[3], db[3];
};

SDSCENE_HD const sd_plane_box* lattice_box(const SceneIn& in, int k) { return k == 0 ? in.road_box : (in.fence_box ? in.fence_box + (k - 1) : nullptr); }
SDSCENE_HD const double* lattice_plane(const SceneIn& in, int k) {
    return k == 0 ? in.rec->plane : (k == 1 ? in.f2f->plane_left : in.f2f->plane_right);
}

SDPLY_HD void build_table(const SceneIn& in, SegTable* t) {
    uint64_t cnt[kSegs];
    for (int s = 0; s < kSegs; ++s) cnt[s] = 0;
    bool bad = false, over = false;
    if (in.mask & (1u << ROAD)) {
        if (in.n_road < 0 || in.n_road > in.cap_road) bad = true;
        else cnt[ROAD] = (uint64_t)in.n_road;
    }
    if ((in.mask & (1u << RW_LINE)) && in.rec->found) {
        for (int j = 0; j < 3; ++j) bad = bad || !in_range((double)in.rec->left_pt[j]) || !in_range((double)in.rec->right_pt[j]);
        cnt[RW_LINE] = kLineRows;
    }
    if (in.f2f) {
        const int64_t nl = (in.mask & (1u << FENCE_L)) && in.left_xyz ? in.f2f->counts[5] : 0;
        const int64_t nr = (in.mask & (1u << FENCE_R)) && in.right_xyz ? in.f2f->counts[6] : 0;
        if (nl < 0 || nr < 0 || nl + nr > in.cap_fence) bad = true;
        else {
            cnt[FENCE_L] = (uint64_t)nl;
            cnt[FENCE_R] = (uint64_t)nr;
        }
        if ((in.mask & (1u << F2F_LINE)) && in.f2f->ok) {
            for (int j = 0; j < 3; ++j) bad = bad || !in_range(in.f2f->left_pt[j]) || !in_range(in.f2f->right_pt[j]);
            cnt[F2F_LINE] = kLineRows;
        }
    }
    for (int k = 0; k < 3; ++k) {
        const int s = k == 0 ? ROAD_PLANE : (k == 1 ? PLANE_L : PLANE_R);
        t->na[k] = 0;
        t->da[k] = t->db[k] = 0.0;
        const sd_plane_box* box = lattice_box(in, k);
        if (!(in.mask & (1u << s)) || !box || (k > 0 && !in.f2f) || box->n == 0) continue;
        uint32_t na, nb;
        if (box->n < 0 || !lattice_axis(box->lo_a, box->hi_a, &na, &t->da[k]) || !lattice_axis(box->lo_b, box->hi_b, &nb, &t->db[k])) {
            bad = true;
            continue;
        }
        const uint64_t rows = (uint64_t)na * nb;
        if (rows > in.lattice_cap) over = true;
        else {
            t->na[k] = na;
            cnt[s] = rows;
        }
    }
    uint64_t total = 0;
    for (int s = 0; s < kSegs; ++s) total += cnt[s];
    if (total > kMaxRows) bad = true;
    t->flag = bad ? 1 : (over ? 3 : 0);
    t->pad[0] = t->pad[1] = t->pad[2] = 0;
    uint32_t p = 0;
    for (int s = 0; s < kSegs; ++s) {
        t->count[s] = t->flag ? 0u : (uint32_t)cnt[s];
        t->prefix[s] = p;
        p += t->count[s];
    }
    t->prefix[kSegs] = p;
}

// row r (< prefix[8]) of the frame before the filter.  (Always inlined: a call would put the caller's SceneIn into scratch memory.)
SDSCENE_HD void row_point(const SceneIn& in, const SegTable& t, uint32_t r, double* p, uint8_t* c) {
    int s = 0;
    uint32_t first = 0;
    for (int j = 1; j < kSegs; ++j) {      // (the prefix is monotone: the last segment that begins at or before r is r's)
        if (r >= t.prefix[j]) {
            s = j;
            first = t.prefix[j];
        }
    }
    const uint32_t i = r - first;
    // (the six pointers are read into locals first: a select between two fields of `in` becomes an indexed load of the struct, which then
    // lives in scratch memory)
    const float *x0 = in.road_xyz, *x1 = in.left_xyz, *x2 = in.right_xyz;
    const uint8_t *g0 = in.road_rgb, *g1 = in.left_rgb, *g2 = in.right_rgb;
    if (s == ROAD || s == FENCE_L || s == FENCE_R) {
        const float* x = s == ROAD ? x0 : (s == FENCE_L ? x1 : x2);
        const uint8_t* g = s == ROAD ? g0 : (s == FENCE_L ? g1 : g2);
        for (int j = 0; j < 3; ++j) {
            p[j] = (double)x[3 * (size_t)i + j];
            c[j] = g[3 * (size_t)i + j];
        }
        return;
    }
    if (s == RW_LINE) {
        const double l[3] = {(double)in.rec->left_pt[0], (double)in.rec->left_pt[1], (double)in.rec->left_pt[2]};
        const double q[3] = {(double)in.rec->right_pt[0], (double)in.rec->right_pt[1], (double)in.rec->right_pt[2]};
        line_row(l, q, (int)i, p);
        c[0] = 250;
        c[1] = 0;
        c[2] = 0;
        return;
    }
    if (s == F2F_LINE) {
        line_row(in.f2f->left_pt, in.f2f->right_pt, (int)i, p);
        c[0] = 0;
        c[1] = 255;
        c[2] = 0;
        return;
    }
    const int k = s == ROAD_PLANE ? 0 : (s == PLANE_L ? 1 : 2);
    const sd_plane_box* box = lattice_box(in, k);
    const double* pl = lattice_plane(in, k);
    // (selects, not t.na[k]: a table held in registers must not be indexed at run time)
    const uint32_t na = k == 0 ? t.na[0] : (k == 1 ? t.na[1] : t.na[2]);
    const double da = k == 0 ? t.da[0] : (k == 1 ? t.da[1] : t.da[2]), db = k == 0 ? t.db[0] : (k == 1 ? t.db[1] : t.db[2]);
    const double a = lattice_sample(box->lo_a, da, i % na), b = lattice_sample(box->lo_b, db, i / na);
    if (k == 0) {              // pcl.plane_grid(axis=1): y = Cx * x + Cz * z + C
        p[0] = a;
        p[1] = lattice_lift(pl[0], a, pl[2], b, pl[3]);
        p[2] = b;
        c[0] = c[1] = c[2] = 200;
    } else {                   // axis=0: x = Cy * y + Cz * z + C
        p[0] = lattice_lift(pl[1], a, pl[2], b, pl[3]);
        p[1] = a;
        p[2] = b;
        c[0] = 40;
        c[1] = 70;
        c[2] = 40;
    }
}

// ---- workspace of the device route (scene_gpu.hip): sdply::Layout's regions over nblk = blocks_bound(..., mask) row blocks, and a segment table per frame
struct Layout : sdarena::Walker {
    size_t nb, B;
    Layout(int B_, int cap_road, int cap_fence, uint32_t lattice_cap, uint32_t mask)
        : nb((size_t)B_ * (size_t)blocks_bound(cap_road, cap_fence, lattice_cap, mask)), B((size_t)B_) {}
    size_t bmin = take(nb * 8, 8), boff = take(nb * 8, 8);                            // f64, u64 [B][nblk], 8-byte aligned
    size_t zmin = take(B * 8, 8), fbase = take(B * 8, 8);                             // f64, u64 [B], 8
    size_t tab = take(B * sizeof(SegTable), 8);                                       // SegTable [B], 8
    size_t blen = take(nb * 4, 4), bcnt = take(nb * 4, 4), bbad = take(nb * 4, 4);    // u32 [B][nblk], 4
    size_t slack = end();                                                             // 64 bytes of historical slack: nothing reads or writes them
    size_t total = end_with_slack(64);
};

}  // namespace sdscene
