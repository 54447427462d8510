// The arithmetic of the depth profile (sd_road_width_profile / sd_f2f_profile and their _host twins; contract: include/semdepth.h),
// stated ONCE for the kernels of rw_profile.hip, f2f_kernel of pcl.hip and the host loops of host_rw_profile.cpp: the window of a depth,
// which rows it holds, the end-point keys, the record of a window, which windows hold a given z, and the fence solve.  Both sides call
// these functions, so they agree on every bit; what differs is only who walks the rows.  Plain C++17 under g++; every file that includes
// it is compiled with -ffp-contract=off (the fence solve must not fuse its multiply-adds).
#pragma once
#include "../../include/semdepth.h"

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "arena.hpp"

#if defined(__HIPCC__)
#define SD_RWP_HD __host__ __device__
#else
#define SD_RWP_HD
#endif

namespace sdrwp {

constexpr int RWP_SLICE = 2048;       // rows of a cloud one workgroup walks at a time
constexpr int RWP_MAX_SLICES = 64;    // workgroups per frame at most: past RWP_SLICE * RWP_MAX_SLICES rows a workgroup walks several slices
constexpr int RWP_THREADS = 256;      // threads of a partial workgroup (>= SD_PROFILE_MAX_DEPTHS: one thread writes one window's partial)
static_assert(RWP_THREADS >= SD_PROFILE_MAX_DEPTHS, "one thread per window writes the slice's partial");

// One window, in the order the kernels search: ascending depth.  `index` is the caller's position of that depth.
struct Window {
    double lo, hi;
    int32_t index, reserved;
};
// What one slice knows of one window.
struct Partial {
    uint64_t kmin, kmax;
    int32_t count, reserved;
};
constexpr uint64_t kNoKey = ~(uint64_t)0;

SD_RWP_HD inline uint32_t fbits(float v) {
    uint32_t u;
    __builtin_memcpy(&u, &v, 4);
    return u;
}
SD_RWP_HD inline float bits_f(uint32_t u) {
    float v;
    __builtin_memcpy(&v, &u, 4);
    return v;
}
SD_RWP_HD inline double bits_d(uint64_t u) {
    double v;
    __builtin_memcpy(&v, &u, 8);
    return v;
}
SD_RWP_HD inline uint32_t f2key(float v) {       // monotone float -> uint (pcl.hip's key)
    const uint32_t u = fbits(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// The window of depth d: e = d - depth_offset first (sd_road_width forms it before its last step), then the two edges.
SD_RWP_HD inline void window_of(double d, double depth_offset, double window, double& lo, double& hi) {
    const double e = d - depth_offset;
    hi = -(e - window);
    lo = -(e + window);
}
// Both comparisons strict and in float64 (pcl.py:271-290).
SD_RWP_HD inline bool inside(float z, double lo, double hi) {
    const double zz = (double)z;
    return zz < hi && zz > lo;
}
// min of key_left picks the smallest x, then the lowest row; min of key_right the largest x, then the lowest row
SD_RWP_HD inline uint64_t key_left(float x, uint32_t row) { return ((uint64_t)f2key(x) << 32) | row; }
SD_RWP_HD inline uint64_t key_right(float x, uint32_t row) { return ((uint64_t)(~f2key(x)) << 32) | row; }

// Index range rule.  With the windows in ascending depth, lo and hi are non-increasing (every rounding above is monotone), so
// "z < hi[i]" holds on a prefix [0, b) and "z > lo[i]" on a suffix [a, D): the windows that hold z are [a, b), empty when a >= b
// (and for a NaN z, which no comparison admits).  lo / hi may be two arrays (stride 1) or the fields of Window records.
template <class LO, class HI>
SD_RWP_HD inline void range_of(float z, LO lo, HI hi, int D, int& a, int& b) {
    const double zz = (double)z;
    int l = 0, r = D;
    while (l < r) {       // first i with !(zz < hi(i))
        const int m = (l + r) >> 1;
        if (zz < hi(m)) l = m + 1; else r = m;
    }
    b = l;
    l = 0;
    r = b;
    while (l < r) {       // first i with zz > lo(i); past b nothing is asked
        const int m = (l + r) >> 1;
        if (zz > lo(m)) r = m; else l = m + 1;
    }
    a = l;
}

// The record of one window from its merged keys and count; xyz is the frame's cloud.  Every byte is written.
SD_RWP_HD inline void write_record(sd_rw_depth_result* out, uint64_t kmin, uint64_t kmax, int32_t count, const float* xyz) {
    sd_rw_depth_result r;
    if (kmin == kNoKey) {
        r.found = 0;
        r.width = bits_d(0x7ff8000000000000ull);
        r.x_left = r.x_right = bits_f(0x7fc00000u);
        for (int j = 0; j < 3; ++j) { r.left_pt[j] = r.x_left; r.right_pt[j] = r.x_left; }
    } else {
        const uint32_t il = (uint32_t)(kmin & 0xFFFFFFFFull), ir = (uint32_t)(kmax & 0xFFFFFFFFull);
        r.found = 1;
        for (int j = 0; j < 3; ++j) { r.left_pt[j] = xyz[(size_t)il * 3 + j]; r.right_pt[j] = xyz[(size_t)ir * 3 + j]; }
        r.x_left = r.left_pt[0];
        r.x_right = r.right_pt[0];
        r.width = fabs((double)r.x_left - (double)r.x_right);
    }
    r.n_window = count;
    *out = r;
}

// pcl.planes_intersection_at_certain_depth (pcl.py:212-237) for the two fence planes against the road plane at z, and the distance
// between the two points (semantic_depth.py:321-328).  Cramer's rule in float64 (the reference inverts the 2x2 with LAPACK).
SD_RWP_HD inline double fence_solve(const double* rp, const double* left, const double* right, double z, double pt[2][3]) {
    const double* pl[2] = {left, right};
    for (int s = 0; s < 2; ++s) {
        const double a = rp[0], bb = rp[1], c = pl[s][0], d = pl[s][1];
        const double e = -(rp[2] * z + rp[3]), f = -(pl[s][2] * z + pl[s][3]);
        const double det = a * d - bb * c;
        pt[s][0] = (e * d - bb * f) / det;
        pt[s][1] = (a * f - e * c) / det;
        pt[s][2] = z;
    }
    const double dx = pt[0][0] - pt[1][0], dy = pt[0][1] - pt[1][1], dz = pt[0][2] - pt[1][2];
    return sqrt(dx * dx + dy * dy + dz * dz);
}

// A NaN of the profile's fence record is THE quiet NaN: which NaN a 0 / 0 gives differs between processors, the record must not.
SD_RWP_HD inline double one_nan(double v) { return v == v ? v : bits_d(0x7ff8000000000000ull); }

// The fence record at `depth` (z = -depth; no depth_offset, as in sd_fence_to_fence).  Every byte is written.
SD_RWP_HD inline void write_fence_record(sd_f2f_depth_result* out, const sd_rw_result& road, const sd_f2f_result& fence, double depth) {
    sd_f2f_depth_result r;
    double pt[2][3];
    const double dist = fence_solve(road.plane, fence.plane_left, fence.plane_right, -depth, pt);
    r.ok = (dist == dist) && fence.counts[5] > 0 && fence.counts[6] > 0;
    r.dist = one_nan(dist);
    for (int j = 0; j < 3; ++j) { r.left_pt[j] = one_nan(pt[0][j]); r.right_pt[j] = one_nan(pt[1][j]); }
    r.reserved = 0;
    *out = r;
}

// slices (= workgroups) per frame of a launch over clouds of `cap` rows
inline int slices_of(int cap) {
    const long long g = ((long long)cap + RWP_SLICE - 1) / RWP_SLICE;
    return (int)std::min<long long>(std::max<long long>(g, 1), RWP_MAX_SLICES);
}
// ---- workspace of the device route (rw_profile.hip), 16-byte aligned
struct Layout : sdarena::Walker {
    size_t D, parts;
    Layout(int B, int cap, int D_) : D((size_t)D_), parts((size_t)B * slices_of(cap) * D_) {}
    size_t windows = take(D * sizeof(Window), 16);           // Window [D], sorted: the caller copies them here in stream order before the launches
    size_t partial = take(parts * sizeof(Partial), 16);      // Partial [B][slices_of(cap)][D]: written by the first launch, read by the second
    size_t total = end();
};
inline size_t workspace_bytes(int B, int cap, int D) { return Layout(B, cap, D).total; }

// The D windows in ascending depth, each with the caller's index of its depth (a stable sort: equal depths keep the caller's order,
// and each of them is a window of its own).  out has room for D records.
inline void sorted_windows(const double* depths, int D, double window, double depth_offset, Window* out) {
    int order[SD_PROFILE_MAX_DEPTHS];
    for (int i = 0; i < D; ++i) order[i] = i;
    std::stable_sort(order, order + D, [&](int a, int b) { return depths[a] < depths[b]; });
    for (int i = 0; i < D; ++i) {
        window_of(depths[order[i]], depth_offset, window, out[i].lo, out[i].hi);
        out[i].index = order[i];
        out[i].reserved = 0;
    }
}

}  // namespace sdrwp
