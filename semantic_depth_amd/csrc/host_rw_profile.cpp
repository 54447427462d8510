// Host twins of the depth profile (sd_road_width_profile_host / sd_f2f_profile_host; contract: include/semdepth.h): argument checks plus
// one loop over the rows / the depths through rw_profile.hpp, the arithmetic the kernels of rw_profile.hip use.  No HIP call is made here.
#include "../../include/semdepth.h"
#include "rw_profile.hpp"

#include <cmath>

static_assert(sizeof(sd_rw_depth_result) == 48 && sizeof(sd_f2f_depth_result) == 64, "include/semdepth.h: depth record sizes");
static_assert(sizeof(sdrwp::Window) == 24 && sizeof(sdrwp::Partial) == 24, "rw_profile.hpp: workspace records");

extern "C" size_t sd_rw_profile_workspace(int B, int cap, int D) {
    if (B < 1 || B > 65535 || cap < 1 || D < 1 || D > SD_PROFILE_MAX_DEPTHS) return 0;
    return sdrwp::workspace_bytes(B, cap, D);
}

extern "C" sd_status sd_road_width_profile_host(const float* xyz_host, int n, const double* depths, int D, double window, double depth_offset,
                                                sd_rw_depth_result* results_host) {
    using namespace sdrwp;
    if (n < 0 || (n > 0 && !xyz_host) || !depths || !results_host || D < 1 || D > SD_PROFILE_MAX_DEPTHS) return SD_ERR_INVALID;
    if (!std::isfinite(window) || !std::isfinite(depth_offset) || !(window > 0)) return SD_ERR_INVALID;
    for (int i = 0; i < D; ++i)
        if (!std::isfinite(depths[i])) return SD_ERR_INVALID;
    Window win[SD_PROFILE_MAX_DEPTHS];
    Partial acc[SD_PROFILE_MAX_DEPTHS];
    sorted_windows(depths, D, window, depth_offset, win);
    for (int w = 0; w < D; ++w) acc[w] = Partial{kNoKey, kNoKey, 0, 0};
    for (int i = 0; i < n; ++i) {
        const float x = xyz_host[(size_t)i * 3], z = xyz_host[(size_t)i * 3 + 2];
        int a, e;
        range_of(z, [&](int k) { return win[k].lo; }, [&](int k) { return win[k].hi; }, D, a, e);
        if (a >= e) continue;
        const uint64_t kl = key_left(x, (uint32_t)i), kr = key_right(x, (uint32_t)i);
        for (int w = a; w < e; ++w) {
            acc[w].kmin = kl < acc[w].kmin ? kl : acc[w].kmin;
            acc[w].kmax = kr < acc[w].kmax ? kr : acc[w].kmax;
            acc[w].count += 1;
        }
    }
    for (int w = 0; w < D; ++w) write_record(results_host + win[w].index, acc[w].kmin, acc[w].kmax, acc[w].count, xyz_host);
    return SD_OK;
}

extern "C" sd_status sd_f2f_profile_host(const sd_rw_result* road, const sd_f2f_result* f2f, const double* depths, int D,
                                         sd_f2f_depth_result* results_host) {
    if (!road || !f2f || !depths || !results_host || D < 1 || D > SD_PROFILE_MAX_DEPTHS) return SD_ERR_INVALID;
    for (int i = 0; i < D; ++i)
        if (!std::isfinite(depths[i])) return SD_ERR_INVALID;
    for (int i = 0; i < D; ++i) sdrwp::write_fence_record(results_host + i, *road, *f2f, depths[i]);
    return SD_OK;
}
