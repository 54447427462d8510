// Depth profile on gfx950 (sd_road_width_profile / sd_f2f_profile; HBM / latency bound, no MFMA): the road record of ONE denoised cloud
// per frame at D depths, and the fence-to-fence distance of ONE set of planes per frame at D depths.  The arithmetic is rw_profile.hpp's
// (shared with the host twins); this file only walks the rows.  Compiled with -ffp-contract=off like pcl.hip.
//
// Two launches in stream order, nothing handed between workgroups inside a launch and no global atomics: a slice's workgroup reduces into
// LDS (64-bit min, integer add: both independent of the order they arrive in) and stores its partial; the merge takes the min / sum over
// the slices in index order.  The bytes therefore depend neither on the number of slices nor on scheduling.
#include "rw_profile_gpu.hpp"

namespace sd {

using namespace sdrwp;

// grid (G slices, B frames), RWP_THREADS threads.  windows: D records in ascending depth.  partial: [B][G][D].
__global__ __launch_bounds__(RWP_THREADS) void rw_profile_partial_kernel(const float* __restrict__ xyz_all, const int32_t* __restrict__ n_all,
                                                                         int cap, const Window* __restrict__ windows, int D,
                                                                         Partial* __restrict__ partial) {
    __shared__ double s_lo[SD_PROFILE_MAX_DEPTHS], s_hi[SD_PROFILE_MAX_DEPTHS];
    __shared__ unsigned long long s_kmin[SD_PROFILE_MAX_DEPTHS], s_kmax[SD_PROFILE_MAX_DEPTHS];
    __shared__ int s_cnt[SD_PROFILE_MAX_DEPTHS];
    const int g = blockIdx.x, G = gridDim.x, b = blockIdx.y, tid = threadIdx.x;
    const float* xyz = xyz_all + (size_t)b * cap * 3;
    const int n = min(n_all[b], cap);
    for (int i = tid; i < D; i += RWP_THREADS) {
        s_lo[i] = windows[i].lo;
        s_hi[i] = windows[i].hi;
        s_kmin[i] = kNoKey;
        s_kmax[i] = kNoKey;
        s_cnt[i] = 0;
    }
    __syncthreads();
    // slices g, g + G, g + 2 G, ... of the frame (one slice per workgroup up to RWP_SLICE * RWP_MAX_SLICES rows)
    for (long long s0 = (long long)g * RWP_SLICE; s0 < n; s0 += (long long)G * RWP_SLICE) {
        const int end = (int)min((long long)n, s0 + RWP_SLICE);
        for (int i = (int)s0 + tid; i < end; i += RWP_THREADS) {
            const float x = xyz[(size_t)i * 3], z = xyz[(size_t)i * 3 + 2];
            int a, e;
            range_of(z, [&](int k) { return s_lo[k]; }, [&](int k) { return s_hi[k]; }, D, a, e);
            if (a < e) {
                const unsigned long long kl = key_left(x, (uint32_t)i), kr = key_right(x, (uint32_t)i);
                for (int w = a; w < e; ++w) {
                    atomicMin(&s_kmin[w], kl);
                    atomicMin(&s_kmax[w], kr);
                    atomicAdd(&s_cnt[w], 1);
                }
            }
        }
    }
    __syncthreads();
    Partial* out = partial + ((size_t)b * G + g) * D;
    for (int i = tid; i < D; i += RWP_THREADS) {
        Partial p;
        p.kmin = s_kmin[i];
        p.kmax = s_kmax[i];
        p.count = s_cnt[i];
        p.reserved = 0;
        out[i] = p;
    }
}

// one thread per (frame, window): min / sum over the G partials in slice order, the two rows, the record at the caller's depth index
__global__ __launch_bounds__(RWP_THREADS) void rw_profile_merge_kernel(const float* __restrict__ xyz_all, int cap, int B, int G,
                                                                       const Window* __restrict__ windows, int D,
                                                                       const Partial* __restrict__ partial, sd_rw_depth_result* __restrict__ results) {
    const long long t = (long long)blockIdx.x * RWP_THREADS + threadIdx.x;
    if (t >= (long long)B * D) return;
    const int b = (int)(t / D), w = (int)(t % D);
    uint64_t kmin = kNoKey, kmax = kNoKey;
    int32_t count = 0;
    for (int g = 0; g < G; ++g) {
        const Partial& p = partial[((size_t)b * G + g) * D + w];
        kmin = p.kmin < kmin ? p.kmin : kmin;
        kmax = p.kmax < kmax ? p.kmax : kmax;
        count += p.count;
    }
    write_record(results + (size_t)b * D + windows[w].index, kmin, kmax, count, xyz_all + (size_t)b * cap * 3);
}

hipError_t launch_rw_profile(const float* xyz, const int32_t* n, int B, int cap, int D, void* workspace, sd_rw_depth_result* results, hipStream_t s) {
    const int G = slices_of(cap);
    const Layout l(B, cap, D);
    const Window* windows = reinterpret_cast<const Window*>(static_cast<uint8_t*>(workspace) + l.windows);
    Partial* partial = reinterpret_cast<Partial*>(static_cast<uint8_t*>(workspace) + l.partial);
    hipLaunchKernelGGL(rw_profile_partial_kernel, dim3(G, B), dim3(RWP_THREADS), 0, s, xyz, n, cap, windows, D, partial);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const long long threads = (long long)B * D;
    hipLaunchKernelGGL(rw_profile_merge_kernel, dim3((unsigned)((threads + RWP_THREADS - 1) / RWP_THREADS)), dim3(RWP_THREADS), 0, s, xyz, cap, B, G,
                       windows, D, partial, results);
    return hipGetLastError();
}

// one thread per (frame, depth); the depths travel as a kernel argument (2 KiB)
__global__ __launch_bounds__(RWP_THREADS) void f2f_profile_kernel(const sd_rw_result* __restrict__ road, const sd_f2f_result* __restrict__ fence, int B,
                                                                  F2fDepths depths, int D, sd_f2f_depth_result* __restrict__ results) {
    const long long t = (long long)blockIdx.x * RWP_THREADS + threadIdx.x;
    if (t >= (long long)B * D) return;
    const int b = (int)(t / D), i = (int)(t % D);
    write_fence_record(results + (size_t)b * D + i, road[b], fence[b], depths.d[i]);
}

hipError_t launch_f2f_profile(const sd_rw_result* road, const sd_f2f_result* fence, int B, const F2fDepths& depths, int D,
                              sd_f2f_depth_result* results, hipStream_t s) {
    const long long threads = (long long)B * D;
    hipLaunchKernelGGL(f2f_profile_kernel, dim3((unsigned)((threads + RWP_THREADS - 1) / RWP_THREADS)), dim3(RWP_THREADS), 0, s, road, fence, B, depths,
                       D, results);
    return hipGetLastError();
}

}  // namespace sd
