// Device half of the disparity images (sd_disp_image; HBM bound, about ten bytes per output pixel, no MFMA): float32 disparity maps of B
// frames in device memory -> one colour-mapped u8 image per frame at the original frame size (contract: include/semdepth.h).  Every
// decision is a function of disp_image_rule.hpp, which sd_disp_image_host runs too: the images are the same bytes.  Compiled with
// -ffp-contract=off: the byte scaling is a float32 difference and a float32 product.  Launches, all on the caller's stream:
//   disp_init_kernel    the frames' four cells (key minimum, key maximum, lo8, hi8) set to their neutral values, flags to 0, and, when the
//                       caller gave no multipliers, those to 1
//   disp_range_kernel   per (block, frame): the minimum and maximum key of its finite scaled values -- four floats per lane, wave shuffles, LDS
//                       across the waves -- sent to the frame's cells with one 32-bit integer atomicMin and one atomicMax.  Integer minima
//                       and maxima: neither the grid nor the order of arrival changes the cells.
//   disp_bytes_kernel   per (block, frame): the range from the cells once per workgroup, then four pixels per lane to one dword of the byte
//                       image; a lane that meets a non-finite value stores 1 to the frame's flag (every writer stores the same value)
//   the resample        launch_pil_resample_u8 (seg_eval_gpu.hip) on the byte image, channels = 1; not launched when the sizes agree
//   disp_range8_kernel  per (block, frame): minimum and maximum byte of the resized frame, to the cells as above
//   disp_colour_kernel  per (block, frame): the workgroup builds the frame's 256-entry byte -> B | G << 8 | R << 16 table in LDS from
//                       (lo8, hi8, cmap), then a lane maps four pixels (one dword) to twelve bytes stored as three dwords
// The four-per-lane forms need a frame size that is a multiple of four and aligned bases (every frame then starts aligned); otherwise the
// same kernels run one pixel per lane with byte stores.
#include "disp_image_gpu.hpp"

#include "seg_eval_gpu.hpp"

#include <algorithm>

namespace sd {
namespace {

using namespace sddisp;

constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kWaves = kThreads / kWave;

struct Cells {
    uint32_t kmin, kmax, lo8, hi8;
};

__global__ __launch_bounds__(kThreads) void disp_init_kernel(Cells* cells, float* mult, int32_t* flags, int B, int has_mult) {
    const int b = blockIdx.x * kThreads + threadIdx.x;
    if (b >= B) return;
    cells[b] = Cells{kKeyNone, 0u, 255u, 0u};
    if (!has_mult) mult[b] = 1.0f;
    flags[b] = 0;
}

// minimum / maximum of one pair per lane over the workgroup, valid on thread 0 (s: 2 * kWaves words of LDS)
__device__ __forceinline__ void block_min_max(uint32_t& lo, uint32_t& hi, uint32_t* s) {
    const int t = threadIdx.x;
    for (int d = kWave / 2; d; d >>= 1) {
        const uint32_t ol = __shfl_xor(lo, d), oh = __shfl_xor(hi, d);
        lo = ol < lo ? ol : lo;
        hi = oh > hi ? oh : hi;
    }
    if ((t & (kWave - 1)) == 0) {
        s[2 * (t / kWave)] = lo;
        s[2 * (t / kWave) + 1] = hi;
    }
    __syncthreads();
    if (t == 0)
        for (int w = 1; w < kWaves; ++w) {
            lo = s[2 * w] < lo ? s[2 * w] : lo;
            hi = s[2 * w + 1] > hi ? s[2 * w + 1] : hi;
        }
}

// grid (blocks, B); n = pixels of a frame.  V = 4: n is a multiple of 4 and disp is 16-byte aligned.
template <int V>
__global__ __launch_bounds__(kThreads) void disp_range_kernel(const float* __restrict__ disp, size_t n, const float* __restrict__ mult,
                                                              Cells* __restrict__ cells) {
    __shared__ uint32_t s_red[2 * kWaves];
    const uint32_t b = blockIdx.y;
    const float* d = disp + (size_t)b * n;
    const float m = mult[b];
    const size_t units = n / V, stride = (size_t)gridDim.x * kThreads;
    uint32_t kmin = kKeyNone, kmax = 0;
    for (size_t u = (size_t)blockIdx.x * kThreads + threadIdx.x; u < units; u += stride) {
        float v[V];
        if constexpr (V == 4) {
            const float4 q = reinterpret_cast<const float4*>(d)[u];
            v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
        } else {
            v[0] = d[u];
        }
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float sv = scaled(v[j], m);
            if (finite_f32(sv)) {
                const uint32_t k = key_of(sv);
                kmin = k < kmin ? k : kmin;
                kmax = k > kmax ? k : kmax;
            }
        }
    }
    block_min_max(kmin, kmax, s_red);
    if (threadIdx.x == 0 && kmin <= kmax) {
        atomicMin(&cells[b].kmin, kmin);
        atomicMax(&cells[b].kmax, kmax);
    }
}

// grid (blocks, B).  V = 4: as above (the byte image begins the 16-byte aligned workspace part, so every frame's dwords are aligned).
template <int V>
__global__ __launch_bounds__(kThreads) void disp_bytes_kernel(const float* __restrict__ disp, size_t n, const float* __restrict__ mult,
                                                              const Cells* __restrict__ cells, uint8_t* __restrict__ bytes,
                                                              int32_t* __restrict__ flags) {
    __shared__ Range s_range;
    const uint32_t b = blockIdx.y;
    if (threadIdx.x == 0) s_range = make_range(cells[b].kmin, cells[b].kmax);
    __syncthreads();
    const Range r = s_range;
    const float* d = disp + (size_t)b * n;
    uint8_t* o = bytes + (size_t)b * n;
    const float m = mult[b];
    const size_t units = n / V, stride = (size_t)gridDim.x * kThreads;
    bool bad = false;
    for (size_t u = (size_t)blockIdx.x * kThreads + threadIdx.x; u < units; u += stride) {
        float v[V];
        if constexpr (V == 4) {
            const float4 q = reinterpret_cast<const float4*>(d)[u];
            v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
        } else {
            v[0] = d[u];
        }
        uint32_t word = 0;
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float sv = scaled(v[j], m);
            uint32_t p = 0;
            if (finite_f32(sv))
                p = byte_of(sv, r);
            else
                bad = true;
            word |= p << (8 * j);
        }
        if (V == 4)
            reinterpret_cast<uint32_t*>(o)[u] = word;
        else
            o[u] = (uint8_t)word;
    }
    if (bad) flags[b] = 1;
}

// grid (blocks, B); n = pixels of a resized frame.  V = 4: n is a multiple of 4 (img begins a 16-byte aligned workspace part).
template <int V>
__global__ __launch_bounds__(kThreads) void disp_range8_kernel(const uint8_t* __restrict__ img, size_t n, Cells* __restrict__ cells) {
    __shared__ uint32_t s_red[2 * kWaves];
    const uint32_t b = blockIdx.y;
    const uint8_t* p = img + (size_t)b * n;
    const size_t units = n / V, stride = (size_t)gridDim.x * kThreads;
    uint32_t lo = 255, hi = 0;
    for (size_t u = (size_t)blockIdx.x * kThreads + threadIdx.x; u < units; u += stride) {
        const uint32_t word = V == 4 ? reinterpret_cast<const uint32_t*>(p)[u] : (uint32_t)p[u];
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const uint32_t q = (word >> (8 * j)) & 0xff;
            lo = q < lo ? q : lo;
            hi = q > hi ? q : hi;
        }
    }
    block_min_max(lo, hi, s_red);
    if (threadIdx.x == 0 && lo <= hi) {
        atomicMin(&cells[b].lo8, lo);
        atomicMax(&cells[b].hi8, hi);
    }
}

// grid (blocks, B).  V = 4: n is a multiple of 4 and dst is 4-byte aligned (a frame's 3 * n bytes then keep every frame's dwords aligned).
template <int V>
__global__ __launch_bounds__(kThreads) void disp_colour_kernel(const uint8_t* __restrict__ img, size_t n, const Cells* __restrict__ cells, int cmap,
                                                               uint8_t* __restrict__ dst) {
    __shared__ uint32_t s_tab[256];
    static_assert(kThreads == 256, "one table entry per thread");
    const uint32_t b = blockIdx.y;
    s_tab[threadIdx.x] = bgr_of(cmap, index_of((int)threadIdx.x, (int)cells[b].lo8, (int)cells[b].hi8));
    __syncthreads();
    const uint8_t* p = img + (size_t)b * n;
    uint8_t* o = dst + (size_t)b * n * 3;
    const size_t units = n / V, stride = (size_t)gridDim.x * kThreads;
    for (size_t u = (size_t)blockIdx.x * kThreads + threadIdx.x; u < units; u += stride) {
        if (V == 4) {
            const uint32_t word = reinterpret_cast<const uint32_t*>(p)[u];
            const uint32_t c0 = s_tab[word & 0xff], c1 = s_tab[(word >> 8) & 0xff], c2 = s_tab[(word >> 16) & 0xff], c3 = s_tab[word >> 24];
            uint32_t* q = reinterpret_cast<uint32_t*>(o + u * 12);
            q[0] = c0 | c1 << 24;
            q[1] = c1 >> 8 | c2 << 16;
            q[2] = c2 >> 16 | c3 << 8;
        } else {
            const uint32_t c = s_tab[p[u]];
            o[u * 3] = (uint8_t)c;
            o[u * 3 + 1] = (uint8_t)(c >> 8);
            o[u * 3 + 2] = (uint8_t)(c >> 16);
        }
    }
}

// workgroups per frame: one per 256 units, at most what keeps the whole grid near 4096 workgroups (and never below 16 for a large frame)
unsigned frame_blocks(size_t units, int B) {
    const size_t want = (units + kThreads - 1) / kThreads;
    const size_t cap = std::max<size_t>(16, 4096 / (size_t)B);
    return (unsigned)std::max<size_t>(1, std::min(want, cap));
}

}  // namespace

hipError_t launch_disp_image(const float* disp, int B, int h, int w, int out_h, int out_w, int cmap, int has_mult, uint8_t* dst, int32_t* flags,
                             const sdpil::Windows& wx, uint8_t* workspace, hipStream_t s) {
    const Layout l(B, h, w, out_h, out_w);
    Cells* cells = reinterpret_cast<Cells*>(workspace + l.cells);
    float* mult = reinterpret_cast<float*>(workspace + l.mult);
    uint8_t* bytes = workspace + l.bytes;
    const size_t n = (size_t)h * w, n2 = (size_t)out_h * out_w;
    const bool resize = resized(h, w, out_h, out_w);
    const uint8_t* img = resize ? workspace + l.resized : bytes;

    hipLaunchKernelGGL(disp_init_kernel, dim3((unsigned)((B + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, cells, mult, flags, B, has_mult);
    const bool vec_in = n % 4 == 0 && (reinterpret_cast<uintptr_t>(disp) & 15) == 0;
    const dim3 grid_in(frame_blocks(vec_in ? n / 4 : n, B), (unsigned)B);
    if (vec_in) {
        hipLaunchKernelGGL(disp_range_kernel<4>, grid_in, dim3(kThreads), 0, s, disp, n, mult, cells);
        hipLaunchKernelGGL(disp_bytes_kernel<4>, grid_in, dim3(kThreads), 0, s, disp, n, mult, cells, bytes, flags);
    } else {
        hipLaunchKernelGGL(disp_range_kernel<1>, grid_in, dim3(kThreads), 0, s, disp, n, mult, cells);
        hipLaunchKernelGGL(disp_bytes_kernel<1>, grid_in, dim3(kThreads), 0, s, disp, n, mult, cells, bytes, flags);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (resize) {
        e = launch_pil_resample_u8(bytes, B, h, w, 1, 1, 0, workspace + l.resized, out_h, out_w, wx, workspace + l.pil, s);
        if (e != hipSuccess) return e;
    }
    const bool vec8 = n2 % 4 == 0;
    const dim3 grid8(frame_blocks(vec8 ? n2 / 4 : n2, B), (unsigned)B);
    if (vec8)
        hipLaunchKernelGGL(disp_range8_kernel<4>, grid8, dim3(kThreads), 0, s, img, n2, cells);
    else
        hipLaunchKernelGGL(disp_range8_kernel<1>, grid8, dim3(kThreads), 0, s, img, n2, cells);
    const bool vec_out = vec8 && (reinterpret_cast<uintptr_t>(dst) & 3) == 0;
    const dim3 grid_out(frame_blocks(vec_out ? n2 / 4 : n2, B), (unsigned)B);
    if (vec_out)
        hipLaunchKernelGGL(disp_colour_kernel<4>, grid_out, dim3(kThreads), 0, s, img, n2, cells, cmap, dst);
    else
        hipLaunchKernelGGL(disp_colour_kernel<1>, grid_out, dim3(kThreads), 0, s, img, n2, cells, cmap, dst);
    return hipGetLastError();
}

}  // namespace sd
