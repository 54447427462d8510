// Device half of the rendered clouds (sd_render_rw): the denoised road clouds and the sd_rw_result records of B frames in device memory ->
// one top-view image per frame, u8 [B,height,width,3] BGR (contract: include/semdepth.h).  A frame is the rows of ply_format.hpp's Frame,
// the rows of its _rw.ply: its n cloud points, then the 1001 points of the road-width line when the record has one; a workgroup owns 256
// consecutive rows of one frame, a lane one row.  Five launches, no host synchronisation, no floating-point atomics:
//   render_scan_kernel     per (frame, block): the minimum z of its finite rows in double -> workspace slots
//   render_min_kernel      one workgroup per frame: the slots reduced -> the frame's minimum z, flags[b] = 0 / 1
//   render_clear_kernel    the depth keys u64 [B,height,width] set to all ones, sixteen bytes per lane and turn
//   render_splat_kernel    per (frame, block): a lane projects its row ONCE and issues a 64-bit integer atomicMin (a vector global atomic) on
//                          every pixel of its square whose key it can still lower; the minimum of integers does not depend on the order in
//                          which workgroups arrive
//   render_resolve_kernel  a lane owns four consecutive pixels of the batch: it reads their keys, fetches the winning rows' colours from the
//                          cloud (or the line's, or the background) and stores twelve bytes as three aligned words
// Every decision is a function of render_rule.hpp, which sd_render_rw_host runs too: the images are the same bytes.
#include "render_gpu.hpp"

namespace sd {
namespace {

using namespace sdrender;

constexpr int kThreads = kBlockRows;
constexpr int kWaves = kThreads / 64;
constexpr unsigned kMaxGrid = 1u << 16;        // workgroups of the two pixel kernels; they stride over the rest

struct RenderArgs {
    const float* xyz;
    const uint8_t* rgb;
    const int32_t* n;
    const sd_rw_result* records;
    int B, cap;
    uint32_t nblk;
    sd_render_camera cam;
    uint8_t* dst;
    int32_t* flags;
    unsigned long long* keys;      // [B,height,width]
    double *bmin, *zmin;           // [B,nblk], [B]
    size_t pixels;                 // B * height * width
};

__device__ __forceinline__ sdply::Frame load_frame(const RenderArgs& a, uint32_t b) {
    const sd_rw_result& r = a.records[b];
    return make_frame(a.xyz + (size_t)b * a.cap * 3, a.rgb + (size_t)b * a.cap * 3, a.n[b], a.cap, r.left_pt, r.right_pt, r.found);
}

// the minimum of one value per lane over the workgroup, on lane 0 (s: kWaves doubles of LDS)
__device__ __forceinline__ double block_min(double z, double* s) {
    const int t = threadIdx.x;
    for (int d = 32; d; d >>= 1) {
        const double o = __shfl_xor(z, d);
        z = o < z ? o : z;
    }
    if ((t & 63) == 0) s[t >> 6] = z;
    __syncthreads();
    if (t == 0)
        for (int w = 1; w < kWaves; ++w) z = s[w] < z ? s[w] : z;
    return z;
}

__global__ __launch_bounds__(kThreads) void render_scan_kernel(RenderArgs a) {
    __shared__ double s_min[kWaves];
    const int t = threadIdx.x;
    const uint32_t blk = blockIdx.x, b = blockIdx.y;
    const sdply::Frame f = load_frame(a, b);
    const int64_t r = (int64_t)blk * kBlockRows + t;
    double z = __builtin_huge_val();
    if (r < f.rows) {
        double p[3];
        uint8_t c[3];
        sdply::row_point(f, (int)r, p, c);
        if (finite3(p)) z = p[2];
    }
    z = block_min(z, s_min);
    if (t == 0) a.bmin[(size_t)b * a.nblk + blk] = z;
}

__global__ __launch_bounds__(kThreads) void render_min_kernel(RenderArgs a) {
    __shared__ double s_min[kWaves];
    const int t = threadIdx.x;
    const uint32_t b = blockIdx.x;
    double z = __builtin_huge_val();
    for (uint32_t i = t; i < a.nblk; i += kThreads) {
        const double o = a.bmin[(size_t)b * a.nblk + i];
        z = o < z ? o : z;
    }
    z = block_min(z, s_min);
    if (t == 0) {
        const int32_t n = a.n[b];
        a.zmin[b] = z;
        a.flags[b] = n < 0 || n > a.cap ? 1 : 0;
    }
}

__global__ __launch_bounds__(kThreads) void render_clear_kernel(RenderArgs a) {
    const size_t pairs = a.pixels / 2, stride = (size_t)gridDim.x * kThreads;
    ulonglong2* k2 = reinterpret_cast<ulonglong2*>(a.keys);                 // the keys begin the 16-byte aligned workspace
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < pairs; i += stride) k2[i] = make_ulonglong2(kEmptyKey, kEmptyKey);
    if ((a.pixels & 1) && blockIdx.x == 0 && threadIdx.x == 0) a.keys[a.pixels - 1] = kEmptyKey;
}

__global__ __launch_bounds__(kThreads) void render_splat_kernel(RenderArgs a) {
    const uint32_t blk = blockIdx.x, b = blockIdx.y;
    const sdply::Frame f = load_frame(a, b);
    const int64_t r = (int64_t)blk * kBlockRows + threadIdx.x;
    if (r >= f.rows) return;
    double p[3];
    uint8_t c[3];
    sdply::row_point(f, (int)r, p, c);
    if (!finite3(p) || !(p[2] > a.zmin[b])) return;
    Hit h;
    if (!project(a.cam, p, &h)) return;
    const Box box = splat_box(a.cam, h);
    const unsigned long long key = make_key(h.zbits, (uint32_t)r);
    unsigned long long* frame = a.keys + (size_t)b * a.cam.height * a.cam.width;
    // A pixel's key only ever falls, so a key that is not below a value READ from the pixel -- however old that value is -- cannot lower it: the
    // atomic is issued only for the others.  The final keys are the same; most rows of a dense cloud lose to a nearer row and issue none.
    for (int y = box.y0; y <= box.y1; ++y)
        for (int x = box.x0; x <= box.x1; ++x) {
            unsigned long long* q = frame + (size_t)y * a.cam.width + x;
            if (key < __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(q, key);
        }
}

__global__ __launch_bounds__(kThreads) void render_resolve_kernel(RenderArgs a) {
    const size_t frame_px = (size_t)a.cam.height * a.cam.width;
    const size_t groups = (a.pixels + kGroup - 1) / kGroup, stride = (size_t)gridDim.x * kThreads;
    for (size_t g = (size_t)blockIdx.x * kThreads + threadIdx.x; g < groups; g += stride) {
        const size_t p0 = g * kGroup;
        const int cnt = a.pixels - p0 < (size_t)kGroup ? (int)(a.pixels - p0) : kGroup;
        union {
            uint8_t bytes[3 * kGroup];
            uint32_t words[3];
        } out;
#pragma unroll
        for (int j = 0; j < kGroup; ++j) {
            if (j >= cnt) continue;
            const size_t b = (p0 + j) / frame_px;
            const unsigned long long key = a.keys[p0 + j];
            // (a key that is not empty names a row below this frame's rows, so n[b] is inside 0..cap where it is used)
            resolve(a.cam, key, a.rgb + b * (size_t)a.cap * 3, key == kEmptyKey ? 0 : a.n[b], out.bytes + 3 * j);
        }
        uint8_t* q = a.dst + 3 * p0;                                         // dst is 4-byte aligned and 3 * p0 a multiple of twelve
        if (cnt == kGroup) {
            uint32_t* w = reinterpret_cast<uint32_t*>(q);
            w[0] = out.words[0];
            w[1] = out.words[1];
            w[2] = out.words[2];
        } else {
#pragma unroll
            for (int j = 0; j < 3 * kGroup; ++j)
                if (j < 3 * cnt) q[j] = out.bytes[j];
        }
    }
}

unsigned pixel_grid(size_t items) {
    const size_t g = (items + kThreads - 1) / kThreads;
    return (unsigned)(g < 1 ? 1 : g > kMaxGrid ? kMaxGrid : g);
}

}  // namespace

hipError_t launch_render_rw(const float* xyz, const uint8_t* rgb, const int32_t* n, int B, int cap, const sd_rw_result* records,
                            const sd_render_camera& cam, uint8_t* dst, int32_t* flags, uint8_t* workspace, hipStream_t s) {
    const size_t nblk = sdply::blocks_per_frame(cap);
    RenderArgs a{};
    a.xyz = xyz; a.rgb = rgb; a.n = n; a.records = records; a.B = B; a.cap = cap; a.nblk = (uint32_t)nblk;
    a.cam = cam; a.dst = dst; a.flags = flags;
    a.pixels = sdrender::key_count(B, cam);
    const sdrender::Layout l(B, cap, cam);
    a.keys = reinterpret_cast<unsigned long long*>(workspace + l.keys);
    a.bmin = reinterpret_cast<double*>(workspace + l.bmin);
    a.zmin = reinterpret_cast<double*>(workspace + l.zmin);
    const dim3 grid((unsigned)nblk, (unsigned)B);
    hipLaunchKernelGGL(render_scan_kernel, grid, dim3(kThreads), 0, s, a);
    hipLaunchKernelGGL(render_min_kernel, dim3((unsigned)B), dim3(kThreads), 0, s, a);
    hipLaunchKernelGGL(render_clear_kernel, dim3(pixel_grid(a.pixels / 2)), dim3(kThreads), 0, s, a);
    hipLaunchKernelGGL(render_splat_kernel, grid, dim3(kThreads), 0, s, a);
    hipLaunchKernelGGL(render_resolve_kernel, dim3(pixel_grid((a.pixels + kGroup - 1) / kGroup)), dim3(kThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace sd
