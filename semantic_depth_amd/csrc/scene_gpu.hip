// Device half of the scene PLY writer (sd_scene_format): the final road clouds, the denoised fence clouds, the records of both chains and
// the boxes of the three plane fits of B frames in device memory -> the text of every frame's scene file (or of its _ROAD / _FENCE file:
// the mask), packed back to back (contract: include/semdepth.h).  A frame is the rows of scene_format.hpp's eight segments; a workgroup
// owns 256 consecutive rows of one frame, a lane one row.  The grid is sized from the host-known bound of a frame's rows under the mask; a workgroup
// behind the frame's last row exits at once and neither writes nor is read.  Six launches, no host synchronisation, no floating-point atomics:
//   scene_table_kernel    one thread per frame: the segment table (row counts, prefix, n_a and the steps of each lattice, flags 1 and 3)
//   scene_scan_kernel     per (frame, block): the minimum z of its rows in double and the range verdict -> workspace slots
//   scene_min_kernel      one workgroup per frame: the used slots reduced -> the frame's minimum z, flags[b] = 0 / 1 / 3
//   scene_length_kernel   per (frame, block): rows above the minimum, their exact text length -> block sums
//   scene_layout_kernel   ONE workgroup: exclusive scans of the block sums inside each frame and of the frame sizes across the frames, the
//                         capacity flags, offsets[], the headers
//   scene_rows_kernel     per (frame, block): the kept rows formatted into their compacted place in LDS, then stored to the block's byte range
// The five behind the table are ply_gpu.hip's over another row source; every digit is a function of ply_format.hpp and every row one of
// scene_format.hpp, which sd_scene_format_host runs too: the files are the same bytes.
#include "scene_gpu.hpp"

namespace sd {
namespace {

using namespace sdply;
using sdscene::SceneIn;
using sdscene::SegTable;

constexpr int kThreads = kBlockRows;
constexpr int kWaves = kThreads / 64;

struct SceneArgs {
    SceneBatch in;
    uint32_t nblk;
    uint8_t* text;
    uint64_t capacity;
    uint64_t* offsets;
    int32_t* flags;
    double *bmin, *zmin;
    uint64_t *boff, *fbase;
    SegTable* tab;
    uint32_t *blen, *bcnt, *bbad;
};

__device__ __forceinline__ SceneIn load_in(const SceneArgs& a, uint32_t b) {
    const SceneBatch& s = a.in;
    SceneIn in;
    const size_t ro = (size_t)b * s.cap_road * 3, fo = (size_t)b * s.cap_fence * 3;
    in.road_xyz = s.road_xyz + ro;
    in.road_rgb = s.road_rgb + ro;
    in.left_xyz = s.left_xyz ? s.left_xyz + fo : nullptr;
    in.left_rgb = s.left_rgb ? s.left_rgb + fo : nullptr;
    in.right_xyz = s.right_xyz ? s.right_xyz + fo : nullptr;
    in.right_rgb = s.right_rgb ? s.right_rgb + fo : nullptr;
    in.n_road = s.n_road[b];
    in.cap_road = s.cap_road;
    in.cap_fence = s.cap_fence;
    in.rec = s.records + b;
    in.f2f = s.f2f ? s.f2f + b : nullptr;
    in.road_box = s.road_boxes ? s.road_boxes + b : nullptr;
    in.fence_box = s.fence_boxes ? s.fence_boxes + 2 * (size_t)b : nullptr;
    in.mask = s.mask;
    in.lattice_cap = s.lattice_cap;
    return in;
}

__device__ __forceinline__ uint32_t used_blocks(const SegTable& t) { return (t.prefix[sdscene::kSegs] + kBlockRows - 1) / kBlockRows; }

// exclusive scan of one value per lane over the workgroup (s: kThreads words of LDS); *total = the sum
template <class T>
__device__ __forceinline__ T block_exclusive_scan(T v, T* s, T* total) {
    const int t = threadIdx.x;
    __syncthreads();                                  // (s may still be read from the call before)
    s[t] = v;
    __syncthreads();
    for (int d = 1; d < kThreads; d <<= 1) {
        const T u = t >= d ? s[t - d] : (T)0;
        __syncthreads();
        s[t] += u;
        __syncthreads();
    }
    *total = s[kThreads - 1];
    return s[t] - v;
}

__global__ __launch_bounds__(64) void scene_table_kernel(SceneArgs a) {
    const uint32_t b = blockIdx.x * 64 + threadIdx.x;
    if (b >= (uint32_t)a.in.B) return;
    const SceneIn in = load_in(a, b);
    sdscene::build_table(in, a.tab + b);
}

__global__ __launch_bounds__(kThreads) void scene_scan_kernel(SceneArgs a) {
    __shared__ double s_min[kWaves];
    __shared__ uint32_t s_bad[kWaves];
    const int t = threadIdx.x;
    const uint32_t blk = blockIdx.x, b = blockIdx.y;
    const SegTable& tab = a.tab[b];
    if (blk >= used_blocks(tab)) return;
    const SceneIn in = load_in(a, b);
    const uint32_t r = blk * kBlockRows + t;
    double z = __builtin_huge_val();
    uint32_t bad = 0;
    if (r < tab.prefix[sdscene::kSegs]) {
        double p[3];
        uint8_t c[3];
        sdscene::row_point(in, tab, r, p, c);
        bad = !in_range(p[0]) || !in_range(p[1]) || !in_range(p[2]);
        z = p[2];
    }
    for (int d = 32; d; d >>= 1) {
        const double o = __shfl_xor(z, d);
        z = o < z ? o : z;
        bad |= __shfl_xor(bad, d);
    }
    if ((t & 63) == 0) {
        s_min[t >> 6] = z;
        s_bad[t >> 6] = bad;
    }
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < kWaves; ++w) {
            z = s_min[w] < z ? s_min[w] : z;
            bad |= s_bad[w];
        }
        const size_t id = (size_t)b * a.nblk + blk;
        a.bmin[id] = z;
        a.bbad[id] = bad;
    }
}

__global__ __launch_bounds__(kThreads) void scene_min_kernel(SceneArgs a) {
    __shared__ double s_min[kWaves];
    __shared__ uint32_t s_bad[kWaves];
    const int t = threadIdx.x;
    const uint32_t b = blockIdx.x;
    const SegTable& tab = a.tab[b];
    const uint32_t used = used_blocks(tab);
    double z = __builtin_huge_val();
    uint32_t bad = 0;
    for (uint32_t i = t; i < used; i += kThreads) {
        const size_t id = (size_t)b * a.nblk + i;
        const double o = a.bmin[id];
        z = o < z ? o : z;
        bad |= a.bbad[id];
    }
    for (int d = 32; d; d >>= 1) {
        const double o = __shfl_xor(z, d);
        z = o < z ? o : z;
        bad |= __shfl_xor(bad, d);
    }
    if ((t & 63) == 0) {
        s_min[t >> 6] = z;
        s_bad[t >> 6] = bad;
    }
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < kWaves; ++w) {
            z = s_min[w] < z ? s_min[w] : z;
            bad |= s_bad[w];
        }
        a.zmin[b] = z;
        a.flags[b] = tab.flag ? tab.flag : (bad ? 1 : 0);
    }
}

__global__ __launch_bounds__(kThreads) void scene_length_kernel(SceneArgs a) {
    __shared__ uint32_t s_len[kWaves], s_cnt[kWaves];
    const int t = threadIdx.x;
    const uint32_t blk = blockIdx.x, b = blockIdx.y;
    const SegTable& tab = a.tab[b];
    if (blk >= used_blocks(tab) || a.flags[b]) return;        // (the layout and the rows kernel do not read a flagged frame's slots)
    const SceneIn in = load_in(a, b);
    const double zmin = a.zmin[b];
    const uint32_t r = blk * kBlockRows + t;
    uint32_t len = 0, cnt = 0;
    if (r < tab.prefix[sdscene::kSegs]) {
        double p[3];
        uint8_t c[3];
        sdscene::row_point(in, tab, r, p, c);
        if (p[2] > zmin) {
            len = (uint32_t)row_len(make_row(p, c));
            cnt = 1;
        }
    }
    for (int d = 32; d; d >>= 1) {
        len += __shfl_xor(len, d);
        cnt += __shfl_xor(cnt, d);
    }
    if ((t & 63) == 0) {
        s_len[t >> 6] = len;
        s_cnt[t >> 6] = cnt;
    }
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < kWaves; ++w) {
            len += s_len[w];
            cnt += s_cnt[w];
        }
        const size_t id = (size_t)b * a.nblk + blk;
        a.blen[id] = len;
        a.bcnt[id] = cnt;
    }
}

// one workgroup: where every block and every frame goes, which frames do not fit, and everything of the text that is not a row
__global__ __launch_bounds__(kThreads) void scene_layout_kernel(SceneArgs a) {
    __shared__ uint64_t s_scan[kThreads];
    __shared__ uint32_t s_cnt[kThreads];
    __shared__ int32_t s_flag;
    __shared__ uint32_t s_used;
    const int t = threadIdx.x;
    uint64_t off = 0;                                 // (the same value on every lane)
    for (int b = 0; b < a.in.B; ++b) {
        __syncthreads();
        if (t == 0) {
            s_flag = a.flags[b];
            s_used = used_blocks(a.tab[b]);
            a.offsets[b] = off;
        }
        __syncthreads();
        if (s_flag) continue;
        const uint32_t used = s_used;
        uint64_t body = 0;
        uint32_t count = 0;
        for (uint32_t c0 = 0; c0 < used; c0 += kThreads) {
            const uint32_t i = c0 + t;
            const size_t id = (size_t)b * a.nblk + i;
            uint64_t total;
            uint32_t ctotal;
            const uint64_t len = i < used ? a.blen[id] : 0;
            const uint64_t excl = block_exclusive_scan<uint64_t>(len, s_scan, &total);
            block_exclusive_scan<uint32_t>(i < used ? a.bcnt[id] : 0u, s_cnt, &ctotal);
            if (i < used) a.boff[id] = body + excl;
            body += total;
            count += ctotal;
        }
        const int hdr = header_len(count);
        const uint64_t size = (uint64_t)hdr + body;
        if (size > a.capacity - off) {                // off <= capacity always
            if (t == 0) a.flags[b] = 2;
            continue;
        }
        if (t == 0) a.fbase[b] = off + (uint64_t)hdr;
        for (int i = t; i < hdr; i += kThreads) a.text[off + (uint64_t)i] = header_byte(i, count);
        off += size;
    }
    if (t == 0) a.offsets[a.in.B] = off;
}

__global__ __launch_bounds__(kThreads) void scene_rows_kernel(SceneArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t buf[kBlockRows * kRowCap + 8];
    __shared__ uint32_t s_scan[kThreads];
    const int t = threadIdx.x;
    const uint32_t blk = blockIdx.x, b = blockIdx.y;
    const SegTable& tab = a.tab[b];
    if (blk >= used_blocks(tab) || a.flags[b]) return;
    const size_t id = (size_t)b * a.nblk + blk;
    const uint32_t total = a.blen[id];
    if (!total) return;
    const SceneIn in = load_in(a, b);
    const double zmin = a.zmin[b];
    const uint32_t r = blk * kBlockRows + t;
    Row row;
    uint32_t len = 0;
    if (r < tab.prefix[sdscene::kSegs]) {
        double p[3];
        uint8_t c[3];
        sdscene::row_point(in, tab, r, p, c);
        if (p[2] > zmin) {
            row = make_row(p, c);
            len = (uint32_t)row_len(row);
        }
    }
    uint32_t sum;
    const uint32_t excl = block_exclusive_scan<uint32_t>(len, s_scan, &sum);
    // the block's bytes sit in LDS at the misalignment of their destination, so that LDS word i is one aligned word of the text
    uint8_t* dst = a.text + a.fbase[b] + a.boff[id];
    const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 3);
    if (len) put_row(buf + mis + excl, row);
    __syncthreads();
    const uint32_t head = (4 - mis) & 3, h = head < total ? head : total;
    const uint32_t words = (total - h) / 4;
    if ((uint32_t)t < h) dst[t] = buf[mis + t];
    const uint32_t* src = reinterpret_cast<const uint32_t*>(buf + mis + h);          // mis + h is 0 or 4 whenever words > 0
    uint32_t* out = reinterpret_cast<uint32_t*>(dst + h);
    for (uint32_t i = t; i < words; i += kThreads) out[i] = src[i];
    const uint32_t done = h + 4 * words;
    if ((uint32_t)t < total - done) dst[done + t] = buf[mis + done + t];
}

}  // namespace

hipError_t launch_scene_format(const SceneBatch& in, uint8_t* text, size_t capacity, uint64_t* offsets, int32_t* flags, uint8_t* workspace,
                               hipStream_t s) {
    const int B = in.B;
    const size_t nblk = (size_t)sdscene::blocks_bound(in.cap_road, in.cap_fence, in.lattice_cap, in.mask);
    SceneArgs a{};
    a.in = in; a.nblk = (uint32_t)nblk;
    a.text = text; a.capacity = capacity; a.offsets = offsets; a.flags = flags;
    const sdscene::Layout l(B, in.cap_road, in.cap_fence, in.lattice_cap, in.mask);
    a.bmin = reinterpret_cast<double*>(workspace + l.bmin);
    a.boff = reinterpret_cast<uint64_t*>(workspace + l.boff);
    a.zmin = reinterpret_cast<double*>(workspace + l.zmin);
    a.fbase = reinterpret_cast<uint64_t*>(workspace + l.fbase);
    a.tab = reinterpret_cast<SegTable*>(workspace + l.tab);
    a.blen = reinterpret_cast<uint32_t*>(workspace + l.blen);
    a.bcnt = reinterpret_cast<uint32_t*>(workspace + l.bcnt);
    a.bbad = reinterpret_cast<uint32_t*>(workspace + l.bbad);
    const dim3 grid((unsigned)nblk, (unsigned)B);
    hipLaunchKernelGGL(scene_table_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, s, a);
    hipLaunchKernelGGL(scene_scan_kernel, grid, dim3(kThreads), 0, s, a);
    hipLaunchKernelGGL(scene_min_kernel, dim3((unsigned)B), dim3(kThreads), 0, s, a);
    hipLaunchKernelGGL(scene_length_kernel, grid, dim3(kThreads), 0, s, a);
    hipLaunchKernelGGL(scene_layout_kernel, dim3(1), dim3(kThreads), 0, s, a);
    hipLaunchKernelGGL(scene_rows_kernel, grid, dim3(kThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace sd
