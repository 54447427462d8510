// Device half of the road PLY writer (sd_ply_format_rw): the denoised road clouds and the sd_rw_result records of B frames in device
// memory -> the text of every frame's <name>_rw.ply, packed back to back (contract: include/semdepth.h).  A frame is the rows of
// ply_format.hpp's Frame: its n cloud points, then the 1001 points of the road-width line when the record has one; a workgroup owns 256
// consecutive rows of one frame, a lane one row.  Five launches, no host synchronisation, no floating-point atomics:
//   ply_scan_kernel     per (frame, block): the minimum z of its rows in double and the range verdict (finite, |v| < 2^31) -> workspace slots
//   ply_min_kernel      one workgroup per frame: the slots reduced -> the frame's minimum z, flags[b] = 0 / 1
//   ply_length_kernel   per (frame, block): rows above the minimum, their exact text length (the rounded integer parts) -> block sums
//   ply_layout_kernel   ONE workgroup: exclusive scans of the block sums inside each frame and of the frame sizes across the frames, the
//                       capacity flags, offsets[], the headers
//   ply_rows_kernel     per (frame, block): the kept rows formatted straight into their compacted place in LDS (block-local scan of the
//                       lengths), then stored to the block's byte range: whole words on aligned addresses, head and tail bytes apart
// Every digit is a function of ply_format.hpp, which sd_ply_format_rw_host runs too: the files are the same bytes.
#include "ply_gpu.hpp"

namespace sd {
namespace {

using namespace sdply;

constexpr int kThreads = kBlockRows;
constexpr int kWaves = kThreads / 64;

struct PlyArgs {
    const float* xyz;
    const uint8_t* rgb;
    const int32_t* n;
    const sd_rw_result* records;
    int B, cap;
    uint32_t nblk;
    uint8_t* text;
    uint64_t capacity;
    uint64_t* offsets;
    int32_t* flags;
    double *bmin, *zmin;
    uint64_t *boff, *fbase;
    uint32_t *blen, *bcnt, *bbad;
};

__device__ __forceinline__ Frame load_frame(const PlyArgs& a, uint32_t b) {
    const sd_rw_result& r = a.records[b];
    return make_frame(a.xyz + (size_t)b * a.cap * 3, a.rgb + (size_t)b * a.cap * 3, a.n[b], a.cap, r.left_pt, r.right_pt, r.found);
}

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

__global__ __launch_bounds__(kThreads) void ply_scan_kernel(PlyArgs a) {
    __shared__ double s_min[kWaves];
    __shared__ uint32_t s_bad[kWaves];
    const int t = threadIdx.x;
    const uint32_t blk = blockIdx.x, b = blockIdx.y;
    const Frame f = load_frame(a, b);
    const int64_t r = (int64_t)blk * kBlockRows + t;
    double z = __builtin_huge_val();
    uint32_t bad = f.bad;
    if (r < f.rows) {
        double p[3];
        uint8_t c[3];
        row_point(f, (int)r, p, c);
        bad |= !in_range(p[0]) || !in_range(p[1]) || !in_range(p[2]);
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

__global__ __launch_bounds__(kThreads) void ply_min_kernel(PlyArgs a) {
    __shared__ double s_min[kWaves];
    __shared__ uint32_t s_bad[kWaves];
    const int t = threadIdx.x;
    const uint32_t b = blockIdx.x;
    double z = __builtin_huge_val();
    uint32_t bad = 0;
    for (uint32_t i = t; i < a.nblk; i += kThreads) {
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
        a.flags[b] = bad ? 1 : 0;
    }
}

__global__ __launch_bounds__(kThreads) void ply_length_kernel(PlyArgs a) {
    __shared__ uint32_t s_len[kWaves], s_cnt[kWaves];
    const int t = threadIdx.x;
    const uint32_t blk = blockIdx.x, b = blockIdx.y;
    if (a.flags[b]) return;                           // (the layout and the rows kernel do not read a flagged frame's slots)
    const Frame f = load_frame(a, b);
    const double zmin = a.zmin[b];
    const int64_t r = (int64_t)blk * kBlockRows + t;
    uint32_t len = 0, cnt = 0;
    if (r < f.rows) {
        double p[3];
        uint8_t c[3];
        row_point(f, (int)r, p, c);
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
__global__ __launch_bounds__(kThreads) void ply_layout_kernel(PlyArgs a) {
    __shared__ uint64_t s_scan[kThreads];
    __shared__ uint32_t s_cnt[kThreads];
    __shared__ int32_t s_flag;
    const int t = threadIdx.x;
    uint64_t off = 0;                                 // (the same value on every lane)
    for (int b = 0; b < a.B; ++b) {
        __syncthreads();
        if (t == 0) {
            s_flag = a.flags[b];
            a.offsets[b] = off;
        }
        __syncthreads();
        if (s_flag) continue;
        uint64_t body = 0;
        uint32_t count = 0;
        for (uint32_t c0 = 0; c0 < a.nblk; c0 += kThreads) {
            const uint32_t i = c0 + t;
            const size_t id = (size_t)b * a.nblk + i;
            uint64_t total;
            uint32_t ctotal;
            const uint64_t len = i < a.nblk ? a.blen[id] : 0;
            const uint64_t excl = block_exclusive_scan<uint64_t>(len, s_scan, &total);
            block_exclusive_scan<uint32_t>(i < a.nblk ? a.bcnt[id] : 0u, s_cnt, &ctotal);
            if (i < a.nblk) a.boff[id] = body + excl;
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
    if (t == 0) a.offsets[a.B] = off;
}

__global__ __launch_bounds__(kThreads) void ply_rows_kernel(PlyArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t buf[kBlockRows * kRowCap + 8];
    __shared__ uint32_t s_scan[kThreads];
    const int t = threadIdx.x;
    const uint32_t blk = blockIdx.x, b = blockIdx.y;
    if (a.flags[b]) return;
    const size_t id = (size_t)b * a.nblk + blk;
    const uint32_t total = a.blen[id];
    if (!total) return;
    const Frame f = load_frame(a, b);
    const double zmin = a.zmin[b];
    const int64_t r = (int64_t)blk * kBlockRows + t;
    Row row;
    uint32_t len = 0;
    if (r < f.rows) {
        double p[3];
        uint8_t c[3];
        row_point(f, (int)r, p, c);
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

hipError_t launch_ply_format(const float* xyz, const uint8_t* rgb, const int32_t* n, int B, int cap, const sd_rw_result* records, uint8_t* text,
                             size_t capacity, uint64_t* offsets, int32_t* flags, uint8_t* workspace, hipStream_t s) {
    const size_t nblk = blocks_per_frame(cap);
    PlyArgs a{};
    a.xyz = xyz; a.rgb = rgb; a.n = n; a.records = records; a.B = B; a.cap = cap; a.nblk = (uint32_t)nblk;
    a.text = text; a.capacity = capacity; a.offsets = offsets; a.flags = flags;
    const Layout l(B, cap);
    a.bmin = reinterpret_cast<double*>(workspace + l.bmin);
    a.boff = reinterpret_cast<uint64_t*>(workspace + l.boff);
    a.zmin = reinterpret_cast<double*>(workspace + l.zmin);
    a.fbase = reinterpret_cast<uint64_t*>(workspace + l.fbase);
    a.blen = reinterpret_cast<uint32_t*>(workspace + l.blen);
    a.bcnt = reinterpret_cast<uint32_t*>(workspace + l.bcnt);
    a.bbad = reinterpret_cast<uint32_t*>(workspace + l.bbad);
    const dim3 grid((unsigned)nblk, (unsigned)B);
    hipLaunchKernelGGL(ply_scan_kernel, grid, dim3(kThreads), 0, s, a);
    hipLaunchKernelGGL(ply_min_kernel, dim3((unsigned)B), dim3(kThreads), 0, s, a);
    hipLaunchKernelGGL(ply_length_kernel, grid, dim3(kThreads), 0, s, a);
    hipLaunchKernelGGL(ply_layout_kernel, dim3(1), dim3(kThreads), 0, s, a);
    hipLaunchKernelGGL(ply_rows_kernel, grid, dim3(kThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace sd
