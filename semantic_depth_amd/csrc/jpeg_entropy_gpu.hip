// JPEG entropy decoding on the device (sd_jpeg_entropy_decode): one lane per restart interval, running sdjent::decode_interval -- the
// function the CPU statement runs -- on the scan bytes the host staged.  A workgroup is one wave of 64 lanes serving 64 consecutive
// intervals of ONE frame (a frame with more intervals takes several workgroups), so the frame's Huffman tables are staged once into
// LDS: 1488 bytes per table (the 1 KB look-ahead plus the slow-path tables), only the slots the scan names, 11.6 KB when all eight are.
// Lanes of a wave diverge (each follows its own code lengths); that is accepted here, see DESIGN.md.
// The coefficients are cleared by a kernel of their own (every eligible frame's descriptor extent, nothing behind it and no other
// frame's slot) and the lanes store only non-zero coefficients: a lane never holds a 64-entry block it would have to index dynamically.
#include "jpeg_entropy_gpu.hpp"

namespace sd {
namespace {

constexpr int kLanes = 64;
constexpr int kClearThreads = 256, kClearBlocks = 32;

struct EntArgs {
    const uint8_t* bytes;
    size_t byte_stride;
    const sd_jpeg_entropy_frame* frames;
    const sd_jpeg_huff_table* tables;
    const sd_jpeg_interval* intervals;
    size_t interval_stride;
    int16_t* coef;
    size_t coef_stride;           // int16 elements
    int32_t* status;
};

// int16 elements of the frame's coefficients, from the record alone (frame_ok() has tied it to the descriptor's count)
__device__ inline size_t record_coef_elems(const sd_jpeg_entropy_frame& fr) {
    size_t n = 0;
    for (int c = 0; c < fr.ncomp; ++c) n += (size_t)fr.mcus_x * fr.comp_h[c] * fr.mcus_y * fr.comp_v[c] * 64;
    return n;
}

__global__ __launch_bounds__(kClearThreads) void jpeg_entropy_clear_kernel(EntArgs a) {
    const uint32_t b = blockIdx.y;
    if (blockIdx.x == 0 && threadIdx.x == 0) a.status[b] = 0;
    const sd_jpeg_entropy_frame& fr = a.frames[b];
    if (!fr.eligible) return;
    // 16-byte stores: the frame's slot begins at a multiple of 16 bytes and its element count is a multiple of 64
    const size_t n16 = record_coef_elems(fr) / 8;
    uint4* dst = reinterpret_cast<uint4*>(a.coef + (size_t)b * a.coef_stride);
    for (size_t i = (size_t)blockIdx.x * kClearThreads + threadIdx.x; i < n16; i += (size_t)kClearBlocks * kClearThreads)
        dst[i] = make_uint4(0, 0, 0, 0);                       // i < n16: inside the frame's coefficients
}

__global__ __launch_bounds__(kLanes) void jpeg_entropy_kernel(EntArgs a) {
    __shared__ sd_jpeg_huff_table tabs[sdjent::kTables];
    __shared__ sd_jpeg_entropy_frame fr;
    const int t = threadIdx.x;
    const uint32_t b = blockIdx.y;
    const sd_jpeg_entropy_frame& g = a.frames[b];
    const int first = (int)blockIdx.x * kLanes;
    if (!g.eligible || first >= g.n_intervals) return;         // (uniform over the workgroup)
    constexpr int kFrameWords = sizeof(sd_jpeg_entropy_frame) / 4, kTableWords = sizeof(sd_jpeg_huff_table) / 4;
    if (t < kFrameWords) reinterpret_cast<uint32_t*>(&fr)[t] = reinterpret_cast<const uint32_t*>(&g)[t];
    uint32_t named = 0;                                        // comp_dc / comp_ac are 0..3 (frame_ok()): bits 0..7
    for (int c = 0; c < g.ncomp; ++c) named |= (1u << g.comp_dc[c]) | (16u << g.comp_ac[c]);
    for (int slot = 0; slot < sdjent::kTables; ++slot) {
        if (!(named >> slot & 1)) continue;
        const uint32_t* src = reinterpret_cast<const uint32_t*>(a.tables + (size_t)b * sdjent::kTables + slot);
        uint32_t* dst = reinterpret_cast<uint32_t*>(&tabs[slot]);
        for (int i = t; i < kTableWords; i += kLanes) dst[i] = src[i];
    }
    __syncthreads();
    const int i = first + t;
    if (i >= fr.n_intervals) return;
    const sd_jpeg_interval iv = a.intervals[(size_t)b * a.interval_stride + i];      // i < n_intervals <= interval_stride
    const int r = sdjent::decode_interval(a.bytes + (size_t)b * a.byte_stride, iv.begin, iv.end, fr, tabs, i, a.coef + (size_t)b * a.coef_stride);
    if (r != sdjent::kOk) a.status[b] = r;                     // (any refusing lane's code: the word only has to be non-zero)
}

static_assert(sizeof(sd_jpeg_entropy_frame) % 4 == 0 && sizeof(sd_jpeg_huff_table) % 4 == 0, "the staging loops copy dwords");

}  // namespace

hipError_t launch_jpeg_entropy_decode(const uint8_t* bytes, size_t byte_stride, const sd_jpeg_frame_desc*, const sd_jpeg_entropy_frame* frames_host,
                                      const sd_jpeg_interval* intervals_host, size_t interval_stride, const sd_jpeg_huff_table* tables_host, int B,
                                      int16_t* coef, size_t coef_stride_elems, int32_t* status, uint8_t* workspace, hipStream_t s) {
    EntArgs a{};
    a.bytes = bytes; a.byte_stride = byte_stride; a.interval_stride = interval_stride; a.coef = coef; a.coef_stride = coef_stride_elems; a.status = status;
    const sdjent::Layout l(B, interval_stride);
    sd_jpeg_entropy_frame* frames = reinterpret_cast<sd_jpeg_entropy_frame*>(workspace + l.frames);
    sd_jpeg_huff_table* tables = reinterpret_cast<sd_jpeg_huff_table*>(workspace + l.tables);
    sd_jpeg_interval* intervals = reinterpret_cast<sd_jpeg_interval*>(workspace + l.intervals);
    a.frames = frames; a.tables = tables; a.intervals = intervals;
    hipError_t e = hipMemcpyAsync(frames, frames_host, (size_t)B * sizeof(sd_jpeg_entropy_frame), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return e;
    // (the tables of every frame in one copy: an ineligible frame's slots are never read)
    e = hipMemcpyAsync(tables, tables_host, (size_t)B * sdjent::kTables * sizeof(sd_jpeg_huff_table), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return e;
    int most = 0;
    for (int b = 0; b < B; ++b)
        if (frames_host[b].eligible) most = frames_host[b].n_intervals > most ? frames_host[b].n_intervals : most;
    const bool any = most > 0;
    // the ranges of every frame in ONE strided copy: the first `most` entries of each frame's row (rows of ineligible frames and entries
    // behind a frame's own count are never read)
    if (any) {
        const size_t pitch = interval_stride * sizeof(sd_jpeg_interval);
        e = hipMemcpy2DAsync(intervals, pitch, intervals_host, pitch, (size_t)most * sizeof(sd_jpeg_interval), (size_t)B, hipMemcpyHostToDevice, s);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(jpeg_entropy_clear_kernel, dim3(kClearBlocks, (unsigned)B), dim3(kClearThreads), 0, s, a);
    if (any) hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)((most + kLanes - 1) / kLanes), (unsigned)B), dim3(kLanes), 0, s, a);
    return hipGetLastError();
}

}  // namespace sd
