// JPEG entropy decoding on the device in self-synchronising pieces (sd_jpeg_sync_decode): the passes of jpeg_sync.hpp, a lane per piece
// of subseq_bytes of the clean stream the host staged.  A workgroup serves kGroup = 256 consecutive pieces of ONE frame, so the frame's
// record and the Huffman tables its scan names are staged once into LDS (1488 bytes per table, 11.6 KB when all eight are named) and a
// workgroup's stream bytes are one contiguous run, fetched by each lane as aligned 8-byte words.
//   jpeg_sync_clear_kernel   zeroes the eligible frames' coefficients and every status word
//   jpeg_sync_spec_kernel    the speculative pass: round 0, then at most 255 rounds that end as soon as no lane of the workgroup walks on;
//                            the workgroup's records live in LDS until the rounds are over
//   jpeg_sync_across_kernel  a lane per workgroup g >= 1, started from the end record workgroup g - 1 had after the speculative pass
//                            (a copy of its own, which this kernel only reads)
//   jpeg_sync_place_kernel   exclusive scan of the unit counts, one workgroup per frame
//   jpeg_sync_write_kernel   decodes every piece from its predecessor's record, stores the coefficients and verifies the chain
//   jpeg_sync_dc_kernel      segmented inclusive scan of the DC differences, one workgroup per (frame, component)
// No kernel waits for another workgroup and none uses atomics; every loop is bounded by a count the host checked.  The status words are
// written by ordinary stores of a non-zero code (any flagging lane's: the word only has to be non-zero).  Lanes of a wave diverge, each
// following its own code lengths, as in jpeg_entropy_gpu.hip.
#include "jpeg_sync_gpu.hpp"

namespace sd {
namespace {

using namespace sdjsync;

constexpr int kClearThreads = 256, kClearBlocks = 32;
constexpr int kAcrossLanes = 64;
constexpr int kScanThreads = 1024;

struct SyncArgs {
    const uint8_t* bytes;
    size_t byte_stride;
    const sd_jpeg_sync_frame* frames;
    const sd_jpeg_huff_table* tables;
    const sd_jpeg_sync_interval* intervals;
    size_t interval_stride;
    Rec* rec;                     // [B][piece_stride]
    Rec* group_end;               // [B][piece_stride / kGroup]
    uint32_t* before;             // [B][piece_stride]: units of the frame's pieces before this one
    size_t piece_stride;
    uint32_t S;
    int16_t* coef;
    size_t coef_stride;           // int16 elements
    int32_t* status;
};

// int16 elements of the frame's coefficients, from the record alone (frame_ok() has tied it to the descriptor's count)
__device__ inline size_t record_coef_elems(const sd_jpeg_sync_frame& fr) {
    size_t n = 0;
    for (int c = 0; c < fr.ncomp; ++c) n += (size_t)fr.mcus_x * fr.comp_h[c] * fr.mcus_y * fr.comp_v[c] * 64;
    return n;
}

// the frame's record and the tables its scan names -> LDS, by all `threads` lanes of the workgroup; the caller synchronises
__device__ inline void stage(const SyncArgs& a, uint32_t b, sd_jpeg_sync_frame* fr, sd_jpeg_huff_table* tabs, int t, int threads) {
    const sd_jpeg_sync_frame& g = a.frames[b];
    constexpr int kFrameWords = sizeof(sd_jpeg_sync_frame) / 4, kTableWords = sizeof(sd_jpeg_huff_table) / 4;
    for (int i = t; i < kFrameWords; i += threads) reinterpret_cast<uint32_t*>(fr)[i] = reinterpret_cast<const uint32_t*>(&g)[i];
    uint32_t named = 0;                                        // comp_dc / comp_ac are 0..3 (frame_ok()): bits 0..7
    for (int c = 0; c < g.ncomp; ++c) named |= (1u << g.comp_dc[c]) | (16u << g.comp_ac[c]);
    for (int slot = 0; slot < kTables; ++slot) {
        if (!(named >> slot & 1)) continue;
        const uint32_t* src = reinterpret_cast<const uint32_t*>(a.tables + (size_t)b * kTables + slot);
        uint32_t* dst = reinterpret_cast<uint32_t*>(&tabs[slot]);
        for (int i = t; i < kTableWords; i += threads) dst[i] = src[i];
    }
}
static_assert(sizeof(sd_jpeg_sync_frame) % 4 == 0 && sizeof(sd_jpeg_huff_table) % 4 == 0 && sizeof(Rec) == 16, "the staging loops copy dwords");

__global__ __launch_bounds__(kClearThreads) void jpeg_sync_clear_kernel(SyncArgs a) {
    const uint32_t b = blockIdx.y;
    if (blockIdx.x == 0 && threadIdx.x == 0) a.status[b] = 0;
    const sd_jpeg_sync_frame& fr = a.frames[b];
    if (!fr.eligible) return;
    // 16-byte stores: the frame's slot begins at a multiple of 16 bytes and its element count is a multiple of 64
    const size_t n16 = record_coef_elems(fr) / 8;
    uint4* dst = reinterpret_cast<uint4*>(a.coef + (size_t)b * a.coef_stride);
    for (size_t i = (size_t)blockIdx.x * kClearThreads + threadIdx.x; i < n16; i += (size_t)kClearBlocks * kClearThreads)
        dst[i] = make_uint4(0, 0, 0, 0);                       // i < n16: inside the frame's coefficients
}

__global__ __launch_bounds__(kGroup) void jpeg_sync_spec_kernel(SyncArgs a) {
    __shared__ sd_jpeg_huff_table tabs[kTables];
    __shared__ sd_jpeg_sync_frame fr;
    __shared__ Rec rec[kGroup];
    const int t = threadIdx.x;
    const uint32_t b = blockIdx.y, base = blockIdx.x * (uint32_t)kGroup;
    const sd_jpeg_sync_frame& g = a.frames[b];
    if (!g.eligible || base >= g.n_pieces) return;             // (uniform over the workgroup)
    stage(a, b, &fr, tabs, t, kGroup);
    __syncthreads();
    const uint32_t P = fr.n_pieces, i = base + t;
    const uint32_t group_last = base + kGroup - 1 < P - 1 ? base + kGroup - 1 : P - 1;
    const uint8_t* bytes = a.bytes + (size_t)b * a.byte_stride;
    const sd_jpeg_sync_interval* ivs = a.intervals + (size_t)b * a.interval_stride;
    State s{0, 0, 0};
    sd_jpeg_sync_interval v{0, 0, 0, 0};
    uint32_t last = 0;
    bool active = false;
    if (i < P) {                                               // i < n_pieces <= piece_stride
        const Piece pc = locate(ivs, fr.n_intervals, P, i, a.S);
        rec[t] = spec_first(bytes, fr, tabs, pc, s);
        v = ivs[pc.iv];                                        // pc.iv < n_intervals <= interval_stride
        last = pc.iv_last < group_last ? pc.iv_last : group_last;
        active = i < last;
    }
    // a round: lane t on piece i + r <= last <= group_last, so t + r < kGroup; each piece has one lane per round, and the barrier of
    // __syncthreads_or orders a round's record stores before the next round's loads
    for (int r = 1; r < kGroup; ++r) {
        if (!__syncthreads_or(active)) break;
        if (active) {
            bool stop;
            rec[t + r] = walk_on(bytes, fr, tabs, v, i + r, a.S, s, rec[t + r], &stop);
            if (stop || i + r >= last) active = false;
        }
    }
    __syncthreads();
    if (i < P) {
        a.rec[(size_t)b * a.piece_stride + i] = rec[t];
        if (i == group_last) a.group_end[(size_t)b * (a.piece_stride / kGroup) + blockIdx.x] = rec[t];
    }
}

__global__ __launch_bounds__(kAcrossLanes) void jpeg_sync_across_kernel(SyncArgs a) {
    __shared__ sd_jpeg_huff_table tabs[kTables];
    __shared__ sd_jpeg_sync_frame fr;
    const int t = threadIdx.x;
    const uint32_t b = blockIdx.y;
    const sd_jpeg_sync_frame& gf = a.frames[b];
    const uint32_t g = 1 + blockIdx.x * (uint32_t)kAcrossLanes + t;
    if (!gf.eligible || (uint64_t)(1 + blockIdx.x * (uint32_t)kAcrossLanes) * kGroup >= gf.n_pieces) return;      // (uniform)
    stage(a, b, &fr, tabs, t, kAcrossLanes);
    __syncthreads();
    const uint32_t P = fr.n_pieces, first = g * (uint32_t)kGroup;
    if (first >= P) return;
    const uint8_t* bytes = a.bytes + (size_t)b * a.byte_stride;
    const sd_jpeg_sync_interval* ivs = a.intervals + (size_t)b * a.interval_stride;
    const Piece pc = locate(ivs, fr.n_intervals, P, first, a.S);
    if (pc.iv_first == first) return;                          // an interval begins here: the speculative start was the true one
    const sd_jpeg_sync_interval v = ivs[pc.iv];
    const uint32_t group_last = first + kGroup - 1 < P - 1 ? first + kGroup - 1 : P - 1, last = pc.iv_last < group_last ? pc.iv_last : group_last;
    Rec* rec = a.rec + (size_t)b * a.piece_stride;
    State s = unpack(a.group_end[(size_t)b * (a.piece_stride / kGroup) + g - 1]);      // g - 1 < the frame's workgroups
    for (uint32_t j = first; j <= last; ++j) {                 // j < P: this workgroup's pieces, which no other lane of this kernel touches
        bool stop;
        rec[j] = walk_on(bytes, fr, tabs, v, j, a.S, s, rec[j], &stop);
        if (stop) break;
    }
}

// inclusive scan of x over the workgroup's kScanThreads lanes through `buf`
__device__ inline uint32_t block_scan(uint32_t x, uint32_t* buf, int t) {
    buf[t] = x;
    __syncthreads();
    for (int d = 1; d < kScanThreads; d <<= 1) {
        const uint32_t y = t >= d ? buf[t - d] : 0u;
        __syncthreads();
        buf[t] += y;
        __syncthreads();
    }
    return buf[t];
}

__global__ __launch_bounds__(kScanThreads) void jpeg_sync_place_kernel(SyncArgs a) {
    __shared__ uint32_t buf[kScanThreads];
    const int t = threadIdx.x;
    const uint32_t b = blockIdx.x;
    const sd_jpeg_sync_frame& fr = a.frames[b];
    if (!fr.eligible) return;
    const uint32_t P = fr.n_pieces;
    const Rec* rec = a.rec + (size_t)b * a.piece_stride;
    uint32_t* before = a.before + (size_t)b * a.piece_stride;
    uint32_t carry = 0;                                        // (a frame holds fewer than 2^30 units: kMaxBytes)
    for (uint32_t base = 0; base < P; base += kScanThreads) {
        const uint32_t i = base + t, n = i < P ? rec[i].n : 0u;
        const uint32_t incl = block_scan(n, buf, t);
        if (i < P) before[i] = carry + incl - n;
        carry += buf[kScanThreads - 1];
        __syncthreads();
    }
}

__global__ __launch_bounds__(kGroup) void jpeg_sync_write_kernel(SyncArgs a) {
    __shared__ sd_jpeg_huff_table tabs[kTables];
    __shared__ sd_jpeg_sync_frame fr;
    const int t = threadIdx.x;
    const uint32_t b = blockIdx.y, base = blockIdx.x * (uint32_t)kGroup;
    const sd_jpeg_sync_frame& g = a.frames[b];
    if (!g.eligible || base >= g.n_pieces) return;             // (uniform over the workgroup)
    stage(a, b, &fr, tabs, t, kGroup);
    __syncthreads();
    const uint32_t P = fr.n_pieces, i = base + t;
    if (i >= P) return;
    const uint8_t* bytes = a.bytes + (size_t)b * a.byte_stride;
    const sd_jpeg_sync_interval* ivs = a.intervals + (size_t)b * a.interval_stride;
    const Rec* rec = a.rec + (size_t)b * a.piece_stride;
    const uint32_t* before = a.before + (size_t)b * a.piece_stride;
    const Piece pc = locate(ivs, fr.n_intervals, P, i, a.S);
    const State start = pc.iv_first == i ? State{pc.begin_bit, 0, 0} : unpack(rec[i - 1]);        // i - 1 >= iv_first >= 0
    const int r = write_piece(bytes, fr, tabs, pc, i, start, (int64_t)(before[i] - before[pc.iv_first]), rec[i], a.coef + (size_t)b * a.coef_stride);
    if (r) a.status[b] = r;
}

__global__ __launch_bounds__(kScanThreads) void jpeg_sync_dc_kernel(SyncArgs a) {
    __shared__ long long val[kScanThreads];
    __shared__ uint8_t flag[kScanThreads];
    __shared__ sd_jpeg_sync_frame fr;
    const int t = threadIdx.x, c = blockIdx.x;
    const uint32_t b = blockIdx.y;
    const sd_jpeg_sync_frame& g = a.frames[b];
    if (!g.eligible || c >= g.ncomp) return;                   // (uniform over the workgroup)
    for (int i = t; i < (int)(sizeof(fr) / 4); i += kScanThreads) reinterpret_cast<uint32_t*>(&fr)[i] = reinterpret_cast<const uint32_t*>(&g)[i];
    __syncthreads();
    int16_t* coef = a.coef + (size_t)b * a.coef_stride;
    const int64_t n = dc_blocks(fr, c);
    long long carry = 0;
    bool bad = false;
    for (int64_t base = 0; base < n; base += kScanThreads) {
        const int64_t j = base + t;
        bool head = false;
        int16_t* blk = nullptr;
        long long x = 0;
        if (j < n) {                                           // j < the component's blocks: dc_block() is a block of the frame
            blk = coef + dc_block(fr, c, j, &head);
            x = blk[0];
        }
        if (t == 0 && !head) x += carry;                       // the segment that crosses into this chunk
        val[t] = x;
        flag[t] = head;
        __syncthreads();
        for (int d = 1; d < kScanThreads; d <<= 1) {           // segmented: a lane whose run already holds a head takes nothing more
            const bool take = t >= d && !flag[t];
            const long long y = take ? val[t - d] : 0;
            const uint8_t f = take ? flag[t - d] : 0;
            __syncthreads();
            if (take) { val[t] += y; flag[t] = f; }
            __syncthreads();
        }
        const long long pred = val[t];
        if (j < n) {
            if (pred < -32767 || pred > 32767) bad = true;
            blk[0] = (int16_t)pred;
        }
        carry = val[kScanThreads - 1];
        __syncthreads();
    }
    if (bad) a.status[b] = sdjent::kBadPredictor;
}

}  // namespace

hipError_t launch_jpeg_sync_decode(const uint8_t* bytes, size_t byte_stride, const sd_jpeg_sync_frame* frames_host, const sd_jpeg_sync_interval* intervals_host,
                                   size_t interval_stride, const sd_jpeg_huff_table* tables_host, int B, int subseq_bytes, size_t max_pieces, int16_t* coef,
                                   size_t coef_stride_elems, int32_t* status, uint8_t* workspace, hipStream_t s) {
    SyncArgs a{};
    const size_t P = sdjsync::piece_stride(max_pieces);
    a.bytes = bytes; a.byte_stride = byte_stride; a.interval_stride = interval_stride; a.coef = coef; a.coef_stride = coef_stride_elems; a.status = status;
    a.piece_stride = P; a.S = (uint32_t)subseq_bytes;
    const sdjsync::Layout l(B, interval_stride, max_pieces);
    sd_jpeg_sync_frame* frames = reinterpret_cast<sd_jpeg_sync_frame*>(workspace + l.frames);
    sd_jpeg_huff_table* tables = reinterpret_cast<sd_jpeg_huff_table*>(workspace + l.tables);
    sd_jpeg_sync_interval* intervals = reinterpret_cast<sd_jpeg_sync_interval*>(workspace + l.intervals);
    a.rec = reinterpret_cast<Rec*>(workspace + l.rec);
    a.group_end = reinterpret_cast<Rec*>(workspace + l.group_end);
    a.before = reinterpret_cast<uint32_t*>(workspace + l.before);
    a.frames = frames; a.tables = tables; a.intervals = intervals;
    hipError_t e = hipMemcpyAsync(frames, frames_host, (size_t)B * sizeof(sd_jpeg_sync_frame), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return e;
    e = hipMemcpyAsync(tables, tables_host, (size_t)B * kTables * sizeof(sd_jpeg_huff_table), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return e;
    int most = 0;
    for (int b = 0; b < B; ++b)
        if (frames_host[b].eligible) most = frames_host[b].n_intervals > most ? frames_host[b].n_intervals : most;
    const bool any = most > 0;
    if (any) {                                                 // the first `most` ranges of every frame's row in one strided copy
        const size_t pitch = interval_stride * sizeof(sd_jpeg_sync_interval);
        e = hipMemcpy2DAsync(intervals, pitch, intervals_host, pitch, (size_t)most * sizeof(sd_jpeg_sync_interval), (size_t)B, hipMemcpyHostToDevice, s);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(jpeg_sync_clear_kernel, dim3(kClearBlocks, (unsigned)B), dim3(kClearThreads), 0, s, a);
    if (any) {
        const unsigned groups = (unsigned)(P / kGroup);
        hipLaunchKernelGGL(jpeg_sync_spec_kernel, dim3(groups, (unsigned)B), dim3(kGroup), 0, s, a);
        if (groups > 1) hipLaunchKernelGGL(jpeg_sync_across_kernel, dim3((groups - 1 + kAcrossLanes - 1) / kAcrossLanes, (unsigned)B), dim3(kAcrossLanes), 0, s, a);
        hipLaunchKernelGGL(jpeg_sync_place_kernel, dim3((unsigned)B), dim3(kScanThreads), 0, s, a);
        hipLaunchKernelGGL(jpeg_sync_write_kernel, dim3(groups, (unsigned)B), dim3(kGroup), 0, s, a);
        hipLaunchKernelGGL(jpeg_sync_dc_kernel, dim3(3, (unsigned)B), dim3(kScanThreads), 0, s, a);
    }
    return hipGetLastError();
}

}  // namespace sd
