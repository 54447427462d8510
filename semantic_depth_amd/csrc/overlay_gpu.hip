// Device half of the measurement lines of the result images (sd_overlay_draw): the road and fence records of B frames and, with a depth
// profile, their end points at D depths, all in device memory -> line segments painted in place into the composed images (contract:
// include/semdepth.h; projection, slots and boxes: overlay_rule.hpp, paint rule: text_draw.hpp's hit(), all of which the host functions of
// host_overlay.cpp run too, so both paint the same pixels).  Two launches, no host synchronisation, no atomics:
//   overlay_setup_kernel    one workgroup of 256 lanes per frame: lane i projects the four end points of profile entry i into LDS; behind a
//                           barrier lane i writes its four fixed slots (left edge i -> i + 1, right edge, road rung, fence rung): the
//                           segment, whether it paints, and its pixel box widened by the radius and clipped to [clip_top, h) x [0, w).  The
//                           lanes' flags and boxes are folded per wave (64-bit ballot, shuffles), then lane 0 writes the record's two
//                           lines, the frame's flag and the union box of the frame's slots.
//   overlay_raster_kernel   grid = (64 x 16 pixel tiles of the image, frames); a tile outside the frame's union box exits at once.  The
//                           others walk the slots in chunks of 256, from the LAST chunk to the first: the lanes whose slot paints and whose
//                           box meets the tile are counted by ballot, a prefix over the four waves gives each kept slot its place in LDS,
//                           in slot order; every lane tests its four pixels from the last kept slot to the first and stops at the first
//                           hit -- the highest slot that covers the pixel -- storing its three bytes.  Only painted pixels are stored.
#include "overlay_gpu.hpp"

#include <climits>

namespace sd {
namespace {

using namespace sdoverlay;

constexpr int kThreads = 256, kWaves = kThreads / 64;
static_assert(kMaxDepths <= kThreads, "one lane per profile entry");

struct Kept {
    sdtext::Seg seg;
    int32_t box[4];
    int32_t r;
    uint8_t bgr[3], pad;
};

__device__ inline void fold_box(int32_t* u, const int32_t* b) {
    u[0] = min(u[0], b[0]);
    u[1] = min(u[1], b[1]);
    u[2] = max(u[2], b[2]);
    u[3] = max(u[3], b[3]);
}
// writes every byte of the slot; folds its box into u when it paints; returns whether it flags the frame
__device__ inline bool put_slot(OverlaySlot& out, int32_t state, const sd_overlay_segment& seg, int h, int w, int clip_top, int32_t* u) {
    OverlaySlot s{};
    if (state == kOk) {
        s.seg = seg;
        s.valid = seg_box(seg, h, w, clip_top, s.box) ? 1 : 0;
        if (s.valid) fold_box(u, s.box);
    }
    out = s;
    return state == kDropped;
}

__global__ __launch_bounds__(kThreads) void overlay_setup_kernel(OverlayArgs a) {
    __shared__ EntryPts pts[kThreads + 1];
    __shared__ int32_t wave_box[kWaves][4];
    __shared__ int32_t wave_flag[kWaves];
    const int b = (int)blockIdx.x, i = (int)threadIdx.x, D = a.D;
    const OverlayCamDev cam = a.cams[b];
    const View v = make_view(cam.cx, cam.cy, cam.f, a.net_h, a.net_w, a.h, a.w);
    EntryPts e{absent(), absent(), absent(), absent()};
    if (i < D) e = entry_points(v, a.rw_profile + (size_t)b * D + i, a.f2f_profile ? a.f2f_profile + (size_t)b * D + i : nullptr);
    pts[i] = e;
    if (i == 0) pts[kThreads] = EntryPts{absent(), absent(), absent(), absent()};
    __syncthreads();
    OverlaySlot* slots = a.slots + (size_t)b * slots_of(D);
    int32_t u[4] = {INT_MAX, INT_MAX, INT_MIN, INT_MIN};
    bool flag = false;
    if (i < D) {
        const EntryPts next = i + 1 < D ? pts[i + 1] : pts[kThreads];
        sd_overlay_segment seg{};
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int32_t state = entry_slot(g, e, next, a.style, &seg);
            flag |= put_slot(slots[g * D + i], state, seg, a.h, a.w, a.style.clip_top, u);
        }
    }
    // fold the lanes of each wave, then the waves
    const unsigned long long m = __ballot(flag);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        u[0] = min(u[0], __shfl_xor(u[0], off, 64));
        u[1] = min(u[1], __shfl_xor(u[1], off, 64));
        u[2] = max(u[2], __shfl_xor(u[2], off, 64));
        u[3] = max(u[3], __shfl_xor(u[3], off, 64));
    }
    if ((i & 63) == 0) {
        wave_flag[i >> 6] = m != 0ull ? 1 : 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) wave_box[i >> 6][k] = u[k];
    }
    __syncthreads();
    if (i != 0) return;
    int32_t f = 0;
#pragma unroll
    for (int wv = 0; wv < kWaves; ++wv) {
        f |= wave_flag[wv];
        fold_box(u, wave_box[wv]);
    }
    sd_overlay_segment seg{};
    int32_t state = record_slot(v, a.records[b], a.style, &seg);
    f |= put_slot(slots[4 * D], state, seg, a.h, a.w, a.style.clip_top, u) ? 1 : 0;
    state = fence_slot(v, a.f2f ? a.f2f + b : nullptr, a.style, &seg);
    f |= put_slot(slots[4 * D + 1], state, seg, a.h, a.w, a.style.clip_top, u) ? 1 : 0;
    a.flags[b] = f;
#pragma unroll
    for (int k = 0; k < 4; ++k) a.heads[b].box[k] = u[k];
}

__global__ __launch_bounds__(kThreads) void overlay_raster_kernel(OverlayArgs a) {
    __shared__ Kept kept[kThreads];
    __shared__ int wave_count[kWaves];
    const int b = (int)blockIdx.y;
    const int tx = (int)blockIdx.x % a.tiles_x, ty = (int)blockIdx.x / a.tiles_x;
    const int X0 = tx * kOverlayTileW, Y0 = ty * kOverlayTileH;
    const int X1 = min(X0 + kOverlayTileW - 1, a.w - 1), Y1 = min(Y0 + kOverlayTileH - 1, a.h - 1);
    const int32_t* ub = a.heads[b].box;
    if (ub[0] > X1 || ub[2] < X0 || ub[1] > Y1 || ub[3] < Y0) return;      // (an empty union box fails here too)
    const int nslots = slots_of(a.D);
    const OverlaySlot* slots = a.slots + (size_t)b * nslots;
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    const int px = X0 + lane, py0 = Y0 + wave;
    unsigned open = 0;      // the lane's pixels that are inside the frame and not painted yet
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (px <= X1 && py0 + 4 * k <= Y1) open |= 1u << k;

    for (int c0 = (nslots - 1) / kThreads * kThreads; c0 >= 0; c0 -= kThreads) {
        const int s = c0 + t;
        bool keep = false;
        if (s < nslots) {
            const OverlaySlot& g = slots[s];
            keep = g.valid != 0 && g.box[0] <= X1 && g.box[2] >= X0 && g.box[1] <= Y1 && g.box[3] >= Y0;
        }
        const unsigned long long m = __ballot(keep);
        if (lane == 0) wave_count[wave] = __popcll(m);
        __syncthreads();
        int base = 0, total = 0;
#pragma unroll
        for (int wv = 0; wv < kWaves; ++wv) {
            const int c = wave_count[wv];
            base += wv < wave ? c : 0;
            total += c;
        }
        if (keep) {
            const OverlaySlot& g = slots[s];
            Kept& kp = kept[base + __popcll(m & ((1ull << lane) - 1ull))];
            kp.seg = seg_of(g.seg);
#pragma unroll
            for (int k = 0; k < 4; ++k) kp.box[k] = g.box[k];
            kp.r = (int32_t)g.seg.thickness * 128;
            kp.bgr[0] = g.seg.bgr[0];
            kp.bgr[1] = g.seg.bgr[1];
            kp.bgr[2] = g.seg.bgr[2];
            kp.pad = 0;
        }
        __syncthreads();
        for (int j = total - 1; j >= 0 && open != 0u; --j) {
            const Kept& kp = kept[j];
            if (px < kp.box[0] || px > kp.box[2]) continue;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int py = py0 + 4 * k;
                // inside the slot's box a pixel is inside the frame and at or below clip_top
                if ((open >> k & 1u) && py >= kp.box[1] && py <= kp.box[3] && sdtext::hit(kp.seg, px, py, kp.r)) {
                    uint8_t* d = a.dst + (((size_t)b * a.h + py) * a.w + px) * 3;
                    d[0] = kp.bgr[0];
                    d[1] = kp.bgr[1];
                    d[2] = kp.bgr[2];
                    open &= ~(1u << k);
                }
            }
        }
        __syncthreads();      // the next chunk overwrites kept and wave_count
    }
}

}  // namespace

void overlay_layout(OverlayArgs& a, uint8_t* workspace) {
    const sdoverlay::Layout l(a.B, a.D);
    a.cams = reinterpret_cast<OverlayCamDev*>(workspace + l.cams);
    a.heads = reinterpret_cast<OverlayFrameHead*>(workspace + l.heads);
    a.slots = reinterpret_cast<OverlaySlot*>(workspace + l.slots);
}

hipError_t launch_overlay_draw(OverlayArgs a, hipStream_t s) {
    a.tiles_x = (a.w + kOverlayTileW - 1) / kOverlayTileW;
    const int tiles_y = (a.h + kOverlayTileH - 1) / kOverlayTileH;
    hipLaunchKernelGGL(overlay_setup_kernel, dim3((unsigned)a.B), dim3(kThreads), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(overlay_raster_kernel, dim3((unsigned)(a.tiles_x * tiles_y), (unsigned)a.B), dim3(kThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace sd
