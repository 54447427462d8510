// The workspace arena of a handle (sd_query_memory / sd_bind_memory): one walk, every region 256-byte aligned.  No HIP: capi.cpp and
// scripts/check_layouts.cpp read the same structs, whose member declarations are the walk (DESIGN.md "where scratch layouts live").
#pragma once
#include "tail_layout.hpp"

namespace sd {

constexpr int RSZ_MAX = 16384;        // largest destination extent of sd_resize_cubic_u8
constexpr int SAT_IMG_PAD = 512;      // per-image clamp slots past a pass's images: the rows of a partial last GEMM tile (< 512) past the last image

// the per-frame counters of the road and fence chains: CNT_SLOTS rows of i32 [max_batch]
enum CntSlot {
    CNT_SPARE_0,
    CNT_RW_ZCUT, CNT_RW_MAD_Y, CNT_RW_MAD_X, CNT_RW_PLANE, CNT_RW_SOR, CNT_RW_ROR,      // sd_road_width: the cloud after each stage
    CNT_SPARE_7,
    // sd_fence_to_fence, in the order of sd_f2f_result::counts: the fence cloud, after MAD(y), after the |z| threshold, left, right, left final, right final
    CNT_F2F_FENCE, CNT_F2F_MAD_Y, CNT_F2F_Z, CNT_F2F_LEFT, CNT_F2F_RIGHT, CNT_F2F_LEFT_FINAL, CNT_F2F_RIGHT_FINAL,
    CNT_SPARE_15, CNT_SPARE_16, CNT_SPARE_17, CNT_SPARE_18, CNT_SPARE_19, CNT_SPARE_20, CNT_SPARE_21, CNT_SPARE_22, CNT_SPARE_23,
    CNT_SLOTS
};
constexpr int CNT_F2F_ROWS = CNT_F2F_RIGHT_FINAL - CNT_F2F_FENCE + 1;      // the seven rows launch_f2f reads, packed to stride B
static_assert(CNT_SLOTS == 24 && CNT_F2F_ROWS == 7, "the counter region is 24 rows; sd_f2f_result has seven counts");

// the fp16 clamp counters (offsets inside the arena's `sat` region)
struct SatLayout : sdarena::Walker {
    size_t B, img_slots;      // img_slots: split_fmt.hpp sat_check, 2 images per frame at most + SAT_IMG_PAD
    explicit SatLayout(int max_batch) : B((size_t)max_batch), img_slots(2 * (size_t)max_batch + SAT_IMG_PAD) {}
    size_t count = take(sizeof(uint64_t), 8);                 // u64, 8-byte aligned: the global count (sd_saturation_count)
    size_t img = take(img_slots * sizeof(uint32_t), 4);       // u32 [img_slots], 4: per-image slots of one pass
    size_t frames = take(B * sizeof(uint32_t), 4);            // u32 [max_batch], 4: the per-frame counts (sd_saturation_frames)
    size_t orphans = take(sizeof(uint32_t), 4);               // u32, 4: the clamps no frame owns (zero-padded rows of a partial last GEMM tile; sd_saturation_settle)
    size_t total = end(256);
};

// the tap tables of one cubic resize geometry: i32 [RSZ_MAX][4] each, 16-byte aligned
struct RszLayout : sdarena::Walker {
    size_t xi = take((size_t)RSZ_MAX * 4 * sizeof(int), 16), xa = take((size_t)RSZ_MAX * 4 * sizeof(int), 16);      // x tap indices | x weights
    size_t yi = take((size_t)RSZ_MAX * 4 * sizeof(int), 16), ya = take((size_t)RSZ_MAX * 4 * sizeof(int), 16);      // y tap indices | y weights
    size_t total = end();
};

struct ArenaDims {
    int max_batch, H, W, cap;
    size_t fcn_act_bytes, mono_act_bytes;      // the plans' activation arenas (plan.cpp lays them out)
    size_t splitk_bytes;                       // sd_set_small_batch: the partial sums of the largest split layer (0 without the switch)
};
constexpr size_t kScalarSlotBytes = 256, kZeroPageBytes = 4096 - 256;
struct Arena : sdarena::Walker {
    ArenaDims d;
    size_t B, pts;
    O3dLayout views;      // (the Open3D region's own layout: its total, and the fence chain's views over it)
    explicit Arena(const ArenaDims& dims = {}) : d(dims), B((size_t)dims.max_batch), pts((size_t)dims.max_batch * dims.cap), views(dims.max_batch, dims.cap) {}
    size_t fcn = take(d.fcn_act_bytes, 256), mono = take(d.mono_act_bytes, 256);      // activations of the two networks
    size_t fuse = take(FuseLayout(d.max_batch, d.H, d.W).total, 256);
    size_t fuse1 = take(Fuse1Layout(d.max_batch, d.H, d.W).total, 256);
    size_t cams = take(sizeof(CamDev) * B, 256);                                      // CamDev [max_batch]
    size_t bufA = take(pts * 3 * sizeof(float), 256), bufB = take(pts * 3 * sizeof(float), 256);      // f32 [max_batch][cap][3]: the clouds ping-pong between them
    size_t rgbA = take(pts * 3, 256), rgbB = take(pts * 3, 256);      // u8 [max_batch][cap][3]: colours travel with the points through every filter (semantic_depth.py:206-245)
    size_t cnt = take(B * sizeof(int32_t) * CNT_SLOTS, 256);          // i32 [CNT_SLOTS][max_batch]
    size_t plane = take(B * sizeof(double) * 4, 256);                 // f64 [max_batch][4]: the road plane
    size_t o3d = take(views.total, 256);                              // O3dLayout
    size_t scalar = take(kScalarSlotBytes, 256);                      // i32 in a 256-byte slot: the count of a single-cloud call
    size_t zero = take(kZeroPageBytes, 256);                          // zero-filled by sd_bind_memory and never written: the kernels' zero16 source
    size_t f2f_counts = take(B * CNT_F2F_ROWS * sizeof(int32_t), 256);      // i32 [CNT_F2F_ROWS][B]: the fence chain's counts packed for launch_f2f
    size_t f2f_planes = take(B * 12 * sizeof(double), 256);           // f64 [3][B][4]: road | left | right
    size_t sat = take(SatLayout(d.max_batch).total, 256);
    size_t cmp = take(CmpLayout(d.max_batch).total, 256);
    size_t rsz = take(RszLayout().total, 256), rsz_cmp = take(RszLayout().total, 256);      // sd_resize_cubic_u8, and the same for sd_compose_result_frames
    size_t splitk = take(d.splitk_bytes, 256);                        // (last: the other offsets do not depend on the switch)
    size_t total = end(256);
    // cannot fail at any size in use: the views take 15 bytes per point and the Open3D region has 161 per point
    bool fence_views_fit = views.fence_views_end <= views.total;
};

}  // namespace sd
