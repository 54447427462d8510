// Scratch layouts of the fusion and road-width kernels (fuse.hip, pcl.hip), with the sizes and records they are made of.  No HIP: the
// kernels, capi.cpp and scripts/check_layouts.cpp read the same structs, whose member declarations are the walk (DESIGN.md "where
// scratch layouts live").
#pragma once
#include <cstddef>
#include <cstdint>

#include "arena.hpp"

namespace sd {

// ---------------------------------------------------------------------------------------------- fuse.hip
struct CamDev { double q[16]; float mult; };   // Q rounded to f32 then widened; multiplier as f32

// three-launch forms: per-block kept counts and their exclusive scan, 256 pixels per block (the 4-pixel forms use fewer blocks of the same buffers)
struct FuseLayout : sdarena::Walker {
    size_t blk;      // bytes of one [B][nblk][2] array
    FuseLayout(int B, int H, int W) : blk((size_t)B * (((size_t)H * W + 255) / 256) * 2 * sizeof(int32_t)) {}
    size_t blk_counts = take(blk, 4);      // i32 [B][nblk][2], 4-byte aligned
    size_t blk_offsets = take(blk, 4);     // i32 [B][nblk][2], 4
    size_t total = end();
};

#ifndef SD_F1_SUB
#define SD_F1_SUB 8
#endif
constexpr int F1_SUB = SD_F1_SUB;               // sub-tiles of 1024 pixels (256 threads x 4 pixels) per block
constexpr int F1_PIX = 1024 * F1_SUB;           // pixels per block: one ticket, one look-back, one published word
// one-pass form (fuse_onepass_kernel)
struct Fuse1Layout : sdarena::Walker {
    size_t B, nblk;
    Fuse1Layout(int B_, int H, int W) : B((size_t)B_), nblk(((size_t)H * W + F1_PIX - 1) / F1_PIX) {}
    size_t state = take(B * nblk * 8, 8);      // u64 [B][nblk], 8-byte aligned: look-back words (epoch | flag | road count | fence count)
    size_t ticket = take(B * 4, 4);            // i32 [B], 4: arrival tickets (zero between launches)
    size_t slack = end();                      // 256 bytes of historical slack: zeroed with the rest, otherwise untouched
    size_t total = end_with_slack(256);
};

// camera sweep (fuse_sweep_write_kernel): the caller's workspace; every byte read is written by the same call
struct SweepLayout : sdarena::Walker {
    size_t ncam, blk;
    SweepLayout(int B, int T, int H, int W) : ncam((size_t)T * B), blk((size_t)B * (((size_t)H * W + 255) / 256) * 2 * sizeof(int32_t)) {}
    size_t cams = take(ncam * sizeof(CamDev), 16);      // CamDev [T][B], 16-byte aligned: the caller's upload
    size_t blk_counts = take(blk, 16);                  // i32 [B][nblk][2], 16
    size_t blk_offsets = take(blk, 16);                 // i32 [B][nblk][2], 16
    size_t total = end(16);
};

// ---------------------------------------------------------------------------------------------- pcl.hip: multi-block compaction
constexpr int CMP_MED_KEYS = 16384, CMP_SLICES = 64;      // pcl.hip's MED_CAP and CMP_G (declared there, held equal by a static_assert)
constexpr int CMP_PARAMS = 8;        // doubles per frame: MAD {median, mad}; plane {C0, C1, C2}; statistical filter {threshold}
struct MedG { unsigned klo, khi, cnt, below, nan, done; float med, madv; };      // per-frame state of a multi-block median
struct CmpLayout : sdarena::Walker {
    size_t B;
    explicit CmpLayout(int B_) : B((size_t)B_) {}
    size_t params = take(B * CMP_PARAMS * sizeof(double), 256);      // f64 [B][CMP_PARAMS], 256-byte aligned
    size_t blk_cnt = take(B * CMP_SLICES * sizeof(int), 256);        // i32 [B][CMP_G], 256
    size_t med = take(B * sizeof(MedG), 256);                        // MedG [B], 256
    size_t medbuf = take(B * CMP_MED_KEYS * sizeof(unsigned), 256);  // u32 [B][MED_CAP], 256
    size_t slack = end();      // historical slack: 1024 bytes were added to the unpadded sizes, the padding above comes out of them
    size_t total = end_with_slack(1024);
};

// ---------------------------------------------------------------------------------------------- pcl.hip: Open3D filters
constexpr int GRID_CELLS = 1 << 19;
constexpr int KMAX = 16;
constexpr int SCAN_SEG = 2048;     // cells per scan segment
constexpr int SCAN_NSEG = GRID_CELLS / SCAN_SEG;
struct GridMeta { double ox, oy, oz, inv; double cell; int gx, gy, gz, occupied; double ext[3], mn[3], mxz; int nonfinite, pad_; };
struct O3dLayout : sdarena::Walker {      // every region 256-byte aligned, per-frame strides
    size_t B, pts;
    O3dLayout(int B_, int cap) : B((size_t)B_), pts((size_t)B_ * cap) {}
    size_t meta = take(sizeof(GridMeta) * B, 256);
    size_t mean_d = take(pts * 8, 256);                          // f64 [B][cap]  (by original index)
    size_t cell_cnt = take(B * GRID_CELLS * 4 + B * 32, 256);    // i32 [B][GRID_CELLS]: counts, then scatter cursors; behind them i32 [B][8] bounding-box accumulators
    size_t cell_start = take(B * (GRID_CELLS + 1) * 4, 256);     // i32 [B][GRID_CELLS + 1]
    size_t seg_sum = take(B * SCAN_NSEG * 4, 256);               // i32 [B][SCAN_NSEG]
    size_t cell_of = take(pts * 4, 256);                         // i32 [B][cap]
    size_t sidx = take(pts * 4, 256);                            // i32 [B][cap]: original index of the j-th sorted point
    size_t sxyz = take(pts * 16, 256);                           // f32 [B][cap][4]: the cell-sorted copy, one 16-byte load per candidate (w unused)
    size_t keep = take(pts, 256);                                // u8 [B][cap]
    size_t hard_n = take(B * 4, 256);                            // i32 [B]: statistical filter: queries deferred to the wave-cooperative search (list in cell_of)
    size_t hard_best = take(pts * KMAX * 8, 256);                // f64 [B][cap][KMAX]: their k best distances after the per-thread shells (ascending, inf padded)
    size_t slack = end();      // historical slack: 8192 + 256 bytes were added to the unpadded sizes, the padding above comes out of them
    size_t total = end_with_slack(8192 + 256);
    // views of the fence chain (sd_fence_to_fence), which runs while the Open3D filters are idle: its left cloud and the colours of it.
    // They overlap the regions above on purpose and must end inside `total` (the handle's arena checks it when it is built)
    sdarena::Walker views;
    size_t fence_left_xyz = views.take(pts * 3 * sizeof(float), 256);      // f32 [B][cap][3], 256
    size_t fence_left_rgb = views.take(pts * 3, 256);                      // u8 [B][cap][3], 256
    size_t fence_views_end = views.end();
};

}  // namespace sd
