// LDS-DMA conv pipeline of the split engine: variant choice and dispatch.  The kernel template lives in conv_dma_kernel.hpp; each block shape
// is instantiated in its own translation unit (conv_dma_v*.hip: twelve kernels each -- three gather modes x four precisions), so that a clean
// build compiles them side by side instead of sixty kernels in one three-minute hipcc run.
#include "conv_dma_kernel.hpp"

namespace sd {

void launch_dma_v1(const ConvParams& p, long M, hipStream_t s);      // 128 x 256
void launch_dma_v2(const ConvParams& p, long M, hipStream_t s);      // 256 x 128
void launch_dma_v3(const ConvParams& p, long M, hipStream_t s);      // 256 x 64
void launch_dma_v4(const ConvParams& p, long M, hipStream_t s);      // 256 x 32
void launch_dma_v5(const ConvParams& p, long M, hipStream_t s);      // 256 x 256

// the block shape 1..5 of a layer (0: not applicable).  Called by resolve_conv_form only; reads no pointer and nothing of the call
int conv_dma_variant(const ConvParams& p) {
    if (!p.vec || p.Cout % 32 || p.Kpad < 64) return 0;
    // the block shape is chosen on a FULL pass of the engine (ConvParams::Nmax), not on the frames of this call: a call with fewer frames runs the same
    // kernels on fewer tiles, so a frame's result cannot depend on the call it is computed in even where two block shapes round differently (ADVICE r5 #3;
    // conv_dma3_eligible has counted this way since round 5)
    const long M = (long)(p.Nmax > 0 ? p.Nmax : p.N) * p.Hout * p.Wout;
    const long thr = (p.pool || p.out_planar16 || p.fold) ? 0 : 96;     // (a folded layer runs here whatever the batch: its results must not depend on it) tiles needed: the DMA pipeline at half occupancy still beats the register-staged
                                          // kernel (a fused pool exists only here: such layers always take this kernel)
    const bool big = !(p.sw & SW_NO_DMA_BIG);
    // 256 x 256 (one workgroup per CU): 128 flop per byte of L2 -> LDS DMA, the resource the long-K GEMMs run against.  The one-product
    // form of 128 x 256 / 256 x 128 fits TWO workgroups per CU (72 KB of ring, 124 VGPRs): one's epilogue and pipeline fill run under
    // the other's k-loop, which wins below ~32 k-tiles (measured: K <= 640 +5..14 %, K = 768..1280 equal, K >= 1536 and fc6 -2..4 %)
    const bool x3 = p.scheme == SC_BF16X3, shortk = p.scheme == SC_F16X1 && p.Kpad < 1024;
    if (x3 && (p.pool || p.out_planar16)) return 0;           // (bf16 x 3: plain outputs only)
    if (p.fold && x3) return 0;                               // (folded GEMMs of bf16 x 3: conv_dma3.hip)
    if (big && !x3 && !shortk && !p.pool && p.Cout % 256 == 0 && ((M + 255) / 256) * (p.Cout / 256) * (p.fold ? 4 : 1) >= 512) return 5;
    if (p.Cout % 256 == 0 && ((M + 127) / 128) * (p.Cout / 256) >= thr) return 1;     // 128 x 256
    if (p.Cout % 128 == 0 && ((M + 255) / 256) * (p.Cout / 128) >= thr) return 2;     // 256 x 128
    if (p.Cout % 64 == 0 && p.Cout % 128 != 0 && ((M + 255) / 256) * (p.Cout / 64) >= thr) return 3;      // 256 x 64
    if (p.Cout == 32 && !p.pool && !p.out_planar16 && (M + 255) / 256 >= thr) return 4;      // 256 x 32 (monodepth-vgg conv1b)
    return 0;
}

hipError_t launch_conv_dma(const ConvParams& p, int block, hipStream_t s) {
    static void (*const launch[5])(const ConvParams&, long, hipStream_t) = {launch_dma_v1, launch_dma_v2, launch_dma_v3, launch_dma_v4, launch_dma_v5};
    if (!p.zero16 || block < 1 || block > 5 || (block == 5 && p.scheme == SC_BF16X3)) return hipErrorInvalidValue;
    launch[block - 1](p, (long)p.N * p.Hout * p.Wout, s);
    return hipGetLastError();
}

}  // namespace sd
