// resolve_conv_form: the priority chain of the conv layers (DESIGN.md "which kernel runs a layer") and the label of every form.
#include "conv_form.hpp"

namespace sd {

// label "<family>_<scheme tag>kernel<instantiation>".  own_x1: the family has a one-product fp16 instantiation of its own (conv_dma, conv_direct); the
// others run SC_F16X1 as SC_F16W
static std::string kernel(const char* family, Scheme s, bool own_x1, const std::string& inst) {
    const char* const tag = s == SC_BF16X3 ? "x3_" : s == SC_HS ? "hs_" : s == SC_F16X1 && own_x1 ? "f16x1_" : s == SC_F16W || s == SC_F16X1 ? "f16w_" : "";
    return std::string(family) + tag + "kernel" + inst;
}

static void resolve_conv(ConvForm& f, const HandleFacts& hf, const NetPlan& p, const OpDesc& op, int images) {
    ConvParams& c = f.conv;
    const TensorDesc &d = p.tensors[op.dst], &s0 = p.tensors[op.src[0]];
    c.nsrc = op.nsrc; c.Ctot = op.Ctot; c.Hin = s0.H * (op.up[0] ? 2 : 1); c.Win = s0.W * (op.up[0] ? 2 : 1);
    c.pool = op.fuse_pool; c.Hout = d.H << c.pool; c.Wout = d.W << c.pool; c.Cout = d.C; c.CoutPad = p.weights[op.w].CoutPad;
    c.kh = c.kw = op.k; c.stride = op.sstride[0]; c.pad = op.pad; c.K = op.K; c.Kpad = op.Kpad; c.vec = op.vec; c.vtiles = op.Kvec / 32;
    c.act = op.act; c.m_fastest = op.m_fastest; c.Nmax = p.images; c.scheme = op.scheme; c.out_fmt = d.fmt; c.out_planar16 = d.planar16; c.sw = hf.sw;
    const bool allvec = op.vec && op.Kvec == op.Kpad, residual = op.residual >= 0;
    c.simple = op.nsrc == 1 && allvec && op.sstride[0] == 1 && !op.up[0] && op.k * op.k <= 64 && op.Kpad == op.k * op.k * s0.C;
    if (!c.simple && op.nsrc == 2 && op.k == 1 && allvec && !op.up[0] && !op.up[1] && op.pad == 0 && s0.C % 32 == 0 && p.tensors[op.src[1]].C % 32 == 0 &&
        op.Kpad == s0.C + p.tensors[op.src[1]].C)
        c.simple = 2;
    const bool ph3 = op.scheme == SC_BF16X3 || op.scheme == SC_HS;     // the phased 256 x 256 GEMM block of conv_dma3.hip exists for these two
    // its k x k stride-1 layers on one source (fc6): one output row of 256 / Wout images per tile, taps on padding rows skipped.  CALL-DEPENDENT (kept as it is):
    // a call runs row-grouped only when its image count is a multiple of the group (run_plan: N % rowgrp).  The group never changes the kernel: it needs
    // k >= 3 and the one gather mode that reads it (flat) needs k == 1
    if (ph3 && !op.fold && op.nsrc == 1 && allvec && op.k >= 3 && op.sstride[0] == 1 && !op.up[0] && !c.pool && op.Kpad == op.k * op.k * s0.C && c.Wout > 0 &&
        256 % c.Wout == 0 && !(hf.sw & SW_NO_ROWSKIP))
        f.rowgrp = 256 / c.Wout;
    // its precomputed gathers (ConvParams::flat / noup): 32-bit byte offsets inside a plane of every source, strides 1 or 2
    c.flat = (ph3 && op.k == 1 && !op.fold && !op.up[0] && !(op.nsrc > 1 && op.up[1]) && op.nsrc <= 2 && !(hf.sw & SW_NO_FLAT)) ? 1 : 0;
    c.noup = (ph3 && op.nsrc == 1 && !(hf.sw & SW_NO_FLAT)) ? 1 : 0;
    for (int j = 0; j < op.nsrc; ++j) {
        const TensorDesc& t = p.tensors[op.src[j]];
        if ((size_t)p.images * t.H * t.W * t.C * 2 >= ((size_t)1 << 32)) c.flat = c.noup = 0;
        // (a folded op keeps up[0] = 1 from the plan, but its table reads the source at its own resolution: tap layers without upsample)
        if ((op.up[j] && !op.fold) || op.sstride[j] < 1 || op.sstride[j] > 2) c.noup = 0;
    }
    if (op.fold) { c.fold = 1; c.simple = 0; c.Hin = s0.H; c.Win = s0.W; c.Hout = s0.H; c.Wout = s0.W; c.kh = c.kw = 2; }     // (the GEMM's pixel space is the source itself)
    const bool nodma = (hf.sw & SW_NO_DMA) != 0, split = p.engine != ENG_F32, s16 = !(hf.sw & SW_MFMA32);
    const int mode = conv_dma3_mode(c);
    // 1. split-K: a GEMM of a small-batch f16x2 handle that conv_dma3's ring can carry with a precomputed gather; the rule counts the rows of a FULL pass
    if (hf.small_batch && op.scheme == SC_HS && !nodma && allvec && !op.fuse_pool && !op.fold && !d.planar16 && !residual && d.C % 256 == 0 && c.CoutPad == d.C &&
        (c.flat || (c.noup && op.k >= 3 && op.sstride[0] == 1)))
        f.slices = conv_splitk_slices((long)p.images * d.H * d.W, d.C, op.Kpad, hf.cus);
    // 2.-4. conv_dma3, conv_dma, conv_stem
    const bool dma3 = f.slices < 2 && split && !nodma && conv_dma3_eligible(c, mode, residual);
    const int block = f.slices < 2 && !dma3 && split && !nodma ? conv_dma_variant(c) : 0;
    const bool stem = f.slices < 2 && split && !dma3 && !block && conv_stem_eligible(c, residual);
    if (f.slices > 1 || dma3) {
        // (16x16x32 MFMAs: every bf16 x 3 layer and the three-product engine's 1x1 layers, r05_mfma16_ab.txt; a slice is a range of the whole K axis: no row groups)
        f.family = dma3 ? CF_DMA3 : CF_SPLITK; f.variant = mode; f.s16 = s16 && (c.scheme != SC_HS || mode == 1);
        if (!dma3) { c.ksplit = f.slices; f.rowgrp = 0; }
        f.label = !dma3 ? "conv_splitk_hs_kernel" : c.scheme == SC_HS ? "conv_dma_hs_phased_kernel" : "conv_dma3_kernel";      // (one bucket for all gathers)
        f.verbose = f.label + "<" + std::to_string(mode) + ">";
        return;
    }
    if (c.out_planar16 && !stem && !block) f.error = "sub-planar output needs the LDS-DMA or the stem conv kernel";
    else if (c.pool && !block) f.error = "fused pool needs the LDS-DMA conv kernel";
    else if (c.fold && !(block && c.scheme != SC_BF16X3)) f.error = "an upsample-folded conv needs the conv_dma3 kernel (bf16 x 3) or a two-plane form of conv_dma";
    else if (block) {
        static const char* const blocks[5] = {"<2,4,2,2>", "<4,2,2,2>", "<4,2,2,1>", "<8,1,1,1>", "<2,4,4,2>"};      // 128x256, 256x128, 256x64, 256x32, 256x256
        f.family = CF_DMA; f.variant = block; f.label = kernel("conv_dma_", c.scheme, true, blocks[block - 1]);
    } else if (stem) {
        f.family = CF_STEM; f.label = kernel("conv_stem_", c.scheme, false, "");
    } else if (split) {
        // 5. CALL-DEPENDENT (kept as it is): conv_split's 128 x 256 tile needs 512 tiles of THIS call, so a layer with Cout % 256 == 0 may change tile with the call
        static const char* const tiles[5] = {"<2,4,2,2", "<4,2,2,2", "<2,2,2,2", "<4,1,2,2", "<4,1,2,1"};      // 128x256, 256x128, 128x128, 256x64, 256x32
        f.family = CF_SPLIT; f.variant = conv_split_variant(c, images); f.reads_images = c.Cout % 256 == 0;
        const char* const vec = c.scheme != SC_BF16X2 ? ">" : c.vec ? ",true>" : ",false>";     // (one HS bucket; the bf16 x 2 label names the gather)
        f.label = kernel("conv_split_", c.scheme, false, c.scheme == SC_HS ? "" : std::string(tiles[f.variant]) + vec);
    } else {
        const int tn = conv_tile_n(c.Cout);
        f.family = CF_IGEMM;
        f.label = std::string("conv_igemm_kernel") + (tn == 128 ? "<2,2,4,4" : tn == 64 ? "<4,1,4,4" : tn == 32 ? "<4,1,4,2" : "<4,1,4,1") + (c.vec ? ",true>" : ",false>");
    }
}

static void resolve_direct(ConvForm& f, const HandleFacts& hf, const NetPlan& p, const OpDesc& op) {
    ConvDirectParams& c = f.dir;
    const TensorDesc& d = p.tensors[op.dst];
    c.nchunks = op.nchunks; c.pool = op.fuse_pool; c.H = d.H << c.pool; c.W = d.W << c.pool;
    c.nsplit = op.nsplit; c.Cout = d.C / op.nsplit; c.Cstride = d.C; c.out_planar16 = d.planar16; c.nreal = (d.Ctf > 0 && d.Ctf < d.C) ? d.Ctf : 0;
    c.all_up = 1;
    for (int i = 0; i < op.nsrc; ++i) c.all_up = c.all_up && op.up[i] == 1;
    c.fold = op.fold; c.act = op.act; c.Nmax = p.images; c.rows_per_wave = 2; c.scheme = op.scheme; c.out_fmt = d.fmt; c.sw = hf.sw;
    // the tile shape: <= 32 or 64 channels per pass; the 16-wide MFMA form of the full-resolution decoder tail (8-row tiles unless behind an upsample);
    // source-resolution halo tiles when every source sits behind a x2 upsample
    DirectVariant& v = f.direct;
    v.nb = c.Cout <= 32 ? 1 : 2;
    v.n16 = c.Cout <= 16 && c.nsplit == 1 && !c.pool && !(hf.sw & SW_NO_N16);
    v.up = c.all_up && !(c.H & 1) && !(c.W & 1);
    v.th = v.n16 && !v.up ? 8 : 16;
    // the chunk split (small-batch level 2): 64-channel-pass HS layers, not folded, not the all-upsampled instantiation, no padded channels; a FULL pass's work items
    if (hf.small_batch >= 2 && op.scheme == SC_HS && d.fmt == PL_HS && op.nsplit >= 1 && d.C == 64 * op.nsplit && !op.fold && !c.nreal && !v.up)
        f.slices = conv_splitc_slices(conv_direct_items(c.W, c.H, p.images, op.nsplit), op.nchunks, hf.cus);
    const std::string nb = std::to_string(v.nb);
    f.family = f.slices > 1 ? CF_DIRECT_SPLITC : op.scheme == SC_BF16X3 ? CF_DIRECT3 : CF_DIRECT;
    if (f.slices > 1) { c.csplit = f.slices; f.label = "conv_direct_splitc_hs_kernel"; }
    else if (op.scheme == SC_BF16X3) f.label = c.fold ? "conv_direct_x3_fold_kernel<" + nb + ">" : "conv_direct_x3_kernel<" + nb + ",2>";
    else if (c.fold && op.scheme == SC_HS) f.label = "conv_direct_hs_fold_kernel<" + nb + ">";
    else if (op.scheme == SC_F16XW) f.label = "conv_direct_f16w_x2_kernel<2,2>";
    else f.label = kernel("conv_direct_", op.scheme, true, v.n16 ? "<1,n16>" : v.nb == 1 ? "<1,2>" : "<2,2>");
}

ConvForm resolve_conv_form(const HandleFacts& hf, const NetPlan& p, const OpDesc& op, int images) {
    ConvForm f;
    if (op.kind == OP_CONV) resolve_conv(f, hf, p, op, images);
    else if (op.kind == OP_CONV_DIRECT) resolve_direct(f, hf, p, op);
    else if (op.kind == OP_DEC_TAIL1) { f.family = CF_DEC_TAIL1; f.label = engine_forms(p.engine).conv == SC_HS ? "dec_tail1_hs_kernel" : "dec_tail1_x3_kernel"; }
    if (f.verbose.empty()) f.verbose = f.label;
    return f;
}

}  // namespace sd
