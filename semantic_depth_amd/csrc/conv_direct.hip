// Direct 3x3 stride-1 convolution of the split engines: every such layer whose width is a multiple of 32 (VGG conv1_2..conv5_3,
// the ResNet 3x3 layers, the whole monodepth decoder incl. the disparity heads 4..2), with optional x2 nearest-neighbour
// upsample and concatenated sources.
//
// An im2col GEMM fetches every activation nine times (once per tap).  Here a workgroup (8 waves) owns a 16 x 32 pixel
// output tile and, per 16-channel chunk of the input, DMAs the 18 x 34 pixel HALO TILE once into LDS (32 B per pixel and
// plane, octet slot XOR-swizzled by (pixel >> 3) & 1 on the source side so the shifted ds_read_b128 fragment reads stay
// conflict free) together with the chunk's 9 x 16 x 64 weights; the nine taps read their shifted MFMA fragments straight
// out of the halo tile, each input row fragment serving three taps: 89 B of LDS-DMA per MFMA against 170-256 B of the
// im2col blocks of conv_dma.hip.  Two stages: the DMA of chunk c+1 runs under the MFMAs of chunk c, one barrier per chunk.
// Each wave: 2 rows x 32 pixels x 64 channels, 3 x v_mfma_f32_32x32x16_bf16 per product.  Layers with more than 64 output
// channels are passes of 64 (work item = tile x pass).  Variants: NB = 1 (<= 32 channels), N16 (<= 16 channels on the
// 16-wide MFMA, 8-row tiles with two workgroups per CU), UP (all sources upsampled: source-resolution LDS tile), fused
// 2x2 max pool, sub-planar (16-channel planes) sources and outputs.
#include <cstdlib>
#include "kernels.hpp"
#include "split_fmt.hpp"

namespace sd {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// one LDS-DMA (64 lanes x 16 B, lane-linear destination); inline asm so hipcc does not serialise them (see conv_dma.hip)
__device__ __forceinline__ void ddma16(const void* gsrc, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}

constexpr int D_TW = 32, D_HW = D_TW + 2;                // output tile / halo tile width
constexpr int D_WAVES = 8;
// NB = 32-channel blocks of output channels (Cout <= 32 NB); MT = output rows per wave (tile height 8 MT).
// MT = 2 halves the halo and weight traffic per pixel; MT = 1 keeps the source footprint of the workgroups of one XCD
// inside its 4 MiB L2 when a source pixel is wider than one 16-channel chunk (each chunk pass touches only 32 B of a
// pixel's 128-B line, so a line evicted between passes is fetched from the fabric again).
// UP: every source is read through a x2 nearest-neighbour upsample (the upconv layers): the LDS tile then holds the
// (HH/2 + 1) x 18 SOURCE pixels under the halo instead of their HH x 34 replicas (a quarter of the DMA instructions and
// bytes); halo pixel (hy, hx) reads source pixel ((hy + 1) >> 1, (hx + 1) >> 1) of the tile (tile origins are even).
template <int NB, int MT, bool UP = false> struct DirectCfg {
    static constexpr int TH = 8 * MT, HH = TH + 2;
    static constexpr int SH = UP ? HH / 2 + 1 : HH, SW = UP ? D_HW / 2 + 1 : D_HW;      // stored tile
    static constexpr int XI = (SH * SW * 2 + 63) / 64;        // DMA instructions per halo plane (2 slots per pixel)
    static constexpr int XUNITS = XI * 64;
    static constexpr int XS = (2 * XI + D_WAVES - 1) / D_WAVES;    // X-DMA slots per wave
    static constexpr int WI = 9 * NB;                    // DMA instructions per weight plane
    static constexpr int WUNITS = 9 * 2 * 32 * NB;       // taps x octets x output channels
    static constexpr int STAGE = 2 * XUNITS + 2 * WUNITS;
};


// the chunk descriptor through the scalar cache (a compiler-visible vector load would bring a vmcnt(0) that drains the DMAs)
typedef int i32x8d __attribute__((ext_vector_type(8)));
__device__ __forceinline__ DirectChunk load_chunk(const DirectChunk* ptr) {
    i32x8d v;
    asm volatile("s_load_dwordx8 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "s"(ptr) : "memory");
    DirectChunk e;
    e.base = reinterpret_cast<const void*>(((unsigned long long)(unsigned)v[1] << 32) | (unsigned)v[0]);
    e.H = v[2]; e.W = v[3]; e.C = v[4]; e.up = v[5]; e.nvalid = v[6]; e.pad = v[7];
    return e;
}

// persistent: workgroup b walks tiles b, b + grid, ...; the (tile, chunk) sequence is one software pipeline, so the first
// chunk of the next tile lands while the current tile's epilogue runs.
// F16: ONE fp16 activation plane, two fp16 weight planes, two MFMA products per product (split_fmt.hpp)
// N16 (Cout <= 16, NB = 1): the 32-row MFMA would spend half its rows on padding, so the products run on
// v_mfma_f32_16x16x32 instead: K = 32 is one PAIR of taps x 16 channels, a wave's 2 x 32 pixels are four 16-pixel blocks.
// W1 (with F16): ONE MFMA product per product -- the w_lo plane is neither fetched nor multiplied (plain fp16 x fp16, f32 accumulate)
// X2 (with F16): the input is fp16 hi + lo planes and only w_hi is used: TWO products x_hi*w_hi + x_lo*w_hi (split_fmt.hpp)
// H2 (with F16 and X2; SD_PREC_F16X2): fp16 hi + SCALED lo input planes x fp16 hi + lo weight planes, THREE products
// x_hi*w_hi + x_hi*w_lo + x_lo*(w_hi * 2^-11), the accumulator times ConvDirectParams::alpha, HS output planes (split_fmt.hpp "HS")
// FOLD (with H2 and UP; round 6: the upconv layers of SD_PREC_F16X2 that stay on this kernel -- upconv3 / upconv2): the upsample-folded form -- per output parity
// (y & 1, x & 1) a 2x2 conv on the SOURCE with the 3x3 taps that read the same source pixel added up (plan.hpp OpDesc::fold): 16 tap matrices per chunk instead of
// 9, but 4 instead of 9 MFMA groups per output pixel.  Wave w owns parity w & 3 and the source rows 4 (w >> 2) .. + 3 of the tile: its two 32-pixel MFMA column groups
// are 2 source rows x 16 source columns each (the fragment scheme of conv_direct3.hip's fold).  The X fragments of a chunk (2 column shifts x 4 row offsets x 2 planes)
// are read once and stay in registers; a chunk is 4 NB MFMA groups, so the DMA slots go out two per group.
// SPLITC (with H2, NB = 2, not UP / FOLD / N16; sd_set_small_batch level 2, profiled as conv_direct_splitc_hs_kernel): the chunk-range form.  A work item is
// (tile, slice, pass): it walks the contiguous chunk range conv_splitk_range(nchunks, csplit, slice) only -- the issue cursor too, so the first chunk of the next
// item's range still lands under this item's epilogue -- and stores its raw f32 accumulators to ConvDirectParams::partial[slice][pixel][Cstride] at conv
// resolution; alpha, bias, activation, pool, split and clamp belong to splitc_reduce_kernel.  The passes of one (tile, slice) stay neighbouring items.
template <int NB, int MT, bool F16, bool N16 = false, bool UP = false, bool W1 = false, bool X2 = false, bool H2 = false, bool FOLD = false, bool SPLITC = false>
__global__ __launch_bounds__(512, (N16 && MT == 1) ? 2 : 1) void conv_direct_kernel(const ConvDirectParams p) {
    static_assert(!SPLITC || (H2 && NB == 2 && MT == 2 && !N16 && !UP && !FOLD), "the chunk-range form exists for the 64-channel-pass HS kernel");
    static_assert(!N16 || NB == 1, "N16 is a variant of the 32-channel kernel");
    static_assert(!H2 || (F16 && X2 && !W1), "H2 is the fp16 form with both planes of both operands");
    static_assert(!FOLD || (H2 && UP && !N16 && MT == 2), "the folded form: three-product engine, source-resolution tiles");
    constexpr int NTAP = FOLD ? 16 : 9;                  // tap matrices per chunk
    constexpr bool ONEW = W1 || (X2 && !H2);           // only the w_hi plane is fetched and multiplied
    using Cfg = DirectCfg<NB, MT, UP>;
    constexpr int S_HH = Cfg::SH, S_HW = Cfg::SW;
    // LDS pixel slot of halo pixel (hy, hx)
    auto hpix = [](int hy, int hx) { return UP ? ((hy + 1) >> 1) * S_HW + ((hx + 1) >> 1) : hy * S_HW + hx; };
    // weights: a (plane, chunk) block in memory is [tap][octet][32 NB][8]; the LDS image is the same, except N16, which keeps
    // only the 16 output channels it multiplies ([tap][octet][16][8], 288 units in 5 DMA instructions)
    constexpr int D_GW = NTAP * 2 * 32 * NB;             // ([tap][octet][32 NB channels]; FOLD: [parity 4][2x2 tap 4][octet][32 NB])
    constexpr int D_WI = N16 ? 5 : NTAP * NB, D_WUNITS = N16 ? 320 : D_GW;
    // a stage holds the planes the form reads -- X hi [+ lo] | W hi [+ lo] -- and is at least as large as the epilogue's transposition
    // slabs, which live in a consumed stage.  (The fp16 forms of the 16-channel kernels thereby fit THREE workgroups per CU instead of
    // two: these layers -- two chunks of little arithmetic per tile -- are bound by the latency of the two-stage ring.)
    constexpr int XPL = (F16 && !X2) ? 1 : 2, WPL = ONEW ? 1 : 2;
    constexpr int SLAB = N16 ? D_WAVES * 2 * 32 * 48 / 16 : D_WAVES * 32 * (64 * NB + 16) / 16;
    constexpr int STAGE_MIN = XPL * Cfg::XUNITS + WPL * D_WUNITS;
    constexpr int D_STAGE = STAGE_MIN < SLAB ? SLAB : STAGE_MIN;
    constexpr int D_TH = Cfg::TH, D_HH = Cfg::HH, D_XI = Cfg::XI, D_XUNITS = Cfg::XUNITS, XS = Cfg::XS;
    __shared__ __attribute__((aligned(16))) u32x4 lds[2 * D_STAGE];
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int tiles_x = p.W / D_TW, tiles_y = (p.H + D_TH - 1) / D_TH;
    const int total = tiles_x * tiles_y * p.N;
    const u32x4* const zero = reinterpret_cast<const u32x4*>(p.zero16);
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) void*)lds;      // LDS byte address
    const int frow = lane & 31, fk = lane >> 5;

    // work item = (tile, pass of <= 64 output channels); the passes of a tile are neighbouring items
    const int items = SPLITC ? total * p.nsplit * p.csplit : total * p.nsplit;
    struct Tile { int img, ty0, tx0, half, slice, c0, c1; };     // (slice, chunks [c0, c1): SPLITC only)
    auto tile_of = [&](int it) {
        if ((items & 7) == 0) it = (it & 7) * (items >> 3) + (it >> 3);     // neighbouring items (shared halos) on one XCD
        Tile r;
        int tid = it / p.nsplit;
        r.half = it - tid * p.nsplit;
        if constexpr (SPLITC) {
            const int t2 = tid / p.csplit;
            int cnt;
            r.slice = tid - t2 * p.csplit;
            conv_splitk_range(p.nchunks, p.csplit, r.slice, r.c0, cnt);
            r.c1 = r.c0 + cnt;
            tid = t2;
        }
        const int bx = tid % tiles_x; tid /= tiles_x;
        r.tx0 = bx * D_TW; r.ty0 = (tid % tiles_y) * D_TH; r.img = tid / tiles_y;
        return r;
    };

    // halo geometry of this lane's X-DMA slots (instruction j = wave + 8 i): constant over tiles and chunks.
    // packed: ry | rx << 8 | 8 * octet << 16 | inside-halo << 20
    constexpr int WS = (WPL * D_WI + D_WAVES - 1) / D_WAVES;       // weight-DMA slots per wave
    int geo[XS];
#pragma unroll
    for (int i = 0; i < XS; ++i) {
        const int j = wave + D_WAVES * i;
        const int u = (j - (j >= D_XI ? D_XI : 0)) * 64 + lane;      // (slots with j >= XPL * XI are never issued)
        const int pix = u >> 1;
        const int oct = (u & 1) ^ ((pix >> 3) & 1);
        const int ry = pix / S_HW, rx = pix - ry * S_HW;
        geo[i] = ry | (rx << 8) | (oct << 19) | ((pix < S_HH * S_HW ? 1 : 0) << 20);
    }
    // lane offsets (16-byte units) of the weight slots inside a (plane, chunk) block
    int wu[WS];
#pragma unroll
    for (int i = 0; i < WS; ++i) {
        const int jw = wave + D_WAVES * i;
        const int u = (jw - (jw >= D_WI ? D_WI : 0)) * 64 + lane;
        wu[i] = N16 ? (u >= 288 ? -1 : (u >> 4) * 32 + (u & 15)) : u;
    }

    // The DMA issue of one (tile, chunk) item is cut into SLOTS (one DMA instruction each) that the product loop spreads between
    // its first MFMA groups; what depends on the tile only -- source pixel coordinates and the in-image mask of every slot -- is
    // computed once per tile, so a slot costs about a dozen VALU operations per chunk.
    // Round-2 decomposition of conv4_2 (one product, 32 frames): whole kernel 0.975 ms; no DMA issued (MFMA + LDS reads) 0.761
    // = 1.62 PF/s; no MFMA (DMA only) 0.577; neither 0.128.  Tried against the 0.21 ms the two cost each other, and measured
    // equal or slower: a four-stage ring with counted vmcnt waits (-8..15 %), the weight blocks through VGPRs and ds_write_b128
    // instead of the DMA path (-15 %), the slots at the top of the chunk vs spread through it (+-1 %).  Latency is therefore not
    // what the DMA costs; the kernels run at the chip's power limit (profiles/r01_mfma_sustained_probe.txt), and bytes moved per
    // MFMA -- 38 KB per 36 MFMAs and wave here -- are the remaining lever.
    int sgy[XS], sgx[XS];
    unsigned okA = 0, okB = 0;            // bit i: slot i reads an existing pixel (okB: ... and the first channel octet of a chunk)
    auto set_tile = [&](const Tile& tl) {
        okA = 0; okB = 0;
#pragma unroll
        for (int i = 0; i < XS; ++i) {
            const int ry = geo[i] & 0xff, rx = (geo[i] >> 8) & 0xff;
            // UP: source coordinates directly (an output-resolution pixel is outside the image exactly when its source pixel is)
            const int gy = (UP ? (tl.ty0 >> 1) : tl.ty0) - 1 + ry, gx = (UP ? (tl.tx0 >> 1) : tl.tx0) - 1 + rx;
            const bool in = ((geo[i] >> 20) & 1) && (unsigned)gy < (unsigned)(UP ? p.H >> 1 : p.H) && (unsigned)gx < (unsigned)(UP ? p.W >> 1 : p.W);
            sgy[i] = gy; sgx[i] = gx;
            okA |= (in ? 1u : 0u) << i;
            okB |= ((in && !((geo[i] >> 19) & 1)) ? 1u : 0u) << i;
        }
    };
    // stage image: Xh[1280] [Xl[1280]] Wh[576 NB] [Wl[576 NB]] (the planes the form reads); X unit = [halo pixel][octet ^ ((pixel >> 3) & 1)]
    struct ChunkCtx { const uint16_t* img; size_t plane; unsigned rowel, C, okm, sbyte; int up; const u32x4* w; };
    auto begin_chunk = [&](const DirectChunk& ch, const Tile& tl, int c, int stage) {
        ChunkCtx k;
        k.plane = (size_t)p.Nmax * ch.H * ch.W * (ch.pad ? ch.pad : ch.C);      // elements (pad: channels of a sub-planar tensor)
        k.img = reinterpret_cast<const uint16_t*>(ch.base) + (size_t)tl.img * ch.H * ch.W * ch.C;
        k.rowel = (unsigned)(ch.W * ch.C); k.C = (unsigned)ch.C; k.up = UP ? 0 : ch.up;
        k.okm = ch.nvalid >= 2 ? okA : okB;
        k.sbyte = lds0 + (unsigned)(stage * D_STAGE * 16);
        k.w = p.wt + ((size_t)(2 * tl.half) * p.nchunks + c) * D_GW;
        return k;
    };
    auto xslot = [&](const ChunkCtx& k, int i) {
        const int j = wave + D_WAVES * i;
        if (j >= XPL * D_XI) return;                   // fp16 activations: ONE plane (X2: hi + lo)
        const unsigned off = (unsigned)(sgy[i] >> k.up) * k.rowel + ((unsigned)(sgx[i] >> k.up) * k.C + ((unsigned)(geo[i] >> 16) & 8u));
        const uint16_t* src = (j >= D_XI ? k.img + k.plane : k.img) + off;
        ddma16(((k.okm >> i) & 1u) ? reinterpret_cast<const u32x4*>(src) : zero, k.sbyte + (unsigned)(j * 1024));
    };
    auto wslot = [&](const ChunkCtx& k, int i) {
        const int jw = wave + D_WAVES * i;
        if (jw >= WPL * D_WI) return;                  // both weight planes (W1, X2: w_hi only)
        const u32x4* gw = (jw >= D_WI ? k.w + (size_t)p.nchunks * D_GW : k.w) + wu[i];
        ddma16(N16 && wu[i] < 0 ? zero : gw, k.sbyte + (unsigned)((XPL * D_XUNITS + jw * 64) * 16));
    };
    constexpr int NSLOT = XS + WS;
    auto slot = [&](const ChunkCtx& k, int sidx) { if (sidx < XS) xslot(k, sidx); else if (sidx < NSLOT) wslot(k, sidx - XS); };

    // the bias vector lives in LDS (zero past the layer's channels) and is read by the epilogue: no registers held
    // through the product loop
    __shared__ __attribute__((aligned(16))) float sbias[N16 ? 4 : 512];
    if constexpr (!N16) sbias[threadIdx.x] = (int)threadIdx.x < p.nsplit * p.Cout ? p.bias[threadIdx.x] : 0.f;
    const int c16 = lane & 15, kg16 = lane >> 4;           // N16 fragment coordinates
    f32x4 bias16 = {0.f, 0.f, 0.f, 0.f};
    if (N16 && 4 * kg16 < (p.nreal ? p.nreal : p.Cout)) bias16 = *reinterpret_cast<const f32x4*>(p.bias + 4 * kg16);      // (bias slots are padded to 4)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

    int tid = blockIdx.x;
    if (tid >= items) return;
    Tile cur = tile_of(tid);
    // the issue cursor: the (tile, chunk) item that goes into the ring next
    int itid = tid, ic = 0;
    Tile icur = cur;
    set_tile(icur);
    if constexpr (SPLITC) ic = icur.c0;
    auto advance = [&]() {
        if constexpr (SPLITC) {
            if (++ic == icur.c1) { itid += gridDim.x; if (itid < items) { icur = tile_of(itid); set_tile(icur); ic = icur.c0; } }
        } else {
            if (++ic == p.nchunks) { ic = 0; itid += gridDim.x; if (itid < items) { icur = tile_of(itid); set_tile(icur); } }
        }
    };
    if constexpr (SPLITC) {
        const ChunkCtx k = begin_chunk(load_chunk(p.chunks + ic), icur, ic, 0);
#pragma unroll
        for (int sidx = 0; sidx < NSLOT; ++sidx) slot(k, sidx);
        advance();
    } else {
        const ChunkCtx k = begin_chunk(load_chunk(p.chunks), icur, 0, 0);
#pragma unroll
        for (int sidx = 0; sidx < NSLOT; ++sidx) slot(k, sidx);
        advance();
    }
    int g = 0;                                     // stages consumed so far
    for (; tid < items; tid += gridDim.x) {
        const int half = cur.half;
        f32x16 acc[MT][NB];
#pragma unroll
        for (int a = 0; a < MT; ++a)
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[a][nb][r] = 0.f;
        f32x4 acc16[MT][2];
#pragma unroll
        for (int a = 0; a < MT; ++a)
#pragma unroll
            for (int pb = 0; pb < 2; ++pb) acc16[a][pb] = (f32x4){0.f, 0.f, 0.f, 0.f};
        const int nck = SPLITC ? cur.c1 - cur.c0 : p.nchunks;       // chunks this item walks
        for (int c = 0; c < nck; ++c, ++g) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();          // stage g has landed for every wave; everyone is done with stage g-1
            const bool more = itid < items;        // item g + 1 exists: its DMAs go into stage (g + 1) & 1 during this chunk
            ChunkCtx k;
            if constexpr (N16) {
                if (more) {
                    k = begin_chunk(load_chunk(p.chunks + ic), icur, ic, (g + 1) & 1);
#pragma unroll
                    for (int sidx = 0; sidx < NSLOT; ++sidx) slot(k, sidx);
                }
            }
            const u32x4* Xh = lds + (g & 1) * D_STAGE;
            const u32x4* Xl = Xh + D_XUNITS;
            const u32x4* Wh = Xh + XPL * D_XUNITS;
            const u32x4* Wl = Wh + D_WUNITS;
            if constexpr (N16) {
                const u32x4 z4 = {0u, 0u, 0u, 0u};
#pragma unroll
                for (int tp = 0; tp < 5; ++tp) {             // tap pairs (0,1) (2,3) (4,5) (6,7) (8,-)
                    const int tap = 2 * tp + (kg16 >> 1), oct = kg16 & 1;
                    const bool live = tap < 9;
                    const int dy = (tap * 11) >> 5, dx = tap - 3 * dy;         // tap / 3, tap % 3 for tap < 10
                    const int wi = (tap * 2 + oct) * 16 + c16;
                    const u32x4 wh = live ? Wh[wi] : z4;
                    const u32x4 wl = ONEW ? wh : (live ? Wl[wi] : z4);
                    const u32x4 whs = H2 ? hs_wscaled(wh) : wh;          // the weight operand of the x_lo product
#pragma unroll
                    for (int a = 0; a < MT; ++a)
#pragma unroll
                        for (int pb = 0; pb < 2; ++pb) {
                            const int lp = hpix(MT * wave + a + dy, 16 * pb + c16 + dx);
                            const int idx = lp * 2 + (oct ^ ((lp >> 3) & 1));
                            const u32x4 xh = live ? Xh[idx] : z4;
                            const u32x4 xl = (F16 && !X2) ? xh : (live ? Xl[idx] : z4);
#pragma unroll
                            for (int pr = 0; pr < 3; ++pr) {      // x_hi*w_lo, x_lo*w_hi, x_hi*w_hi; fp16 activations have no lo plane
                                if ((F16 && !X2 && pr == 1) || (ONEW && pr == 0)) continue;
                                acc16[a][pb] = mfma_frag16<F16>(pr == 0 ? wl : pr == 1 ? whs : wh, pr == 1 ? xl : xh, acc16[a][pb]);
                            }
                        }
                }
            } else if constexpr (FOLD) {
                constexpr int NGRPF = 4 * NB, SPG = (NSLOT + NGRPF - 1) / NGRPF;       // MFMA groups of a chunk (2x2 tap, 32-channel block); DMA slots per group
                const int fpar = wave & 3, fpy = fpar >> 1, fpx = fpar & 1, fhh = wave >> 2;
                // fragment (column shift tb, row offset ro = 2 a + ta): lane = (source row frow >> 4, source column frow & 15) -> pixel (4 hh + ro + row + py, column + tb + px)
                // of the stored source tile
                u32x4 xh[2][4], xl[2][4];
#pragma unroll
                for (int tb = 0; tb < 2; ++tb)
#pragma unroll
                    for (int ro = 0; ro < 4; ++ro) {
                        const int lp = (4 * fhh + ro + (frow >> 4) + fpy) * S_HW + (frow & 15) + tb + fpx;
                        const int idx = lp * 2 + (fk ^ ((lp >> 3) & 1));
                        xh[tb][ro] = Xh[idx];
                        xl[tb][ro] = Xl[idx];
                    }
                u32x4 wqh[3], wql[3];
                auto wloadf = [&](int grp) {
                    const int tp = grp / NB, nb = grp % NB;
                    const int wi = ((fpar * 4 + tp) * 2 + fk) * (32 * NB) + nb * 32 + frow;
                    wqh[grp % 3] = Wh[wi];
                    wql[grp % 3] = Wl[wi];
                };
                wloadf(0);
                wloadf(1);
#pragma unroll
                for (int grp = 0; grp < NGRPF; ++grp) {
                    const int tp = grp / NB, ta = tp >> 1, tb = tp & 1, nb = grp % NB;
                    if (grp + 2 < NGRPF) wloadf(grp + 2);
                    __builtin_amdgcn_sched_barrier(0);
                    {
                        const u32x4 wh = wqh[grp % 3], wl = wql[grp % 3];
                        const u32x4 whs = hs_wscaled(wh);
#pragma unroll
                        for (int pr = 0; pr < 3; ++pr)            // x_hi*w_lo, x_lo*w_hi, x_hi*w_hi: the product order of the plain form
#pragma unroll
                            for (int a = 0; a < MT; ++a)
                                acc[a][nb] = mfma_frag<true>(pr == 0 ? wl : pr == 1 ? whs : wh, pr == 1 ? xl[tb][2 * a + ta] : xh[tb][2 * a + ta], acc[a][nb]);
                    }
                    if (grp == 0 && more) {
                        __builtin_amdgcn_sched_barrier(0);
                        k = begin_chunk(load_chunk(p.chunks + ic), icur, ic, (g + 1) & 1);
                    }
                    if (more) {
                        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                        for (int sidx = grp * SPG; sidx < (grp + 1) * SPG; ++sidx) slot(k, sidx);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
            } else {
            constexpr int NGRP = 9 * NB;               // MFMA groups of a chunk; the DMA slots follow groups 1 .. NSLOT
            static_assert(NSLOT <= NGRP, "one DMA slot per MFMA group");
            // The LDS reads run AHEAD of the MFMAs that consume them (an explicit software pipeline: left to itself hipcc puts every weight
            // fragment's ds_read + s_waitcnt directly in front of its 1-3 products x MT MFMAs, and the two waves of a SIMD then do not have
            // enough MFMAs per group to cover an LDS round trip -- the one-product layers least of all): the weight fragment(s) of group
            // g + 2 and the next X row(s) (row dy + 2 / the first two rows of the next dx) are issued before group g's MFMAs.
            constexpr bool HASWL = !ONEW, HASXL = !(F16 && !X2);
            u32x4 xh[MT + 2], xl[HASXL ? MT + 2 : 1];
            u32x4 wqh[3], wql[HASWL ? 3 : 1];
            auto wload = [&](int grp) {
                const int dx = grp / (3 * NB), dy = (grp / NB) % 3, nb = grp % NB;
                const int wi = ((dy * 3 + dx) * 2 + fk) * (32 * NB) + nb * 32 + frow;
                wqh[grp % 3] = Wh[wi];
                if constexpr (HASWL) wql[grp % 3] = Wl[wi];
            };
            auto xrow = [&](int dx, int r) {
                const int lp = hpix(MT * wave + r, frow + dx);
                const int idx = lp * 2 + (fk ^ ((lp >> 3) & 1));
                xh[r] = Xh[idx];
                if constexpr (HASXL) xl[r] = Xl[idx];
            };
            wload(0);
            wload(1);
#pragma unroll
            for (int r = 0; r < MT; ++r) xrow(0, r);
#pragma unroll
            for (int grp = 0; grp < NGRP; ++grp) {
                const int dx = grp / (3 * NB), dy = (grp / NB) % 3, nb = grp % NB;
                if (grp + 2 < NGRP) wload(grp + 2);
                if (nb == 0) {
                    if (dy < 2) xrow(dx, dy + MT);
                    else if (dx < 2) {
#pragma unroll
                        for (int r = 0; r < MT; ++r) xrow(dx + 1, r);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
                {
                    const u32x4 wh = wqh[grp % 3];
                    const u32x4 wl = HASWL ? wql[HASWL ? grp % 3 : 0] : wh;
                    const u32x4 whs = H2 ? hs_wscaled(wh) : wh;          // the weight operand of the x_lo product (4 v_pk_mul_f16 beside 3 MT MFMAs)
#pragma unroll
                    for (int pr = 0; pr < 3; ++pr) {          // x_hi*w_lo, x_lo*w_hi, x_hi*w_hi; fp16 activations have no lo plane
                        if ((F16 && !X2 && pr == 1) || (ONEW && pr == 0)) continue;
#pragma unroll
                        for (int a = 0; a < MT; ++a)
                            acc[a][nb] = mfma_frag<F16>(pr == 0 ? wl : pr == 1 ? whs : wh, pr == 1 ? xl[HASXL ? a + dy : 0] : xh[a + dy], acc[a][nb]);
                    }
                }
                if (grp == 0 && more) {
                    // the descriptor's scalar load is issued AND waited for here, behind the first MFMA group (whose execution it
                    // overlaps); kept in one piece: SGPRs of a load in flight must not be live across code the compiler may spill in
                    __builtin_amdgcn_sched_barrier(0);
                    k = begin_chunk(load_chunk(p.chunks + ic), icur, ic, (g + 1) & 1);
                }
                if (grp < NSLOT && more) {
                    __builtin_amdgcn_sched_barrier(0);
                    slot(k, grp);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            }
            if (more) advance();
        }

        // ---- epilogue: bias + activation, split once, LDS transpose (in the stage just consumed; the other one is being
        //      filled for the next tile), 16-byte runs of 8 channels per pixel and plane ----
        if constexpr (SPLITC) {
            // the raw accumulators of this (tile, slice, pass): lane = pixel frow of the wave's row, channels 8 r4 + 4 fk .. + 3 of the pass -- one 16-byte store each,
            // the two lanes of a pixel 32 contiguous bytes, the 8 stores of a lane the pass's 256 bytes of its pixel.  No LDS: nothing waits for the other waves.
            // Rows of a partial last tile are not stored (the reduce never reads them)
#pragma unroll
            for (int a = 0; a < MT; ++a) {
                const int y = cur.ty0 + MT * wave + a;
                if (y >= p.H) continue;
                float* o = p.partial + ((size_t)cur.slice * p.N * p.H * p.W + (size_t)(cur.img * p.H + y) * p.W + cur.tx0 + frow) * p.Cstride + half * 64 + 4 * fk;
#pragma unroll
                for (int r4 = 0; r4 < 4 * NB; ++r4) {
                    const int nb = r4 >> 2, q = r4 & 3;
                    *reinterpret_cast<f32x4*>(o + 8 * r4) = (f32x4){acc[a][nb][4 * q], acc[a][nb][4 * q + 1], acc[a][nb][4 * q + 2], acc[a][nb][4 * q + 3]};
                }
            }
            if (tid + (int)gridDim.x < items) cur = tile_of(tid + gridDim.x);
            continue;
        }
        __builtin_amdgcn_s_barrier();
        auto epilogue = [&](auto tag, auto otag) {
            constexpr int ACT = decltype(tag)::value;
            constexpr int OF = decltype(otag)::value;          // output planes (the consumers' format): 0 bf16 hi+lo, 1 ONE fp16, 2 fp16 hi+lo
            constexpr bool O16 = OF == 1;
            constexpr int ROW = 64 * NB + 16;
            constexpr int SEGS = 4 * NB, PPP = 64 / SEGS;        // 16-byte segments per pixel, pixels per store pass
            // per wave: hi slab and lo slab of 32 pixels (a lo slab that does not fit the stage reuses the hi slab)
            constexpr bool TWO = D_WAVES * 2 * 32 * ROW <= D_STAGE * 16;
            static_assert(D_WAVES * 32 * ROW <= D_STAGE * 16, "epilogue slab must fit one stage");
            unsigned char* sh = reinterpret_cast<unsigned char*>(lds + ((g - 1) & 1) * D_STAGE) + wave * ((TWO ? 2 : 1) * 32 * ROW);
            unsigned char* sl = TWO ? sh + 32 * ROW : sh;
            const int seg = lane % SEGS, prow = lane / SEGS;
            uint16_t* const out_hi = reinterpret_cast<uint16_t*>(p.out);
            const int n0 = half * p.Cout;                 // first output channel of this split
            f32x4 bias[4 * NB];
#pragma unroll
            for (int r4 = 0; r4 < 4 * NB; ++r4) bias[r4] = *reinterpret_cast<const f32x4*>(sbias + (N16 ? 0 : n0 + 8 * r4 + 4 * fk));
            // output address of 8 channels (segment sg) of pixel px: NHWC, or 16-channel sub-planes
            auto oaddr = [&](size_t px, size_t npix, int sg) {
                const int ch = n0 + sg * 8;
                return p.out_planar16 ? out_hi + ((size_t)(ch >> 4) * p.Nmax * npix + px) * 16 + (ch & 8) : out_hi + px * p.Cstride + ch;
            };
            if constexpr (N16) {
                // lane holds channels 4 kg16 .. + 3 of pixel 16 pb + c16; slab row = 16 channels (32 B) + pad per plane
                constexpr int R16 = 32 + 16;
                static_assert(D_WAVES * 2 * 32 * R16 <= D_STAGE * 16, "N16 epilogue slabs must fit one stage");
                unsigned char* s16 = reinterpret_cast<unsigned char*>(lds + ((g - 1) & 1) * D_STAGE) + wave * (2 * 32 * R16);
#pragma unroll
                for (int a = 0; a < MT; ++a) {
                    const int y = cur.ty0 + MT * wave + a;
#pragma unroll
                    for (int pb = 0; pb < 2; ++pb) {
                        f32x4 v = H2 ? acc16[a][pb] * p.alpha + bias16 : acc16[a][pb] + bias16;
                        v = act_split4<ACT>(v);
                        if (p.nreal) {
#pragma unroll
                            for (int r = 0; r < 4; ++r) v[r] = 4 * kg16 + r < p.nreal ? v[r] : 0.f;
                        }
                        uint2 h, l;
                        split4_fmt<OF>(v, h, l, p.sat, [&] { return cur.img; });
                        if (4 * kg16 < p.Cout) {
                            *reinterpret_cast<uint2*>(s16 + (16 * pb + c16) * R16 + kg16 * 8) = h;
                            if constexpr (!O16) *reinterpret_cast<uint2*>(s16 + 32 * R16 + (16 * pb + c16) * R16 + kg16 * 8) = l;
                        }
                    }
                    __builtin_amdgcn_wave_barrier();
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    {   // 32 pixels x 2 segments of 8 channels = 64 lanes, one pass per plane
                        const int pix = lane >> 1, sg = lane & 1;
                        const u32x4 h = *reinterpret_cast<const u32x4*>(s16 + pix * R16 + sg * 16);
                        if (y < p.H && sg * 8 < p.Cout) {
                            uint16_t* o = oaddr((size_t)(cur.img * p.H + y) * p.W + cur.tx0 + pix, (size_t)p.H * p.W, sg);
                            *reinterpret_cast<u32x4*>(o) = h;
                            if constexpr (!O16) *reinterpret_cast<u32x4*>(o + p.out_plane) = *reinterpret_cast<const u32x4*>(s16 + 32 * R16 + pix * R16 + sg * 16);
                        }
                    }
                    __builtin_amdgcn_wave_barrier();
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                }
                return;
            }
            if (MT == 2 && p.pool) {
                // fused 2x2 max pool: vertical max across the wave's two rows (same lane), horizontal across lane pairs
                // (pixel = lane & 31), THEN bias + activation (monotonic) on a quarter of the values
                uint2 hh[4 * NB], ll[4 * NB];
#pragma unroll
                for (int r4 = 0; r4 < 4 * NB; ++r4) {
                    if (8 * r4 >= p.Cout) continue;
                    const int nb = r4 >> 2, q = r4 & 3;
                    f32x4 v;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float m = fmaxf(acc[0][nb][4 * q + r], acc[MT - 1][nb][4 * q + r]);
                        v[r] = fmaxf(m, __shfl_xor(m, 1));
                    }
                    if constexpr (H2) v = v * p.alpha + bias[r4]; else v += bias[r4];
                    v = act_split4<ACT>(v);
                    split4_fmt<OF>(v, hh[r4], ll[r4], p.sat, [&] { return cur.img; });
                }
                const int pp = frow >> 1;                    // pooled pixel of this lane pair
#pragma unroll
                for (int pl = 0; pl < 2; ++pl) {
                    if ((TWO || O16) && pl == 1) break;          // fp16 outputs: the hi plane only
                    if (!(lane & 1)) {
#pragma unroll
                        for (int r4 = 0; r4 < 4 * NB; ++r4) {
                            if (8 * r4 >= p.Cout) continue;
                            const int nl = 8 * r4 + 4 * fk;
                            if (TWO) {
                                *reinterpret_cast<uint2*>(sh + pp * ROW + nl * 2) = hh[r4];
                                if constexpr (!O16) *reinterpret_cast<uint2*>(sl + pp * ROW + nl * 2) = ll[r4];
                            } else {
                                *reinterpret_cast<uint2*>(sh + pp * ROW + nl * 2) = pl ? ll[r4] : hh[r4];
                            }
                        }
                    }
                    __builtin_amdgcn_wave_barrier();
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    const int yp = (cur.ty0 >> 1) + wave, Hp = p.H >> 1, Wp = p.W >> 1;
#pragma unroll
                    for (int ps = 0; ps < (16 + PPP - 1) / PPP; ++ps) {
                        const int pix = ps * PPP + prow;
                        if (pix < 16 && yp < Hp && seg * 8 < p.Cout) {
                            const u32x4 h = *reinterpret_cast<const u32x4*>(sh + pix * ROW + seg * 16);
                            uint16_t* o = oaddr((size_t)(cur.img * Hp + yp) * Wp + (cur.tx0 >> 1) + pix, (size_t)Hp * Wp, seg);
                            if (TWO) {
                                *reinterpret_cast<u32x4*>(o) = h;
                                if constexpr (!O16) *reinterpret_cast<u32x4*>(o + p.out_plane) = *reinterpret_cast<const u32x4*>(sl + pix * ROW + seg * 16);
                            } else {
                                *reinterpret_cast<u32x4*>(pl ? o + p.out_plane : o) = h;
                            }
                        }
                    }
                    __builtin_amdgcn_wave_barrier();
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                }
                return;
            }
#pragma unroll
            for (int a = 0; a < MT; ++a) {
                const int y = cur.ty0 + MT * wave + a;
                uint2 hh[4 * NB], ll[4 * NB];
#pragma unroll
                for (int r4 = 0; r4 < 4 * NB; ++r4) {
                    if (8 * r4 >= p.Cout) continue;         // rows past Cout are padding, never stored
                    const int nb = r4 >> 2, q = r4 & 3;
                    f32x4 v = {acc[a][nb][4 * q], acc[a][nb][4 * q + 1], acc[a][nb][4 * q + 2], acc[a][nb][4 * q + 3]};
                    if constexpr (H2) v = v * p.alpha + bias[r4]; else v += bias[r4];
                    v = act_split4<ACT>(v);
                    split4_fmt<OF>(v, hh[r4], ll[r4], p.sat, [&] { return cur.img; });
                }
#pragma unroll
                for (int pl = 0; pl < 2; ++pl) {
                    if ((TWO || O16) && pl == 1) break;          // fp16 outputs: the hi plane only
#pragma unroll
                    for (int r4 = 0; r4 < 4 * NB; ++r4) {
                        if (8 * r4 >= p.Cout) continue;
                        const int nl = 8 * r4 + 4 * fk;
                        if (TWO) {
                            *reinterpret_cast<uint2*>(sh + frow * ROW + nl * 2) = hh[r4];
                            if constexpr (!O16) *reinterpret_cast<uint2*>(sl + frow * ROW + nl * 2) = ll[r4];
                        } else {
                            *reinterpret_cast<uint2*>(sh + frow * ROW + nl * 2) = pl ? ll[r4] : hh[r4];
                        }
                    }
                    __builtin_amdgcn_wave_barrier();
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
                    for (int ps = 0; ps < 32 / PPP; ++ps) {
                        const int pix = ps * PPP + prow;
                        const u32x4 h = *reinterpret_cast<const u32x4*>(sh + pix * ROW + seg * 16);
                        u32x4 l = h;
                        if (TWO && !O16) l = *reinterpret_cast<const u32x4*>(sl + pix * ROW + seg * 16);
                        // FOLD: pixel pix of column group a = source (row 4 hh + 2 a + (pix >> 4), column pix & 15) of this wave's parity
                        const int yo = FOLD ? cur.ty0 + 2 * (4 * (wave >> 2) + 2 * a + (pix >> 4)) + ((wave & 3) >> 1) : y;
                        const int xo = FOLD ? cur.tx0 + 2 * (pix & 15) + (wave & 1) : cur.tx0 + pix;
                        if (yo < p.H && seg * 8 < p.Cout) {
                            uint16_t* o = oaddr((size_t)(cur.img * p.H + yo) * p.W + xo, (size_t)p.H * p.W, seg);
                            if (TWO) {
                                *reinterpret_cast<u32x4*>(o) = h;
                                if constexpr (!O16) *reinterpret_cast<u32x4*>(o + p.out_plane) = l;
                            } else {
                                *reinterpret_cast<u32x4*>(pl ? o + p.out_plane : o) = h;
                            }
                        }
                    }
                    __builtin_amdgcn_wave_barrier();
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                }
            }
        };
        auto ep = [&](auto tag) {
            if constexpr (H2) { epilogue(tag, IntTag<3>{}); return; }           // (an HS layer writes HS planes, nothing else)
            else {
                if constexpr (!N16) { if (p.out_fmt == PL_F16X2) { epilogue(tag, IntTag<2>{}); return; } }
                if (p.out_fmt != PL_BF16X2) epilogue(tag, IntTag<1>{}); else epilogue(tag, IntTag<0>{});      // (PL_F16)
            }
        };
        if (p.act == ACT_RELU) ep(ActTag<ACT_RELU>{});
        else if (p.act == ACT_ELU) ep(ActTag<ACT_ELU>{});
        else if (N16 && p.act == ACT_SIGMOID03) ep(ActTag<ACT_SIGMOID03>{});
        else ep(ActTag<ACT_NONE>{});
        if (tid + (int)gridDim.x < items) cur = tile_of(tid + gridDim.x);
    }
}

// v: the tile shape the form resolved (conv_form.cpp) -- 64-channel passes, <= 32 channels, or the 16-wide MFMA form; up: source-resolution halo tiles
hipError_t launch_conv_direct(const ConvDirectParams& p, DirectVariant v, hipStream_t s) {
    if ((p.act == ACT_SIGMOID03 || p.nreal) && !v.n16) return hipErrorInvalidValue;
    if (p.out_fmt == PL_F16X2 && p.Cout <= 16 && p.nsplit == 1 && !p.pool) return hipErrorInvalidValue;      // (the 16-wide form writes PL_BF16X2 and PL_F16)
    if (p.W % D_TW || p.Cout > 64 || p.Cout % 8 || p.nsplit < 1 || p.nsplit > 8 || (p.nsplit > 1 && p.Cout != 64)) return hipErrorInvalidValue;
    static int cus = 0;
    if (!cus) {
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return hipErrorInvalidDevice;
        cus = prop.multiProcessorCount;
    }
    ConvDirectParams q = p;
    if (p.pool && (p.rows_per_wave != 2 || (p.H & 1) || (p.W & 1))) return hipErrorInvalidValue;
    if (p.rows_per_wave != 2) return hipErrorInvalidValue;       // (8-row tiles of the 32/64-channel kernels were measured no better and are not built)
    // N16 layers (full-resolution decoder tail: two chunks of little arithmetic per tile) are bound by the DMA latency of
    // a two-stage ring: 8-row tiles, 64 KiB of LDS, TWO workgroups per CU cover each other's waits
    // every source behind a x2 upsample: source-resolution halo tiles (48 KiB of LDS for N16 with 16-row tiles: they stay)
    const auto [nb, n16, up, th] = v;
    const int tiles = (int)conv_direct_items(p.W, p.H, p.N, p.nsplit, th);
    // persistent grid: as many workgroups as the instantiation keeps resident (1-3 per CU, by LDS and registers)
#define SD_DIRECT_(NB_, MT_, F16_, N16_, UP_, W1_, X2_, ...) \
    do { static int per_cu = 0; \
         if (!per_cu && (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, conv_direct_kernel<NB_, MT_, F16_, N16_, UP_, W1_, X2_, ##__VA_ARGS__>, 512, 0) != hipSuccess || per_cu < 1)) per_cu = 1; \
         const int slots = (cus - p.reserve_cus > 0 ? cus - p.reserve_cus : 1) * per_cu; \
         const dim3 grid((unsigned)(tiles < slots ? tiles : slots)); \
         hipLaunchKernelGGL((conv_direct_kernel<NB_, MT_, F16_, N16_, UP_, W1_, X2_, ##__VA_ARGS__>), grid, dim3(512), 0, s, q); } while (0)
#define SD_DIRECT_H2(NB_) do { if (up) SD_DIRECT_(NB_, 2, true, false, true, false, true, true); else SD_DIRECT_(NB_, 2, true, false, false, false, true, true); } while (0)
// N16: 8-row tiles without an upsample, 16-row up-tiles behind one
#define SD_DIRECT_N16(F16_, W1_, ...) do { if (up) SD_DIRECT_(1, 2, F16_, true, true, W1_, ##__VA_ARGS__); else SD_DIRECT_(1, 1, F16_, true, false, W1_, ##__VA_ARGS__); } while (0)
    if (p.fold) {               // upsample-folded upconv layers of SD_PREC_F16X2: source-resolution tiles, 16 tap matrices per chunk
        if (p.scheme != SC_HS || p.out_fmt != PL_HS || !up || p.pool || n16) return hipErrorInvalidValue;
        if (nb == 1) SD_DIRECT_(1, 2, true, false, true, false, true, true, true); else SD_DIRECT_(2, 2, true, false, true, false, true, true, true);
        return hipGetLastError();
    }
#define SD_DIRECT(NB_, F16_, W1_) do { if (up) SD_DIRECT_(NB_, 2, F16_, false, true, W1_, false); else SD_DIRECT_(NB_, 2, F16_, false, false, W1_, false); } while (0)
    switch (p.scheme) {
        case SC_HS:             // every tile shape of the bf16 form
            if (p.out_fmt != PL_HS) return hipErrorInvalidValue;
            if (n16) SD_DIRECT_N16(true, false, true, true); else if (nb == 1) SD_DIRECT_H2(1); else SD_DIRECT_H2(2);
            break;
        case SC_F16XW:          // the 64-channel-pass form only (the planner asks for nothing else)
            if (n16 || nb == 1 || up) return hipErrorInvalidValue;
            SD_DIRECT_(2, 2, true, false, false, false, true);
            break;
        case SC_F16X1: if (n16) SD_DIRECT_N16(true, true, false); else if (nb == 1) SD_DIRECT(1, true, true); else SD_DIRECT(2, true, true); break;
        case SC_F16W: if (n16) SD_DIRECT_N16(true, false, false); else if (nb == 1) SD_DIRECT(1, true, false); else SD_DIRECT(2, true, false); break;
        case SC_BF16X2: if (n16) SD_DIRECT_N16(false, false, false); else if (nb == 1) SD_DIRECT(1, false, false); else SD_DIRECT(2, false, false); break;
        default: return hipErrorInvalidValue;
    }
#undef SD_DIRECT_N16
#undef SD_DIRECT_H2
#undef SD_DIRECT_
#undef SD_DIRECT
    return hipGetLastError();
}

// sd_set_small_batch level 2, the rule (semdepth.h sd_small_batch_split_direct): slices of the chunk axis of a layer with `items` work items in a FULL pass and
// `nchunks` 16-channel chunks on a chip of `cus` CUs.  Fixed by reasoning: a layer with items >= cus fills the chip; S is the smallest value with items * S >= cus,
// at most 16, and a slice keeps at least 4 chunks (36 MFMA groups per product plane: below it the two-stage ring's prologue dominates).  Measured
// (profiles/latency_b1_direct.json): a layer is admitted when 2 * items <= cus, and above a quarter of the chip (4 * items > cus, where S = 2) only
// with at least 16 chunks -- the two half-filled layers with 4-5 chunks per slice (conv2_2 of a 256 x 512 frame, iconv3 of a 512 x 1024 one) gained nothing, conv4_x with
// 8-16 per slice did
int conv_splitc_slices(long items, int nchunks, int cus) {
    if (items <= 0 || nchunks <= 0 || cus <= 0 || items >= cus || 2 * items > cus || (4 * items > cus && nchunks < 16)) return 1;
    long S = (cus + items - 1) / items;
    if (S > 16) S = 16;
    if (S > nchunks / 4) S = nchunks / 4;
    return S < 2 ? 1 : (int)S;
}

// the chunk-range form of the 64-channel-pass HS kernel: the same persistent grid rule over (tile, slice, pass) items
hipError_t launch_conv_direct_splitc(const ConvDirectParams& p, hipStream_t s) {
    if (p.scheme != SC_HS || p.out_fmt != PL_HS || p.Cout != 64 || p.nsplit < 1 || p.nsplit > 8 || p.W % D_TW || p.rows_per_wave != 2 || p.fold || p.nreal ||
        (p.all_up && !(p.H & 1) && !(p.W & 1)) || (p.pool && ((p.H & 1) || (p.W & 1))) || p.csplit < 2 || p.csplit > 16 || p.nchunks / p.csplit < 1 || !p.partial)
        return hipErrorInvalidValue;
    static int cus = 0, per_cu = 0;
    if (!cus) {
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return hipErrorInvalidDevice;
        cus = prop.multiProcessorCount;
    }
    auto* const kern = conv_direct_kernel<2, 2, true, false, false, false, true, true, false, true>;
    if (!per_cu && (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, 512, 0) != hipSuccess || per_cu < 1)) per_cu = 1;
    const long items = conv_direct_items(p.W, p.H, p.N, p.nsplit) * p.csplit;
    const long slots = (long)(cus - p.reserve_cus > 0 ? cus - p.reserve_cus : 1) * per_cu;
    hipLaunchKernelGGL(kern, dim3((unsigned)(items < slots ? items : slots)), dim3(512), 0, s, p);
    return hipGetLastError();
}

}  // namespace sd
