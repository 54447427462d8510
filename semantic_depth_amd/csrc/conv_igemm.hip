// Implicit-GEMM convolution for gfx950 on the exact-f32 MFMA (v_mfma_f32_16x16x4_f32).
//
//   out[m][n] = act( bias[n] + residual[m][n] + sum_k X[m][k] * Wt[k][n] )
//   m = (image, oy, ox) output pixel, n = output channel, k = (tap, source, channel) in tf.concat / HWIO order.
//
// Covers every dense conv of the two networks:
//   * kh x kw in {1,3,5,7}, stride 1 or 2, explicit zero pad (TF SAME for odd k stride 1 == monodepth's pad+VALID)
//   * up to three channel-concatenated sources, each optionally read through a x2 nearest-neighbour upsample
//     (monodepth upconv = upsample_nn + conv; concat[upconv, skip, udisp]) — nothing is materialised
//   * epilogue: + bias, + residual (resnet shortcut), ReLU / ELU
//
// Tiling (256 threads = 4 waves of 64):
//   block tile BM pixels x BN channels x BK=32; wave tile (MT*16) x (NT*16) built from 16x16x4 MFMAs.
//   The weight fragment is the MFMA A operand (rows = channels), the activation fragment the B operand
//   (cols = pixels), so a lane ends up with 4 consecutive channels of one pixel -> one 16-byte NHWC store.
//   LDS images are [k/4][row][4] floats: a wave's ds_read_b128 of 16 rows x 4 k-quads is bank-conflict free
//   and one read feeds four MFMAs (k is walked in the permuted order 16g + 4*kk + j, same for both operands).
//   Global->register prefetch of tile t+1 is issued before the MFMAs of tile t; 2-3 blocks per CU overlap
//   each other's barriers.  f32 MFMA rate is 1/16 of bf16, so LDS/L2 traffic is far from binding here.
#include "kernels.hpp"

namespace sd {

typedef float f32x4 __attribute__((ext_vector_type(4)));


template <int WAVES_M, int WAVES_N, int MT, int NT>
struct Tile {
    static constexpr int BM = WAVES_M * MT * 16;
    static constexpr int BN = WAVES_N * NT * 16;
    static constexpr int A_LD = BM / 32;                   // float4 loads per thread per k-tile (activations)
    static constexpr int B_LD = (BN * 8 + 255) / 256;      // float4 loads per thread per k-tile (weights)
    static constexpr int LDS_FLOATS = (BM + BN) * 32;
};

template <int WAVES_M, int WAVES_N, int MT, int NT, bool VEC>
__global__ __launch_bounds__(256) void conv_igemm_kernel(const ConvParams p, int M, int tilesM, int tilesN) {
    using T = Tile<WAVES_M, WAVES_N, MT, NT>;
    constexpr int BM = T::BM, BN = T::BN;
    __shared__ __attribute__((aligned(16))) float lds[T::LDS_FLOATS];
    float* As = lds;              // [8][BM][4]
    float* Bs = lds + BM * 32;    // [8][BN][4]

    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = t >> 6;
    const int wm0 = (wave % WAVES_M) * (MT * 16);
    const int wn0 = (wave / WAVES_M) * (NT * 16);

    // XCD-aware tile order: hardware places block b on XCD b % 8; give every XCD a contiguous run of tile ids so that
    // neighbouring pixel tiles (shared halo rows) and the blocks sharing a weight panel meet in the same L2
    int tid_;
    {
        const int nwg = tilesM * tilesN, bid = blockIdx.x, xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
        tid_ = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
    }
    int tm, tn;
    if (p.m_fastest) { tm = tid_ % tilesM; tn = tid_ / tilesM; }
    else             { tn = tid_ % tilesN; tm = tid_ / tilesN; }
    const int bm0 = tm * BM, bn0 = tn * BN;

    // the one output pixel this thread gathers for
    const int m_l = t % BM;
    const int kq0 = t / BM;                 // 0 (BM=256) or 0/1 (BM=128)
    constexpr int KQ_STEP = 256 / BM;       // 1 or 2
    const int m = bm0 + m_l;
    const bool m_ok = m < M;
    int img, oy, ox;
    {
        const int hw = p.Hout * p.Wout;
        const int mm = m_ok ? m : 0;
        img = mm / hw;
        const int r = mm - img * hw;
        oy = r / p.Wout;
        ox = r - oy * p.Wout;
    }

    const float* const wt = p.wt;
    const KEntry* __restrict__ const ktab = p.ktab;
    const int CoutPad = p.CoutPad;

    f32x4 ra[T::A_LD];
    f32x4 rb[T::B_LD];
    const int ktiles = p.Kpad / 32, vtiles = p.vtiles;

    auto load_tile = [&](int kt) {
        // ---- weights: contiguous [kq][n][4] panel ----
#pragma unroll
        for (int i = 0; i < T::B_LD; ++i) {
            const int idx = t + 256 * i;
            const int n_l = idx % BN, kq = idx / BN;
            if (BN * 8 >= 256 || idx < BN * 8)
                rb[i] = *reinterpret_cast<const f32x4*>(wt + ((size_t)(kt * 8 + kq) * CoutPad + bn0 + n_l) * 4);
        }
        // ---- activations: im2col gather ----
        if (VEC || kt < vtiles) {
            const KEntry e = ktab[kt];   // wave-uniform -> one s_load_dwordx8
            // vec tile: 32 consecutive channels of one tap of one source
            const int st = (e.flags >> 4) & 3, up = e.flags & 1;       // per-source stride / x2 upsample
            int iy = oy * st + e.dy, ix = ox * st + e.dx;
            const bool ok = (e.flags & 0x10000) && m_ok && iy >= 0 && ix >= 0 && iy < (e.H << up) && ix < (e.W << up);
            iy >>= up; ix >>= up;
            const float* base = e.base + ((size_t)(img * e.H + iy) * e.W + ix) * e.C;
#pragma unroll
            for (int i = 0; i < T::A_LD; ++i) {
                const int kq = kq0 + KQ_STEP * i;
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (ok) v = *reinterpret_cast<const f32x4*>(base + kq * 4);
                ra[i] = v;
            }
        } else {
            // quad tile: 8 descriptors, each <= 4 consecutive channels of one (tap, source); kq is wave-uniform, so each
            // descriptor is one scalar load and the descriptors of a tile are independent of each other
            const KEntry* __restrict__ const qtab = ktab + ktiles + (kt - vtiles) * 8;   // this tile's 8 quad descriptors
#pragma unroll
            for (int i = 0; i < T::A_LD; ++i) {
                const int kq = __builtin_amdgcn_readfirstlane(kq0 + KQ_STEP * i);
                const KEntry q4 = qtab[kq];
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                const int st = (q4.flags >> 4) & 3, up = q4.flags & 1;
                int iy = oy * st + q4.dy, ix = ox * st + q4.dx;
                const bool ok = (q4.flags & 0x10000) && m_ok && iy >= 0 && ix >= 0 && iy < (q4.H << up) && ix < (q4.W << up);
                iy >>= up; ix >>= up;
                const int nv = (q4.flags >> 8) & 7;
                const float* q = q4.base + ((size_t)(img * q4.H + iy) * q4.W + ix) * q4.C;
                if (ok) {
                    if (nv == 4) v = *reinterpret_cast<const f32x4*>(q);
                    else if (nv == 2) { const float2 t2 = *reinterpret_cast<const float2*>(q); v[0] = t2.x; v[1] = t2.y; }
                    else { for (int j = 0; j < nv; ++j) v[j] = q[j]; }
                }
                ra[i] = v;
            }
        }
    };

    f32x4 acc[MT][NT];
#pragma unroll
    for (int a = 0; a < MT; ++a)
#pragma unroll
        for (int b = 0; b < NT; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};

    load_tile(0);
    const int frow = lane & 15, fk = lane >> 4;
    for (int kt = 0; kt < ktiles; ++kt) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < T::A_LD; ++i) {
            const int kq = kq0 + KQ_STEP * i;
            *reinterpret_cast<f32x4*>(As + (kq * BM + m_l) * 4) = ra[i];
        }
#pragma unroll
        for (int i = 0; i < T::B_LD; ++i) {
            const int idx = t + 256 * i;
            if (BN * 8 >= 256 || idx < BN * 8) *reinterpret_cast<f32x4*>(Bs + idx * 4) = rb[i];
        }
        __syncthreads();
        if (kt + 1 < ktiles) load_tile(kt + 1);
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            f32x4 wf[NT], xf[MT];
#pragma unroll
            for (int b = 0; b < NT; ++b)
                wf[b] = *reinterpret_cast<const f32x4*>(Bs + ((4 * g + fk) * BN + wn0 + b * 16 + frow) * 4);
#pragma unroll
            for (int a = 0; a < MT; ++a)
                xf[a] = *reinterpret_cast<const f32x4*>(As + ((4 * g + fk) * BM + wm0 + a * 16 + frow) * 4);
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int b = 0; b < NT; ++b)
#pragma unroll
                    for (int a = 0; a < MT; ++a)
                        acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[b][j], xf[a][j], acc[a][b], 0, 0, 0);
        }
    }

    // ---- epilogue: D[row = channel (lane>>4)*4 + r][col = pixel lane&15] ----
    auto epilogue = [&](auto tag) {
        constexpr int ACT = decltype(tag)::value;
#pragma unroll
        for (int b = 0; b < NT; ++b) {
            const int n = bn0 + wn0 + b * 16 + (lane >> 4) * 4;
            if (n >= p.Cout) continue;
            const f32x4 bi = *reinterpret_cast<const f32x4*>(p.bias + n);
#pragma unroll
            for (int a = 0; a < MT; ++a) {
                const int mo = bm0 + wm0 + a * 16 + (lane & 15);
                if (mo >= M) continue;
                f32x4 v = acc[a][b] + bi;
                const size_t o = (size_t)mo * p.Cout + n;
                if (p.residual) v += *reinterpret_cast<const f32x4*>(p.residual + o);
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = act_f32<ACT>(v[r]);
                *reinterpret_cast<f32x4*>(p.out + o) = v;
            }
        }
    };
    if (p.act == ACT_RELU) epilogue(ActTag<ACT_RELU>{});
    else if (p.act == ACT_ELU) epilogue(ActTag<ACT_ELU>{});
    else epilogue(ActTag<ACT_NONE>{});
}

template <int WAVES_M, int WAVES_N, int MT, int NT>
static hipError_t launch_cfg(const ConvParams& p, hipStream_t s) {
    using T = Tile<WAVES_M, WAVES_N, MT, NT>;
    const long M = (long)p.N * p.Hout * p.Wout;
    const int tilesM = (int)((M + T::BM - 1) / T::BM);
    const int tilesN = (p.Cout + T::BN - 1) / T::BN;
    dim3 grid((unsigned)(tilesM * tilesN));
    if (p.vec)
        hipLaunchKernelGGL((conv_igemm_kernel<WAVES_M, WAVES_N, MT, NT, true>), grid, dim3(256), 0, s, p, (int)M, tilesM, tilesN);
    else
        hipLaunchKernelGGL((conv_igemm_kernel<WAVES_M, WAVES_N, MT, NT, false>), grid, dim3(256), 0, s, p, (int)M, tilesM, tilesN);
    return hipGetLastError();
}

// tile choice is a function of Cout only, so the planner can size CoutPad without seeing the kernel
int conv_tile_n(int Cout) {
    if (Cout % 128 == 0) return 128;
    if (Cout % 64 == 0) return 64;
    if (Cout % 32 == 0) return 32;
    return 16;
}

hipError_t launch_conv_igemm(const ConvParams& p, hipStream_t s) {
    switch (conv_tile_n(p.Cout)) {
        case 128: return launch_cfg<2, 2, 4, 4>(p, s);   // 128 x 128
        case 64:  return launch_cfg<4, 1, 4, 4>(p, s);   // 256 x 64
        case 32:  return launch_cfg<4, 1, 4, 2>(p, s);   // 256 x 32
        default:  return launch_cfg<4, 1, 4, 1>(p, s);   // 256 x 16
    }
}

}  // namespace sd
