// Second half of a split-K GEMM of the three-product engine (SD_PREC_F16X2, sd_set_small_batch): the k-range form of conv_dma3.hip's HS ring leaves
// the raw f32 accumulators of slice s in partial[s][M][Cout]; this kernel adds the S partials of an output value in ASCENDING slice order (f32, no
// atomics: the sum is a fixed chain, the same bits on every run and for every call size) and applies the epilogue of conv_dma3's HS path with the
// same helpers -- v * alpha + bias, act_split4<ACT>, split4_hs with the clamp counter and its per-image attribution -- before it writes the hi and
// the scaled-lo plane as 16-byte runs.  A lane owns 8 consecutive channels of one pixel (32 contiguous bytes per slice, a wave 2 KB): the kernel
// is HBM-bound on the partials (fc6 at S = 8: 67 MB).
#include "kernels.hpp"
#include "split_fmt.hpp"

namespace sd {

typedef float rf32x4 __attribute__((ext_vector_type(4)));
typedef unsigned ru32x4 __attribute__((ext_vector_type(4)));

template <int ACT>
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const ConvParams p, int M) {
    const int c8 = p.Cout >> 3;
    const long item = (long)blockIdx.x * 256 + threadIdx.x;
    if (item >= (long)M * c8) return;
    const int row = (int)(item / c8), ch = (int)(item - (long)row * c8) * 8;
    const size_t o = (size_t)row * p.Cout + ch, slice = (size_t)M * p.Cout;
    const float* __restrict__ part = p.partial + o;
    rf32x4 a = *reinterpret_cast<const rf32x4*>(part), b = *reinterpret_cast<const rf32x4*>(part + 4);
#pragma unroll 4
    for (int s = 1; s < p.ksplit; ++s) {
        a += *reinterpret_cast<const rf32x4*>(part + (size_t)s * slice);
        b += *reinterpret_cast<const rf32x4*>(part + (size_t)s * slice + 4);
    }
    a = a * p.alpha + *reinterpret_cast<const rf32x4*>(p.bias + ch);
    b = b * p.alpha + *reinterpret_cast<const rf32x4*>(p.bias + ch + 4);
    a = act_split4<ACT>(a);
    b = act_split4<ACT>(b);
    uint2 ha, la, hb, lb;
    split4_hs(a, ha, la, p.sat, [&] { return sat_img_of_row<true>(p, row); });
    split4_hs(b, hb, lb, p.sat, [&] { return sat_img_of_row<true>(p, row); });
    uint16_t* const out = reinterpret_cast<uint16_t*>(p.out) + o;
    *reinterpret_cast<ru32x4*>(out) = ru32x4{ha.x, ha.y, hb.x, hb.y};
    *reinterpret_cast<ru32x4*>(out + p.out_plane) = ru32x4{la.x, la.y, lb.x, lb.y};
}

hipError_t launch_splitk_reduce(const ConvParams& p, hipStream_t s) {
    if (p.scheme != SC_HS || p.ksplit < 2 || !p.partial || p.Cout % 8 || p.rowgrp || p.fold || p.pool || p.out_planar16 || p.residual) return hipErrorInvalidValue;
    const long M = (long)p.N * p.Hout * p.Wout, items = M * (p.Cout >> 3);
    const dim3 grid((unsigned)((items + 255) / 256));
    if (p.act == ACT_RELU) hipLaunchKernelGGL((splitk_reduce_kernel<ACT_RELU>), grid, dim3(256), 0, s, p, (int)M);
    else if (p.act == ACT_ELU) hipLaunchKernelGGL((splitk_reduce_kernel<ACT_ELU>), grid, dim3(256), 0, s, p, (int)M);
    else hipLaunchKernelGGL((splitk_reduce_kernel<ACT_NONE>), grid, dim3(256), 0, s, p, (int)M);
    return hipGetLastError();
}

// Second half of a chunk-split 3x3 direct conv (sd_set_small_batch level 2): conv_direct.hip's chunk-range form leaves the raw f32 accumulators of slice s in
// partial[s][img * H * W + y * W + x][Cstride] at CONV resolution.  A lane owns 8 channels of one OUTPUT pixel: it adds the S partials of a conv pixel in ascending
// slice order and then applies the value sequence of the direct kernel's H2 epilogue -- POOL: the max over the 2x2 window as the fused-pool epilogue takes it (the
// vertical max of the left column, then of the right column, then the two); v * alpha + bias; act_split4<ACT>; split4_hs with the clamp counter and the image of
// the output row -- and writes 16-byte runs of the hi and the scaled-lo plane (NHWC or 16-channel sub-planes, whichever the consumers read).  HBM/L2-bound on the partials (conv4_x of a 512 x 1024 frame, S = 2: 33 MB).
template <int ACT, bool POOL>
__global__ __launch_bounds__(256) void splitc_reduce_kernel(const ConvDirectParams p, int M) {
    const int c8 = p.Cstride >> 3;
    const long item = (long)blockIdx.x * 256 + threadIdx.x;
    if (item >= (long)M * c8) return;
    const int row = (int)(item / c8), ch = (int)(item - (long)row * c8) * 8;
    const size_t slice = (size_t)p.N * p.H * p.W * p.Cstride;
    auto sum = [&](size_t px, rf32x4& a, rf32x4& b) {         // conv pixel px: the S partials in ascending order
        const float* __restrict__ part = p.partial + px * p.Cstride + ch;
        a = *reinterpret_cast<const rf32x4*>(part); b = *reinterpret_cast<const rf32x4*>(part + 4);
#pragma unroll 4
        for (int s = 1; s < p.csplit; ++s) {
            a += *reinterpret_cast<const rf32x4*>(part + (size_t)s * slice);
            b += *reinterpret_cast<const rf32x4*>(part + (size_t)s * slice + 4);
        }
    };
    rf32x4 a, b;
    if constexpr (POOL) {
        const int Wp = p.W >> 1, Hp = p.H >> 1;
        const int xp = row % Wp, q = row / Wp, yp = q % Hp, img = q / Hp;
        const size_t px = ((size_t)img * p.H + 2 * yp) * p.W + 2 * xp;
        rf32x4 a1, b1, a2, b2, a3, b3;
        sum(px, a, b); sum(px + p.W, a1, b1); sum(px + 1, a2, b2); sum(px + p.W + 1, a3, b3);
        a = __builtin_elementwise_max(__builtin_elementwise_max(a, a1), __builtin_elementwise_max(a2, a3));
        b = __builtin_elementwise_max(__builtin_elementwise_max(b, b1), __builtin_elementwise_max(b2, b3));
    } else {
        sum((size_t)row, a, b);
    }
    a = a * p.alpha + *reinterpret_cast<const rf32x4*>(p.bias + ch);
    b = b * p.alpha + *reinterpret_cast<const rf32x4*>(p.bias + ch + 4);
    a = act_split4<ACT>(a);
    b = act_split4<ACT>(b);
    uint2 ha, la, hb, lb;
    auto img_of = [&] { return row / ((p.H >> (POOL ? 1 : 0)) * (p.W >> (POOL ? 1 : 0))); };
    split4_hs(a, ha, la, p.sat, img_of);
    split4_hs(b, hb, lb, p.sat, img_of);
    // NHWC, or (out_planar16) 16-channel sub-planes [C / 16][Nmax * Hout * Wout][16]: the direct epilogue's oaddr
    const size_t npix = (size_t)(p.H >> (POOL ? 1 : 0)) * (p.W >> (POOL ? 1 : 0));
    uint16_t* const out = reinterpret_cast<uint16_t*>(p.out) +
                          (p.out_planar16 ? ((size_t)(ch >> 4) * p.Nmax * npix + row) * 16 + (ch & 8) : (size_t)row * p.Cstride + ch);
    *reinterpret_cast<ru32x4*>(out) = ru32x4{ha.x, ha.y, hb.x, hb.y};
    *reinterpret_cast<ru32x4*>(out + p.out_plane) = ru32x4{la.x, la.y, lb.x, lb.y};
}

hipError_t launch_splitc_reduce(const ConvDirectParams& p, hipStream_t s) {
    if (p.scheme != SC_HS || p.out_fmt != PL_HS || p.csplit < 2 || !p.partial || p.Cstride % 8 || p.Cout * p.nsplit != p.Cstride || p.fold || p.nreal || (p.out_planar16 && p.Cstride % 16) ||
        (p.pool && ((p.H & 1) || (p.W & 1))))
        return hipErrorInvalidValue;
    const long M = (long)p.N * (p.H >> p.pool) * (p.W >> p.pool), items = M * (p.Cstride >> 3);
    const dim3 grid((unsigned)((items + 255) / 256));
#define SD_SPLITC_REDUCE(ACT_) do { if (p.pool) hipLaunchKernelGGL((splitc_reduce_kernel<ACT_, true>), grid, dim3(256), 0, s, p, (int)M); \
                                    else hipLaunchKernelGGL((splitc_reduce_kernel<ACT_, false>), grid, dim3(256), 0, s, p, (int)M); } while (0)
    if (p.act == ACT_RELU) SD_SPLITC_REDUCE(ACT_RELU);
    else if (p.act == ACT_ELU) SD_SPLITC_REDUCE(ACT_ELU);
    else SD_SPLITC_REDUCE(ACT_NONE);
#undef SD_SPLITC_REDUCE
    return hipGetLastError();
}

}  // namespace sd
