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

}  // namespace sd
