// The test mode's input stage and its score, stated once for host and device (contract: include/semdepth.h).
//
// fcn8s/fcn.py:408,412 resize the frame AND the label image with scipy.misc.imresize(img, image_shape), which for uint8 input is
// PIL.Image.resize((W, H), BILINEAR): Pillow's ImagingResample for 8-bit images with the bilinear filter (support 1).  Along one axis
// with `in` source and `out` destination samples:
//   scale = in / out (double), fs = max(scale, 1), support = fs, center = (d + 0.5) * scale
//   xmin = max((int)(center - support + 0.5), 0), xmax = min((int)(center + support + 0.5), in), n = xmax - xmin
//   w_i = max(0, 1 - |(i + xmin - center + 0.5) * (1 / fs)|), normalised by their sum in double      (i = 0 .. n-1)
//   k_i = (int)(0.5 + w_i * 2^22)                                                                     (bilinear: no negative weight)
//   out = clip_u8((2^21 + sum k_i * src[xmin + i]) >> 22)
// horizontal pass, then vertical pass, WITH the uint8 rounding between them; channels are independent.  An axis whose size does not change
// has the windows {2^22} / {2^22, 0}: passing through it is the copy Pillow makes by skipping it.
// The windows are made on the host in double (pil_windows below); a kernel that recomputed them in float would not reproduce the integers.
// Everything behind the windows is integer arithmetic, the same on host and device: no -ffp-contract question arises.
//
// The score: helper.prepare_ground_truth (:149-177) is a 256-entry table label id -> class (road 0, fence 1, everything else 2), and
// tf.metrics.mean_iou's state is the 3 x 3 count matrix [label class][predicted class].  seg_cell names the counter a pixel adds to.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "arena.hpp"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SDPIL_HD __host__ __device__
#else
#define SDPIL_HD
#endif

namespace sdpil {

constexpr int kPrecisionBits = 22;           // Pillow's PRECISION_BITS = 32 - 8 - 2
constexpr int kMaxExtent = 16384;            // largest source / destination extent
constexpr int kMaxFactor = 32;               // largest downscale factor per axis
constexpr int kMaxTaps = 2 * kMaxFactor + 1; // window of the largest factor: 65 taps
constexpr int kCells = 10;                   // counters per frame: the 3 x 3 matrix and the predictions above 2

// windows of one axis: bounds[2 d] = xmin, bounds[2 d + 1] = n; k[i * out + d] = k_i of window d (tap-major: the lanes of a wave take
// neighbouring windows), zero beyond a window's n.  taps = the longest window.
struct Windows {
    int in = 0, out = 0, taps = 0;
    std::vector<int32_t> bounds, k;
};

inline bool axis_ok(int in, int out) {
    return in >= 1 && out >= 1 && in <= kMaxExtent && out <= kMaxExtent && (long long)in <= (long long)out * kMaxFactor;
}

inline void pil_windows(int in, int out, Windows& w) {
    const double scale = (double)in / (double)out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = 1.0 * fs;          // bilinear: support 1
    const double ss = 1.0 / fs;
    std::vector<double> pre;
    std::vector<int32_t> kk;                  // window-major while the longest window is not known
    w.in = in;
    w.out = out;
    w.taps = 0;
    w.bounds.assign((size_t)out * 2, 0);
    std::vector<size_t> first((size_t)out);
    for (int d = 0; d < out; ++d) {
        const double center = (d + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in) xmax = in;
        const int n = xmax - xmin;
        pre.assign((size_t)n, 0.0);
        double ww = 0.0;
        for (int i = 0; i < n; ++i) {
            double x = (i + xmin - center + 0.5) * ss;
            if (x < 0.0) x = -x;
            const double wi = x < 1.0 ? 1.0 - x : 0.0;
            pre[(size_t)i] = wi;
            ww += wi;
        }
        first[(size_t)d] = kk.size();
        for (int i = 0; i < n; ++i) {
            const double wi = ww != 0.0 ? pre[(size_t)i] / ww : pre[(size_t)i];
            kk.push_back((int32_t)(0.5 + wi * (double)(1 << kPrecisionBits)));
        }
        w.bounds[(size_t)d * 2] = xmin;
        w.bounds[(size_t)d * 2 + 1] = n;
        if (n > w.taps) w.taps = n;
    }
    w.k.assign((size_t)w.taps * out, 0);
    for (int d = 0; d < out; ++d)
        for (int i = 0; i < w.bounds[(size_t)d * 2 + 1]; ++i) w.k[(size_t)i * out + d] = kk[first[(size_t)d] + i];
}

SDPIL_HD inline uint8_t clip_u8(int32_t acc) {
    const int32_t v = acc >> kPrecisionBits;
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}
constexpr int32_t kHalf = 1 << (kPrecisionBits - 1);

// the counter a pixel adds to: cell 3 * class(label) + prediction, or cell 9 for a prediction that names no class
SDPIL_HD inline int seg_cell(int table_class, int pred) { return pred > 2 ? 9 : table_class * 3 + pred; }

// the longest window an axis can have, without making the windows: 2 * support + 1 rounded up
inline int taps_bound(int in, int out) {
    const long long f = in > out ? ((long long)in + out - 1) / out : 1;
    return (int)(2 * f + 1);
}
inline size_t mid_pitch(int dst_w, int channels) { return ((size_t)dst_w * channels + 3) / 4 * 4; }     // dword rows for the vertical pass

// ---- workspace of the device route (seg_eval_gpu.hip); every part 16-byte aligned
struct Layout : sdarena::Walker {
    size_t B, sh, sw, dh, dw, pitch;
    Layout(int B_, int src_h, int src_w, int dst_h, int dst_w, int channels)
        : B((size_t)B_), sh((size_t)src_h), sw((size_t)src_w), dh((size_t)dst_h), dw((size_t)dst_w), pitch(mid_pitch(dst_w, channels)) {}
    size_t x_bounds = take(dw * 2 * 4, 16);                               // i32 [dst_w][2]: first source sample and length of every x window
    size_t x_k = take(taps_bound((int)sw, (int)dw) * dw * 4, 16);         // i32 [dst_w][taps_bound(src_w, dst_w)]: their weights
    size_t y_bounds = take(dh * 2 * 4, 16);                               // i32 [dst_h][2]
    size_t y_k = take(taps_bound((int)sh, (int)dh) * dh * 4, 16);         // i32 [dst_h][taps_bound(src_h, dst_h)]
    size_t mid = take(B * sh * pitch, 16);                                // u8 [B][src_h][mid_pitch]: the horizontal pass's rows, read by the vertical pass
    size_t total = end(16);
};
inline size_t workspace_bytes(int B, int src_h, int src_w, int dst_h, int dst_w, int channels) { return Layout(B, src_h, src_w, dst_h, dst_w, channels).total; }

}  // namespace sdpil
