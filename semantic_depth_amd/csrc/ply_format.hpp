// The coder of the device PLY route (sd_ply_format_rw / sd_ply_format_rw_host; contract: include/semdepth.h), stated ONCE for the kernels
// of ply_gpu.hip and the host function of host_ply.cpp: "%f" of a double in integer arithmetic, "%d" of a colour, the vertex row, the
// header, the 1001 points of the road-width line and which row of a frame is which point.  Both sides call these functions, so they agree
// on every digit; what differs is only who walks the rows (one loop on the host, one lane per row on the device).  The text is that of
// outputs.rw_ply_bytes (point_cloud_2_ply.py's header and "%f %f %f %d %d %d" rows behind its minimum-z filter).
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include <stddef.h>
#include <stdint.h>

#include "arena.hpp"

#if defined(__HIPCC__)
#define SDPLY_HD __host__ __device__ inline
#else
#define SDPLY_HD inline
#endif

namespace sdply {

constexpr int kRowCap = 69;          // "-2147483648.000000" three times, three blanks, "255" three times, two blanks, the newline
constexpr int kLineRows = 1001;      // create_3Dline_from_3Dpoints: the left end, then left + t * v for t = 0, 0.001, ... 0.999
constexpr int kBlockRows = 256;      // rows one workgroup formats

#define SDPLY_PRE "ply\n    format ascii 1.0\n    element vertex "
#define SDPLY_SUF                                                                                                                     \
    "\n    property float x\n    property float y\n    property float z\n    property uchar red\n    property uchar green\n"          \
    "    property uchar blue\n    end_header\n    "
constexpr int kPreLen = (int)sizeof(SDPLY_PRE) - 1, kSufLen = (int)sizeof(SDPLY_SUF) - 1;
constexpr int kHeaderCap = kPreLen + 10 + kSufLen;      // a vertex count has at most 10 digits

SDPLY_HD size_t blocks_per_frame(int cap) { return ((size_t)cap + kLineRows + kBlockRows - 1) / kBlockRows; }
SDPLY_HD size_t frame_bound(int cap) { return (size_t)kHeaderCap + ((size_t)cap + kLineRows) * kRowCap; }

SDPLY_HD uint64_t dbits(double v) {
    uint64_t u;
    __builtin_memcpy(&u, &v, 8);
    return u;
}
// finite and |v| < 2^31: what the device formats (anything else sends the frame to the host route)
SDPLY_HD bool in_range(double v) { return (dbits(v) & 0x7fffffffffffffffull) < 0x41E0000000000000ull; }

SDPLY_HD int u32_digits(uint32_t v) {
    return 1 + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) + (v >= 1000000u) + (v >= 10000000u) +
           (v >= 100000000u) + (v >= 1000000000u);
}
SDPLY_HD int put_u32(uint8_t* p, uint32_t v) {
    const int d = u32_digits(v);
    for (int i = d - 1; i >= 0; --i) {
        p[i] = (uint8_t)('0' + v % 10u);
        v /= 10u;
    }
    return d;
}

// "%f" of an in_range double: the sign bit, the integer part and the six decimals, rounded half-even on the exact binary value.
// fixed_dec is the same for any number of decimals up to six (unit = 10^decimals): "%.2f" of text_draw.hpp is fixed_dec(v, 100).
struct Fixed {
    uint32_t ip, frac, neg;
};
SDPLY_HD Fixed fixed_dec(double v, uint32_t unit) {
    const uint64_t u = dbits(v);
    Fixed f;
    f.neg = (uint32_t)(u >> 63);
    f.ip = 0;
    f.frac = 0;
    const int e = (int)((u >> 52) & 0x7ff);
    if (e == 0) return f;                                // zero, or below 2^-1022
    const uint64_t mant = (u & ((1ull << 52) - 1)) | (1ull << 52);
    const int k = 1075 - e;                              // |v| = mant * 2^-k; in_range: k >= 22
    if (k >= 74) return f;                               // mant * unit <= mant * 10^6 < 2^73 <= 2^(k-1): below half a unit of the last decimal
    uint64_t mf = mant;
    if (k <= 52) {
        f.ip = (uint32_t)(mant >> k);
        mf = mant & ((1ull << k) - 1);
    }
    const unsigned __int128 one = 1;
    const unsigned __int128 p = (unsigned __int128)mf * unit;            // < 2^73
    uint32_t q = (uint32_t)(p >> k);                                     // <= unit - 1 (k <= 52) or <= 1 (k >= 53 ... 73)
    const unsigned __int128 rem = p & ((one << k) - 1), half = one << (k - 1);
    if (rem > half || (rem == half && (q & 1u))) ++q;
    if (q == unit) {                                     // the carry out of the fraction
        q = 0;
        ++f.ip;
    }
    f.frac = q;
    return f;
}
SDPLY_HD Fixed fixed6(double v) { return fixed_dec(v, 1000000u); }
SDPLY_HD int fixed_len(const Fixed& f) { return (int)f.neg + u32_digits(f.ip) + 7; }
SDPLY_HD int put_fixed(uint8_t* p, const Fixed& f) {
    int n = 0;
    if (f.neg) p[n++] = '-';
    n += put_u32(p + n, f.ip);
    p[n++] = '.';
    uint32_t q = f.frac;
    for (int i = 5; i >= 0; --i) {
        p[n + i] = (uint8_t)('0' + q % 10u);
        q /= 10u;
    }
    return n + 6;
}

// one vertex row "x y z r g b\n"
struct Row {
    Fixed c[3];
    uint8_t rgb[3];
};
SDPLY_HD Row make_row(const double* p, const uint8_t* rgb) {
    Row r;
    for (int j = 0; j < 3; ++j) {
        r.c[j] = fixed6(p[j]);
        r.rgb[j] = rgb[j];
    }
    return r;
}
SDPLY_HD int row_len(const Row& r) {
    return fixed_len(r.c[0]) + fixed_len(r.c[1]) + fixed_len(r.c[2]) + u32_digits(r.rgb[0]) + u32_digits(r.rgb[1]) + u32_digits(r.rgb[2]) + 6;
}
SDPLY_HD int put_row(uint8_t* p, const Row& r) {
    int n = 0;
    for (int j = 0; j < 3; ++j) {
        n += put_fixed(p + n, r.c[j]);
        p[n++] = ' ';
    }
    for (int j = 0; j < 3; ++j) {
        n += put_u32(p + n, r.rgb[j]);
        p[n++] = j == 2 ? '\n' : ' ';
    }
    return n;
}

// PointCloud2Ply.ply_header.format(vertex_count=count)
SDPLY_HD int header_len(uint32_t count) { return kPreLen + u32_digits(count) + kSufLen; }
SDPLY_HD uint8_t header_byte(int i, uint32_t count) {
    if (i < kPreLen) return (uint8_t)SDPLY_PRE[i];
    const int d = u32_digits(count);
    if (i < kPreLen + d) {
        for (int j = kPreLen + d - 1; j > i; --j) count /= 10u;
        return (uint8_t)('0' + count % 10u);
    }
    return (uint8_t)SDPLY_SUF[i - kPreLen - d];
}

// the road-width line of a found frame (pcl.create_3Dline_from_3Dpoints on the record's end points widened to double): both ends are
// lifted by 0.01 in y, v = right - left; row 0 is the left end, row 1 + i is left + (i * 0.001) * v -- a product, then a sum, each rounded
struct Line {
    double l[3], v[3];
};
SDPLY_HD Line make_line(const float* left, const float* right) {
#pragma clang fp contract(off)
    Line ln;
    for (int j = 0; j < 3; ++j) {
        double a = (double)left[j], b = (double)right[j];
        if (j == 1) {
            a += 0.01;
            b += 0.01;
        }
        ln.l[j] = a;
        ln.v[j] = b - a;
    }
    return ln;
}
SDPLY_HD void line_point(const Line& ln, int row, double* out) {
#pragma clang fp contract(off)
    if (row == 0) {
        for (int j = 0; j < 3; ++j) out[j] = ln.l[j];
        return;
    }
    const double t = (double)(row - 1) * 0.001;
    for (int j = 0; j < 3; ++j) {
        const double tv = t * ln.v[j];
        out[j] = ln.l[j] + tv;
    }
}

// one frame as the rows of rw_ply_bytes before its filter: the n cloud points, then the line when the record has one.  A row is kept iff
// its z is above the minimum z of all rows (strictly: every row at the minimum goes).
struct Frame {
    const float* xyz;        // f32 [n,3]
    const uint8_t* rgb;      // u8 [n,3]
    int n, rows, found;
    Line line;
    bool bad;                // n outside 0..cap, or an end point that is not in_range
};
SDPLY_HD Frame make_frame(const float* xyz, const uint8_t* rgb, int n, int cap, const float* left, const float* right, int found) {
    Frame f;
    f.xyz = xyz;
    f.rgb = rgb;
    f.found = found != 0;
    f.bad = n < 0 || n > cap;
    f.n = f.bad ? 0 : n;
    f.rows = f.n + (f.found ? kLineRows : 0);
    for (int j = 0; j < 3; ++j) f.line.l[j] = f.line.v[j] = 0.0;
    if (f.found) {
        for (int j = 0; j < 3; ++j) f.bad = f.bad || !in_range((double)left[j]) || !in_range((double)right[j]);
        f.line = make_line(left, right);
    }
    return f;
}
SDPLY_HD void row_point(const Frame& f, int r, double* p, uint8_t* c) {
    if (r < f.n) {
        for (int j = 0; j < 3; ++j) {
            p[j] = (double)f.xyz[3 * (size_t)r + j];
            c[j] = f.rgb[3 * (size_t)r + j];
        }
        return;
    }
    line_point(f.line, r - f.n, p);
    c[0] = 250;
    c[1] = 0;
    c[2] = 0;
}

// ---- workspace of the device route (ply_gpu.hip): the declarations are the walk; packed, every region ends on a multiple of the next one's alignment
struct Layout : sdarena::Walker {
    size_t nb, B;       // row blocks of all frames (nblk = blocks_per_frame(cap) each), frames
    Layout(int B_, int cap) : nb((size_t)B_ * blocks_per_frame(cap)), B((size_t)B_) {}
    size_t bmin = take(nb * 8, 8);       // f64 [B][nblk], 8-byte aligned: per row block the minimum z of its rows
    size_t boff = take(nb * 8, 8);       // u64 [B][nblk], 8: the block's offset inside the frame's rows
    size_t zmin = take(B * 8, 8);        // f64 [B], 8: the frame's minimum z
    size_t fbase = take(B * 8, 8);       // u64 [B], 8: where the frame's rows begin in the text
    size_t blen = take(nb * 4, 4);       // u32 [B][nblk], 4: the block's bytes
    size_t bcnt = take(nb * 4, 4);       // u32 [B][nblk], 4: its kept rows
    size_t bbad = take(nb * 4, 4);       // u32 [B][nblk], 4: its range verdict
    size_t slack = end();                // 64 bytes of historical slack: nothing reads or writes them
    size_t total = end_with_slack(64);
};

}  // namespace sdply
