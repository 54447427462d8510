// The text of the result images (sd_text_draw_rw / sd_text_draw_host; contract: include/semdepth.h), stated ONCE for the kernels of
// text_gpu.hip and the host functions of host_text.cpp: the stroke font, "%.2f" of a double, the strings and origins of the sequence tool's
// banner (outputs.overlay_items_sequence) and the rule that says which pixels a stroke paints.  Both sides call these functions, so they
// agree on every pixel; what differs is only who walks the pixels.  cv2.putText's own glyphs (OpenCV's Hershey tables) are not reproduced.
//
// Font: an upright sans stroke font CONSTRUCTED by scripts/make_text_font.py -- straight strokes between grid points chosen there and arcs
// of ellipses sampled by formula and rounded to the grid; the table below is that script's output (a test compares them) and takes no
// vertex list from any other font.  Only the metrics the reference's layout was made for are kept: integer unit grid, baseline y = 0, y up,
// cap height 21, x-height 14, descenders to -7, every vertex inside [0, advance] x [-7, 21], advance <= 24, at most 32 straight segments
// per glyph.  Glyphs: space, 0-9, A-Z, a-z and . , : ; ' - + / ( ) % =; every other byte draws the box glyph.
//
// Raster rule, in exact integers of 1/256 pixel: the vertex (ux, uy) of the glyph at pen position p (the sum of the advances before it)
// sits at X = org.x * 256 + (p + ux) * scale_q8, Y = org.y * 256 - uy * scale_q8; pixel (px, py) has its centre at (px * 256, py * 256)
// and is painted iff its squared distance to some segment AB of the item is <= r^2, r = thickness * 128.  With d = B - A and w = P - A:
// w.d <= 0 -> |w|^2 <= r^2;  w.d >= |d|^2 -> |P - B|^2 <= r^2;  otherwise (w x d)^2 <= r^2 |d|^2.  A degenerate segment is a disc.
// Magnitudes under the caps below (extents <= 16384, |org| <= 32768, scale_q8 <= 4096, thickness <= 32, text <= 64 bytes):
// |vertex| <= 2^23 + 64 * 24 * 4096 < 2^24, pixel centre < 2^22, so |w| < 2^25 per axis; |d| <= 28 * 4096 < 2^17 per axis; hence
// |w.d| and |w x d| < 2^43 and |w|^2 < 2^51 fit an int64, r^2 |d|^2 < 2^24 * 2^35 = 2^59, and (w x d)^2 < 2^86 takes the 128-bit product.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include <stddef.h>
#include <stdint.h>

#include "../../include/semdepth.h"
#include "ply_format.hpp"

#if defined(__HIPCC__)
#define SDTEXT_HD __host__ __device__ inline
#else
#define SDTEXT_HD inline
#endif

namespace sdtext {

constexpr int kMaxBytes = SD_TEXT_MAX_BYTES, kMaxSegs = SD_TEXT_MAX_SEGS, kMaxItems = SD_TEXT_MAX_ITEMS;
constexpr int kMaxScaleQ8 = SD_TEXT_MAX_SCALE_Q8, kMaxThickness = SD_TEXT_MAX_THICKNESS, kMaxOrg = SD_TEXT_MAX_ORG, kMaxExtent = 16384;
constexpr int kMaxAdvance = 24, kAscent = 21, kDescent = 7;
constexpr int kMaxDepthBytes = 23;       // "Cannot compute width of road at " + depth + " m depth:" is then at most 64 bytes

struct Glyph {
    uint16_t first;      // its first row of kSeg
    uint8_t n, adv;      // segments, advance in units
};
// a segment is {x0, y0, x1, y1} in units
// BEGIN font table (scripts/make_text_font.py)
constexpr int kSegCount = 585, kGlyphCount = 76;
constexpr int8_t kSeg[kSegCount][4] = {
    // the box of every other byte
    {2, 0, 12, 0}, {12, 0, 12, 21}, {12, 21, 2, 21}, {2, 21, 2, 0},
    // space
    // %
    {18, 21, 4, 0}, {6, 21, 9, 20}, {9, 20, 10, 16}, {10, 16, 9, 12}, {9, 12, 6, 11}, {6, 11, 3, 12}, {3, 12, 2, 16}, {2, 16, 3, 20},
    {3, 20, 6, 21}, {16, 10, 19, 9}, {19, 9, 20, 5}, {20, 5, 19, 1}, {19, 1, 16, 0}, {16, 0, 13, 1}, {13, 1, 12, 5}, {12, 5, 13, 9},
    {13, 9, 16, 10},
    // '
    {4, 21, 3, 15},
    // (
    {8, 21, 6, 17}, {6, 17, 4, 13}, {4, 13, 4, 7}, {4, 7, 4, 1}, {4, 1, 6, -3}, {6, -3, 8, -7},
    // )
    {2, 21, 4, 17}, {4, 17, 6, 13}, {6, 13, 6, 7}, {6, 7, 6, 1}, {6, 1, 4, -3}, {4, -3, 2, -7},
    // +
    {9, 15, 9, 1}, {2, 8, 16, 8},
    // ,
    {3, 0, 5, 0}, {5, 0, 5, 2}, {5, 2, 3, 2}, {3, 2, 3, 0}, {5, 0, 4, -3}, {4, -3, 3, -4},
    // -
    {2, 8, 12, 8},
    // .
    {3, 0, 5, 0}, {5, 0, 5, 2}, {5, 2, 3, 2}, {3, 2, 3, 0},
    // /
    {12, 21, 2, -4},
    // 0
    {9, 21, 11, 20}, {11, 20, 13, 18}, {13, 18, 15, 15}, {15, 15, 15, 11}, {15, 11, 15, 6}, {15, 6, 13, 3}, {13, 3, 11, 1}, {11, 1, 9, 0},
    {9, 0, 7, 1}, {7, 1, 5, 3}, {5, 3, 3, 6}, {3, 6, 3, 10}, {3, 10, 3, 15}, {3, 15, 5, 18}, {5, 18, 7, 20}, {7, 20, 9, 21},
    // 1
    {5, 16, 9, 21}, {9, 21, 9, 0},
    // 2
    {3, 17, 5, 20}, {5, 20, 8, 21}, {8, 21, 11, 21}, {11, 21, 13, 19}, {13, 19, 15, 16}, {15, 16, 15, 13}, {15, 13, 13, 11}, {13, 11, 3, 0},
    {3, 0, 15, 0},
    // 3
    {5, 19, 7, 21}, {7, 21, 11, 21}, {11, 21, 13, 19}, {13, 19, 14, 15}, {14, 15, 12, 12}, {12, 12, 9, 11}, {9, 11, 9, 11}, {9, 11, 12, 10},
    {12, 10, 15, 8}, {15, 8, 15, 4}, {15, 4, 13, 1}, {13, 1, 10, 0}, {10, 0, 6, 1}, {6, 1, 4, 3},
    // 4
    {12, 0, 12, 21}, {12, 21, 2, 6}, {2, 6, 16, 6},
    // 5
    {14, 21, 5, 21}, {5, 21, 4, 12}, {4, 12, 4, 11}, {4, 11, 8, 13}, {8, 13, 11, 13}, {11, 13, 14, 10}, {14, 10, 15, 6}, {15, 6, 14, 2},
    {14, 2, 10, 0}, {10, 0, 7, 1}, {7, 1, 4, 3},
    // 6
    {3, 7, 4, 10}, {4, 10, 6, 12}, {6, 12, 9, 13}, {9, 13, 12, 12}, {12, 12, 14, 10}, {14, 10, 15, 7}, {15, 7, 14, 3}, {14, 3, 12, 1},
    {12, 1, 9, 0}, {9, 0, 6, 1}, {6, 1, 4, 3}, {4, 3, 3, 6}, {3, 6, 3, 8}, {3, 8, 4, 13}, {4, 13, 5, 17}, {5, 17, 8, 20},
    {8, 20, 11, 21}, {11, 21, 14, 20},
    // 7
    {3, 21, 15, 21}, {15, 21, 7, 0},
    // 8
    {9, 21, 12, 20}, {12, 20, 13, 19}, {13, 19, 14, 16}, {14, 16, 13, 14}, {13, 14, 12, 12}, {12, 12, 9, 11}, {9, 11, 7, 12}, {7, 12, 5, 14},
    {5, 14, 4, 16}, {4, 16, 5, 19}, {5, 19, 6, 20}, {6, 20, 9, 21}, {9, 11, 12, 10}, {12, 10, 14, 8}, {14, 8, 15, 6}, {15, 6, 14, 3},
    {14, 3, 12, 1}, {12, 1, 9, 0}, {9, 0, 6, 1}, {6, 1, 4, 3}, {4, 3, 3, 5}, {3, 5, 4, 8}, {4, 8, 6, 10}, {6, 10, 9, 11},
    // 9
    {15, 14, 14, 11}, {14, 11, 12, 9}, {12, 9, 9, 8}, {9, 8, 6, 9}, {6, 9, 4, 11}, {4, 11, 3, 14}, {3, 14, 4, 18}, {4, 18, 6, 20},
    {6, 20, 9, 21}, {9, 21, 12, 20}, {12, 20, 14, 18}, {14, 18, 15, 15}, {15, 15, 15, 13}, {15, 13, 14, 8}, {14, 8, 13, 4}, {13, 4, 10, 1},
    {10, 1, 7, 0}, {7, 0, 4, 1},
    // :
    {3, 0, 5, 0}, {5, 0, 5, 2}, {5, 2, 3, 2}, {3, 2, 3, 0}, {3, 10, 5, 10}, {5, 10, 5, 12}, {5, 12, 3, 12}, {3, 12, 3, 10},
    // ;
    {3, 0, 5, 0}, {5, 0, 5, 2}, {5, 2, 3, 2}, {3, 2, 3, 0}, {5, 0, 4, -3}, {4, -3, 3, -4}, {3, 10, 5, 10}, {5, 10, 5, 12},
    {5, 12, 3, 12}, {3, 12, 3, 10},
    // =
    {2, 11, 16, 11}, {2, 5, 16, 5},
    // A
    {2, 0, 9, 21}, {9, 21, 16, 0}, {4, 6, 14, 6},
    // B
    {3, 0, 3, 21}, {3, 21, 9, 21}, {9, 21, 12, 20}, {12, 20, 13, 19}, {13, 19, 14, 16}, {14, 16, 13, 14}, {13, 14, 12, 12}, {12, 12, 9, 11},
    {9, 11, 3, 11}, {10, 11, 13, 10}, {13, 10, 15, 8}, {15, 8, 16, 6}, {16, 6, 15, 3}, {15, 3, 13, 1}, {13, 1, 10, 0}, {10, 0, 3, 0},
    // C
    {15, 19, 13, 20}, {13, 20, 10, 21}, {10, 21, 7, 20}, {7, 20, 5, 18}, {5, 18, 4, 14}, {4, 14, 3, 11}, {3, 11, 4, 7}, {4, 7, 5, 3},
    {5, 3, 7, 1}, {7, 1, 10, 0}, {10, 0, 13, 1}, {13, 1, 15, 2},
    // D
    {3, 0, 3, 21}, {3, 21, 8, 21}, {8, 21, 11, 20}, {11, 20, 13, 19}, {13, 19, 15, 17}, {15, 17, 17, 14}, {17, 14, 17, 11}, {17, 11, 17, 7},
    {17, 7, 15, 4}, {15, 4, 13, 2}, {13, 2, 11, 1}, {11, 1, 8, 0}, {8, 0, 3, 0},
    // E
    {3, 0, 3, 21}, {3, 21, 14, 21}, {3, 11, 12, 11}, {3, 0, 14, 0},
    // F
    {3, 0, 3, 21}, {3, 21, 14, 21}, {3, 11, 11, 11},
    // G
    {15, 19, 13, 20}, {13, 20, 10, 21}, {10, 21, 7, 20}, {7, 20, 5, 17}, {5, 17, 3, 14}, {3, 14, 3, 10}, {3, 10, 4, 6}, {4, 6, 5, 3},
    {5, 3, 8, 1}, {8, 1, 11, 0}, {11, 0, 13, 1}, {13, 1, 16, 3}, {16, 3, 17, 7}, {17, 7, 18, 10}, {18, 10, 12, 11},
    // H
    {3, 0, 3, 21}, {17, 0, 17, 21}, {3, 11, 17, 11},
    // I
    {3, 0, 3, 21},
    // J
    {10, 21, 10, 6}, {10, 6, 9, 3}, {9, 3, 8, 1}, {8, 1, 6, 0}, {6, 0, 4, 1}, {4, 1, 3, 3}, {3, 3, 2, 6},
    // K
    {3, 0, 3, 21}, {16, 21, 3, 8}, {7, 12, 16, 0},
    // L
    {3, 21, 3, 0}, {3, 0, 13, 0},
    // M
    {3, 0, 3, 21}, {3, 21, 11, 4}, {11, 4, 19, 21}, {19, 21, 19, 0},
    // N
    {3, 0, 3, 21}, {3, 21, 17, 0}, {17, 0, 17, 21},
    // O
    {11, 21, 13, 20}, {13, 20, 16, 18}, {16, 18, 17, 15}, {17, 15, 18, 11}, {18, 11, 17, 6}, {17, 6, 16, 3}, {16, 3, 13, 1}, {13, 1, 11, 0},
    {11, 0, 8, 1}, {8, 1, 5, 3}, {5, 3, 4, 6}, {4, 6, 3, 10}, {3, 10, 4, 15}, {4, 15, 5, 18}, {5, 18, 8, 20}, {8, 20, 10, 21},
    // P
    {3, 0, 3, 21}, {3, 21, 9, 21}, {9, 21, 12, 20}, {12, 20, 14, 18}, {14, 18, 15, 16}, {15, 16, 14, 13}, {14, 13, 12, 11}, {12, 11, 9, 10},
    {9, 10, 3, 10},
    // Q
    {11, 21, 13, 20}, {13, 20, 16, 18}, {16, 18, 17, 15}, {17, 15, 18, 11}, {18, 11, 17, 6}, {17, 6, 16, 3}, {16, 3, 13, 1}, {13, 1, 11, 0},
    {11, 0, 8, 1}, {8, 1, 5, 3}, {5, 3, 4, 6}, {4, 6, 3, 10}, {3, 10, 4, 15}, {4, 15, 5, 18}, {5, 18, 8, 20}, {8, 20, 10, 21},
    {12, 5, 19, -2},
    // R
    {3, 0, 3, 21}, {3, 21, 9, 21}, {9, 21, 12, 20}, {12, 20, 14, 18}, {14, 18, 15, 16}, {15, 16, 14, 13}, {14, 13, 12, 11}, {12, 11, 9, 10},
    {9, 10, 3, 10}, {9, 10, 16, 0},
    // S
    {14, 18, 12, 20}, {12, 20, 8, 21}, {8, 21, 5, 20}, {5, 20, 3, 17}, {3, 17, 3, 13}, {3, 13, 6, 11}, {6, 11, 9, 10}, {9, 10, 9, 10},
    {9, 10, 13, 9}, {13, 9, 15, 7}, {15, 7, 15, 4}, {15, 4, 13, 1}, {13, 1, 10, 0}, {10, 0, 6, 0}, {6, 0, 3, 3},
    // T
    {8, 0, 8, 21}, {1, 21, 15, 21},
    // U
    {3, 21, 3, 7}, {3, 7, 4, 4}, {4, 4, 5, 2}, {5, 2, 7, 1}, {7, 1, 10, 0}, {10, 0, 13, 1}, {13, 1, 15, 2}, {15, 2, 16, 4},
    {16, 4, 17, 7}, {17, 7, 17, 21},
    // V
    {2, 21, 9, 0}, {9, 0, 16, 21},
    // W
    {2, 21, 7, 0}, {7, 0, 12, 17}, {12, 17, 17, 0}, {17, 0, 22, 21},
    // X
    {3, 21, 15, 0}, {15, 21, 3, 0},
    // Y
    {2, 21, 9, 10}, {9, 10, 9, 0}, {16, 21, 9, 10},
    // Z
    {3, 21, 15, 21}, {15, 21, 3, 0}, {3, 0, 15, 0},
    // a
    {13, 14, 13, 0}, {13, 7, 12, 4}, {12, 4, 11, 1}, {11, 1, 8, 0}, {8, 0, 6, 1}, {6, 1, 4, 4}, {4, 4, 3, 7}, {3, 7, 4, 11},
    {4, 11, 5, 13}, {5, 13, 8, 14}, {8, 14, 11, 13}, {11, 13, 12, 11}, {12, 11, 13, 7},
    // b
    {3, 21, 3, 0}, {13, 7, 12, 4}, {12, 4, 11, 1}, {11, 1, 8, 0}, {8, 0, 6, 1}, {6, 1, 4, 4}, {4, 4, 3, 7}, {3, 7, 4, 11},
    {4, 11, 5, 13}, {5, 13, 8, 14}, {8, 14, 11, 13}, {11, 13, 12, 11}, {12, 11, 13, 7},
    // c
    {12, 12, 9, 14}, {9, 14, 7, 14}, {7, 14, 4, 12}, {4, 12, 3, 9}, {3, 9, 3, 5}, {3, 5, 4, 2}, {4, 2, 7, 0}, {7, 0, 9, 0},
    {9, 0, 12, 2},
    // d
    {13, 21, 13, 0}, {13, 7, 12, 4}, {12, 4, 11, 1}, {11, 1, 8, 0}, {8, 0, 6, 1}, {6, 1, 4, 4}, {4, 4, 3, 7}, {3, 7, 4, 11},
    {4, 11, 5, 13}, {5, 13, 8, 14}, {8, 14, 11, 13}, {11, 13, 12, 11}, {12, 11, 13, 7},
    // e
    {3, 7, 13, 7}, {13, 7, 12, 10}, {12, 10, 11, 13}, {11, 13, 8, 14}, {8, 14, 6, 13}, {6, 13, 4, 11}, {4, 11, 3, 8}, {3, 8, 3, 4},
    {3, 4, 5, 1}, {5, 1, 7, 0}, {7, 0, 10, 0}, {10, 0, 12, 3},
    // f
    {9, 21, 6, 21}, {6, 21, 5, 19}, {5, 19, 4, 17}, {4, 17, 4, 0}, {1, 14, 8, 14},
    // g
    {13, 14, 13, -2}, {13, -2, 12, -4}, {12, -4, 11, -6}, {11, -6, 8, -7}, {8, -7, 6, -6}, {6, -6, 4, -4}, {13, 7, 12, 4}, {12, 4, 11, 1},
    {11, 1, 8, 0}, {8, 0, 6, 1}, {6, 1, 4, 4}, {4, 4, 3, 7}, {3, 7, 4, 11}, {4, 11, 5, 13}, {5, 13, 8, 14}, {8, 14, 11, 13},
    {11, 13, 12, 11}, {12, 11, 13, 7},
    // h
    {3, 21, 3, 0}, {3, 9, 3, 9}, {3, 9, 4, 12}, {4, 12, 6, 13}, {6, 13, 8, 14}, {8, 14, 11, 13}, {11, 13, 12, 12}, {12, 12, 13, 9},
    {13, 9, 13, 0},
    // i
    {3, 20, 3, 21}, {3, 14, 3, 0},
    // j
    {5, 20, 5, 21}, {5, 14, 5, -3}, {5, -3, 5, -5}, {5, -5, 4, -6}, {4, -6, 2, -7},
    // k
    {3, 21, 3, 0}, {12, 14, 3, 5}, {6, 8, 13, 0},
    // l
    {3, 21, 3, 3}, {3, 3, 3, 1}, {3, 1, 4, 0}, {4, 0, 6, 0},
    // m
    {3, 14, 3, 0}, {3, 10, 3, 10}, {3, 10, 4, 12}, {4, 12, 6, 14}, {6, 14, 8, 14}, {8, 14, 10, 12}, {10, 12, 11, 10}, {11, 10, 11, 0},
    {11, 10, 11, 10}, {11, 10, 12, 12}, {12, 12, 14, 14}, {14, 14, 16, 14}, {16, 14, 18, 12}, {18, 12, 19, 10}, {19, 10, 19, 0},
    // n
    {3, 14, 3, 0}, {3, 9, 3, 9}, {3, 9, 4, 12}, {4, 12, 6, 13}, {6, 13, 8, 14}, {8, 14, 11, 13}, {11, 13, 12, 12}, {12, 12, 13, 9},
    {13, 9, 13, 0},
    // o
    {8, 14, 10, 13}, {10, 13, 12, 11}, {12, 11, 13, 9}, {13, 9, 13, 5}, {13, 5, 12, 3}, {12, 3, 10, 1}, {10, 1, 8, 0}, {8, 0, 6, 1},
    {6, 1, 4, 3}, {4, 3, 3, 5}, {3, 5, 3, 9}, {3, 9, 4, 11}, {4, 11, 6, 13}, {6, 13, 8, 14},
    // p
    {3, 14, 3, -7}, {13, 7, 12, 4}, {12, 4, 11, 1}, {11, 1, 8, 0}, {8, 0, 6, 1}, {6, 1, 4, 4}, {4, 4, 3, 7}, {3, 7, 4, 11},
    {4, 11, 5, 13}, {5, 13, 8, 14}, {8, 14, 11, 13}, {11, 13, 12, 11}, {12, 11, 13, 7},
    // q
    {13, 14, 13, -7}, {13, 7, 12, 4}, {12, 4, 11, 1}, {11, 1, 8, 0}, {8, 0, 6, 1}, {6, 1, 4, 4}, {4, 4, 3, 7}, {3, 7, 4, 11},
    {4, 11, 5, 13}, {5, 13, 8, 14}, {8, 14, 11, 13}, {11, 13, 12, 11}, {12, 11, 13, 7},
    // r
    {3, 14, 3, 0}, {3, 9, 3, 9}, {3, 9, 4, 12}, {4, 12, 6, 13}, {6, 13, 8, 14}, {8, 14, 11, 13},
    // s
    {10, 12, 8, 14}, {8, 14, 6, 14}, {6, 14, 4, 12}, {4, 12, 3, 10}, {3, 10, 4, 8}, {4, 8, 7, 7}, {7, 7, 7, 7}, {7, 7, 10, 6},
    {10, 6, 11, 4}, {11, 4, 10, 2}, {10, 2, 8, 0}, {8, 0, 6, 0}, {6, 0, 4, 2},
    // t
    {4, 20, 4, 3}, {4, 3, 4, 1}, {4, 1, 5, 0}, {5, 0, 7, 0}, {1, 14, 8, 14},
    // u
    {3, 14, 3, 5}, {3, 5, 4, 2}, {4, 2, 5, 1}, {5, 1, 8, 0}, {8, 0, 11, 1}, {11, 1, 12, 2}, {12, 2, 13, 5}, {13, 14, 13, 0},
    // v
    {2, 14, 7, 0}, {7, 0, 12, 14},
    // w
    {2, 14, 6, 0}, {6, 0, 10, 12}, {10, 12, 14, 0}, {14, 0, 18, 14},
    // x
    {2, 14, 12, 0}, {12, 14, 2, 0},
    // y
    {2, 14, 7, 0}, {12, 14, 7, 0}, {7, 0, 5, -5}, {5, -5, 3, -7}, {3, -7, 2, -7},
    // z
    {2, 14, 12, 14}, {12, 14, 2, 0}, {2, 0, 12, 0},
};
constexpr Glyph kGlyph[kGlyphCount] = {
    {0, 4, 14}, {4, 0, 12}, {4, 17, 22}, {21, 1, 6}, {22, 6, 10}, {28, 6, 10}, {34, 2, 18}, {36, 6, 8},
    {42, 1, 14}, {43, 4, 8}, {47, 1, 14}, {48, 16, 18}, {64, 2, 18}, {66, 9, 18}, {75, 14, 18}, {89, 3, 18},
    {92, 11, 18}, {103, 18, 18}, {121, 2, 18}, {123, 24, 18}, {147, 18, 18}, {165, 8, 8}, {173, 10, 8}, {183, 2, 18},
    {185, 3, 18}, {188, 16, 19}, {204, 12, 20}, {216, 13, 20}, {229, 4, 17}, {233, 3, 16}, {236, 15, 21}, {251, 3, 20},
    {254, 1, 6}, {255, 7, 14}, {262, 3, 18}, {265, 2, 15}, {267, 4, 22}, {271, 3, 20}, {274, 16, 21}, {290, 9, 18},
    {299, 17, 21}, {316, 10, 18}, {326, 15, 18}, {341, 2, 16}, {343, 10, 20}, {353, 2, 18}, {355, 4, 24}, {359, 2, 18},
    {361, 3, 18}, {364, 3, 18}, {367, 13, 16}, {380, 13, 16}, {393, 9, 15}, {402, 13, 16}, {415, 12, 16}, {427, 5, 10},
    {432, 18, 16}, {450, 9, 16}, {459, 2, 6}, {461, 5, 8}, {466, 3, 15}, {469, 4, 8}, {473, 15, 22}, {488, 9, 16},
    {497, 14, 16}, {511, 13, 16}, {524, 13, 16}, {537, 6, 11}, {543, 13, 14}, {556, 5, 10}, {561, 8, 16}, {569, 2, 14},
    {571, 4, 20}, {575, 2, 14}, {577, 5, 14}, {582, 3, 14},
};
constexpr uint8_t kIndex[128] = {
    0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
    0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
    1, 0, 0, 0, 0, 2, 0, 3, 4, 5, 0, 6, 7, 8, 9, 10,
    11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 0, 23, 0, 0,
    0, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34, 35, 36, 37, 38,
    39, 40, 41, 42, 43, 44, 45, 46, 47, 48, 49, 0, 0, 0, 0, 0,
    0, 50, 51, 52, 53, 54, 55, 56, 57, 58, 59, 60, 61, 62, 63, 64,
    65, 66, 67, 68, 69, 70, 71, 72, 73, 74, 75, 0, 0, 0, 0, 0,
};
// END font table
SDTEXT_HD Glyph glyph_of(unsigned code) { return kGlyph[code < 128u ? kIndex[code] : 0]; }

SDTEXT_HD bool item_ok(const sd_text_item& it) {
    return it.len >= 0 && it.len <= kMaxBytes && it.scale_q8 >= 1 && it.scale_q8 <= kMaxScaleQ8 && it.thickness >= 1 && it.thickness <= kMaxThickness &&
           it.org_x >= -kMaxOrg && it.org_x <= kMaxOrg && it.org_y >= -kMaxOrg && it.org_y <= kMaxOrg;
}

// a segment of the glyph at pen position `pen`, in 1/256 pixel
struct Seg {
    int32_t ax, ay, bx, by;
};
SDTEXT_HD Seg seg_at(const sd_text_item& it, int pen, int row) {
    Seg s;
    s.ax = it.org_x * 256 + (pen + kSeg[row][0]) * it.scale_q8;
    s.ay = it.org_y * 256 - kSeg[row][1] * it.scale_q8;
    s.bx = it.org_x * 256 + (pen + kSeg[row][2]) * it.scale_q8;
    s.by = it.org_y * 256 - kSeg[row][3] * it.scale_q8;
    return s;
}
// the rule: is the centre of pixel (px, py) within r of the segment?
SDTEXT_HD bool hit(const Seg& s, int px, int py, int r) {
    const int64_t dx = (int64_t)s.bx - s.ax, dy = (int64_t)s.by - s.ay;
    const int64_t wx = (int64_t)px * 256 - s.ax, wy = (int64_t)py * 256 - s.ay;
    const int64_t r2 = (int64_t)r * r, t = wx * dx + wy * dy, dd = dx * dx + dy * dy;
    if (t <= 0) return wx * wx + wy * wy <= r2;
    if (t >= dd) {
        const int64_t vx = wx - dx, vy = wy - dy;
        return vx * vx + vy * vy <= r2;
    }
    const int64_t c = wx * dy - wy * dx;
    const uint64_t ca = (uint64_t)(c < 0 ? -c : c);
    return (unsigned __int128)ca * ca <= (unsigned __int128)(uint64_t)r2 * (uint64_t)dd;
}

SDTEXT_HD int floor256(int v) { return v >= 0 ? v / 256 : -((-v + 255) / 256); }
SDTEXT_HD int ceil256(int v) { return -floor256(-v); }
// the pixels [x0, x1] x [y0, y1] outside which an item of `units` advance units paints nothing, clipped to the h x w frame (empty: x0 > x1 or y0 > y1)
SDTEXT_HD void item_box(const sd_text_item& it, int units, int h, int w, int* box) {
    const int r = it.thickness * 128, ox = it.org_x * 256, oy = it.org_y * 256;
    const int x0 = ceil256(ox - r), x1 = floor256(ox + units * it.scale_q8 + r);
    const int y0 = ceil256(oy - kAscent * it.scale_q8 - r), y1 = floor256(oy + kDescent * it.scale_q8 + r);
    box[0] = x0 < 0 ? 0 : x0;
    box[1] = y0 < 0 ? 0 : y0;
    box[2] = x1 > w - 1 ? w - 1 : x1;
    box[3] = y1 > h - 1 ? h - 1 : y1;
}

// "{:.2f}".format(v): nan whatever the sign, inf / -inf, else the sign whenever the sign bit is set, the integer part and two decimals
// rounded half-even on the exact binary value (ply_format.hpp's routine at two decimals).  A finite |v| >= 2^31 prints as inf / -inf
// (the one deviation from Python).  At most 14 bytes.
SDTEXT_HD int put_fixed2(uint8_t* p, double v) {
    const uint64_t u = sdply::dbits(v);
    int n = 0;
    if ((u & 0x7fffffffffffffffull) > 0x7ff0000000000000ull) {
        p[0] = 'n'; p[1] = 'a'; p[2] = 'n';
        return 3;
    }
    if (u >> 63) p[n++] = '-';
    if (!sdply::in_range(v)) {
        p[n] = 'i'; p[n + 1] = 'n'; p[n + 2] = 'f';
        return n + 3;
    }
    const sdply::Fixed f = sdply::fixed_dec(v, 100u);
    n += sdply::put_u32(p + n, f.ip);
    p[n++] = '.';
    p[n++] = (uint8_t)('0' + f.frac / 10u);
    p[n++] = (uint8_t)('0' + f.frac % 10u);
    return n;
}

// ---- the sequence tool's layout (outputs.overlay_items_sequence) ----
constexpr int kSeqScaleQ8 = 512, kSeqScaleBigQ8 = 563, kSeqThickness = 2;      // fontScale 2 and lround(2.2 * 256); the largest the device route draws

SDTEXT_HD int put_str(uint8_t* p, const char* s) {
    int n = 0;
    while (s[n]) {
        p[n] = (uint8_t)s[n];
        ++n;
    }
    return n;
}
SDTEXT_HD int put_bytes(uint8_t* p, const uint8_t* s, int len) {
    for (int i = 0; i < len; ++i) p[i] = s[i];
    return len;
}
// origin (int(fx * w), int(fy * h)) as Python computes it: the product in doubles, then truncated
struct Colour {
    uint8_t b, g, r;
};
SDTEXT_HD void seq_head(sd_text_item& it, double fx, double fy, int h, int w, int scale_q8, Colour c) {
    it.org_x = (int32_t)(fx * (double)w);
    it.org_y = (int32_t)(fy * (double)h);
    it.scale_q8 = scale_q8;
    it.thickness = kSeqThickness;
    it.bgr[0] = c.b;
    it.bgr[1] = c.g;
    it.bgr[2] = c.r;
    it.reserved = 0;
}
SDTEXT_HD void seq_tail(sd_text_item& it, int n) {
    it.len = n;
    for (int i = n; i < kMaxBytes; ++i) it.text[i] = 0;
}
// the items of one record on an h x w image, `depth` = the dlen <= kMaxDepthBytes bytes of "{:.2f}".format(depth); returns their number
// (4 found, 1 not found).  Every byte of the returned items is written.  The items of a frame share ONE colour, `col`, chosen once here:
// text_gpu.hip runs the items of a frame as parallel slices of its grid, which gives what list order gives only while that holds.
SDTEXT_HD int sequence_items(const sd_rw_result& rec, const uint8_t* depth, int dlen, int h, int w, sd_text_item* out) {
    int n;
    const Colour col = rec.found == 0 ? Colour{0, 255, 0} : Colour{255, 255, 255};
    if (rec.found == 0) {
        seq_head(out[0], 0.28, 0.035, h, w, kSeqScaleBigQ8, col);
        n = put_str(out[0].text, "Cannot compute width of road at ");
        n += put_bytes(out[0].text + n, depth, dlen);
        n += put_str(out[0].text + n, " m depth:");
        seq_tail(out[0], n);
        return 1;
    }
    seq_head(out[0], 0.36, 0.05, h, w, kSeqScaleBigQ8, col);
    n = put_str(out[0].text, "At ");
    n += put_bytes(out[0].text + n, depth, dlen);
    n += put_str(out[0].text + n, " m depth:");
    seq_tail(out[0], n);
    seq_head(out[1], 0.05, 0.13, h, w, kSeqScaleQ8, col);
    n = put_fixed2(out[1].text, -(double)rec.left_pt[0]);
    n += put_str(out[1].text + n, "m to road's left end");
    seq_tail(out[1], n);
    seq_head(out[2], 0.5, 0.13, h, w, kSeqScaleQ8, col);
    n = put_fixed2(out[2].text, (double)rec.right_pt[0]);
    n += put_str(out[2].text + n, "m to road's right end");
    seq_tail(out[2], n);
    seq_head(out[3], 0.35, 0.22, h, w, kSeqScaleQ8, col);
    n = put_str(out[3].text, "Road's width: ");
    n += put_fixed2(out[3].text + n, rec.width);
    n += put_str(out[3].text + n, " m");
    seq_tail(out[3], n);
    return 4;
}

// ---- workspace of the device route (text_gpu.hip)
// what text_layout_kernel leaves per frame for text_raster_kernel: the items, and per item its pixel box and the pen position of every character
struct Extra {
    int32_t box[4];                      // x0, y0, x1, y1, clipped to the frame; empty when x0 > x1 or y0 > y1
    uint16_t pen[kMaxBytes + 2];         // pen[c] = the advances of the characters before c, pen[len] = the item's
};
struct FrameWs {
    int32_t n, pad[3];
    sd_text_item it[kMaxItems];
    Extra ex[kMaxItems];
};
struct Layout : sdarena::Walker {
    explicit Layout(int B) : frames(take((size_t)B * sizeof(FrameWs), 4)) {}
    size_t frames;              // FrameWs [B], 4-byte aligned
    size_t total = end();
};

}  // namespace sdtext
