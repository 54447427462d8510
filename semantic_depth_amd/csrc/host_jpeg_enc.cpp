// Host side of the result video's frames: the CPU statement of sd_jpeg_encode_bgr for one frame -- one plain loop over the MCUs with a
// byte vector behind a bit accumulator.  Every decision -- colour, padding, the box, the transform, the quantiser, every Huffman symbol, the
// header -- is a function of jpeg_enc.hpp, which the kernels of jpeg_enc_gpu.hip run too.  No handle, no GPU.
#include "../../include/semdepth.h"
#include "jpeg_enc.hpp"

#include <cstring>
#include <new>
#include <vector>

namespace {

struct ByteSink {
    std::vector<uint8_t>& out;
    uint64_t acc = 0;
    int nacc = 0;
    void byte(uint8_t v) {
        out.push_back(v);
        if (v == 0xFF) out.push_back(0);
    }
    void put(uint32_t bits, int n) {
        acc = (acc << n) | bits;
        nacc += n;
        for (; nacc >= 8; nacc -= 8) byte((uint8_t)(acc >> (nacc - 8)));
    }
    void pad() {                                  // 1-bits up to the byte boundary
        if (nacc) put((1u << (8 - nacc)) - 1, 8 - nacc);
    }
};

}  // namespace

extern "C" sd_status sd_jpeg_encode_bgr_host(const uint8_t* frame_host, int height, int width, int quality, uint8_t* out_host, size_t cap,
                                             size_t* size_out) {
    using namespace sdjenc;
    if (!frame_host || !out_host || !size_out) return SD_ERR_INVALID;
    if (height < 1 || width < 1 || height > kMaxExtent || width > kMaxExtent || quality < 1 || quality > 100) return SD_ERR_INVALID;
    std::vector<uint8_t> out;
    try {
        out.resize(kHeaderLen);
        uint16_t div[2][64];
        make_header(out.data(), div, height, width, quality);
        ByteSink sink{out};
        const int mw = mcus_w(width), mh = mcu_rows(height);
        int16_t zz[64];
        int blk[64];
        for (int my = 0; my < mh; ++my) {
            int pred[3] = {0, 0, 0};
            for (int mx = 0; mx < mw; ++mx) {
                // the MCU's 16 x 16 samples, the last column and row replicated
                int Y[16][16], Cb[16][16], Cr[16][16];
                for (int y = 0; y < 16; ++y)
                    for (int x = 0; x < 16; ++x) {
                        const int sy = my * 16 + y < height ? my * 16 + y : height - 1, sx = mx * 16 + x < width ? mx * 16 + x : width - 1;
                        const uint8_t* p = frame_host + ((size_t)sy * width + sx) * 3;
                        Y[y][x] = ycc_y(p[0], p[1], p[2]);
                        Cb[y][x] = ycc_cb(p[0], p[1], p[2]);
                        Cr[y][x] = ycc_cr(p[0], p[1], p[2]);
                    }
                for (int k = 0; k < 6; ++k) {
                    const int comp = k < 4 ? 0 : k - 3;
                    for (int y = 0; y < 8; ++y)
                        for (int x = 0; x < 8; ++x) {
                            int v;
                            if (k < 4) {
                                v = Y[(k >> 1) * 8 + y][(k & 1) * 8 + x];
                            } else {
                                const auto& c = k == 4 ? Cb : Cr;
                                v = box4(c[2 * y][2 * x], c[2 * y][2 * x + 1], c[2 * y + 1][2 * x], c[2 * y + 1][2 * x + 1]);
                            }
                            blk[y * 8 + x] = v - 128;
                        }
                    for (int y = 0; y < 8; ++y) fdct8<true>(blk + 8 * y);
                    for (int x = 0; x < 8; ++x) {
                        int col[8];
                        for (int y = 0; y < 8; ++y) col[y] = blk[y * 8 + x];
                        fdct8<false>(col);
                        for (int y = 0; y < 8; ++y) {
                            const int z = kInvZigzag[y * 8 + x];
                            zz[z] = (int16_t)quantise(col[y], div[comp != 0][z]);
                        }
                    }
                    encode_block(zz, zz[0] - pred[comp], comp != 0, sink);
                    pred[comp] = zz[0];
                }
            }
            sink.pad();
            out.push_back(0xFF);
            out.push_back(my + 1 < mh ? (uint8_t)(0xD0 + (my & 7)) : (uint8_t)0xD9);
        }
    } catch (const std::bad_alloc&) {
        return SD_ERR_INVALID;
    }
    if (out.size() > cap) return SD_ERR_INVALID;
    memcpy(out_host, out.data(), out.size());
    *size_out = out.size();
    return SD_OK;
}
