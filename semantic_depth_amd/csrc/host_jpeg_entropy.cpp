// Host side of the JPEG entropy route: the batch form of the plan (sd_jpeg_entropy_plan in host_jpeg.cpp: a header parse and a byte walk
// for the restart markers) and the CPU statement of the device decoder -- the checks of jpeg_entropy.hpp, then a plain loop over the
// intervals calling the function the kernel calls.  Plain C++17: scripts/fuzz_jpeg_entropy.cpp builds this file with g++ alone.
#include "../../include/semdepth.h"
#include "jpeg_entropy.hpp"

#include "file_pool.hpp"

#include <cstring>
#include <vector>

extern "C" sd_status sd_plan_files_jpeg_entropy(const char* const* paths, int n, int height, int width, uint8_t* bytes_out_host, size_t byte_stride,
                                                sd_jpeg_frame_desc* descs_out, sd_jpeg_entropy_frame* frames_out, sd_jpeg_huff_table* tables_out,
                                                sd_jpeg_interval* intervals_out, size_t interval_stride, int threads, int* status_out) {
    if (!paths || n < 0 || height <= 0 || width <= 0 || !bytes_out_host || !descs_out || !frames_out || !tables_out || !intervals_out) return SD_ERR_INVALID;
    if (n > 0) std::memset(frames_out, 0, (size_t)n * sizeof(*frames_out));      // a file that is not planned is not eligible
    return sdfiles::for_each_file(paths, n, threads, status_out, false, [&](int i, const std::vector<uint8_t>& file) -> sd_status {
        sd_jpeg_entropy_frame& fr = frames_out[i];
        sd_status st = sd_jpeg_entropy_plan(file.data(), file.size(), &descs_out[i], &fr, tables_out + (size_t)i * SD_JPEG_ENTROPY_TABLES,
                                            intervals_out + (size_t)i * interval_stride, interval_stride);
        if (st == SD_OK && fr.eligible) {
            const size_t nbytes = (size_t)fr.scan_end - fr.scan_begin;
            if (!sdfiles::oriented_size_is(descs_out[i], height, width) || nbytes > byte_stride) st = SD_ERR_INVALID;
            else std::memcpy(bytes_out_host + (size_t)i * byte_stride, file.data() + fr.scan_begin, nbytes);
        }
        if (st != SD_OK) fr.eligible = 0;
        return st;
    });
}

extern "C" sd_status sd_jpeg_entropy_decode_host(const uint8_t* bytes_host, size_t byte_stride, const sd_jpeg_frame_desc* descs,
                                                 const sd_jpeg_entropy_frame* frames, const sd_jpeg_interval* intervals, size_t interval_stride,
                                                 const sd_jpeg_huff_table* tables, int B, int16_t* coef_out_host, size_t coef_stride_bytes,
                                                 int32_t* status_out) {
    if (!bytes_host || !descs || !frames || !intervals || !tables || B <= 0 || !coef_out_host || !status_out || (coef_stride_bytes & 1)) return SD_ERR_INVALID;
    const char* why = nullptr;
    if (!sdjent::args_ok(byte_stride, descs, frames, intervals, interval_stride, tables, B, coef_stride_bytes, &why)) return SD_ERR_INVALID;
    for (int b = 0; b < B; ++b) {
        status_out[b] = 0;
        const sd_jpeg_entropy_frame& fr = frames[b];
        if (!fr.eligible) continue;
        int16_t* coef = coef_out_host + (size_t)b * (coef_stride_bytes / 2);
        std::memset(coef, 0, sdjpeg::desc_coef_elems(descs[b]) * sizeof(int16_t));
        for (int i = 0; i < fr.n_intervals; ++i) {
            const sd_jpeg_interval& iv = intervals[(size_t)b * interval_stride + i];
            const int r = sdjent::decode_interval(bytes_host + (size_t)b * byte_stride, iv.begin, iv.end, fr, tables + (size_t)b * sdjent::kTables, i, coef);
            if (r != sdjent::kOk && status_out[b] == 0) status_out[b] = r;
        }
    }
    return SD_OK;
}
