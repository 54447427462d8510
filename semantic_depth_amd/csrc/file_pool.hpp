// What the batch readers of the input stage share (sd_decode_files_bgr, sd_decode_files_jpeg_coef, sd_inflate_files_png,
// sd_plan_files_jpeg_entropy, sd_plan_files_jpeg_sync): reading a file, the size check after the EXIF orientation, and the pool of
// threads that claim one file after the other.  Header-only, plain C++17.
#pragma once

#include "../../include/semdepth.h"

#include <atomic>
#include <cstdio>
#include <thread>
#include <vector>

namespace sdfiles {

inline bool read_file(const char* path, std::vector<uint8_t>& buf) {
    FILE* fp = std::fopen(path, "rb");
    if (!fp) return false;
    std::fseek(fp, 0, SEEK_END);
    const long n = std::ftell(fp);
    std::fseek(fp, 0, SEEK_SET);
    if (n <= 0) { std::fclose(fp); return false; }
    buf.resize((size_t)n);
    const size_t got = std::fread(buf.data(), 1, (size_t)n, fp);
    std::fclose(fp);
    return got == (size_t)n;
}

// every frame of a batch has the batch's shape after the orientation (5 to 8 transpose)
inline bool oriented_size_is(const sd_jpeg_frame_desc& d, int height, int width) {
    const bool swap = d.orientation >= 5;
    return (swap ? d.width : d.height) == height && (swap ? d.height : d.width) == width;
}

// per_file(i, file) -> sd_status for every file that could be read, on `threads` threads (<= 0: the hardware's; never more than
// files), each claiming the next unclaimed file.  A path that is NULL or cannot be read is SD_ERR_NOTFOUND, an exception
// SD_ERR_INVALID (none crosses the C ABI or a worker thread).  status_out[i], where given, is file i's status; the call returns
// SD_ERR_INVALID when a file failed -- SD_ERR_FORMAT, "not this reader's format", counts only if format_is_failure.
template <class PerFile>
sd_status for_each_file(const char* const* paths, int n, int threads, int* status_out, bool format_is_failure, PerFile per_file) {
    if (threads <= 0) threads = (int)std::thread::hardware_concurrency();
    threads = threads < 1 ? 1 : (threads > n ? (n > 0 ? n : 1) : threads);
    std::atomic<int> next(0), failed(0);
    auto work = [&]() {
        std::vector<uint8_t> file;
        for (;;) {
            const int i = next.fetch_add(1);
            if (i >= n) break;
            sd_status st = SD_ERR_NOTFOUND;
            try {
                if (paths[i] && read_file(paths[i], file)) st = per_file(i, file);
            } catch (...) {
                st = SD_ERR_INVALID;
            }
            if (status_out) status_out[i] = st;
            if (st != SD_OK && (format_is_failure || st != SD_ERR_FORMAT)) failed.fetch_add(1);
        }
    };
    std::vector<std::thread> pool;
    try {
        for (int t = 1; t < threads; ++t) pool.emplace_back(work);
    } catch (...) {                                             // (thread creation refused: the calling thread and the workers that exist do the batch)
    }
    work();
    for (auto& th : pool) th.join();
    return failed.load() ? SD_ERR_INVALID : SD_OK;
}

}  // namespace sdfiles
