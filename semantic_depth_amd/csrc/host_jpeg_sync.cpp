// Host side of the JPEG sync route: the batch form of the plan (sd_jpeg_sync_plan in host_jpeg.cpp: a header parse and a byte walk that
// writes the clean stream) and the CPU statement of the device decoder -- the checks of jpeg_sync.hpp, then the passes of
// jpeg_sync_gpu.hip with their lanes run in a loop, in the kernels' schedule.  Plain C++17: scripts/fuzz_jpeg_sync.cpp builds this file
// with g++ alone.
#include "../../include/semdepth.h"
#include "jpeg_sync.hpp"

#include "file_pool.hpp"

#include <cstring>
#include <vector>

namespace {

using namespace sdjsync;

// one frame; returns its status word
int decode_frame(const uint8_t* bytes, const sd_jpeg_sync_frame& fr, const sd_jpeg_sync_interval* ivs, const sd_jpeg_huff_table* tables, uint32_t S,
                 int16_t* coef) {
    const uint32_t P = fr.n_pieces, G = (P + kGroup - 1) / kGroup;
    std::vector<Rec> rec(P), group_end(G);
    std::vector<Piece> where(P);
    std::vector<State> held(kGroup);
    std::vector<uint8_t> active(kGroup);
    for (uint32_t i = 0; i < P; ++i) where[i] = locate(ivs, fr.n_intervals, P, i, S);
    // speculative pass: workgroup g, lane t = piece g * kGroup + t
    for (uint32_t g = 0; g < G; ++g) {
        const uint32_t base = g * kGroup, lanes = P - base < (uint32_t)kGroup ? P - base : (uint32_t)kGroup, group_last = base + lanes - 1;
        bool any = false;
        for (uint32_t t = 0; t < lanes; ++t) {
            rec[base + t] = spec_first(bytes, fr, tables, where[base + t], held[t]);
            const uint32_t last = where[base + t].iv_last < group_last ? where[base + t].iv_last : group_last;
            active[t] = base + t < last;
            any |= active[t] != 0;
        }
        for (uint32_t r = 1; r < (uint32_t)kGroup && any; ++r) {       // a round: lane t on piece base + t + r; each piece has one lane
            any = false;
            for (uint32_t t = 0; t < lanes; ++t) {
                if (!active[t]) continue;
                const uint32_t j = base + t + r;
                const Piece& pc = where[base + t];
                bool stop;
                rec[j] = walk_on(bytes, fr, tables, ivs[pc.iv], j, S, held[t], rec[j], &stop);
                const uint32_t last = pc.iv_last < group_last ? pc.iv_last : group_last;
                if (stop || j >= last) active[t] = 0;
                any |= active[t] != 0;
            }
        }
        group_end[g] = rec[group_last];
    }
    // across workgroups: lane g starts from the end record workgroup g - 1 had after the speculative pass
    for (uint32_t g = 1; g < G; ++g) {
        const uint32_t first = g * kGroup;
        const Piece& pc = where[first];
        if (pc.iv_first == first) continue;                            // an interval begins here: the speculative start was the true one
        const uint32_t group_last = first + kGroup - 1 < P - 1 ? first + kGroup - 1 : P - 1, last = pc.iv_last < group_last ? pc.iv_last : group_last;
        State s = unpack(group_end[g - 1]);
        for (uint32_t j = first; j <= last; ++j) {
            bool stop;
            rec[j] = walk_on(bytes, fr, tables, ivs[pc.iv], j, S, s, rec[j], &stop);
            if (stop) break;
        }
    }
    // placement: exclusive scan of the unit counts over the frame's pieces; an interval's ordinals count from its first piece
    std::vector<uint32_t> before(P);
    uint32_t sum = 0;
    for (uint32_t i = 0; i < P; ++i) { before[i] = sum; sum += rec[i].n; }
    // write pass with the verification
    int status = 0;
    for (uint32_t i = 0; i < P; ++i) {
        const Piece& pc = where[i];
        const State start = pc.iv_first == i ? State{pc.begin_bit, 0, 0} : unpack(rec[i - 1]);
        const int r = write_piece(bytes, fr, tables, pc, i, start, (int64_t)(before[i] - before[pc.iv_first]), rec[i], coef);
        if (r && !status) status = r;
    }
    // DC pass: the differences become the predictors, per interval and component
    for (int c = 0; c < fr.ncomp; ++c) {
        const int64_t n = dc_blocks(fr, c);
        int64_t pred = 0;
        for (int64_t j = 0; j < n; ++j) {
            bool head;
            int16_t* blk = coef + dc_block(fr, c, j, &head);
            pred = head ? blk[0] : pred + blk[0];
            if ((pred < -32767 || pred > 32767) && !status) status = sdjent::kBadPredictor;
            blk[0] = (int16_t)pred;
        }
    }
    return status;
}

}  // namespace

extern "C" sd_status sd_plan_files_jpeg_sync(const char* const* paths, int n, int height, int width, int subseq_bytes, uint8_t* bytes_out_host,
                                             size_t byte_stride, sd_jpeg_frame_desc* descs_out, sd_jpeg_sync_frame* frames_out,
                                             sd_jpeg_huff_table* tables_out, sd_jpeg_sync_interval* intervals_out, size_t interval_stride, int threads,
                                             int* status_out) {
    if (!paths || n < 0 || height <= 0 || width <= 0 || !bytes_out_host || !descs_out || !frames_out || !tables_out || !intervals_out ||
        !sdjsync::subseq_ok(subseq_bytes))
        return SD_ERR_INVALID;
    if (n > 0) std::memset(frames_out, 0, (size_t)n * sizeof(*frames_out));      // a file that is not planned is not eligible
    return sdfiles::for_each_file(paths, n, threads, status_out, false, [&](int i, const std::vector<uint8_t>& file) -> sd_status {
        sd_jpeg_sync_frame& fr = frames_out[i];
        uint8_t* clean = bytes_out_host + (size_t)i * byte_stride;
        sd_status st = sd_jpeg_sync_plan(file.data(), file.size(), subseq_bytes, &descs_out[i], &fr, tables_out + (size_t)i * SD_JPEG_ENTROPY_TABLES,
                                         intervals_out + (size_t)i * interval_stride, interval_stride, clean, byte_stride);
        if (st == SD_OK && fr.eligible) {
            if (!sdfiles::oriented_size_is(descs_out[i], height, width)) st = SD_ERR_INVALID;
            else {                                             // the kernels fetch whole aligned words: zeros behind the stream
                const size_t upto = ((size_t)fr.clean_bytes + 15) & ~(size_t)15;
                std::memset(clean + fr.clean_bytes, 0, (upto < byte_stride ? upto : byte_stride) - fr.clean_bytes);
            }
        }
        if (st != SD_OK) fr.eligible = 0;
        return st;
    });
}

extern "C" sd_status sd_jpeg_sync_decode_host(const uint8_t* bytes_host, size_t byte_stride, const sd_jpeg_frame_desc* descs, const sd_jpeg_sync_frame* frames,
                                              const sd_jpeg_sync_interval* intervals, size_t interval_stride, const sd_jpeg_huff_table* tables, int B,
                                              int subseq_bytes, int16_t* coef_out_host, size_t coef_stride_bytes, int32_t* status_out) {
    if (!bytes_host || !descs || !frames || !intervals || !tables || B <= 0 || !coef_out_host || !status_out || (coef_stride_bytes & 1)) return SD_ERR_INVALID;
    const char* why = nullptr;
    if (!sdjsync::args_ok(byte_stride, descs, frames, intervals, interval_stride, tables, B, subseq_bytes, coef_stride_bytes, &why)) return SD_ERR_INVALID;
    try {
        for (int b = 0; b < B; ++b) {
            status_out[b] = 0;
            const sd_jpeg_sync_frame& fr = frames[b];
            if (!fr.eligible) continue;
            int16_t* coef = coef_out_host + (size_t)b * (coef_stride_bytes / 2);
            std::memset(coef, 0, sdjpeg::desc_coef_elems(descs[b]) * sizeof(int16_t));
            status_out[b] = decode_frame(bytes_host + (size_t)b * byte_stride, fr, intervals + (size_t)b * interval_stride, tables + (size_t)b * sdjsync::kTables,
                                         (uint32_t)subseq_bytes, coef);
        }
    } catch (...) {
        return SD_ERR_INVALID;
    }
    return SD_OK;
}
