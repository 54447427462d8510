// dev tool: every scratch layout of the library (DESIGN.md "where scratch layouts live") held to its own statement, on the host: plain
// C++17, no HIP, nothing of workspace size is allocated.
//   g++ -O1 -std=c++17 scripts/check_layouts.cpp -o /tmp/check_layouts && /tmp/check_layouts            (tests/test_workspace_layouts_cpu.py does this)
//   g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 scripts/check_layouts.cpp -o /tmp/check_layouts_san
//   /tmp/check_layouts [random argument sets per layout, default 300] [--dump]
// For every layout, over a grid of arguments that exercises the alignment padding (B 1, 3, 32; extents 1, 17, 250, 1025; D 1, 256; caps 1,
// 257, 65536; every scene mask bit alone and all of them) plus the random sets inside each query's legal range:
//   * the regions lie in ascending order and do not overlap (their sizes are restated here, independently of the layout functions); the
//     fence chain's views over the Open3D region are the declared exception and must lie inside that region
//   * every offset meets the alignment its field comment states
//   * the last region (the historical slack, where there is one) ends at or before `total`
//   * `total` is what the size query has always answered: the closed formulas of the queries before the layouts existed, restated here
// Exit status 1 with the offending layout and its arguments.  --dump prints every region (layout, arguments, name, offset) instead of
// being quiet: the listing two versions of the layouts are compared with.
#include <cinttypes>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../semantic_depth_amd/csrc/disp_image_rule.hpp"
#include "../semantic_depth_amd/csrc/handle_arena.hpp"
#include "../semantic_depth_amd/csrc/jpeg_enc.hpp"
#include "../semantic_depth_amd/csrc/jpeg_sync.hpp"
#include "../semantic_depth_amd/csrc/overlay_rule.hpp"
#include "../semantic_depth_amd/csrc/png_deflate.hpp"
#include "../semantic_depth_amd/csrc/png_unfilter.hpp"
#include "../semantic_depth_amd/csrc/render_rule.hpp"
#include "../semantic_depth_amd/csrc/rw_profile.hpp"
#include "../semantic_depth_amd/csrc/scene_format.hpp"

namespace {

struct Region { const char* name; size_t off, bytes, align; };
bool g_dump = false;
int g_failed = 0;
long g_sets = 0;

size_t up(size_t v, size_t a) { return (v + a - 1) / a * a; }

std::string fmt(const char* f, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, f);
    vsnprintf(buf, sizeof(buf), f, ap);
    va_end(ap);
    return buf;
}

// the regions of one layout in their stated order; a trailing region named "slack" runs to `total`
void check(const std::string& what, const std::vector<Region>& r, size_t total, size_t query_total) {
    ++g_sets;
    auto bad = [&](const std::string& why) { ++g_failed; std::printf("FAIL %s: %s\n", what.c_str(), why.c_str()); };
    for (size_t i = 0; i < r.size(); ++i) {
        if (g_dump) std::printf("%s %s %zu\n", what.c_str(), r[i].name, r[i].off);
        if (r[i].off % r[i].align) bad(fmt("%s at %zu is not %zu-byte aligned", r[i].name, r[i].off, r[i].align));
        if (i + 1 < r.size() && r[i].off + r[i].bytes > r[i + 1].off) bad(fmt("%s [%zu, +%zu) runs into %s at %zu", r[i].name, r[i].off, r[i].bytes, r[i + 1].name, r[i + 1].off));
        if (r[i].off + r[i].bytes > total) bad(fmt("%s [%zu, +%zu) ends behind total %zu", r[i].name, r[i].off, r[i].bytes, total));
    }
    if (g_dump) std::printf("%s total %zu\n", what.c_str(), total);
    if (total != query_total) bad(fmt("total %zu, the size query answers %zu", total, query_total));
}
Region slack(size_t off, size_t total) { return {"slack", off, total >= off ? total - off : (size_t)-1 / 2, 1}; }

// ---------------------------------------------------------------------------------------------- the public workspaces
void ply(int B, int cap) {
    const sdply::Layout l(B, cap);
    const size_t nb = (size_t)B * sdply::blocks_per_frame(cap), b = (size_t)B;
    check(fmt("ply B=%d cap=%d", B, cap),
          {{"bmin", l.bmin, nb * 8, 8}, {"boff", l.boff, nb * 8, 8}, {"zmin", l.zmin, b * 8, 8}, {"fbase", l.fbase, b * 8, 8}, {"blen", l.blen, nb * 4, 4},
           {"bcnt", l.bcnt, nb * 4, 4}, {"bbad", l.bbad, nb * 4, 4}, slack(l.slack, l.total)},
          l.total, nb * (2 * 8 + 3 * 4) + b * 2 * 8 + 64);
}
void scene(int B, int cr, int cf, uint32_t lat, uint32_t mask) {
    const sdscene::Layout l(B, cr, cf, lat, mask);
    const size_t nb = (size_t)B * (size_t)sdscene::blocks_bound(cr, cf, lat, mask), b = (size_t)B, tab = sizeof(sdscene::SegTable);
    check(fmt("scene B=%d cap_road=%d cap_fence=%d lattice_cap=%u mask=%u", B, cr, cf, lat, mask),
          {{"bmin", l.bmin, nb * 8, 8}, {"boff", l.boff, nb * 8, 8}, {"zmin", l.zmin, b * 8, 8}, {"fbase", l.fbase, b * 8, 8}, {"tab", l.tab, b * tab, 8},
           {"blen", l.blen, nb * 4, 4}, {"bcnt", l.bcnt, nb * 4, 4}, {"bbad", l.bbad, nb * 4, 4}, slack(l.slack, l.total)},
          l.total, nb * (2 * 8 + 3 * 4) + b * (2 * 8 + tab) + 64);
}
void render(int B, int cap, int width, int height) {
    sd_render_camera cam{};
    cam.width = width; cam.height = height;
    const sdrender::Layout l(B, cap, cam);
    const size_t px = (size_t)B * height * width, nb = (size_t)B * sdply::blocks_per_frame(cap);
    check(fmt("render B=%d cap=%d width=%d height=%d", B, cap, width, height),
          {{"keys", l.keys, px * 8, 16}, {"bmin", l.bmin, nb * 8, 8}, {"zmin", l.zmin, (size_t)B * 8, 8}, slack(l.slack, l.total)}, l.total,
          (px + nb + (size_t)B) * 8 + 64);
}
void png(int B, int h, int w) {
    const sdpng::Layout l(B, h, w);
    const size_t n = (size_t)B * sdpng::num_chunks(h, w), slot = sdpng::kChunk + sdpng::kChunkSlack;
    check(fmt("png B=%d h=%d w=%d", B, h, w),
          {{"slots", l.slots, n * slot, 16}, {"offsets", l.offsets, n * 8, 8}, {"csize", l.csize, n * 4, 4}, {"adler_a", l.adler_a, n * 4, 4},
           {"adler_b", l.adler_b, n * 4, 4}, slack(l.slack, l.total)},
          l.total, n * slot + n * (3 * 4 + 8) + 64);
}
void png_in(int B) {
    const sdpngin::Layout l(B);
    check(fmt("png_in B=%d", B), {{"descs", l.descs, (size_t)B * sizeof(sd_png_frame_desc), 16}}, l.total, up((size_t)B * sizeof(sd_png_frame_desc), 16));
}
void jpeg(const std::vector<sd_jpeg_frame_desc>& d) {
    sdarena::Walker w;
    std::vector<Region> r;
    std::vector<std::string> names;
    names.reserve(d.size() * 3);
    size_t sum = 0;
    for (size_t b = 0; b < d.size(); ++b) {
        size_t plane[3];
        sdjpeg::take_planes(w, d[b], plane);
        for (int c = 0; c < d[b].ncomp; ++c) {
            const size_t bytes = (size_t)d[b].blocks_w[c] * d[b].blocks_h[c] * 64;
            names.push_back(fmt("plane[%zu][%d]", b, c));
            r.push_back({names.back().c_str(), plane[c], bytes, 256});
            sum += up(bytes, 256);
        }
    }
    const size_t total = sdjpeg::workspace_bytes(d.data(), (int)d.size());
    check(fmt("jpeg B=%zu first=%dx%d", d.size(), d[0].height, d[0].width), r, total, sum);
    if (w.end(256) != total) { ++g_failed; std::printf("FAIL jpeg: the launcher's walk ends at %zu, the query answers %zu\n", w.end(256), total); }
}
void jpeg_enc(int B, int h) {
    const sdjenc::Layout l(B, h);
    const size_t n = (size_t)B * (size_t)sdjenc::mcu_rows(h);
    check(fmt("jpeg_enc B=%d h=%d", B, h), {{"offsets", l.offsets, n * 8, 16}, {"rowsize", l.rowsize, n * 4, 4}}, l.total, up(n * 12, 16));
}
void jpeg_entropy(int B, size_t stride) {
    const sdjent::Layout l(B, stride);
    const size_t f = (size_t)B * sizeof(sd_jpeg_entropy_frame), t = (size_t)B * sdjent::kTables * sizeof(sd_jpeg_huff_table), i = (size_t)B * stride * sizeof(sd_jpeg_interval);
    check(fmt("jpeg_entropy B=%d interval_stride=%zu", B, stride), {{"frames", l.frames, f, 16}, {"tables", l.tables, t, 16}, {"intervals", l.intervals, i, 16}}, l.total,
          up(f, 16) + up(t, 16) + up(i, 16));
}
void jpeg_sync(int B, size_t stride, size_t pieces) {
    const sdjsync::Layout l(B, stride, pieces);
    const size_t g = sdjsync::kGroup, P = (pieces < 1 ? 1 : (pieces + g - 1) / g) * g, b = (size_t)B;
    const size_t f = b * sizeof(sd_jpeg_sync_frame), t = b * sdjsync::kTables * sizeof(sd_jpeg_huff_table), i = b * stride * sizeof(sd_jpeg_sync_interval),
                 rec = b * P * sizeof(sdjsync::Rec), ge = b * (P / g) * sizeof(sdjsync::Rec), bef = b * P * 4;
    check(fmt("jpeg_sync B=%d interval_stride=%zu max_pieces=%zu", B, stride, pieces),
          {{"frames", l.frames, f, 16}, {"tables", l.tables, t, 16}, {"intervals", l.intervals, i, 16}, {"rec", l.rec, rec, 16}, {"group_end", l.group_end, ge, 16},
           {"before", l.before, bef, 16}},
          l.total, up(f, 16) + up(t, 16) + up(i, 16) + up(rec, 16) + up(ge, 16) + up(bef, 16));
}
void overlay(int B, int D) {
    const sdoverlay::Layout l(B, D);
    const size_t b = (size_t)B, slots = b * sdoverlay::slots_of(D) * 40;
    check(fmt("overlay B=%d D=%d", B, D), {{"cams", l.cams, b * 32, 16}, {"heads", l.heads, b * 16, 16}, {"slots", l.slots, slots, 16}}, l.total, b * 48 + slots);
}
void text(int B) {
    const sdtext::Layout l(B);
    check(fmt("text B=%d", B), {{"frames", l.frames, (size_t)B * sizeof(sdtext::FrameWs), 4}}, l.total, (size_t)B * sizeof(sdtext::FrameWs));
}
void rw_profile(int B, int cap, int D) {
    const sdrwp::Layout l(B, cap, D);
    const size_t win = (size_t)D * sizeof(sdrwp::Window), part = (size_t)B * sdrwp::slices_of(cap) * D * sizeof(sdrwp::Partial);
    check(fmt("rw_profile B=%d cap=%d D=%d", B, cap, D), {{"windows", l.windows, win, 16}, {"partial", l.partial, part, 16}}, l.total, up(win, 16) + part);
}
size_t pil_total(int B, int sh, int sw, int dh, int dw, int ch) {
    auto tables = [](int in, int out) { return up((size_t)out * 8, 16) + up((size_t)sdpil::taps_bound(in, out) * out * 4, 16); };
    return tables(sw, dw) + tables(sh, dh) + up((size_t)B * sh * (((size_t)dw * ch + 3) / 4 * 4), 16);
}
void pil(int B, int sh, int sw, int dh, int dw, int ch) {
    const sdpil::Layout l(B, sh, sw, dh, dw, ch);
    check(fmt("pil B=%d src=%dx%d dst=%dx%d channels=%d", B, sh, sw, dh, dw, ch),
          {{"x_bounds", l.x_bounds, (size_t)dw * 8, 16}, {"x_k", l.x_k, (size_t)sdpil::taps_bound(sw, dw) * dw * 4, 16}, {"y_bounds", l.y_bounds, (size_t)dh * 8, 16},
           {"y_k", l.y_k, (size_t)sdpil::taps_bound(sh, dh) * dh * 4, 16}, {"mid", l.mid, (size_t)B * sh * sdpil::mid_pitch(dw, ch), 16}},
          l.total, pil_total(B, sh, sw, dh, dw, ch));
}
void disp(int B, int h, int w, int oh, int ow) {
    const sddisp::Layout l(B, h, w, oh, ow);
    const size_t b = (size_t)B;
    std::vector<Region> r = {{"cells", l.cells, b * 16, 16}, {"mult", l.mult, b * 4, 16}, {"bytes", l.bytes, b * h * w, 16}};
    size_t expect = up(b * 16, 16) + up(b * 4, 16) + up(b * h * w, 16);
    if (h != oh || w != ow) {
        r.push_back({"resized", l.resized, b * oh * ow, 16});
        r.push_back({"pil", l.pil, pil_total(B, h, w, oh, ow, 1), 16});
        expect += up(b * oh * ow, 16) + up(pil_total(B, h, w, oh, ow, 1), 16);
    } else if (l.resized != l.total || l.pil != l.total) {
        ++g_failed; std::printf("FAIL disp B=%d %dx%d: the unused parts do not sit at total\n", B, h, w);
    }
    check(fmt("disp B=%d src=%dx%d dst=%dx%d", B, h, w, oh, ow), r, l.total, expect);
}

// ---------------------------------------------------------------------------------------------- the scratches behind the handle
void fuse(int B, int H, int W) {
    const size_t b = (size_t)B, px = (size_t)H * W, blk = b * ((px + 255) / 256) * 8;
    const sd::FuseLayout l(B, H, W);
    check(fmt("fuse B=%d %dx%d", B, H, W), {{"blk_counts", l.blk_counts, blk, 4}, {"blk_offsets", l.blk_offsets, blk, 4}}, l.total, 2 * blk);
    const sd::Fuse1Layout o(B, H, W);
    const size_t st = b * ((px + sd::F1_PIX - 1) / sd::F1_PIX) * 8;
    check(fmt("fuse_onepass B=%d %dx%d", B, H, W), {{"state", o.state, st, 8}, {"ticket", o.ticket, b * 4, 4}, slack(o.slack, o.total)}, o.total, st + b * 4 + 256);
}
void sweep(int B, int T, int H, int W) {
    const sd::SweepLayout l(B, T, H, W);
    const size_t cams = (size_t)T * B * sizeof(sd::CamDev), blk = (size_t)B * (((size_t)H * W + 255) / 256) * 8;
    check(fmt("fuse_sweep B=%d T=%d %dx%d", B, T, H, W), {{"cams", l.cams, cams, 16}, {"blk_counts", l.blk_counts, blk, 16}, {"blk_offsets", l.blk_offsets, blk, 16}}, l.total,
          up(cams, 16) + 2 * up(blk, 16));
}
void cmp(int B) {
    const sd::CmpLayout l(B);
    const size_t b = (size_t)B;
    check(fmt("cmp B=%d", B),
          {{"params", l.params, b * sd::CMP_PARAMS * 8, 256}, {"blk_cnt", l.blk_cnt, b * sd::CMP_SLICES * 4, 256}, {"med", l.med, b * sizeof(sd::MedG), 256},
           {"medbuf", l.medbuf, b * sd::CMP_MED_KEYS * 4, 256}, slack(l.slack, l.total)},
          l.total, b * (sd::CMP_SLICES * 4 + sd::CMP_PARAMS * 8 + sizeof(sd::MedG) + (size_t)sd::CMP_MED_KEYS * 4) + 1024);
}
void o3d(int B, int cap) {
    const sd::O3dLayout l(B, cap);
    const size_t b = (size_t)B, c = (size_t)cap, pts = b * c, cells = sd::GRID_CELLS;
    const size_t per = sizeof(sd::GridMeta) + cells * 4 + (cells + 1) * 4 + sd::SCAN_NSEG * 4 + c * (4 + 4 + 16 + 8 + 1) + c * sd::KMAX * 8;
    check(fmt("o3d B=%d cap=%d", B, cap),
          {{"meta", l.meta, b * sizeof(sd::GridMeta), 256}, {"mean_d", l.mean_d, pts * 8, 256}, {"cell_cnt", l.cell_cnt, b * cells * 4 + b * 32, 256},
           {"cell_start", l.cell_start, b * (cells + 1) * 4, 256}, {"seg_sum", l.seg_sum, b * sd::SCAN_NSEG * 4, 256}, {"cell_of", l.cell_of, pts * 4, 256},
           {"sidx", l.sidx, pts * 4, 256}, {"sxyz", l.sxyz, pts * 16, 256}, {"keep", l.keep, pts, 256}, {"hard_n", l.hard_n, b * 4, 256},
           {"hard_best", l.hard_best, pts * sd::KMAX * 8, 256}, slack(l.slack, l.total)},
          l.total, b * (per + 4 + 32) + 8192 + 256);
    // the declared views: ascending among themselves, inside the region
    check(fmt("o3d fence views B=%d cap=%d", B, cap), {{"fence_left_xyz", l.fence_left_xyz, pts * 12, 256}, {"fence_left_rgb", l.fence_left_rgb, pts * 3, 256}}, l.total, l.total);
    if (l.fence_views_end != l.fence_left_rgb + pts * 3) { ++g_failed; std::printf("FAIL o3d fence views B=%d cap=%d: end %zu\n", B, cap, l.fence_views_end); }
}
void arena(int B, int H, int W, size_t fcn, size_t mono, size_t splitk) {
    const sd::Arena a({B, H, W, H * W, fcn, mono, splitk});
    const size_t b = (size_t)B, cap = (size_t)H * W;
    const sd::SatLayout s(B);
    const sd::RszLayout rz;
    const size_t sat_total = up(8 + (size_t)(3 * B + sd::SAT_IMG_PAD + 1) * 4, 256), rsz_total = (size_t)sd::RSZ_MAX * 16 * 4;
    const std::string at = fmt("B=%d %dx%d act=%zu,%zu splitk=%zu", B, H, W, fcn, mono, splitk);
    check("sat " + at, {{"count", s.count, 8, 8}, {"img", s.img, (size_t)(2 * B + sd::SAT_IMG_PAD) * 4, 4}, {"frames", s.frames, b * 4, 4}, {"orphans", s.orphans, 4, 4}}, s.total,
          sat_total);
    check("rsz", {{"xi", rz.xi, rsz_total / 4, 16}, {"xa", rz.xa, rsz_total / 4, 16}, {"yi", rz.yi, rsz_total / 4, 16}, {"ya", rz.ya, rsz_total / 4, 16}}, rz.total, rsz_total);
    const size_t fuse_t = sd::FuseLayout(B, H, W).total, fuse1_t = sd::Fuse1Layout(B, H, W).total, o3d_t = sd::O3dLayout(B, H * W).total,
                 cmp_t = sd::CmpLayout(B).total;
    // what sd_query_memory has always answered: every part rounded up to 256, the four parts behind the Open3D scratch once one region of
    // 4096 + counts + planes + counters
    const size_t misc = 4096 + up(b * 7 * 4, 256) + up(b * 12 * 8, 256) + sat_total;
    size_t expect = 0;
    for (size_t part : {fcn, mono, fuse_t, fuse1_t, sizeof(sd::CamDev) * b, b * cap * 12, b * cap * 12, b * cap * 3, b * cap * 3, b * 4 * 24, b * 8 * 4, o3d_t, misc, cmp_t, rsz_total,
                        rsz_total, splitk})
        expect += up(part, 256);
    check("arena " + at,
          {{"fcn", a.fcn, fcn, 256}, {"mono", a.mono, mono, 256}, {"fuse", a.fuse, fuse_t, 256}, {"fuse1", a.fuse1, fuse1_t, 256}, {"cams", a.cams, sizeof(sd::CamDev) * b, 256},
           {"bufA", a.bufA, b * cap * 12, 256}, {"bufB", a.bufB, b * cap * 12, 256}, {"rgbA", a.rgbA, b * cap * 3, 256}, {"rgbB", a.rgbB, b * cap * 3, 256},
           {"cnt", a.cnt, b * 4 * sd::CNT_SLOTS, 256}, {"plane", a.plane, b * 32, 256}, {"o3d", a.o3d, o3d_t, 256}, {"scalar", a.scalar, sd::kScalarSlotBytes, 256},
           {"zero", a.zero, sd::kZeroPageBytes, 256}, {"f2f_counts", a.f2f_counts, b * sd::CNT_F2F_ROWS * 4, 256}, {"f2f_planes", a.f2f_planes, b * 96, 256},
           {"sat", a.sat, s.total, 256}, {"cmp", a.cmp, cmp_t, 256}, {"rsz", a.rsz, rz.total, 256}, {"rsz_cmp", a.rsz_cmp, rz.total, 256}, {"splitk", a.splitk, splitk, 256}},
          a.total, expect);
    if (!a.fence_views_fit) { ++g_failed; std::printf("FAIL arena %s: the fence chain's views do not fit the Open3D region\n", at.c_str()); }
}

sd_jpeg_frame_desc jpeg_desc(int h, int w, int ncomp, int hmax, int vmax) {
    sd_jpeg_frame_desc d{};
    d.height = h; d.width = w; d.ncomp = ncomp; d.hmax = hmax; d.vmax = vmax; d.orientation = 1; d.adobe_transform = -1;
    int64_t off = 0;
    for (int i = 0; i < ncomp; ++i) {
        d.blocks_w[i] = sdjpeg::blocks_w(w, hmax, i ? 1 : hmax); d.blocks_h[i] = sdjpeg::blocks_h(h, vmax, i ? 1 : vmax); d.coef_offset[i] = off;
        off += (int64_t)d.blocks_w[i] * d.blocks_h[i] * 64;
    }
    return d;
}

}  // namespace

int main(int argc, char** argv) {
    int nrand = 300;
    for (int i = 1; i < argc; ++i) {
        if (!std::strcmp(argv[i], "--dump")) g_dump = true;
        else nrand = std::atoi(argv[i]);
    }
    const int Bs[] = {1, 3, 32}, ext[] = {1, 17, 250, 1025}, caps[] = {1, 257, 65536}, Ds[] = {1, 256};
    const uint32_t masks[] = {255, 1, 2, 4, 8, 16, 32, 64, 128, 0};
    const int subs[][2] = {{1, 1}, {2, 1}, {2, 2}};
    for (int B : Bs) {
        png_in(B); text(B); cmp(B);
        for (int cap : caps) {
            ply(B, cap); o3d(B, cap);
            for (int D : Ds) rw_profile(B, cap, D);
            for (int w : ext) for (int h : ext) render(B, cap, w, h);
            for (uint32_t m : masks) for (uint32_t lat : {0u, 1000u, 0xffffffffu}) scene(B, cap, 257, lat, m);
        }
        for (int D : {0, 1, 7, 256}) overlay(B, D);
        for (size_t stride : {0, 1, 17, 1025}) {
            jpeg_entropy(B, stride);
            for (size_t pieces : {0, 1, 255, 256, 257, 65537}) jpeg_sync(B, stride, pieces);
        }
        for (int h : ext) {
            jpeg_enc(B, h);
            for (int w : ext) {
                png(B, h, w); fuse(B, h, w);
                for (int T : {1, 3, 21}) sweep(B, T, h, w);
                for (int oh : {17, 250}) for (int ow : {17, 1025}) {
                    if (sdpil::axis_ok(h, oh) && sdpil::axis_ok(w, ow)) { disp(B, h, w, oh, ow); pil(B, h, w, oh, ow, 1); pil(B, h, w, oh, ow, 3); }
                }
                disp(B, h, w, h, w);
            }
        }
        std::vector<sd_jpeg_frame_desc> d;
        for (int i = 0; i < B; ++i) d.push_back(jpeg_desc(ext[i % 4], ext[(i + 1) % 4], i % 5 == 4 ? 1 : 3, i % 5 == 4 ? 1 : subs[i % 3][0], i % 5 == 4 ? 1 : subs[i % 3][1]));
        jpeg(d);
        for (int H : {128, 250}) for (size_t act : {(size_t)0, (size_t)12345677}) for (size_t splitk : {(size_t)0, (size_t)1000001}) arena(B, H, 2 * H + (H & 2), act, act / 3, splitk);
    }
    std::mt19937_64 rng(20260101);
    auto R = [&](long long lo, long long hi) { return (int)(lo + (long long)(rng() % (uint64_t)(hi - lo + 1))); };
    for (int i = 0; i < nrand; ++i) {
        const int B = i % 3 ? R(1, 64) : R(1, 65535), small = R(1, 2048), cap = i % 2 ? R(0, 300000) : R(0, 0x7fffffff - 2000);
        png_in(B); text(B); cmp(B > 4096 ? B % 4096 + 1 : B);
        ply(B, cap);
        render(B, cap, R(1, 16384), R(1, 16384));
        scene(R(1, 4096), R(0, 400000), R(0, 400000), i % 3 ? (uint32_t)R(0, 100000) : 0xffffffffu, (uint32_t)R(0, 255));
        png(B, R(1, 16384), R(1, 16384));
        jpeg_enc(B, R(1, 16384));
        jpeg_entropy(B, (size_t)R(0, 70000));
        jpeg_sync(B, (size_t)R(0, 70000), (size_t)R(0, 1 << 24));
        overlay(B, R(0, 256));
        rw_profile(B, R(1, 0x7fffffff), R(1, 256));
        {
            const int sh = R(1, 16384), sw = R(1, 16384), dh = R((sh + 31) / 32, 16384), dw = R((sw + 31) / 32, 16384);
            pil(B, sh, sw, dh, dw, i % 2 ? 1 : 3);
            disp(B, sh, sw, i % 5 ? dh : sh, i % 5 ? dw : sw);
        }
        const int H = R(1, 2048), W = R(1, 4096);
        fuse(R(1, 64), H, W);
        sweep(small % 64 + 1, R(1, 65535 / (small % 64 + 1)), H, W);
        o3d(R(1, 64), R(1, 2048 * 1024));
        arena(R(1, 64), R(1, 1024), R(1, 2048), (size_t)rng() % ((size_t)1 << 36), (size_t)rng() % ((size_t)1 << 36), i % 2 ? (size_t)rng() % ((size_t)1 << 30) : 0);
        std::vector<sd_jpeg_frame_desc> d;
        for (int b = 0, n = R(1, 40); b < n; ++b) {
            const int s = R(0, 3);
            d.push_back(s == 3 ? jpeg_desc(R(1, 4000), R(1, 4000), 1, 1, 1) : jpeg_desc(R(1, 4000), R(1, 4000), 3, subs[s][0], subs[s][1]));
        }
        jpeg(d);
    }
    if (!g_dump) std::printf("check_layouts: %ld argument sets, %d failures\n", g_sets, g_failed);
    return g_failed ? 1 : 0;
}
