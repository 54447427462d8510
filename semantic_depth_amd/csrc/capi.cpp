// extern "C" surface of libsemdepth.so (include/semdepth.h).  Owns the layer plans and the launch sequences;
// owns no device memory (the caller binds arenas it allocated, e.g. torch tensors).
#include "../../include/semdepth.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "jpeg_gpu.hpp"
#include "png_gpu.hpp"
#include "jpeg_enc_gpu.hpp"
#include "jpeg_entropy_gpu.hpp"
#include "jpeg_sync_gpu.hpp"
#include "png_in_gpu.hpp"
#include "ply_gpu.hpp"
#include "scene_gpu.hpp"
#include "text_gpu.hpp"
#include "overlay_gpu.hpp"
#include "render_gpu.hpp"
#include "rw_profile_gpu.hpp"
#include "seg_eval_gpu.hpp"
#include "disp_image_gpu.hpp"
#include "kernels.hpp"
#include "plan.hpp"
#include "conv_form.hpp"
#include "handle_arena.hpp"

using namespace sd;

static_assert(sizeof(RwResultDev) == sizeof(sd_rw_result), "sd_rw_result layout");
static_assert(sizeof(F2fResultDev) == sizeof(sd_f2f_result), "sd_f2f_result layout");

struct sd_handle {
    int device = 0, H = 0, W = 0, max_batch = 0, enc = 0, chunk = 0, cap = 0, prec = 0;
    unsigned sw = 0;      // SEMDEPTH_* switches, latched in sd_create
    unsigned fuse_epoch = 0;   // epoch of the look-back words in the one-pass fuse scratch (0: scratch must be zeroed first)
    int last_mono_frames = 0;  // frames of the last sd_monodepth_forward whose raw pair is still in the activation arena (0: none / chunked)
    NetPlan fcn, mono;
    bool bound = false;
    char* wf = nullptr;   // FCN weight arena
    char* wm = nullptr;   // monodepth weight arena
    char* ws = nullptr;   // workspace arena
    Arena a{};            // where everything lives in it (handle_arena.hpp)
    std::vector<int> rsz_host;      // tap tables of the last sd_resize_cubic_u8 geometry (kept alive for the async upload)
    int rsz_key[4] = {0, 0, 0, 0};
    std::vector<int> cmp_rsz_host;  // the same for sd_compose_result_frames (own slot: the input resize and the output compose alternate
    int cmp_rsz_key[4] = {0, 0, 0, 0};   //  every batch with different geometries, and a shared slot would re-upload and synchronise each time)
    int last_fcn_images = 0, last_mono_images = 0;
    int reserve_cus = 0;            // sd_set_reserved_cus: CUs the persistent conv launches leave free
    int small_batch = 0, cus = 0;   // sd_set_small_batch: the split-K forms of the under-filled GEMM layers; the CU count its rule reads (latched with it)
    std::vector<ConvForm> forms[2];   // [sd_net], per op of the plan: the kernel form of a full pass (resolve_forms; default records for the other ops)
    std::vector<CamDev> cams_stage;
    std::vector<CamDev> sweep_stage;     // sd_fuse_backproject_sweep: the [T][B] records of the last call (source of its upload)
    std::vector<OverlayCamDev> overlay_stage;    // sd_overlay_draw: the cameras of the last call (source of its upload)
    std::vector<sdrwp::Window> rwp_stage;    // sd_road_width_profile: the sorted windows of the last call (source of its upload)
    sdpil::Windows pil_x, pil_y;             // sd_resize_pil_bilinear_u8: the windows of the last call (source of its uploads)
    sdpil::Windows disp_x, disp_y;           // sd_disp_image: the same for its resample
    std::vector<float> disp_mult;            // sd_disp_image: the multipliers of the last call (source of their upload)
    std::map<std::pair<int, int>, std::vector<float>> bias_host;   // (net, slot) -> host copy, for bias slots that are summed
    std::map<std::pair<int, int>, std::vector<float>> w_host;      // (net, slot) -> f32 tensor of the SD_PREC_F16X2 slots that share a weight scale (sd_load_weight)
    std::string err;
    // profiling (sd_profile): event pairs around conv launches
    bool prof = false;
    struct ProfRec { std::string kernel; double flops; hipEvent_t a, b; const char* op; int M, N, K; double bytes; };
    std::vector<ProfRec> prof_recs;
    // one event per conv launch: the end event of a conv is the start event of the conv launched right behind it (two events per
    // launch cost 1.8 % of a step: every record is a barrier packet on the stream)
    std::vector<hipEvent_t> prof_pool;
    size_t prof_used = 0;
    hipEvent_t prof_last = nullptr;      // end event of the previous conv launch, if nothing else was launched since
};

namespace {

sd_status fail(sd_handle* h, sd_status code, const std::string& msg) {
    if (h) h->err = msg;
    return code;
}
#define HIPCHK(h, expr)                                                                              \
    do {                                                                                             \
        hipError_t e_ = (expr);                                                                      \
        if (e_ != hipSuccess) return fail(h, SD_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

NetPlan& plan_of(sd_handle* h, sd_net net) { return net == SD_NET_FCN8S ? h->fcn : h->mono; }
const NetPlan& plan_of(const sd_handle* h, sd_net net) { return net == SD_NET_FCN8S ? h->fcn : h->mono; }
char* warena(sd_handle* h, sd_net net) { return net == SD_NET_FCN8S ? h->wf : h->wm; }

// the per-op form tables of a full pass; built where the facts they read become final (sd_create, sd_set_small_batch)
void resolve_forms(sd_handle* h) {
    for (sd_net net : {SD_NET_FCN8S, SD_NET_MONODEPTH}) {
        const NetPlan& p = plan_of(h, net);
        h->forms[net].clear();
        for (const OpDesc& op : p.ops) h->forms[net].push_back(resolve_conv_form({h->sw, h->small_batch, h->cus}, p, op, p.images));
    }
}

// the form of op i in a call of `images` images: the table's, except for the ops whose form reads the call (ConvForm::reads_images), which a partial pass
// resolves again into `called`
const ConvForm& form_of(const sd_handle* h, sd_net net, size_t i, int images, ConvForm& called) {
    const NetPlan& p = plan_of(h, net);
    const ConvForm& f = h->forms[net][i];
    return images == p.images || !f.reads_images ? f : called = resolve_conv_form({h->sw, h->small_batch, h->cus}, p, p.ops[i], images);
}

// sd_set_small_batch: the partial sums of the largest split layer (a chunk-split direct layer keeps them at conv resolution: before a fused pool)
size_t splitk_scratch_bytes(const sd_handle* h) {
    size_t mx = 0;
    for (sd_net net : {SD_NET_FCN8S, SD_NET_MONODEPTH})
        for (size_t i = 0; i < h->forms[net].size(); ++i) {
            const NetPlan& p = plan_of(h, net);
            const OpDesc& op = p.ops[i];
            if (const int S = h->forms[net][i].slices; S > 1)
                mx = std::max(mx, (size_t)S * p.images * (p.tensors[op.dst].H << op.fuse_pool) * (p.tensors[op.dst].W << op.fuse_pool) * p.tensors[op.dst].C * sizeof(float));
        }
    return mx;
}

void carve_workspace(sd_handle* h) {
    h->a = Arena({h->max_batch, h->H, h->W, h->cap, h->fcn.act_bytes, h->mono.act_bytes, splitk_scratch_bytes(h)});
}
// the arena's regions as pointers: the only places that add to h->ws
template <class T = char> T* at(sd_handle* h, size_t off) { return reinterpret_cast<T*>(h->ws + off); }
char* act_base(sd_handle* h, sd_net net) { return at(h, net == SD_NET_FCN8S ? h->a.fcn : h->a.mono); }
void* zero_page(sd_handle* h) { return at(h, h->a.zero); }      // the arena is zero-filled there and nothing writes it

sd_status upload_tables(sd_handle* h, sd_net net) {
    NetPlan& p = plan_of(h, net);
    char* wbase = warena(h, net);
    const char* abase = act_base(h, net);
    for (const OpDesc& op : p.ops) {
        if (op.kind == OP_CONV_DIRECT) {
            std::vector<DirectChunk> chunks;
            build_direct_chunks(p, op, abase, chunks);
            HIPCHK(h, hipMemcpy(wbase + op.tab_offset, chunks.data(), chunks.size() * sizeof(DirectChunk), hipMemcpyHostToDevice));
            continue;
        }
        if (op.kind != OP_CONV) continue;
        std::vector<KEntry> ktab;
        build_conv_tables(p, op, abase, wbase + op.tab_offset, ktab);
        HIPCHK(h, hipMemcpy(wbase + op.tab_offset, ktab.data(), ktab.size() * sizeof(KEntry), hipMemcpyHostToDevice));
    }
    return SD_OK;
}

struct HeadOut { float* logits; uint8_t* road; uint8_t* fence; uint8_t* argmax; };

// next event of the handle's profiling pool (created on demand), nullptr on failure
static hipEvent_t prof_event(sd_handle* h) {
    if (h->prof_used == h->prof_pool.size()) {
        hipEvent_t a;
        if (hipEventCreate(&a) != hipSuccess) return nullptr;
        h->prof_pool.push_back(a);
    }
    return h->prof_pool[h->prof_used++];
}

// the fp16 clamp counters (SatLayout, handle_arena.hpp)
size_t sat_bytes(int max_batch) { return SatLayout(max_batch).total; }
unsigned long long* sat_counter(sd_handle* h) { return at<unsigned long long>(h, h->a.sat + SatLayout(h->max_batch).count); }
unsigned* sat_img(sd_handle* h) { return at<unsigned>(h, h->a.sat + SatLayout(h->max_batch).img); }
int sat_img_slots(sd_handle* h) { return (int)SatLayout(h->max_batch).img_slots; }
unsigned* sat_frames(sd_handle* h) { return at<unsigned>(h, h->a.sat + SatLayout(h->max_batch).frames); }
unsigned* sat_orphans(sd_handle* h) { return at<unsigned>(h, h->a.sat + SatLayout(h->max_batch).orphans); }

// one chunk through a plan.  frames: u8 [nframes,H,W,3] (device), frames frame0.. of the caller's batch
sd_status run_plan(sd_handle* h, sd_net net, const uint8_t* frames, int frame0, int nframes, const HeadOut* head, hipStream_t s) {
    NetPlan& p = plan_of(h, net);
    char* wbase = warena(h, net);
    char* abase = act_base(h, net);
    const int N = nframes * (p.images / p.frames);
    auto T = [&](int t) -> float* { return reinterpret_cast<float*>(abase + p.tensors[t].offset); };
    auto Wp = [&](int w) -> const float* { return reinterpret_cast<const float*>(wbase + p.weights[w].offset); };
    auto PL = [&](int t) -> size_t { const TensorDesc& d = p.tensors[t]; return (size_t)p.images * d.H * d.W * d.C; };   // lo-plane offset
    // algorithmic HBM bytes of a conv op for N of the plan's images: sources + output once, + the weights (sd_profile_bucket::bytes)
    auto op_bytes = [&](const OpDesc& op) -> double {
        double b = 0;
        for (int j = 0; j < op.nsrc; ++j) b += (double)p.tensors[op.src[j]].bytes;
        if (op.dst >= 0) b += (double)p.tensors[op.dst].bytes;
        b = b * N / p.images;
        if (op.w >= 0) b += (double)p.weights[op.w].bytes;
        return b;
    };
    // a conv launch in a profiling bracket: its start event is the end event of the conv launched right before it when nothing else came between
    // (sd_handle::prof_pool).  M x Nc: the record's GEMM extent; `kernel` names the launch for the record
    auto bracketed = [&](const OpDesc& op, hipError_t& e, int M, int Nc, auto&& launch, const char* kernel, double extra_bytes = -1.0) -> sd_status {
        // (extra_bytes >= 0: a launch that carries none of the op's algorithmic work -- the reduce half of a split-K layer: its record holds these bytes)
        if (!h->prof) { e = launch(); return SD_OK; }
        hipEvent_t ea = h->prof_last, eb = nullptr;
        if (!ea) { if (!(ea = prof_event(h))) return fail(h, SD_ERR_HIP, "hipEventCreate"); hipEventRecord(ea, s); }
        if (!(eb = prof_event(h))) return fail(h, SD_ERR_HIP, "hipEventCreate");
        e = launch();
        hipEventRecord(eb, s);
        h->prof_last = eb;
        h->prof_recs.push_back({kernel, extra_bytes >= 0 ? 0.0 : op.flops * N / p.images, ea, eb, op.name.c_str(), M, Nc, op.K, extra_bytes >= 0 ? extra_bytes : op_bytes(op)});
        return SD_OK;
    };
    for (const WeightSlot& wsl : p.weights)
        if (!wsl.loaded) return fail(h, SD_ERR_STATE, "weight not loaded: " + wsl.name);
    h->prof_last = nullptr;                 // (other work may have been put on the stream since the previous call)
    const bool verbose = (h->sw & SW_PROFILE_VERBOSE) != 0;
    ConvForm called;        // (a partial pass: the record of an op whose form reads the call)
    for (size_t i = 0; i < p.ops.size(); ++i) {
        const OpDesc& op = p.ops[i];
        hipError_t e = hipSuccess;
        sd_status st = SD_OK;
        // conv ops: the handle's form names the launcher and its variant (DESIGN.md "which kernel runs a layer"); here only pointers and the call's size are filled in
        const ConvForm& f = form_of(h, net, i, N, called);
        const char* const label = (verbose ? f.verbose : f.label).c_str();
        switch (op.kind) {
            case OP_PRE_VGG:
                e = launch_pre_vgg(frames, T(op.dst), (long)nframes * h->H * h->W, p.tensors[op.dst].fmt, PL(op.dst), s);
                break;
            case OP_PRE_MONO:
                e = launch_pre_mono(frames, T(op.dst), nframes, h->H, h->W, p.tensors[op.dst].fmt, PL(op.dst), p.input_scale == 1.f ? 1 : 0, s);
                break;
            case OP_CONV: {
                if (f.error) return fail(h, SD_ERR_STATE, f.error);
                const TensorDesc& d = p.tensors[op.dst];
                ConvParams c = f.conv;
                c.N = N; c.wt = Wp(op.w); c.bias = Wp(op.b); c.ktab = reinterpret_cast<const KEntry*>(wbase + op.tab_offset);
                c.residual = op.residual >= 0 ? T(op.residual) : nullptr;
                c.out = T(op.dst); c.out_plane = PL(op.dst); c.src0 = T(op.src[0]); c.src0_plane = PL(op.src[0]);
                c.zero16 = zero_page(h);
                c.alpha = op.scheme == SC_HS ? 1.f / p.weights[op.w].wscale : 1.f;
                c.reserve_cus = h->reserve_cus; c.sat = sat_counter(h);
                c.rowgrp = f.rowgrp && N % f.rowgrp == 0 ? f.rowgrp : 0;      // CALL-DEPENDENT (conv_form.cpp): row groups only when the call's images fill them
                const int M = N * c.Hout * c.Wout * (c.fold ? 4 : 1);
                if (f.family == CF_SPLITK) {
                    // sd_set_small_batch: the k-range form of the HS ring into the partial-sum scratch, then the reduce launch with the layer's epilogue
                    c.partial = at<float>(h, h->a.splitk);
                    st = bracketed(op, e, M, d.C, [&] { return launch_conv_dma3(c, f.variant, f.s16, s); }, label);
                    if (st != SD_OK || e != hipSuccess) break;
                    st = bracketed(op, e, M, d.C, [&] { return launch_splitk_reduce(c, s); }, "splitk_reduce_kernel",
                                   (double)M * d.C * (f.slices * sizeof(float) + elem_bytes(d.fmt)));
                    break;
                }
                st = bracketed(op, e, M, d.C, [&] {
                    switch (f.family) {
                        case CF_DMA3: return launch_conv_dma3(c, f.variant, f.s16, s);
                        case CF_DMA: return launch_conv_dma(c, f.variant, s);
                        case CF_STEM: return launch_conv_stem(c, s);
                        case CF_SPLIT: return launch_conv_split(c, f.variant, s);
                        case CF_IGEMM: return launch_conv_igemm(c, s);
                        default: return hipErrorInvalidValue;
                    }
                }, label);
                break;
            }
            case OP_CONV_DIRECT: {
                const TensorDesc& d = p.tensors[op.dst];
                ConvDirectParams c = f.dir;
                c.N = N; c.chunks = reinterpret_cast<const DirectChunk*>(wbase + op.tab_offset);
                c.wt = reinterpret_cast<const u32x4_t*>(Wp(op.w)); c.bias = Wp(op.b); c.out = T(op.dst); c.out_plane = PL(op.dst);
                c.zero16 = zero_page(h);
                c.alpha = op.scheme == SC_HS ? 1.f / p.weights[op.w].wscale : 1.f;
                c.reserve_cus = h->reserve_cus; c.sat = sat_counter(h);
                if (f.family == CF_DIRECT_SPLITC) {
                    // sd_set_small_batch level 2: the chunk-range form into the partial-sum scratch, then the reduce launch with the layer's epilogue
                    c.partial = at<float>(h, h->a.splitk);
                    st = bracketed(op, e, N * c.H * c.W, d.C, [&] { return launch_conv_direct_splitc(c, s); }, label);
                    if (st != SD_OK || e != hipSuccess) break;
                    st = bracketed(op, e, N * c.H * c.W, d.C, [&] { return launch_splitc_reduce(c, s); }, "splitc_reduce_kernel",
                                   (double)N * d.C * ((double)c.H * c.W * f.slices * sizeof(float) + (double)d.H * d.W * elem_bytes(d.fmt)));
                    break;
                }
                st = bracketed(op, e, N * c.H * c.W, d.C,
                               [&] { return f.family == CF_DIRECT3 ? launch_conv_direct3(c, f.direct, s) : launch_conv_direct(c, f.direct, s); }, label);
                break;
            }
            case OP_DEC_TAIL1: {
                const TensorDesc& d = p.tensors[op.dst];
                DecTailParams c{};
                c.a = T(op.src[0]); c.a_plane = PL(op.src[0]); c.d2 = T(op.src[1]); c.d_plane = PL(op.src[1]);
                c.N = N; c.H = d.H; c.W = d.W;
                c.w1 = reinterpret_cast<const u32x4_t*>(Wp(op.w)); c.b1 = Wp(op.b);
                c.w2 = reinterpret_cast<const u32x4_t*>(Wp(op.w2)); c.b2 = Wp(op.b2);
                c.wd = Wp(op.w3); c.bd = Wp(op.b3);
                c.out = T(op.dst); c.sw = h->sw; c.reserve_cus = h->reserve_cus;
                c.scheme = engine_forms(p.engine).conv;
                const bool hs = c.scheme == SC_HS;
                c.alpha = hs ? 1.f / p.weights[op.w].wscale : 1.f; c.alpha2 = hs ? 1.f / p.weights[op.w2].wscale : 1.f;
                st = bracketed(op, e, N * d.H * d.W, 16, [&] { return launch_dec_tail1(c, s); }, label);
                break;
            }
            case OP_SMALLN: {
                const TensorDesc& s0 = p.tensors[op.src[0]];
                SmallNParams c{};
                c.x = T(op.src[0]); c.N = N; c.H = s0.H; c.W = s0.W; c.C = s0.C; c.k = op.k; c.nout = op.nout;
                c.wt = Wp(op.w); c.bias = Wp(op.b); c.out = T(op.dst); c.act = op.act;
                c.in_fmt = s0.fmt; c.out_fmt = p.tensors[op.dst].fmt; c.in_plane = PL(op.src[0]); c.out_plane = PL(op.dst);
                c.in_sub = s0.planar16 ? (size_t)p.images * s0.H * s0.W * 16 : 0;
                c.out_c = p.tensors[op.dst].C;
                c.zero16 = zero_page(h);
                c.sw = h->sw;
                e = launch_conv_smalln(c, s);
                break;
            }
            case OP_POOL2: {
                const TensorDesc& s0 = p.tensors[op.src[0]];
                e = launch_maxpool2(T(op.src[0]), T(op.dst), N, s0.H, s0.W, s0.C, s0.fmt, PL(op.src[0]), PL(op.dst), s);
                break;
            }
            case OP_POOL3Z: {
                const TensorDesc& s0 = p.tensors[op.src[0]];
                e = launch_maxpool3z(T(op.src[0]), T(op.dst), N, s0.H, s0.W, s0.C, s0.fmt, PL(op.src[0]), PL(op.dst), s0.planar16 ? p.images : 0, s);
                break;
            }
            case OP_DECONV4_ADD: {
                const TensorDesc& s0 = p.tensors[op.src[0]];
                e = launch_deconv4s2_add(T(op.src[0]), Wp(op.w), Wp(op.b), T(op.residual), T(op.dst), N, s0.H, s0.W, s);
                break;
            }
            case OP_HEAD16: {
                const TensorDesc& s0 = p.tensors[op.src[0]];
                e = launch_deconv16s8_head(T(op.src[0]), Wp(op.w), Wp(op.b), N, s0.H, s0.W, head->logits, head->road, head->fence,
                                           head->argmax, s);
                break;
            }
        }
        if (st != SD_OK) return st;
        if (op.kind != OP_CONV && op.kind != OP_CONV_DIRECT && op.kind != OP_DEC_TAIL1)
            h->prof_last = nullptr;                 // something else went onto the stream: the next conv records its own start
        if (e != hipSuccess) return fail(h, SD_ERR_HIP, "launch " + op.name + ": " + hipGetErrorString(e));
    }
    (net == SD_NET_FCN8S ? h->last_fcn_images : h->last_mono_images) = N;
    // the pass's per-image clamp counts -> the counts of frames frame0.. (a monodepth frame's fliplr copy is its own frame's)
    HIPCHK(h, launch_sat_fold(sat_img(h), sat_frames(h) + frame0, sat_orphans(h), N,
                              p.images / p.frames == 2 ? 1 : 0, sat_img_slots(h), s));
    return SD_OK;
}

CamDev make_cam(const sd_camera& c) {
    // np.float32([[1,0,0,-cx],[0,-1,0,cy],[0,0,0,-f],[0,0,1/b,0]]) then promoted to double by OpenCV
    CamDev d;
    const float q[16] = {1.f, 0.f, 0.f, (float)(-c.cx), 0.f, -1.f, 0.f, (float)c.cy, 0.f, 0.f, 0.f, (float)(-c.f), 0.f, 0.f, (float)(1.0 / c.b), 0.f};
    for (int i = 0; i < 16; ++i) d.q[i] = (double)q[i];
    d.mult = (float)c.disp_mult;
    return d;
}

int32_t* cnt_slot(sd_handle* h, CntSlot i) { return at<int32_t>(h, h->a.cnt) + (size_t)i * h->max_batch; }

}  // namespace

extern "C" {

#ifndef SD_DEFAULT_PLAN_FCN
#define SD_DEFAULT_PLAN_FCN "conv1_2,conv3_3:x,conv4_1:x,conv4_2:1,conv4_3:1,conv5_1:1,conv5_2:1,conv5_3:1,fc6:1,fc7:1"
#endif
#ifndef SD_DEFAULT_PLAN_MONO
#define SD_DEFAULT_PLAN_MONO "enc/conv1,enc/res*:1,dec/upconv*:1,dec/iconv*:1,dec/disp4,dec/disp3,dec/disp1"
#endif
#ifndef SD_SOURCE_HASH
#define SD_SOURCE_HASH "unhashed"
#endif
// "... src=<hash>": sha256 prefix of the sources this binary was built from (semantic_depth_amd/build.py source_hash);
// the Python loader refuses a library whose hash differs from the tree's
const char* sd_version(void) { return "semdepth 0.4 (gfx950; f32 MFMA, split-bf16 x2 / x3 and fp16 MFMA) src=" SD_SOURCE_HASH; }

const char* sd_status_string(sd_status s) {
    switch (s) {
        case SD_OK: return "ok";
        case SD_ERR_INVALID: return "invalid argument";
        case SD_ERR_HIP: return "HIP error";
        case SD_ERR_STATE: return "invalid state";
        case SD_ERR_NOTFOUND: return "not found";
        case SD_ERR_FORMAT: return "not a JPEG file";
        default: return "unknown";
    }
}

// the default precision plan (SD_PREC_PLAN): the output of scripts/calibrate_precision.py on the MI355X (per-group error of the
// 2-product form against the exact-f32 engine, greedy by error per saved product under 3e-4 per network on 4 frames of 512 x 1024;
// profiles/r02_precision_calibration.json; DESIGN.md §3 "Precision plan" has the table).  FCN-8s: 69 % of its FLOPs on two products
// at 2.9e-4 (left on three: conv1_1, conv2_1, conv3_x, conv4_1 -- the layers whose INPUT tensor also feeds a score head, or whose
// own error is ~2e-4), monodepth-resnet50: 96 % at 2.7e-4 (left on three: the stem and decoder levels 3 and 2).
static const char* const kDefaultPlanFcn = SD_DEFAULT_PLAN_FCN;
static const char* const kDefaultPlanMono = SD_DEFAULT_PLAN_MONO;

static sd_status create_impl(sd_handle** out, int device, int H, int W, int max_batch, sd_encoder enc, sd_precision prec,
                             const char* fcn_f16, const char* mono_f16);

sd_status sd_create(sd_handle** out, int device, int H, int W, int max_batch, sd_encoder enc, sd_precision prec) {
    if (prec != SD_PREC_F32 && prec != SD_PREC_BF16X2 && prec != SD_PREC_MIXED && prec != SD_PREC_PLAN && prec != SD_PREC_BF16X3 && prec != SD_PREC_F16X2)
        return SD_ERR_INVALID;
    const char* fcn = prec == SD_PREC_PLAN ? kDefaultPlanFcn : "";
    // (the calibrated monodepth plan names ResNet-50 layers; the vgg encoder -- the ill-conditioned one of the two in the tests --
    //  stays on three products under SD_PREC_PLAN)
    const char* mono = prec == SD_PREC_PLAN ? (enc == SD_ENC_RESNET50 ? kDefaultPlanMono : "") : (prec == SD_PREC_MIXED ? "*" : "");
    return create_impl(out, device, H, W, max_batch, enc, prec, fcn, mono);
}

sd_status sd_create_with_plan(sd_handle** out, int device, int H, int W, int max_batch, sd_encoder enc, const char* fcn_f16_layers,
                              const char* mono_f16_layers) {
    return create_impl(out, device, H, W, max_batch, enc, SD_PREC_PLAN, fcn_f16_layers ? fcn_f16_layers : "", mono_f16_layers ? mono_f16_layers : "");
}

const char* sd_default_plan(sd_net net) { return net == SD_NET_FCN8S ? kDefaultPlanFcn : kDefaultPlanMono; }

sd_status sd_precision_plan(const sd_handle* h, sd_net net, char* layers_out, size_t cap, double* flop_share_out) {
    if (!h) return SD_ERR_INVALID;
    const NetPlan& p = plan_of(h, net);
    if (layers_out && cap) { std::strncpy(layers_out, p.f16_ops.c_str(), cap - 1); layers_out[cap - 1] = 0; }
    if (flop_share_out) *flop_share_out = p.flops_per_image > 0 ? p.flops_f16 / p.flops_per_image : 0.0;
    return p.f16_ops.size() + 1 > cap && layers_out ? SD_ERR_INVALID : SD_OK;
}

// the conv engine of a precision: SD_PREC_MIXED and SD_PREC_PLAN are the bf16 x 2 engine with a precision plan (sd_create)
static Engine engine_of(sd_precision prec) {
    switch (prec) {
        case SD_PREC_F32: return ENG_F32;
        case SD_PREC_BF16X3: return ENG_BF16X3;
        case SD_PREC_F16X2: return ENG_F16X2;
        default: return ENG_BF16X2;
    }
}

static sd_status create_impl(sd_handle** out, int device, int H, int W, int max_batch, sd_encoder enc, sd_precision prec,
                             const char* fcn_f16, const char* mono_f16) {
    if (!out || H <= 0 || W <= 0 || max_batch <= 0) return SD_ERR_INVALID;
    {
        const std::string bad = sd_disable_unknown();
        if (!bad.empty()) {
            std::fprintf(stderr, "sd_create: SEMDEPTH_DISABLE names no switch '%s' (dma dma3 direct stem fold tail1 pool_fuse planar n16 fuse1 fuse4 flat rowskip dma_big mfma16 png_waves)\n", bad.c_str());
            return SD_ERR_INVALID;
        }
    }
    sd_handle* h = new sd_handle();
    h->sw = latch_switches();
    if (const char* e = std::getenv("SEMDEPTH_RESERVE_CUS")) h->reserve_cus = std::min(128, std::max(0, atoi(e)));
    h->device = device; h->H = H; h->W = W; h->max_batch = max_batch; h->enc = (int)enc; h->cap = H * W; h->prec = (int)prec;
    int chunk = 32;      // frames per network pass: the deep layers (M = 512 px per frame) need ~32 frames to fill 256 CUs;
                         // activations of a 32-frame chunk are ~17 GB at 512x1024, nothing on a 288 GB part
    if (const char* e = std::getenv("SEMDEPTH_CHUNK")) chunk = std::max(1, atoi(e));
    h->chunk = std::min(max_batch, chunk);
    try {
        const Engine eng = engine_of(prec);
        h->fcn = build_fcn8s(h->chunk, H, W, eng, fcn_f16);
        h->mono = build_monodepth(enc == SD_ENC_VGG ? 0 : 1, h->chunk, H, W, eng, mono_f16);
    } catch (const std::exception& ex) {
        std::fprintf(stderr, "sd_create: %s\n", ex.what());
        delete h;
        return SD_ERR_INVALID;
    }
    resolve_forms(h);
    carve_workspace(h);
    if (!h->a.fence_views_fit) {      // (cannot happen at any size in use: 15 bytes per point against the 161 of the Open3D region)
        std::fprintf(stderr, "sd_create: the fence chain's views do not fit the Open3D scratch\n");
        delete h;
        return SD_ERR_STATE;
    }
    *out = h;
    return SD_OK;
}

sd_status sd_destroy(sd_handle* h) {
    if (h)
        for (hipEvent_t e : h->prof_pool) hipEventDestroy(e);      // (the library owns no device memory; the profiling events are its only HIP objects)
    delete h;
    return SD_OK;
}

const char* sd_last_error(const sd_handle* h) { return h ? h->err.c_str() : "null handle"; }

sd_status sd_query_memory(const sd_handle* h, size_t* fcn_w, size_t* mono_w, size_t* ws) {
    if (!h) return SD_ERR_INVALID;
    if (fcn_w) *fcn_w = h->fcn.weight_bytes;
    if (mono_w) *mono_w = h->mono.weight_bytes;
    if (ws) *ws = h->a.total;
    return SD_OK;
}

sd_status sd_bind_memory(sd_handle* h, void* wf, void* wm, void* ws) {
    if (!h || !wf || !wm || !ws) return SD_ERR_INVALID;
    HIPCHK(h, hipSetDevice(h->device));
    h->wf = (char*)wf; h->wm = (char*)wm; h->ws = (char*)ws;
    h->bound = true;
    HIPCHK(h, hipMemset(at(h, h->a.scalar), 0, kScalarSlotBytes + kZeroPageBytes));      // the scalar slot and the zero page behind it
    HIPCHK(h, hipMemset(sat_counter(h), 0, sat_bytes(h->max_batch)));      // the clamp counters
    sd_status st = upload_tables(h, SD_NET_FCN8S);
    if (st != SD_OK) return st;
    return upload_tables(h, SD_NET_MONODEPTH);
}

int sd_weight_count(const sd_handle* h, sd_net net) { return h ? (int)plan_of(h, net).weights.size() : 0; }

sd_status sd_weight_info(const sd_handle* h, sd_net net, int index, char* name_out, int64_t* shape_out, int* rank_out) {
    if (!h) return SD_ERR_INVALID;
    const NetPlan& p = plan_of(h, net);
    if (index < 0 || index >= (int)p.weights.size()) return SD_ERR_INVALID;
    const WeightSlot& s = p.weights[index];
    if (name_out) { std::strncpy(name_out, s.name.c_str(), 63); name_out[63] = 0; }
    if (shape_out) for (int i = 0; i < 4; ++i) shape_out[i] = s.shape[i];
    if (rank_out) *rank_out = s.rank;
    return SD_OK;
}

sd_status sd_load_weight(sd_handle* h, sd_net net, const char* name, const float* data, const int64_t* shape, int rank) {
    if (!h || !name || !data || !shape) return SD_ERR_INVALID;
    if (!h->bound) return fail(h, SD_ERR_STATE, "sd_bind_memory first");
    NetPlan& p = plan_of(h, net);
    auto it = p.weight_by_name.find(name);
    if (it == p.weight_by_name.end()) return fail(h, SD_ERR_NOTFOUND, std::string("unknown weight ") + name);
    WeightSlot& s = p.weights[it->second];
    if (rank != s.rank) return fail(h, SD_ERR_INVALID, std::string("rank mismatch for ") + name);
    for (int i = 0; i < rank; ++i)
        if (shape[i] != s.shape[i]) return fail(h, SD_ERR_INVALID, std::string("shape mismatch for ") + name);
    std::vector<float> scaled;
    size_t nel = 1;
    for (int i = 0; i < rank; ++i) nel *= (size_t)shape[i];
    if (s.scale != 1.f) {               // (monodepth stem with integer input: the weights carry the 1/255)
        scaled.resize(nel);
        for (size_t i = 0; i < nel; ++i) scaled[i] = data[i] * s.scale;
        data = scaled.data();
    }
    const int idx = it->second;
    // re-layout + upload of one slot from its TensorFlow-layout tensor
    auto upload = [&](int j, const float* w) -> sd_status {
        WeightSlot& t = p.weights[j];
        std::vector<float> buf;
        relayout_weight(t, w, buf);
        char* base = warena(h, net) + t.offset;
        if (t.layout == WL_IGEMM) {                     // rows [k_off, k_off+Kpad) of a [Ktotal/4][CoutPad][4] matrix
            HIPCHK(h, hipMemcpy(base + (size_t)t.k_off * t.CoutPad * 4, buf.data(), t.bytes, hipMemcpyHostToDevice));
        } else if (t.layout == WL_IGEMM_SPLIT) {        // the same rows in the hi plane and in the lo plane
            const size_t plane = (size_t)t.Ktotal * t.CoutPad * 2, rows = (size_t)t.Kpad * t.CoutPad * 2, ro = (size_t)t.k_off * t.CoutPad * 2;
            HIPCHK(h, hipMemcpy(base + ro, buf.data(), rows, hipMemcpyHostToDevice));
            HIPCHK(h, hipMemcpy(base + plane + ro, reinterpret_cast<char*>(buf.data()) + rows, rows, hipMemcpyHostToDevice));
            if (t.planes == WP_BF16X3) HIPCHK(h, hipMemcpy(base + 2 * plane + ro, reinterpret_cast<char*>(buf.data()) + 2 * rows, rows, hipMemcpyHostToDevice));
        } else {
            const int root = t.owner >= 0 ? t.owner : j;
            bool grouped = t.owner >= 0;
            for (const WeightSlot& o : p.weights) grouped = grouped || (o.owner == root && o.layout == WL_RAW && &o != &t);
            if (grouped && t.layout == WL_RAW && t.rank == 1) {      // summed bias group (ResNet conv3 + projection)
                h->bias_host[{(int)net, j}] = buf;
                std::vector<float> sum(buf.size(), 0.f);
                for (int q = 0; q < (int)p.weights.size(); ++q)
                    if (q == root || p.weights[q].owner == root) {
                        auto f = h->bias_host.find({(int)net, q});
                        if (f != h->bias_host.end()) for (size_t i = 0; i < sum.size(); ++i) sum[i] += f->second[i];
                    }
                HIPCHK(h, hipMemcpy(base, sum.data(), t.bytes, hipMemcpyHostToDevice));
            } else {
                HIPCHK(h, hipMemcpy(base, buf.data(), t.bytes, hipMemcpyHostToDevice));
            }
        }
        return SD_OK;
    };
    if (s.planes == WP_HS) {
        // SD_PREC_F16X2: the planes hold w' = w * 2^k in fp16 (hi + lo), k chosen HERE per layer so that the largest stored |w'| lies in
        // [2^12, 2^13) -- any finite f32 weight tensor loads (round 5 used a fixed 2^12 and refused |w| >= 16), and a layer of tiny weights
        // keeps the low plane's bits.  A stored value of an upsample-folded layer is a sum of up to four taps: bounded by 4 max |w|.  Slots
        // that feed ONE accumulator (ResNet conv3 + projection shortcut) share the scale: the members' tensors are kept on the host and the
        // ones already loaded are laid out again when a later member moves the group's exponent.
        const int root = s.owner >= 0 ? s.owner : idx;
        std::vector<int> members;
        for (int j = 0; j < (int)p.weights.size(); ++j)
            if ((j == root || p.weights[j].owner == root) && p.weights[j].planes == WP_HS) members.push_back(j);
        const bool grouped = members.size() > 1;
        for (size_t i = 0; i < nel; ++i)
            if (!std::isfinite(data[i])) return fail(h, SD_ERR_INVALID, std::string("weight ") + name + ": non-finite value");
        if (grouped) h->w_host[{(int)net, idx}].assign(data, data + nel);
        float mx = 0.f;
        auto amax = [&](const float* w, size_t n, const WeightSlot& t) {
            float m = 0.f;
            for (size_t i = 0; i < n; ++i) m = std::max(m, std::fabs(w[i]));
            return m * ((t.fold || t.layout == WL_TAIL_UP) ? 4.f : 1.f);
        };
        mx = amax(data, nel, s);
        if (grouped)
            for (int j : members) {
                auto f = h->w_host.find({(int)net, j});
                if (j != idx && f != h->w_host.end()) mx = std::max(mx, amax(f->second.data(), f->second.size(), p.weights[j]));
            }
        int k = 12;
        if (mx > 0.f) k = std::min(100, std::max(-100, 12 - std::ilogb(mx)));
        const float wscale = std::ldexp(1.f, k);
        const bool moved = wscale != p.weights[root].wscale;
        for (int j : members) p.weights[j].wscale = wscale;
        if (grouped && moved)
            for (int j : members) {
                auto f = h->w_host.find({(int)net, j});
                if (j != idx && p.weights[j].loaded && f != h->w_host.end()) {
                    sd_status st = upload(j, f->second.data());
                    if (st != SD_OK) return st;
                }
            }
    }
    {
        sd_status st = upload(idx, data);
        if (st != SD_OK) return st;
    }
    s.loaded = true;
    return SD_OK;
}

sd_status sd_fcn8s_forward(sd_handle* h, const uint8_t* frames, int B, float* logits, uint8_t* road, uint8_t* fence,
                           uint8_t* argmax, void* stream) {
    if (!h || !frames || B <= 0 || B > h->max_batch) return fail(h, SD_ERR_INVALID, "sd_fcn8s_forward: bad arguments");
    if (!h->bound) return fail(h, SD_ERR_STATE, "sd_bind_memory first");
    const size_t npix = (size_t)h->H * h->W;
    for (int b0 = 0; b0 < B; b0 += h->chunk) {
        const int nb = std::min(h->chunk, B - b0);
        HeadOut ho{logits ? logits + (size_t)b0 * npix * 3 : nullptr, road ? road + (size_t)b0 * npix : nullptr,
                   fence ? fence + (size_t)b0 * npix : nullptr, argmax ? argmax + (size_t)b0 * npix : nullptr};
        sd_status st = run_plan(h, SD_NET_FCN8S, frames + (size_t)b0 * npix * 3, b0, nb, &ho, (hipStream_t)stream);
        if (st != SD_OK) return st;
    }
    return SD_OK;
}

// OpenCV's scalar INTER_CUBIC tables for one axis (imgproc/resize.cpp: resize() + interpolateCubic, A = -0.75, weights as
// cvRound(w * 2048) int16, tap indices replicated at the borders); mirrored by oracle/resize.py
static void resize_tables(int dst, int src, int* idx, int* wgt) {
    const double inv = (double)dst / (double)src, scale = 1.0 / inv;
    for (int d = 0; d < dst; ++d) {
        float f = (float)((d + 0.5) * scale - 0.5);
        const int s = (int)std::floor(f);
        const float x = f - (float)s;
        const float A = -0.75f;
        float c[4];
        c[0] = ((A * (x + 1.f) - 5.f * A) * (x + 1.f) + 8.f * A) * (x + 1.f) - 4.f * A;
        c[1] = ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f;
        const float xm = 1.f - x;
        c[2] = ((A + 2.f) * xm - (A + 3.f)) * xm * xm + 1.f;
        c[3] = 1.f - c[0] - c[1] - c[2];
        for (int k = 0; k < 4; ++k) {
            long v = std::lrint((double)(c[k] * 2048.f));          // cvRound: round half to even
            v = v < -32768 ? -32768 : (v > 32767 ? 32767 : v);
            wgt[d * 4 + k] = (int)v;
            int i = s - 1 + k;
            idx[d * 4 + k] = i < 0 ? 0 : (i > src - 1 ? src - 1 : i);
        }
    }
}

// the tap tables of one resize geometry in the workspace slot at `off` (uploaded when the geometry changed; the upload waits for the
// stream first, because the previous tables may still be in use)
static sd_status upload_resize_tables(sd_handle* h, size_t off, int* key_store, std::vector<int>& host, int src_h, int src_w, int dst_h,
                                      int dst_w, hipStream_t s, int** xi, int** xa, int** yi, int** ya) {
    const RszLayout l;
    int* dev = at<int>(h, off);
    *xi = at<int>(h, off + l.xi); *xa = at<int>(h, off + l.xa); *yi = at<int>(h, off + l.yi); *ya = at<int>(h, off + l.ya);
    const int key[4] = {src_h, src_w, dst_h, dst_w};
    if (std::memcmp(key, key_store, sizeof(key)) != 0) {
        HIPCHK(h, hipStreamSynchronize(s));
        host.assign(l.total / sizeof(int), 0);        // (the host copy has the same layout)
        int* hx = host.data();
        resize_tables(dst_w, src_w, hx + l.xi / sizeof(int), hx + l.xa / sizeof(int));
        resize_tables(dst_h, src_h, hx + l.yi / sizeof(int), hx + l.ya / sizeof(int));
        HIPCHK(h, hipMemcpy(dev, hx, host.size() * sizeof(int), hipMemcpyHostToDevice));
        std::memcpy(key_store, key, sizeof(key));
    }
    return SD_OK;
}

sd_status sd_resize_cubic_u8(sd_handle* h, const uint8_t* src, int B, int src_h, int src_w, int channels, uint8_t* dst, int dst_h,
                             int dst_w, void* stream) {
    if (!h || !src || !dst || B <= 0 || src_h <= 0 || src_w <= 0 || channels <= 0 || channels > 4 || dst_h <= 0 || dst_w <= 0 ||
        dst_h > RSZ_MAX || dst_w > RSZ_MAX)
        return fail(h, SD_ERR_INVALID, "sd_resize_cubic_u8: bad arguments (destination extent at most 16384)");
    if (!h->bound) return fail(h, SD_ERR_STATE, "sd_bind_memory first");
    hipStream_t s = (hipStream_t)stream;
    if (src_h == dst_h && src_w == dst_w) {                        // cv2.resize returns a copy
        HIPCHK(h, hipMemcpyAsync(dst, src, (size_t)B * src_h * src_w * channels, hipMemcpyDeviceToDevice, s));
        return SD_OK;
    }
    int *xi, *xa, *yi, *ya;
    const sd_status st = upload_resize_tables(h, h->a.rsz, h->rsz_key, h->rsz_host, src_h, src_w, dst_h, dst_w, s, &xi, &xa, &yi, &ya);
    if (st != SD_OK) return st;
    HIPCHK(h, launch_resize_cubic_u8(src, dst, B, src_h, src_w, dst_h, dst_w, channels, xi, xa, yi, ya, s));
    return SD_OK;
}

sd_status sd_jpeg_reconstruct_workspace(const sd_jpeg_frame_desc* descs_host, int B, size_t* bytes_out) {
    if (!descs_host || B <= 0 || !bytes_out) return SD_ERR_INVALID;
    for (int b = 0; b < B; ++b)
        if (!sdjpeg::desc_ok(descs_host[b])) return SD_ERR_INVALID;
    *bytes_out = sdjpeg::workspace_bytes(descs_host, B);
    return SD_OK;
}

sd_status sd_jpeg_reconstruct_bgr(sd_handle* h, const int16_t* coef_dev, size_t frame_stride_bytes, const sd_jpeg_frame_desc* descs_host, int B,
                                  uint8_t* bgr_dev, size_t bgr_frame_stride, void* workspace_dev, size_t workspace_bytes, void* stream) {
    if (!h || !coef_dev || !descs_host || B <= 0 || !bgr_dev || !workspace_dev)
        return fail(h, SD_ERR_INVALID, "sd_jpeg_reconstruct_bgr: bad arguments");
    // the kernels read a block as 16-byte pieces and store plane rows as 8-byte pieces
    if ((reinterpret_cast<uintptr_t>(coef_dev) & 15) || (frame_stride_bytes & 15) || (reinterpret_cast<uintptr_t>(workspace_dev) & 15))
        return fail(h, SD_ERR_INVALID, "sd_jpeg_reconstruct_bgr: coef_dev, frame_stride_bytes and workspace_dev must be multiples of 16");
    // every index the kernels form follows from a consistent descriptor and these three capacities: nothing is launched otherwise
    for (int b = 0; b < B; ++b) {
        const sd_jpeg_frame_desc& d = descs_host[b];
        if (!sdjpeg::desc_ok(d)) return fail(h, SD_ERR_INVALID, "sd_jpeg_reconstruct_bgr: descriptor " + std::to_string(b) + " is not self-consistent");
        if (sdjpeg::desc_coef_elems(d) * sizeof(int16_t) > frame_stride_bytes)
            return fail(h, SD_ERR_INVALID, "sd_jpeg_reconstruct_bgr: frame " + std::to_string(b) + " has more coefficients than frame_stride_bytes");
        if ((size_t)d.height * d.width * 3 > bgr_frame_stride)
            return fail(h, SD_ERR_INVALID, "sd_jpeg_reconstruct_bgr: frame " + std::to_string(b) + " is larger than bgr_frame_stride");
    }
    if (workspace_bytes < sdjpeg::workspace_bytes(descs_host, B))
        return fail(h, SD_ERR_INVALID, "sd_jpeg_reconstruct_bgr: workspace smaller than sd_jpeg_reconstruct_workspace reports");
    HIPCHK(h, launch_jpeg_reconstruct(coef_dev, frame_stride_bytes / sizeof(int16_t), descs_host, B, bgr_dev, bgr_frame_stride,
                                      static_cast<uint8_t*>(workspace_dev), (hipStream_t)stream));
    return SD_OK;
}

sd_status sd_jpeg_entropy_workspace(int B, size_t interval_stride, size_t* bytes_out) {
    if (B < 1 || B > 65535 || interval_stride < 1 || interval_stride > ((size_t)1 << 24) || !bytes_out) return SD_ERR_INVALID;
    *bytes_out = sdjent::Layout(B, interval_stride).total;
    return SD_OK;
}

sd_status sd_jpeg_entropy_decode(sd_handle* h, const uint8_t* bytes_dev, size_t byte_stride, const sd_jpeg_frame_desc* descs_host,
                                 const sd_jpeg_entropy_frame* frames_host, const sd_jpeg_interval* intervals_host, size_t interval_stride,
                                 const sd_jpeg_huff_table* tables_host, int B, int16_t* coef_dev, size_t coef_stride_bytes, int32_t* status_dev,
                                 void* workspace_dev, size_t workspace_bytes, void* stream) {
    if (!h || !bytes_dev || !descs_host || !frames_host || !intervals_host || !tables_host || B < 1 || B > 65535 || !coef_dev || !status_dev ||
        !workspace_dev || interval_stride < 1 || interval_stride > ((size_t)1 << 24))
        return fail(h, SD_ERR_INVALID, "sd_jpeg_entropy_decode: bad arguments");
    // the lanes fetch aligned dwords of the scan bytes and the clearing kernel stores 16-byte pieces
    if ((reinterpret_cast<uintptr_t>(bytes_dev) & 15) || (byte_stride & 15) || (reinterpret_cast<uintptr_t>(coef_dev) & 15) || (coef_stride_bytes & 15) ||
        (reinterpret_cast<uintptr_t>(workspace_dev) & 15) || (reinterpret_cast<uintptr_t>(status_dev) & 3))
        return fail(h, SD_ERR_INVALID, "sd_jpeg_entropy_decode: bytes_dev, byte_stride, coef_dev, coef_stride_bytes and workspace_dev must be multiples of 16");
    // every index the kernels form follows from records that agree with their descriptors and these capacities: nothing is launched otherwise
    const char* why = "";
    if (!sdjent::args_ok(byte_stride, descs_host, frames_host, intervals_host, interval_stride, tables_host, B, coef_stride_bytes, &why))
        return fail(h, SD_ERR_INVALID, std::string("sd_jpeg_entropy_decode: ") + why);
    if (workspace_bytes < sdjent::Layout(B, interval_stride).total)
        return fail(h, SD_ERR_INVALID, "sd_jpeg_entropy_decode: workspace smaller than sd_jpeg_entropy_workspace reports");
    HIPCHK(h, launch_jpeg_entropy_decode(bytes_dev, byte_stride, descs_host, frames_host, intervals_host, interval_stride, tables_host, B, coef_dev,
                                         coef_stride_bytes / sizeof(int16_t), status_dev, static_cast<uint8_t*>(workspace_dev), (hipStream_t)stream));
    return SD_OK;
}

sd_status sd_jpeg_sync_workspace(int B, size_t interval_stride, size_t max_pieces, size_t* bytes_out) {
    if (B < 1 || B > 65535 || interval_stride < 1 || interval_stride > ((size_t)1 << 24) || max_pieces > ((size_t)1 << 24) || !bytes_out) return SD_ERR_INVALID;
    *bytes_out = sdjsync::Layout(B, interval_stride, max_pieces).total;
    return SD_OK;
}

sd_status sd_jpeg_sync_decode(sd_handle* h, const uint8_t* bytes_dev, size_t byte_stride, const sd_jpeg_frame_desc* descs_host,
                              const sd_jpeg_sync_frame* frames_host, const sd_jpeg_sync_interval* intervals_host, size_t interval_stride,
                              const sd_jpeg_huff_table* tables_host, int B, int subseq_bytes, int16_t* coef_dev, size_t coef_stride_bytes,
                              int32_t* status_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
    if (!h || !bytes_dev || !descs_host || !frames_host || !intervals_host || !tables_host || B < 1 || B > 65535 || !coef_dev || !status_dev ||
        !workspace_dev || interval_stride < 1 || interval_stride > ((size_t)1 << 24))
        return fail(h, SD_ERR_INVALID, "sd_jpeg_sync_decode: bad arguments");
    // the lanes fetch aligned 8-byte words of the clean stream and the clearing kernel stores 16-byte pieces
    if ((reinterpret_cast<uintptr_t>(bytes_dev) & 15) || (byte_stride & 15) || (reinterpret_cast<uintptr_t>(coef_dev) & 15) || (coef_stride_bytes & 15) ||
        (reinterpret_cast<uintptr_t>(workspace_dev) & 15) || (reinterpret_cast<uintptr_t>(status_dev) & 3))
        return fail(h, SD_ERR_INVALID, "sd_jpeg_sync_decode: bytes_dev, byte_stride, coef_dev, coef_stride_bytes and workspace_dev must be multiples of 16");
    // every index the kernels form follows from records that agree with their descriptors and these capacities: nothing is launched otherwise
    const char* why = "";
    if (!sdjsync::args_ok(byte_stride, descs_host, frames_host, intervals_host, interval_stride, tables_host, B, subseq_bytes, coef_stride_bytes, &why))
        return fail(h, SD_ERR_INVALID, std::string("sd_jpeg_sync_decode: ") + why);
    size_t most = 0;
    for (int b = 0; b < B; ++b)
        if (frames_host[b].eligible && frames_host[b].n_pieces > most) most = frames_host[b].n_pieces;
    if (most > ((size_t)1 << 24) || workspace_bytes < sdjsync::Layout(B, interval_stride, most).total)
        return fail(h, SD_ERR_INVALID, "sd_jpeg_sync_decode: workspace smaller than sd_jpeg_sync_workspace reports for the largest frame");
    HIPCHK(h, launch_jpeg_sync_decode(bytes_dev, byte_stride, frames_host, intervals_host, interval_stride, tables_host, B, subseq_bytes, most, coef_dev,
                                      coef_stride_bytes / sizeof(int16_t), status_dev, static_cast<uint8_t*>(workspace_dev), (hipStream_t)stream));
    return SD_OK;
}

sd_status sd_png_reconstruct_workspace(int B, size_t* bytes_out) {
    if (B < 1 || B > 65535 || !bytes_out) return SD_ERR_INVALID;
    *bytes_out = sdpngin::Layout(B).total;
    return SD_OK;
}

sd_status sd_png_reconstruct_bgr(sd_handle* h, const uint8_t* rows_dev, size_t frame_stride, const sd_png_frame_desc* descs_host, int B, int height,
                                 int width, uint8_t* bgr_out_dev, size_t out_stride, int32_t* status_dev, void* workspace_dev, size_t workspace_bytes,
                                 void* stream) {
    if (!h || !rows_dev || !descs_host || !bgr_out_dev || !status_dev || !workspace_dev)
        return fail(h, SD_ERR_INVALID, "sd_png_reconstruct_bgr: bad arguments");
    // the lanes fetch aligned 16-byte pieces of their rows
    if ((reinterpret_cast<uintptr_t>(rows_dev) & 15) || (reinterpret_cast<uintptr_t>(workspace_dev) & 15) || (reinterpret_cast<uintptr_t>(status_dev) & 3))
        return fail(h, SD_ERR_INVALID, "sd_png_reconstruct_bgr: rows_dev, frame_stride and workspace_dev must be multiples of 16");
    // every index the kernel forms follows from descriptors of the call's size and these capacities: nothing is launched otherwise
    const char* why = "";
    if (!png_in_args_ok(frame_stride, descs_host, B, height, width, out_stride, &why)) return fail(h, SD_ERR_INVALID, std::string("sd_png_reconstruct_bgr: ") + why);
    if (workspace_bytes < sdpngin::Layout(B).total)
        return fail(h, SD_ERR_INVALID, "sd_png_reconstruct_bgr: workspace smaller than sd_png_reconstruct_workspace reports");
    HIPCHK(h, launch_png_reconstruct(rows_dev, frame_stride, descs_host, B, height, width, bgr_out_dev, out_stride, status_dev,
                                     static_cast<uint8_t*>(workspace_dev), (h->sw & SW_PNG_ONE_WAVE) ? 1 : sdpngin::kWaves, (hipStream_t)stream));
    return SD_OK;
}

sd_status sd_png_encode_workspace(int B, int height, int width, size_t* workspace_bytes, size_t* stream_stride) {
    if (B < 1 || B > 65535 || height < 1 || width < 1 || height > sdpng::kMaxExtent || width > sdpng::kMaxExtent) return SD_ERR_INVALID;
    if (workspace_bytes) *workspace_bytes = sdpng::Layout(B, height, width).total;
    if (stream_stride) *stream_stride = sdpng::stream_bound(height, width);
    return SD_OK;
}

sd_status sd_png_encode_bgr(sd_handle* h, const uint8_t* frames_dev, size_t frame_stride, int B, int height, int width, uint8_t* streams_dev,
                            size_t stream_stride, uint64_t* sizes_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
    if (!h || !frames_dev || !streams_dev || !sizes_dev || !workspace_dev || B < 1 || B > 65535)
        return fail(h, SD_ERR_INVALID, "sd_png_encode_bgr: bad arguments");
    if (height < 1 || width < 1 || height > sdpng::kMaxExtent || width > sdpng::kMaxExtent)
        return fail(h, SD_ERR_INVALID, "sd_png_encode_bgr: extents must be 1..16384");
    // every index the kernels form follows from the extents and these capacities: nothing is launched otherwise
    if (frame_stride < (size_t)height * width * 3) return fail(h, SD_ERR_INVALID, "sd_png_encode_bgr: frame_stride below height * width * 3");
    if (stream_stride < sdpng::stream_bound(height, width))
        return fail(h, SD_ERR_INVALID, "sd_png_encode_bgr: stream_stride below the bound sd_png_encode_workspace reports");
    if (workspace_bytes < sdpng::Layout(B, height, width).total)
        return fail(h, SD_ERR_INVALID, "sd_png_encode_bgr: workspace smaller than sd_png_encode_workspace reports");
    if ((reinterpret_cast<uintptr_t>(workspace_dev) & 15) || (reinterpret_cast<uintptr_t>(sizes_dev) & 7))
        return fail(h, SD_ERR_INVALID, "sd_png_encode_bgr: workspace_dev must be 16-byte, sizes_dev 8-byte aligned");
    HIPCHK(h, launch_png_encode(frames_dev, frame_stride, B, height, width, streams_dev, stream_stride, sizes_dev,
                                static_cast<uint8_t*>(workspace_dev), (hipStream_t)stream));
    return SD_OK;
}

sd_status sd_jpeg_encode_workspace(int B, int height, int width, size_t* workspace_bytes, size_t* stream_bound) {
    if (B < 1 || B > 65535 || height < 1 || width < 1 || height > sdjenc::kMaxExtent || width > sdjenc::kMaxExtent) return SD_ERR_INVALID;
    if (workspace_bytes) *workspace_bytes = sdjenc::Layout(B, height).total;
    if (stream_bound) *stream_bound = sdjenc::stream_bound(height, width);
    return SD_OK;
}

sd_status sd_jpeg_encode_bgr(sd_handle* h, const uint8_t* frames_dev, size_t frame_stride, int B, int height, int width, int quality,
                             uint8_t* streams_dev, size_t stream_stride, uint64_t* sizes_dev, int32_t* flags_dev, void* workspace_dev,
                             size_t workspace_bytes, void* stream) {
    if (!h || !frames_dev || !streams_dev || !sizes_dev || !flags_dev || !workspace_dev || B < 1 || B > 65535)
        return fail(h, SD_ERR_INVALID, "sd_jpeg_encode_bgr: bad arguments");
    if (height < 1 || width < 1 || height > sdjenc::kMaxExtent || width > sdjenc::kMaxExtent)
        return fail(h, SD_ERR_INVALID, "sd_jpeg_encode_bgr: extents must be 1..16384");
    if (quality < 1 || quality > 100) return fail(h, SD_ERR_INVALID, "sd_jpeg_encode_bgr: quality must be 1..100");
    // every index the kernels form follows from the extents and these capacities: nothing is launched otherwise
    if (frame_stride < (size_t)height * width * 3) return fail(h, SD_ERR_INVALID, "sd_jpeg_encode_bgr: frame_stride below height * width * 3");
    if (stream_stride < (size_t)sdjenc::kHeaderLen) return fail(h, SD_ERR_INVALID, "sd_jpeg_encode_bgr: stream_stride below the header's 613 bytes");
    if (workspace_bytes < sdjenc::Layout(B, height).total)
        return fail(h, SD_ERR_INVALID, "sd_jpeg_encode_bgr: workspace smaller than sd_jpeg_encode_workspace reports");
    if ((reinterpret_cast<uintptr_t>(workspace_dev) & 15) || (reinterpret_cast<uintptr_t>(sizes_dev) & 7) || (reinterpret_cast<uintptr_t>(flags_dev) & 3))
        return fail(h, SD_ERR_INVALID, "sd_jpeg_encode_bgr: workspace_dev must be 16-byte, sizes_dev 8-byte, flags_dev 4-byte aligned");
    HIPCHK(h, launch_jpeg_encode(frames_dev, frame_stride, B, height, width, quality, streams_dev, stream_stride, sizes_dev, flags_dev,
                                 static_cast<uint8_t*>(workspace_dev), (hipStream_t)stream));
    return SD_OK;
}

static_assert(SD_PLY_ROW_CAP == sdply::kRowCap && SD_PLY_HEADER_CAP == sdply::kHeaderCap && SD_PLY_LINE_ROWS == sdply::kLineRows,
              "include/semdepth.h and ply_format.hpp disagree");
constexpr int kPlyMaxCap = 0x7fffffff - sdply::kLineRows - sdply::kBlockRows;      // row indices stay in an int

sd_status sd_ply_format_workspace(int B, int cap, size_t* workspace_bytes, size_t* text_bound) {
    if (B < 1 || B > 65535 || cap < 0 || cap > kPlyMaxCap) return SD_ERR_INVALID;
    if (workspace_bytes) *workspace_bytes = sdply::Layout(B, cap).total;
    if (text_bound) *text_bound = ply_text_bound(B, cap);
    return SD_OK;
}

sd_status sd_ply_format_rw(sd_handle* h, const float* xyz_dev, const uint8_t* rgb_dev, const int32_t* n_dev, int B, int cap,
                           const sd_rw_result* records_dev, uint8_t* text_dev, size_t text_capacity, uint64_t* offsets_dev, int32_t* flags_dev,
                           void* workspace_dev, size_t workspace_bytes, void* stream) {
    if (!h || !xyz_dev || !rgb_dev || !n_dev || !records_dev || !text_dev || !offsets_dev || !flags_dev || !workspace_dev)
        return fail(h, SD_ERR_INVALID, "sd_ply_format_rw: null pointer");
    if (B < 1 || B > 65535 || cap < 0 || cap > kPlyMaxCap) return fail(h, SD_ERR_INVALID, "sd_ply_format_rw: B must be 1..65535, cap >= 0");
    // every index the kernels form follows from B, cap and these capacities: nothing is launched otherwise
    if (workspace_bytes < sdply::Layout(B, cap).total)
        return fail(h, SD_ERR_INVALID, "sd_ply_format_rw: workspace smaller than sd_ply_format_workspace reports");
    if ((reinterpret_cast<uintptr_t>(workspace_dev) & 15) || (reinterpret_cast<uintptr_t>(offsets_dev) & 7) ||
        (reinterpret_cast<uintptr_t>(flags_dev) & 3) || (reinterpret_cast<uintptr_t>(xyz_dev) & 3) || (reinterpret_cast<uintptr_t>(n_dev) & 3) ||
        (reinterpret_cast<uintptr_t>(records_dev) & 7))
        return fail(h, SD_ERR_INVALID, "sd_ply_format_rw: workspace_dev must be 16-byte, offsets_dev and records_dev 8-byte, the rest naturally aligned");
    HIPCHK(h, launch_ply_format(xyz_dev, rgb_dev, n_dev, B, cap, records_dev, text_dev, text_capacity, offsets_dev, flags_dev,
                                static_cast<uint8_t*>(workspace_dev), (hipStream_t)stream));
    return SD_OK;
}

static bool scene_dims_ok(int B, int cap_road, int cap_fence, uint32_t lattice_cap, uint32_t mask) {
    return B >= 1 && B <= 65535 && cap_road >= 0 && cap_fence >= 0 && !(mask & ~(uint32_t)SD_SCENE_ALL) &&
           sdscene::rows_bound(cap_road, cap_fence, lattice_cap, mask) <= (uint64_t)sdscene::kMaxRows - sdply::kBlockRows;
}

sd_status sd_scene_workspace(int B, int cap_road, int cap_fence, uint32_t lattice_cap, uint32_t mask, size_t* workspace_bytes, size_t* text_bound) {
    if (!scene_dims_ok(B, cap_road, cap_fence, lattice_cap, mask)) return SD_ERR_INVALID;
    if (workspace_bytes) *workspace_bytes = sdscene::Layout(B, cap_road, cap_fence, lattice_cap, mask).total;
    if (text_bound) *text_bound = scene_text_bound(B, cap_road, cap_fence, lattice_cap, mask);
    return SD_OK;
}

sd_status sd_scene_format(sd_handle* h, const float* road_xyz_dev, const uint8_t* road_rgb_dev, const int32_t* n_road_dev, int cap_road,
                          const float* left_xyz_dev, const uint8_t* left_rgb_dev, const float* right_xyz_dev, const uint8_t* right_rgb_dev,
                          int cap_fence, int B, const sd_rw_result* records_dev, const sd_f2f_result* f2f_dev,
                          const sd_plane_box* road_boxes_dev, const sd_plane_box* fence_boxes_dev, uint32_t mask, uint32_t lattice_cap,
                          uint8_t* text_dev, size_t text_capacity, uint64_t* offsets_dev, int32_t* flags_dev, void* workspace_dev,
                          size_t workspace_bytes, void* stream) {
    if (!h || !road_xyz_dev || !road_rgb_dev || !n_road_dev || !records_dev || !text_dev || !offsets_dev || !flags_dev || !workspace_dev)
        return fail(h, SD_ERR_INVALID, "sd_scene_format: null pointer");
    const int fence_ptrs = (left_xyz_dev != nullptr) + (left_rgb_dev != nullptr) + (right_xyz_dev != nullptr) + (right_rgb_dev != nullptr);
    if ((fence_ptrs != 0 && fence_ptrs != 4) || (fence_ptrs && !f2f_dev))
        return fail(h, SD_ERR_INVALID, "sd_scene_format: the fence group is all four arrays and f2f_dev, or none");
    if (mask & ~(uint32_t)SD_SCENE_ALL) return fail(h, SD_ERR_INVALID, "sd_scene_format: mask beyond SD_SCENE_ALL");
    if (!scene_dims_ok(B, cap_road, cap_fence, lattice_cap, mask))
        return fail(h, SD_ERR_INVALID, "sd_scene_format: B must be 1..65535, the caps >= 0 and the row bound below 2^31 - 512");
    // every index the kernels form follows from B, the caps, lattice_cap and these capacities: nothing is launched otherwise
    if (workspace_bytes < sdscene::Layout(B, cap_road, cap_fence, lattice_cap, mask).total)
        return fail(h, SD_ERR_INVALID, "sd_scene_format: workspace smaller than sd_scene_workspace reports");
    auto mis = [](const void* p, uintptr_t m) { return (reinterpret_cast<uintptr_t>(p) & m) != 0; };
    if (mis(workspace_dev, 15) || mis(offsets_dev, 7) || mis(records_dev, 7) || mis(f2f_dev, 7) || mis(flags_dev, 3) || mis(road_xyz_dev, 3) ||
        mis(n_road_dev, 3) || mis(left_xyz_dev, 3) || mis(right_xyz_dev, 3) || mis(road_boxes_dev, 3) || mis(fence_boxes_dev, 3))
        return fail(h, SD_ERR_INVALID, "sd_scene_format: workspace_dev must be 16-byte, offsets_dev and the records 8-byte, the rest naturally aligned");
    SceneBatch in{};
    in.road_xyz = road_xyz_dev; in.road_rgb = road_rgb_dev; in.n_road = n_road_dev; in.cap_road = cap_road;
    in.left_xyz = left_xyz_dev; in.left_rgb = left_rgb_dev; in.right_xyz = right_xyz_dev; in.right_rgb = right_rgb_dev; in.cap_fence = cap_fence;
    in.B = B; in.records = records_dev; in.f2f = f2f_dev; in.road_boxes = road_boxes_dev; in.fence_boxes = fence_boxes_dev;
    in.mask = mask; in.lattice_cap = lattice_cap;
    HIPCHK(h, launch_scene_format(in, text_dev, text_capacity, offsets_dev, flags_dev, static_cast<uint8_t*>(workspace_dev), (hipStream_t)stream));
    return SD_OK;
}

size_t sd_text_workspace_bytes(int B) { return B < 1 || B > 65535 ? 0 : sdtext::Layout(B).total; }

sd_status sd_text_draw_rw(sd_handle* h, uint8_t* dst_dev, int B, int dst_h, int dst_w, const sd_rw_result* records_dev, const char* depth_text,
                          void* workspace_dev, size_t workspace_bytes, void* stream) {
    if (!h || !dst_dev || !records_dev || !depth_text || !workspace_dev) return fail(h, SD_ERR_INVALID, "sd_text_draw_rw: null pointer");
    if (B < 1 || B > 65535) return fail(h, SD_ERR_INVALID, "sd_text_draw_rw: B must be 1..65535");
    if (dst_h < 1 || dst_w < 1 || dst_h > sdtext::kMaxExtent || dst_w > sdtext::kMaxExtent)
        return fail(h, SD_ERR_INVALID, "sd_text_draw_rw: extents must be 1..16384");
    const size_t dlen = strnlen(depth_text, sdtext::kMaxDepthBytes + 1);
    if (dlen > (size_t)sdtext::kMaxDepthBytes) return fail(h, SD_ERR_INVALID, "sd_text_draw_rw: depth_text longer than 23 bytes");
    // every index the kernels form follows from B, the extents and this capacity: nothing is launched otherwise
    if (workspace_bytes < sdtext::Layout(B).total) return fail(h, SD_ERR_INVALID, "sd_text_draw_rw: workspace smaller than sd_text_workspace_bytes reports");
    if ((reinterpret_cast<uintptr_t>(workspace_dev) & 15) || (reinterpret_cast<uintptr_t>(records_dev) & 7))
        return fail(h, SD_ERR_INVALID, "sd_text_draw_rw: workspace_dev must be 16-byte, records_dev 8-byte aligned");
    HIPCHK(h, launch_text_draw_rw(dst_dev, B, dst_h, dst_w, records_dev, reinterpret_cast<const uint8_t*>(depth_text), (int)dlen,
                                  static_cast<uint8_t*>(workspace_dev), (hipStream_t)stream));
    return SD_OK;
}

size_t sd_overlay_workspace_bytes(int B, int D) {
    return B < 1 || B > 65535 || D < 0 || D > sdoverlay::kMaxDepths ? 0 : sdoverlay::Layout(B, D).total;
}

sd_status sd_overlay_draw(sd_handle* h, uint8_t* dst_dev, int B, int dst_h, int dst_w, int net_h, int net_w, const sd_camera* cams_host,
                          const sd_rw_result* records_dev, const sd_f2f_result* f2f_dev, const sd_rw_depth_result* rw_profile_dev,
                          const sd_f2f_depth_result* f2f_profile_dev, int D, const sd_overlay_style* style_host, int32_t* flags_dev,
                          void* workspace_dev, size_t workspace_bytes, void* stream) {
    if (!h || !dst_dev || !cams_host || !records_dev || !style_host || !flags_dev || !workspace_dev)
        return fail(h, SD_ERR_INVALID, "sd_overlay_draw: null pointer");
    if (B < 1 || B > 65535) return fail(h, SD_ERR_INVALID, "sd_overlay_draw: B must be 1..65535");
    if (!sdoverlay::sizes_ok(net_h, net_w, dst_h, dst_w)) return fail(h, SD_ERR_INVALID, "sd_overlay_draw: extents must be 1..16384");
    if (D < 0 || D > sdoverlay::kMaxDepths || (D > 0 && !rw_profile_dev))
        return fail(h, SD_ERR_INVALID, "sd_overlay_draw: D must be 0..256 and D > 0 needs rw_profile_dev");
    const sd_overlay_style style = *style_host;       // read once, here: the kernels get this copy by value
    if (!sdoverlay::style_ok(style, dst_h))
        return fail(h, SD_ERR_INVALID, "sd_overlay_draw: style outside the caps (thicknesses 1..32, clip_top 0..dst_h)");
    for (int b = 0; b < B; ++b)
        if (!sdoverlay::camera_ok(cams_host[b])) return fail(h, SD_ERR_INVALID, "sd_overlay_draw: a camera's cx, cy or f is not finite in float32");
    // every index the kernels form follows from B, D, the extents and this capacity: nothing is launched otherwise
    if (workspace_bytes < sdoverlay::Layout(B, D).total)
        return fail(h, SD_ERR_INVALID, "sd_overlay_draw: workspace smaller than sd_overlay_workspace_bytes reports");
    if ((reinterpret_cast<uintptr_t>(workspace_dev) & 15) || (reinterpret_cast<uintptr_t>(records_dev) & 7) ||
        (reinterpret_cast<uintptr_t>(f2f_dev) & 7) || (reinterpret_cast<uintptr_t>(rw_profile_dev) & 7) ||
        (reinterpret_cast<uintptr_t>(f2f_profile_dev) & 7) || (reinterpret_cast<uintptr_t>(flags_dev) & 3))
        return fail(h, SD_ERR_INVALID, "sd_overlay_draw: workspace_dev must be 16-byte, the records 8-byte, flags_dev 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    OverlayArgs a{};
    a.dst = dst_dev; a.records = records_dev; a.f2f = f2f_dev; a.rw_profile = D > 0 ? rw_profile_dev : nullptr;
    a.f2f_profile = D > 0 ? f2f_profile_dev : nullptr; a.flags = flags_dev; a.style = style;
    a.B = B; a.D = D; a.h = dst_h; a.w = dst_w; a.net_h = net_h; a.net_w = net_w;
    overlay_layout(a, static_cast<uint8_t*>(workspace_dev));
    h->overlay_stage.resize((size_t)B);
    for (int b = 0; b < B; ++b)
        h->overlay_stage[(size_t)b] = OverlayCamDev{(double)(float)cams_host[b].cx, (double)(float)cams_host[b].cy, (double)(float)cams_host[b].f, 0.0};
    HIPCHK(h, hipMemcpyAsync(a.cams, h->overlay_stage.data(), sizeof(OverlayCamDev) * (size_t)B, hipMemcpyHostToDevice, s));
    HIPCHK(h, launch_overlay_draw(a, s));
    return SD_OK;
}

sd_status sd_render_workspace(int B, int cap, const sd_render_camera* cam_host, size_t* workspace_bytes) {
    if (B < 1 || B > 65535 || cap < 0 || cap > kPlyMaxCap || !cam_host || !workspace_bytes || !sdrender::valid_camera(*cam_host)) return SD_ERR_INVALID;
    *workspace_bytes = sdrender::Layout(B, cap, *cam_host).total;
    return SD_OK;
}

sd_status sd_render_rw(sd_handle* h, const float* xyz_dev, const uint8_t* rgb_dev, const int32_t* n_dev, int B, int cap,
                       const sd_rw_result* records_dev, const sd_render_camera* cam_host, uint8_t* dst_dev, int32_t* flags_dev,
                       void* workspace_dev, size_t workspace_bytes, void* stream) {
    if (!h || !xyz_dev || !rgb_dev || !n_dev || !records_dev || !cam_host || !dst_dev || !flags_dev || !workspace_dev)
        return fail(h, SD_ERR_INVALID, "sd_render_rw: null pointer");
    if (B < 1 || B > 65535 || cap < 0 || cap > kPlyMaxCap) return fail(h, SD_ERR_INVALID, "sd_render_rw: B must be 1..65535, cap >= 0");
    const sd_render_camera cam = *cam_host;           // read once, here: the kernels get this copy by value
    if (!sdrender::valid_camera(cam))
        return fail(h, SD_ERR_INVALID, "sd_render_rw: camera outside the caps (finite fields, z_near > 0, extents 1..16384, point_size 1..16)");
    // every index the kernels form follows from B, cap, the camera's extents and this capacity: nothing is launched otherwise
    if (workspace_bytes < sdrender::Layout(B, cap, cam).total)
        return fail(h, SD_ERR_INVALID, "sd_render_rw: workspace smaller than sd_render_workspace reports");
    if ((reinterpret_cast<uintptr_t>(workspace_dev) & 15) || (reinterpret_cast<uintptr_t>(records_dev) & 7) ||
        (reinterpret_cast<uintptr_t>(flags_dev) & 3) || (reinterpret_cast<uintptr_t>(xyz_dev) & 3) || (reinterpret_cast<uintptr_t>(n_dev) & 3) ||
        (reinterpret_cast<uintptr_t>(dst_dev) & 3))
        return fail(h, SD_ERR_INVALID, "sd_render_rw: workspace_dev must be 16-byte, records_dev 8-byte, xyz_dev, n_dev, flags_dev and dst_dev 4-byte aligned");
    HIPCHK(h, launch_render_rw(xyz_dev, rgb_dev, n_dev, B, cap, records_dev, cam, dst_dev, flags_dev, static_cast<uint8_t*>(workspace_dev),
                               (hipStream_t)stream));
    return SD_OK;
}

sd_status sd_compose_result_frames(sd_handle* h, const uint8_t* frames, const uint8_t* road_mask, const uint8_t* fence_mask,
                                   const sd_rw_result* records, int B, int src_h, int src_w, const uint8_t* road_color,
                                   const uint8_t* fence_color, int alpha, uint8_t* dst, int dst_h, int dst_w, void* stream) {
    if (!h || !frames || !road_mask || !fence_mask || !records || !dst || !road_color || !fence_color || B <= 0 || src_h <= 0 ||
        src_w <= 0 || dst_h <= 0 || dst_w <= 0 || dst_h > RSZ_MAX || dst_w > RSZ_MAX || alpha < 0 || alpha > 255)
        return fail(h, SD_ERR_INVALID, "sd_compose_result_frames: bad arguments (destination extent at most 16384, alpha 0..255)");
    if (!h->bound) return fail(h, SD_ERR_STATE, "sd_bind_memory first");
    hipStream_t s = (hipStream_t)stream;
    int *xi, *xa, *yi, *ya;
    const sd_status st = upload_resize_tables(h, h->a.rsz_cmp, h->cmp_rsz_key, h->cmp_rsz_host, src_h, src_w, dst_h, dst_w, s, &xi, &xa, &yi, &ya);
    if (st != SD_OK) return st;
    ComposeArgs a{};
    a.xi = xi; a.xa = xa; a.yi = yi; a.ya = ya;
    a.frames = frames; a.road = road_mask; a.fence = fence_mask; a.records = reinterpret_cast<const RwResultDev*>(records); a.dst = dst;
    a.B = B; a.sh = src_h; a.sw = src_w; a.dh = dst_h; a.dw = dst_w; a.alpha = alpha;
    a.banner_y1 = std::min((int)(0.25 * dst_h), dst_h - 1);       // cv2.rectangle((0,0), (w, int(0.25*h)), ..., -1): inclusive, clipped
    a.aligned = (reinterpret_cast<uintptr_t>(dst) & 3) == 0;
    const uint8_t banner[3] = {156, 157, 159};
    for (int c = 0; c < 3; ++c) { a.road_c[c] = road_color[c]; a.fence_c[c] = fence_color[c]; a.banner[c] = banner[c]; }
    HIPCHK(h, launch_compose_result_frames(a, s));
    return SD_OK;
}

sd_status sd_post_process(sd_handle* h, const float* disp_raw, int B, float* disp_pp, void* stream) {
    if (!h || !disp_raw || !disp_pp || B <= 0) return fail(h, SD_ERR_INVALID, "sd_post_process: bad arguments");
    HIPCHK(h, launch_post_process(disp_raw, disp_pp, B, h->H, h->W, (hipStream_t)stream));
    return SD_OK;
}

sd_status sd_monodepth_forward(sd_handle* h, const uint8_t* frames, int B, float* disp_pp, float* disp_raw, void* stream) {
    if (!h || !frames || B <= 0 || B > h->max_batch) return fail(h, SD_ERR_INVALID, "sd_monodepth_forward: bad arguments");
    if (!disp_pp && B > h->chunk && !disp_raw)
        return fail(h, SD_ERR_INVALID, "sd_monodepth_forward: disp_pp may be NULL only when the raw pair survives (B <= chunk) or disp_raw is given");
    if (!h->bound) return fail(h, SD_ERR_STATE, "sd_bind_memory first");
    const size_t npix = (size_t)h->H * h->W;
    hipStream_t s = (hipStream_t)stream;
    const NetPlan& p = h->mono;
    const float* raw = reinterpret_cast<const float*>(act_base(h, SD_NET_MONODEPTH) + p.tensors[p.t_output].offset);
    for (int b0 = 0; b0 < B; b0 += h->chunk) {
        const int nb = std::min(h->chunk, B - b0);
        sd_status st = run_plan(h, SD_NET_MONODEPTH, frames + (size_t)b0 * npix * 3, b0, nb, nullptr, s);
        if (st != SD_OK) return st;
        if (disp_pp) HIPCHK(h, launch_post_process(raw, disp_pp + (size_t)b0 * npix, nb, h->H, h->W, s));
        if (disp_raw)
            HIPCHK(h, hipMemcpyAsync(disp_raw + (size_t)b0 * 2 * npix, raw, (size_t)nb * 2 * npix * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
    h->last_mono_frames = B <= h->chunk ? B : 0;
    return SD_OK;
}

static sd_status fuse_impl(sd_handle* h, const float* disp_pp, const float* disp_raw, float* pp_out, const uint8_t* road, const uint8_t* fence,
                           const uint8_t* frames, const sd_camera* cams, int B, int cap, float* dense, float* road_xyz, uint8_t* road_rgb,
                           int32_t* n_road, float* fence_xyz, uint8_t* fence_rgb, int32_t* n_fence, void* stream) {
    if (!h || (!disp_pp && !disp_raw) || !cams || B <= 0 || B > h->max_batch || cap <= 0) return fail(h, SD_ERR_INVALID, "sd_fuse_backproject: bad arguments");
    if (!h->bound) return fail(h, SD_ERR_STATE, "sd_bind_memory first");
    if ((road_xyz && (!road || !n_road)) || (fence_xyz && (!fence || !n_fence)))
        return fail(h, SD_ERR_INVALID, "sd_fuse_backproject: a cloud output needs its mask and its counter");
    hipStream_t s = (hipStream_t)stream;
    std::vector<CamDev> cd(B);
    for (int b = 0; b < B; ++b) cd[b] = make_cam(cams[b]);
    CamDev* dcams = at<CamDev>(h, h->a.cams);
    if (h->cams_stage.size() != (size_t)B || std::memcmp(h->cams_stage.data(), cd.data(), sizeof(CamDev) * B) != 0) {
        h->cams_stage = cd;
        HIPCHK(h, hipMemcpyAsync(dcams, h->cams_stage.data(), sizeof(CamDev) * B, hipMemcpyHostToDevice, s));
    }
    FuseParams p{};
    p.disp_pp = disp_pp; p.road = road_xyz ? road : nullptr; p.fence = fence_xyz ? fence : nullptr; p.frames = frames; p.cams = dcams;
    p.B = B; p.H = h->H; p.W = h->W; p.cap = cap; p.sw = h->sw;
    p.dense = dense; p.road_xyz = road_xyz; p.road_rgb = frames ? road_rgb : nullptr; p.n_road = n_road;
    p.fence_xyz = fence_xyz; p.fence_rgb = frames ? fence_rgb : nullptr; p.n_fence = n_fence;
    const FuseLayout fl(h->max_batch, h->H, h->W);
    p.blk_counts = at<int32_t>(h, h->a.fuse + fl.blk_counts);
    p.blk_offsets = at<int32_t>(h, h->a.fuse + fl.blk_offsets);
    // one-pass form: look-back words + tickets; the words carry an epoch, so the scratch is zeroed only every 1023 launches
    p.disp_raw = disp_raw; p.pp_out = pp_out;
    const Fuse1Layout f1(h->max_batch, h->H, h->W);
    p.lb_state = at<unsigned long long>(h, h->a.fuse1 + f1.state);
    p.lb_ticket = at<int32_t>(h, h->a.fuse1 + f1.ticket);
    if (h->fuse_epoch == 0 || h->fuse_epoch >= 1023) {
        HIPCHK(h, hipMemsetAsync(at(h, h->a.fuse1), 0, f1.total, s));
        h->fuse_epoch = 0;
    }
    p.epoch = ++h->fuse_epoch;
    HIPCHK(h, launch_fuse(p, s));
    return SD_OK;
}

sd_status sd_fuse_backproject(sd_handle* h, const float* disp_pp, const uint8_t* road, const uint8_t* fence, const uint8_t* frames,
                              const sd_camera* cams, int B, int cap, float* dense, float* road_xyz, uint8_t* road_rgb,
                              int32_t* n_road, float* fence_xyz, uint8_t* fence_rgb, int32_t* n_fence, void* stream) {
    if (!disp_pp) return fail(h, SD_ERR_INVALID, "sd_fuse_backproject: bad arguments");
    return fuse_impl(h, disp_pp, nullptr, nullptr, road, fence, frames, cams, B, cap, dense, road_xyz, road_rgb, n_road, fence_xyz, fence_rgb,
                     n_fence, stream);
}

sd_status sd_postprocess_fuse_backproject(sd_handle* h, const float* disp_raw, float* disp_pp_out, const uint8_t* road, const uint8_t* fence,
                                          const uint8_t* frames, const sd_camera* cams, int B, int cap, float* road_xyz, uint8_t* road_rgb,
                                          int32_t* n_road, float* fence_xyz, uint8_t* fence_rgb, int32_t* n_fence, void* stream) {
    if (!h || !disp_pp_out) return fail(h, SD_ERR_INVALID, "sd_postprocess_fuse_backproject: bad arguments");
    if (!disp_raw) {            // the raw pair of the handle's last sd_monodepth_forward, still in the activation arena
        if (h->last_mono_frames < B || B > h->chunk)
            return fail(h, SD_ERR_STATE, "sd_postprocess_fuse_backproject: no raw disparities of a monodepth pass of >= B frames in the arena");
        const NetPlan& p = h->mono;
        disp_raw = reinterpret_cast<const float*>(act_base(h, SD_NET_MONODEPTH) + p.tensors[p.t_output].offset);
    }
    return fuse_impl(h, nullptr, disp_raw, disp_pp_out, road, fence, frames, cams, B, cap, nullptr, road_xyz, road_rgb, n_road, fence_xyz,
                     fence_rgb, n_fence, stream);
}

size_t sd_fuse_sweep_workspace(int B, int T, int H, int W) {
    if (B < 1 || T < 1 || H < 1 || W < 1 || (long long)T * B > 65535) return 0;
    return SweepLayout(B, T, H, W).total;
}

sd_status sd_fuse_backproject_sweep(sd_handle* h, const float* disp_pp, const uint8_t* road, const uint8_t* fence, const uint8_t* frames,
                                    const sd_camera* cams, int B, int T, int cap, float* road_xyz, uint8_t* road_rgb, int32_t* n_road,
                                    float* fence_xyz, uint8_t* fence_rgb, int32_t* n_fence, void* workspace_dev, size_t workspace_bytes,
                                    void* stream) {
    if (!h || !disp_pp || !road || !cams || !road_xyz || !n_road || !workspace_dev)
        return fail(h, SD_ERR_INVALID, "sd_fuse_backproject_sweep: null pointer");
    if (B < 1 || T < 1 || (long long)T * B > 65535 || cap < 1)
        return fail(h, SD_ERR_INVALID, "sd_fuse_backproject_sweep: B, T and cap must be >= 1 and T * B at most 65535");
    if (fence_xyz ? (!fence || !n_fence) : (fence_rgb != nullptr))
        return fail(h, SD_ERR_INVALID, "sd_fuse_backproject_sweep: the fence cloud needs its mask and its counter, its colours need the cloud");
    if ((road_rgb || fence_rgb) && !frames) return fail(h, SD_ERR_INVALID, "sd_fuse_backproject_sweep: a colour output needs frames");
    // every index the kernels form follows from B, T, cap, the handle's H x W and this capacity: nothing is launched otherwise
    if (workspace_bytes < SweepLayout(B, T, h->H, h->W).total)
        return fail(h, SD_ERR_INVALID, "sd_fuse_backproject_sweep: workspace smaller than sd_fuse_sweep_workspace reports");
    if ((reinterpret_cast<uintptr_t>(workspace_dev) & 15) || (reinterpret_cast<uintptr_t>(disp_pp) & 3) || (reinterpret_cast<uintptr_t>(road_xyz) & 3) ||
        (reinterpret_cast<uintptr_t>(fence_xyz) & 3) || (reinterpret_cast<uintptr_t>(n_road) & 3) || (reinterpret_cast<uintptr_t>(n_fence) & 3))
        return fail(h, SD_ERR_INVALID, "sd_fuse_backproject_sweep: workspace_dev must be 16-byte, the float and counter arrays 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    SweepParams p{};
    p.disp_pp = disp_pp; p.road = road; p.fence = fence_xyz ? fence : nullptr; p.frames = (road_rgb || fence_rgb) ? frames : nullptr;
    p.B = B; p.T = T; p.H = h->H; p.W = h->W; p.cap = cap; p.sw = h->sw;
    p.road_xyz = road_xyz; p.road_rgb = road_rgb; p.n_road = n_road;
    p.fence_xyz = fence_xyz; p.fence_rgb = fence_rgb; p.n_fence = fence_xyz ? n_fence : nullptr;
    fuse_sweep_carve(p, static_cast<uint8_t*>(workspace_dev));
    h->sweep_stage.resize((size_t)T * B);
    for (size_t i = 0; i < (size_t)T * B; ++i) h->sweep_stage[i] = make_cam(cams[i]);
    HIPCHK(h, hipMemcpyAsync(const_cast<CamDev*>(p.cams), h->sweep_stage.data(), sizeof(CamDev) * (size_t)T * B, hipMemcpyHostToDevice, s));
    HIPCHK(h, launch_fuse_sweep(p, s));
    return SD_OK;
}

sd_status sd_road_width(sd_handle* h, const float* road_xyz, const uint8_t* road_rgb, const int32_t* n_road, int B, int cap,
                        const sd_rw_params* prm, sd_rw_result* results, float* final_xyz, uint8_t* final_rgb, int32_t* n_final,
                        void* stream) {
    return sd_road_width_boxes(h, road_xyz, road_rgb, n_road, B, cap, prm, results, final_xyz, final_rgb, n_final, nullptr, stream);
}

static_assert(sizeof(PlaneBoxDev) == sizeof(sd_plane_box) && sizeof(sd_plane_box) == 24, "sd_plane_box is 24 bytes");

sd_status sd_road_width_boxes(sd_handle* h, const float* road_xyz, const uint8_t* road_rgb, const int32_t* n_road, int B, int cap,
                              const sd_rw_params* prm, sd_rw_result* results, float* final_xyz, uint8_t* final_rgb, int32_t* n_final,
                              sd_plane_box* boxes_dev, void* stream) {
    if (!h || !road_xyz || !n_road || !prm || !results || B <= 0 || B > h->max_batch || cap <= 0 || cap > h->cap)
        return fail(h, SD_ERR_INVALID, "sd_road_width: bad arguments");
    if (!h->bound) return fail(h, SD_ERR_STATE, "sd_bind_memory first");
    hipStream_t s = (hipStream_t)stream;
    float* A = at<float>(h, h->a.bufA);
    int32_t *n1 = cnt_slot(h, CNT_RW_ZCUT), *n2 = cnt_slot(h, CNT_RW_MAD_Y), *n3 = cnt_slot(h, CNT_RW_MAD_X), *n4 = cnt_slot(h, CNT_RW_PLANE),
            *n5 = cnt_slot(h, CNT_RW_SOR), *n6 = cnt_slot(h, CNT_RW_ROR);
    double* plane = at<double>(h, h->a.plane);
    void* o3d = at(h, h->a.o3d);
    RwResultDev* res = reinterpret_cast<RwResultDev*>(results);
    // the stages ping-pong between arenas A and B2: with distinct input and output the ordered compaction of a frame runs on
    // 64 workgroups instead of one (pcl.hip: multi-block compaction)
    float* B2 = at<float>(h, h->a.bufB);
    // colours (nullable): the reference carries road_colors through every filter (semantic_depth.py:206-245)
    uint8_t* cA = road_rgb ? at<uint8_t>(h, h->a.rgbA) : nullptr;
    uint8_t* cB = road_rgb ? at<uint8_t>(h, h->a.rgbB) : nullptr;
    void* cmp = at(h, h->a.cmp);
    HIPCHK(h, launch_filter_coord({road_xyz, road_rgb, n_road}, {A, cA, n1}, B, cap, F_LT_NEG, 2, prm->z_cut, cmp, s));
    HIPCHK(h, launch_mad_filter({A, cA, n1}, {B2, cB, n2}, B, cap, 1, prm->mad_y, nullptr, cmp, s));
    HIPCHK(h, launch_mad_filter({B2, cB, n2}, {A, cA, n3}, B, cap, 0, prm->mad_x, nullptr, cmp, s));
    // (the box of the cloud that enters the fit, for the plane lattice of the scene files)
    if (boxes_dev) HIPCHK(h, launch_plane_box({A, cA, n3}, B, cap, 1, reinterpret_cast<PlaneBoxDev*>(boxes_dev), 1, 0, s));
    HIPCHK(h, launch_plane_filter({A, cA, n3}, {B2, cB, n4}, B, cap, 1, prm->plane_thr, plane, cmp, s));
    const int32_t* nlast = n4;
    const float* fin = B2;
    if (prm->use_o3d) {
        HIPCHK(h, launch_sor({B2, cB, n4}, {A, cA, n5}, B, cap, prm->sor_k, prm->sor_ratio, o3d, nullptr, cmp, s));
        HIPCHK(h, launch_ror({A, cA, n5}, {B2, cB, n6}, B, cap, prm->ror_n, prm->ror_r, o3d, cmp, s));
        nlast = n6;
    } else {
        n5 = n4; n6 = n4;
    }
    HIPCHK(h, launch_end_points({fin, nullptr, nlast}, B, cap, prm->depth - prm->depth_offset, prm->window, res, s));
    HIPCHK(h, launch_record_counts(res, B, n_road, n1, n2, n3, n4, n5, n6, plane, s));
    if (final_xyz) HIPCHK(h, hipMemcpyAsync(final_xyz, fin, (size_t)B * cap * 3 * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (final_rgb) {
        if (!road_rgb) return fail(h, SD_ERR_INVALID, "sd_road_width: final_rgb needs road_rgb");
        HIPCHK(h, hipMemcpyAsync(final_rgb, cB, (size_t)B * cap * 3, hipMemcpyDeviceToDevice, s));
    }
    if (n_final) HIPCHK(h, hipMemcpyAsync(n_final, nlast, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    return SD_OK;
}

sd_status sd_fence_to_fence(sd_handle* h, const float* fence_xyz, const uint8_t* fence_rgb, const int32_t* n_fence, int B, int cap,
                            const sd_rw_result* road, const sd_f2f_params* prm, sd_f2f_result* results, float* left_xyz,
                            uint8_t* left_rgb, float* right_xyz, uint8_t* right_rgb, void* stream) {
    return sd_fence_to_fence_boxes(h, fence_xyz, fence_rgb, n_fence, B, cap, road, prm, results, left_xyz, left_rgb, right_xyz, right_rgb, nullptr,
                                   stream);
}

sd_status sd_fence_to_fence_boxes(sd_handle* h, const float* fence_xyz, const uint8_t* fence_rgb, const int32_t* n_fence, int B, int cap,
                                  const sd_rw_result* road, const sd_f2f_params* prm, sd_f2f_result* results, float* left_xyz,
                                  uint8_t* left_rgb, float* right_xyz, uint8_t* right_rgb, sd_plane_box* boxes_dev, void* stream) {
    if (!h || !fence_xyz || !n_fence || !road || !prm || !results || B <= 0 || B > h->max_batch || cap <= 0 || cap > h->cap)
        return fail(h, SD_ERR_INVALID, "sd_fence_to_fence: bad arguments");
    if (!h->bound) return fail(h, SD_ERR_STATE, "sd_bind_memory first");
    hipStream_t s = (hipStream_t)stream;
    const O3dLayout views(h->max_batch, h->cap);       // (the fence chain's views over the idle Open3D region)
    float* A = at<float>(h, h->a.bufA);     // fence, then left fence
    float* Rb = at<float>(h, h->a.bufB);    // right fence
    float* Lb = at<float>(h, h->a.o3d + views.fence_left_xyz);
    uint8_t* cA = fence_rgb ? at<uint8_t>(h, h->a.rgbA) : nullptr;
    uint8_t* cR = fence_rgb ? at<uint8_t>(h, h->a.rgbB) : nullptr;
    uint8_t* cL = fence_rgb ? at<uint8_t>(h, h->a.o3d + views.fence_left_rgb) : nullptr;
    if ((left_rgb || right_rgb) && !fence_rgb) return fail(h, SD_ERR_INVALID, "sd_fence_to_fence: colour outputs need fence_rgb");
    auto C = [&](int j) { return cnt_slot(h, (CntSlot)(CNT_F2F_FENCE + j)); };      // row j of sd_f2f_result::counts
    int32_t* packed = at<int32_t>(h, h->a.f2f_counts);
    double* planes = at<double>(h, h->a.f2f_planes);   // road | left | right, [B][4] each
    double *p_road = planes, *p_left = planes + (size_t)B * 4, *p_right = planes + (size_t)B * 8;
    HIPCHK(h, hipMemcpyAsync(C(0), n_fence, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    HIPCHK(h, launch_gather_planes(reinterpret_cast<const RwResultDev*>(road), B, p_road, s));
    HIPCHK(h, launch_mad_filter({fence_xyz, fence_rgb, n_fence}, {A, cA, C(1)}, B, cap, 1, prm->mad_y, nullptr, nullptr, s));
    HIPCHK(h, launch_filter_coord({A, cA, C(1)}, {A, cA, C(2)}, B, cap, F_ABS_LT, 2, prm->z_max, nullptr, s));
    HIPCHK(h, launch_extract_pcls({A, cA, C(2)}, {Lb, cL, C(3)}, {Rb, cR, C(4)}, B, cap, 0, nullptr, s));
    HIPCHK(h, launch_mad_filter({Lb, cL, C(3)}, {Lb, cL, C(5)}, B, cap, 0, prm->mad_left, nullptr, nullptr, s));
    // (the fits filter in place: each box is taken before its fit)
    if (boxes_dev) HIPCHK(h, launch_plane_box({Lb, cL, C(5)}, B, cap, 0, reinterpret_cast<PlaneBoxDev*>(boxes_dev), 2, 0, s));
    HIPCHK(h, launch_plane_filter({Lb, cL, C(5)}, {Lb, cL, C(5)}, B, cap, 0, prm->plane_thr, p_left, nullptr, s));
    HIPCHK(h, launch_mad_filter({Rb, cR, C(4)}, {Rb, cR, C(6)}, B, cap, 0, prm->mad_right, nullptr, nullptr, s));
    if (boxes_dev) HIPCHK(h, launch_plane_box({Rb, cR, C(6)}, B, cap, 0, reinterpret_cast<PlaneBoxDev*>(boxes_dev), 2, 1, s));
    HIPCHK(h, launch_plane_filter({Rb, cR, C(6)}, {Rb, cR, C(6)}, B, cap, 0, prm->plane_thr, p_right, nullptr, s));
    // denoised left / right fence clouds (the reference writes them to *_FENCE.ply, semantic_depth.py:412-415); sizes = counts[5], counts[6]
    if (left_xyz) HIPCHK(h, hipMemcpyAsync(left_xyz, Lb, (size_t)B * cap * 3 * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (right_xyz) HIPCHK(h, hipMemcpyAsync(right_xyz, Rb, (size_t)B * cap * 3 * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (left_rgb) HIPCHK(h, hipMemcpyAsync(left_rgb, cL, (size_t)B * cap * 3, hipMemcpyDeviceToDevice, s));
    if (right_rgb) HIPCHK(h, hipMemcpyAsync(right_rgb, cR, (size_t)B * cap * 3, hipMemcpyDeviceToDevice, s));
    // counts array for the kernel is [7][B] contiguous: compact the strided slots
    for (int j = 0; j < CNT_F2F_ROWS; ++j)
        HIPCHK(h, hipMemcpyAsync(packed + (size_t)j * B, C(j), (size_t)B * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    HIPCHK(h, launch_f2f(p_road, p_left, p_right, B, prm->depth, packed, reinterpret_cast<F2fResultDev*>(results), s));
    return SD_OK;
}

sd_status sd_road_width_profile(sd_handle* h, const float* xyz_dev, const int32_t* n_dev, int B, int cap, const double* depths_host, int D,
                                double window, double depth_offset, sd_rw_depth_result* results_dev, void* workspace_dev, size_t workspace_bytes,
                                void* stream) {
    if (!h || !xyz_dev || !n_dev || !depths_host || !results_dev || !workspace_dev)
        return fail(h, SD_ERR_INVALID, "sd_road_width_profile: null pointer");
    if (B < 1 || B > 65535 || cap < 1 || D < 1 || D > SD_PROFILE_MAX_DEPTHS)
        return fail(h, SD_ERR_INVALID, "sd_road_width_profile: B in 1..65535, cap >= 1 and D in 1..SD_PROFILE_MAX_DEPTHS");
    if (!std::isfinite(window) || !std::isfinite(depth_offset) || !(window > 0))
        return fail(h, SD_ERR_INVALID, "sd_road_width_profile: window must be finite and > 0, depth_offset finite");
    for (int i = 0; i < D; ++i)
        if (!std::isfinite(depths_host[i])) return fail(h, SD_ERR_INVALID, "sd_road_width_profile: a depth is not finite");
    // every index the kernels form follows from B, cap, D and this capacity: nothing is launched otherwise
    if (workspace_bytes < sdrwp::workspace_bytes(B, cap, D))
        return fail(h, SD_ERR_INVALID, "sd_road_width_profile: workspace smaller than sd_rw_profile_workspace reports");
    if ((reinterpret_cast<uintptr_t>(workspace_dev) & 15) || (reinterpret_cast<uintptr_t>(xyz_dev) & 3) || (reinterpret_cast<uintptr_t>(n_dev) & 3) ||
        (reinterpret_cast<uintptr_t>(results_dev) & 7))
        return fail(h, SD_ERR_INVALID, "sd_road_width_profile: workspace_dev must be 16-byte, results_dev 8-byte, the float and counter arrays 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    h->rwp_stage.resize((size_t)D);
    sdrwp::sorted_windows(depths_host, D, window, depth_offset, h->rwp_stage.data());
    HIPCHK(h, hipMemcpyAsync(static_cast<uint8_t*>(workspace_dev) + sdrwp::Layout(B, cap, D).windows, h->rwp_stage.data(), sizeof(sdrwp::Window) * (size_t)D, hipMemcpyHostToDevice, s));
    HIPCHK(h, launch_rw_profile(xyz_dev, n_dev, B, cap, D, workspace_dev, results_dev, s));
    return SD_OK;
}

sd_status sd_f2f_profile(sd_handle* h, const sd_rw_result* road_dev, const sd_f2f_result* f2f_dev, int B, const double* depths_host, int D,
                         sd_f2f_depth_result* results_dev, void* stream) {
    if (!h || !road_dev || !f2f_dev || !depths_host || !results_dev) return fail(h, SD_ERR_INVALID, "sd_f2f_profile: null pointer");
    if (B < 1 || B > 65535 || D < 1 || D > SD_PROFILE_MAX_DEPTHS)
        return fail(h, SD_ERR_INVALID, "sd_f2f_profile: B in 1..65535 and D in 1..SD_PROFILE_MAX_DEPTHS");
    if ((reinterpret_cast<uintptr_t>(road_dev) & 7) || (reinterpret_cast<uintptr_t>(f2f_dev) & 7) || (reinterpret_cast<uintptr_t>(results_dev) & 7))
        return fail(h, SD_ERR_INVALID, "sd_f2f_profile: the record arrays must be 8-byte aligned");
    F2fDepths depths{};
    for (int i = 0; i < D; ++i) {
        if (!std::isfinite(depths_host[i])) return fail(h, SD_ERR_INVALID, "sd_f2f_profile: a depth is not finite");
        depths.d[i] = depths_host[i];
    }
    HIPCHK(h, launch_f2f_profile(road_dev, f2f_dev, B, depths, D, results_dev, (hipStream_t)stream));
    return SD_OK;
}

// the four window tables of a PIL resample into their places in its workspace `ws` (the windows stay alive in the handle for the copies)
static sd_status upload_pil_tables(sd_handle* h, uint8_t* ws, const sdpil::Layout& l, const sdpil::Windows& x, const sdpil::Windows& y, hipStream_t s) {
    HIPCHK(h, hipMemcpyAsync(ws + l.x_bounds, x.bounds.data(), x.bounds.size() * 4, hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemcpyAsync(ws + l.x_k, x.k.data(), x.k.size() * 4, hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemcpyAsync(ws + l.y_bounds, y.bounds.data(), y.bounds.size() * 4, hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemcpyAsync(ws + l.y_k, y.k.data(), y.k.size() * 4, hipMemcpyHostToDevice, s));
    return SD_OK;
}

sd_status sd_resize_pil_bilinear_u8(sd_handle* h, const uint8_t* src_dev, int B, int src_h, int src_w, int pixel_stride, int channels, int reverse,
                                    uint8_t* dst_dev, int dst_h, int dst_w, void* workspace_dev, size_t workspace_bytes, void* stream) {
    if (!h || !src_dev || !dst_dev || !workspace_dev) return fail(h, SD_ERR_INVALID, "sd_resize_pil_bilinear_u8: null pointer");
    if (B < 1 || B > 65535 || (channels != 1 && channels != 3) || pixel_stride < channels || pixel_stride > 4)
        return fail(h, SD_ERR_INVALID, "sd_resize_pil_bilinear_u8: B in 1..65535, channels 1 or 3, channels <= pixel_stride <= 4");
    if (!sdpil::axis_ok(src_h, dst_h) || !sdpil::axis_ok(src_w, dst_w))
        return fail(h, SD_ERR_INVALID, "sd_resize_pil_bilinear_u8: extents in 1..16384 and a downscale factor of at most 32 per axis");
    // every index the kernels form follows from these sizes, the windows made below and this capacity: nothing is launched otherwise
    if (workspace_bytes < sdpil::workspace_bytes(B, src_h, src_w, dst_h, dst_w, channels) || (reinterpret_cast<uintptr_t>(workspace_dev) & 15))
        return fail(h, SD_ERR_INVALID, "sd_resize_pil_bilinear_u8: workspace smaller than sd_resize_pil_workspace reports, or not 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    // (a second call overwrites the windows the first call's copies read: pageable sources are staged before hipMemcpyAsync returns)
    sdpil::pil_windows(src_w, dst_w, h->pil_x);
    sdpil::pil_windows(src_h, dst_h, h->pil_y);
    if (h->pil_x.taps > sdpil::taps_bound(src_w, dst_w) || h->pil_y.taps > sdpil::taps_bound(src_h, dst_h))
        return fail(h, SD_ERR_STATE, "sd_resize_pil_bilinear_u8: a window is longer than its bound");
    uint8_t* ws = static_cast<uint8_t*>(workspace_dev);
    if (const sd_status st = upload_pil_tables(h, ws, sdpil::Layout(B, src_h, src_w, dst_h, dst_w, channels), h->pil_x, h->pil_y, s); st != SD_OK) return st;
    HIPCHK(h, launch_pil_resample_u8(src_dev, B, src_h, src_w, pixel_stride, channels, reverse ? 1 : 0, dst_dev, dst_h, dst_w, h->pil_x, ws, s));
    return SD_OK;
}

sd_status sd_disp_image(sd_handle* h, const float* disp_dev, const float* mult_host, int B, int height, int width, int out_h, int out_w, int cmap,
                        uint8_t* out_bgr_dev, int32_t* flags_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
    if (!h || !disp_dev || !out_bgr_dev || !flags_dev || !workspace_dev) return fail(h, SD_ERR_INVALID, "sd_disp_image: null pointer");
    if (B < 1 || B > 65535 || !sddisp::valid_map(cmap))
        return fail(h, SD_ERR_INVALID, "sd_disp_image: B in 1..65535, cmap SD_CMAP_GRAY or SD_CMAP_PLASMA");
    if (height < 1 || width < 1 || out_h < 1 || out_w < 1 || !sddisp::valid_sizes(height, width, out_h, out_w))
        return fail(h, SD_ERR_INVALID, "sd_disp_image: extents in 1..16384 and a downscale factor of at most 32 per axis");
    // every index the kernels form follows from these sizes, the windows made below and this capacity: nothing is launched otherwise
    const sddisp::Layout l(B, height, width, out_h, out_w);
    if (workspace_bytes < l.total || (reinterpret_cast<uintptr_t>(workspace_dev) & 15))
        return fail(h, SD_ERR_INVALID, "sd_disp_image: workspace smaller than sd_disp_image_workspace reports, or not 16-byte aligned");
    if ((reinterpret_cast<uintptr_t>(disp_dev) & 3) || (reinterpret_cast<uintptr_t>(flags_dev) & 3))
        return fail(h, SD_ERR_INVALID, "sd_disp_image: disp_dev and flags_dev must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    uint8_t* ws = static_cast<uint8_t*>(workspace_dev);
    const bool resize = sddisp::resized(height, width, out_h, out_w);
    if (resize) {
        sdpil::pil_windows(width, out_w, h->disp_x);
        sdpil::pil_windows(height, out_h, h->disp_y);
        if (h->disp_x.taps > sdpil::taps_bound(width, out_w) || h->disp_y.taps > sdpil::taps_bound(height, out_h))
            return fail(h, SD_ERR_STATE, "sd_disp_image: a window is longer than its bound");
        if (const sd_status st = upload_pil_tables(h, ws + l.pil, sdpil::Layout(B, height, width, out_h, out_w, 1), h->disp_x, h->disp_y, s); st != SD_OK) return st;
    }
    if (mult_host) {
        h->disp_mult.assign(mult_host, mult_host + B);
        HIPCHK(h, hipMemcpyAsync(ws + l.mult, h->disp_mult.data(), (size_t)B * sizeof(float), hipMemcpyHostToDevice, s));
    }
    HIPCHK(h, launch_disp_image(disp_dev, B, height, width, out_h, out_w, cmap, mult_host ? 1 : 0, out_bgr_dev, flags_dev, h->disp_x, ws, s));
    return SD_OK;
}

sd_status sd_seg_confusion(sd_handle* h, const uint8_t* pred_dev, const uint8_t* labels_dev, int B, int height, int width, const uint8_t* table_host,
                           int64_t* counts_dev, void* stream) {
    if (!h || !pred_dev || !labels_dev || !table_host || !counts_dev) return fail(h, SD_ERR_INVALID, "sd_seg_confusion: null pointer");
    if (B < 1 || B > 65535 || height < 1 || width < 1 || height > sdpil::kMaxExtent || width > sdpil::kMaxExtent)
        return fail(h, SD_ERR_INVALID, "sd_seg_confusion: B in 1..65535, height and width in 1..16384");
    if (reinterpret_cast<uintptr_t>(counts_dev) & 7) return fail(h, SD_ERR_INVALID, "sd_seg_confusion: counts_dev must be 8-byte aligned");
    SegTable table;
    for (int i = 0; i < 256; ++i) {
        if (table_host[i] > 2) return fail(h, SD_ERR_INVALID, "sd_seg_confusion: a table value above 2 (classes are 0, 1, 2)");
        table.v[i] = table_host[i];
    }
    HIPCHK(h, launch_seg_confusion(pred_dev, labels_dev, B, height, width, table, counts_dev, (hipStream_t)stream));
    return SD_OK;
}

// ---------------------------------------------------------------- pcl.py function by function (single cloud)
static sd_status set_n(sd_handle* h, int n, int32_t** dn, hipStream_t s) {
    *dn = at<int32_t>(h, h->a.scalar);
    HIPCHK(h, hipMemsetD32Async((hipDeviceptr_t)*dn, n, 1, s));
    return SD_OK;
}
#define PCL_PROLOGUE()                                                                                         \
    if (!h || !xyz || !xyz_out || !n_out || n < 0 || (size_t)n > (size_t)h->max_batch * h->cap)                \
        return fail(h, SD_ERR_INVALID, "pcl: bad arguments");                                                  \
    if (!h->bound) return fail(h, SD_ERR_STATE, "sd_bind_memory first");                                       \
    hipStream_t s = (hipStream_t)stream;                                                                       \
    int32_t* dn = nullptr;                                                                                     \
    { sd_status st_ = set_n(h, n, &dn, s); if (st_ != SD_OK) return st_; }                                     \
    const int cap1 = std::max(n, 1);

sd_status sd_pcl_remove_from_to(sd_handle* h, const float* xyz, const uint8_t* rgb, int n, int axis, double to_meter,
                                float* xyz_out, uint8_t* rgb_out, int32_t* n_out, void* stream) {
    PCL_PROLOGUE();
    HIPCHK(h, launch_filter_coord({xyz, rgb, dn}, {xyz_out, rgb_out, n_out}, 1, cap1, F_LT_NEG, axis, to_meter, at(h, h->a.cmp), s));
    return SD_OK;
}
sd_status sd_pcl_threshold_complete(sd_handle* h, const float* xyz, const uint8_t* rgb, int n, int axis, double threshold,
                                    float* xyz_out, uint8_t* rgb_out, int32_t* n_out, void* stream) {
    PCL_PROLOGUE();
    HIPCHK(h, launch_filter_coord({xyz, rgb, dn}, {xyz_out, rgb_out, n_out}, 1, cap1, F_ABS_LT, axis, threshold, at(h, h->a.cmp), s));
    return SD_OK;
}
sd_status sd_pcl_remove_noise_by_mad(sd_handle* h, const float* xyz, const uint8_t* rgb, int n, int axis, double threshold,
                                     float* xyz_out, uint8_t* rgb_out, int32_t* n_out, float* stats_out, void* stream) {
    PCL_PROLOGUE();
    HIPCHK(h, launch_mad_filter({xyz, rgb, dn}, {xyz_out, rgb_out, n_out}, 1, cap1, axis, threshold, stats_out, at(h, h->a.cmp), s));
    return SD_OK;
}
sd_status sd_pcl_remove_noise_by_fitting_plane(sd_handle* h, const float* xyz, const uint8_t* rgb, int n, int axis, double threshold,
                                               float* xyz_out, uint8_t* rgb_out, int32_t* n_out, double* coeff_out, void* stream) {
    PCL_PROLOGUE();
    if (axis < 0 || axis > 2) return fail(h, SD_ERR_INVALID, "axis");
    HIPCHK(h, launch_plane_filter({xyz, rgb, dn}, {xyz_out, rgb_out, n_out}, 1, cap1, axis, threshold, coeff_out, at(h, h->a.cmp), s));
    return SD_OK;
}
sd_status sd_pcl_extract_pcls(sd_handle* h, const float* xyz, const uint8_t* rgb, int n, int axis, float* left_xyz, uint8_t* left_rgb,
                              int32_t* n_left, float* right_xyz, uint8_t* right_rgb, int32_t* n_right, float* mean_out, void* stream) {
    float* xyz_out = left_xyz;
    int32_t* n_out = n_left;
    PCL_PROLOGUE();
    if (!right_xyz || !n_right || axis < 0 || axis > 2) return fail(h, SD_ERR_INVALID, "pcl: bad arguments");
    HIPCHK(h, launch_extract_pcls({xyz, rgb, dn}, {left_xyz, left_rgb, n_left}, {right_xyz, right_rgb, n_right}, 1, cap1, axis, mean_out, s));
    return SD_OK;
}
sd_status sd_pcl_get_end_points_of_road(sd_handle* h, const float* xyz, int n, double depth, double window, sd_rw_result* out,
                                        void* stream) {
    if (!h || !xyz || !out || n < 0) return fail(h, SD_ERR_INVALID, "pcl: bad arguments");
    if (!h->bound) return fail(h, SD_ERR_STATE, "sd_bind_memory first");
    hipStream_t s = (hipStream_t)stream;
    int32_t* dn = nullptr;
    sd_status st = set_n(h, n, &dn, s);
    if (st != SD_OK) return st;
    HIPCHK(h, launch_end_points({xyz, nullptr, dn}, 1, std::max(n, 1), depth, window, reinterpret_cast<RwResultDev*>(out), s));
    return SD_OK;
}
sd_status sd_o3d_statistical_outlier_removal(sd_handle* h, const float* xyz, const uint8_t* rgb, int n, int nb_neighbors,
                                             double std_ratio, float* xyz_out, uint8_t* rgb_out, int32_t* n_out,
                                             double* mean_dist_out, void* stream) {
    PCL_PROLOGUE();
    if (nb_neighbors < 1 || nb_neighbors > 16) return fail(h, SD_ERR_INVALID, "nb_neighbors must be in 1..16");
    if (O3dLayout(1, cap1).total > O3dLayout(h->max_batch, h->cap).total) return fail(h, SD_ERR_INVALID, "cloud too large");
    HIPCHK(h, launch_sor({xyz, rgb, dn}, {xyz_out, rgb_out, n_out}, 1, cap1, nb_neighbors, std_ratio, at(h, h->a.o3d), mean_dist_out, at(h, h->a.cmp), s));
    return SD_OK;
}
sd_status sd_o3d_radius_outlier_removal(sd_handle* h, const float* xyz, const uint8_t* rgb, int n, int nb_points, double radius,
                                        float* xyz_out, uint8_t* rgb_out, int32_t* n_out, void* stream) {
    PCL_PROLOGUE();
    if (O3dLayout(1, cap1).total > O3dLayout(h->max_batch, h->cap).total) return fail(h, SD_ERR_INVALID, "cloud too large");
    HIPCHK(h, launch_ror({xyz, rgb, dn}, {xyz_out, rgb_out, n_out}, 1, cap1, nb_points, radius, at(h, h->a.o3d), at(h, h->a.cmp), s));
    return SD_OK;
}

// ---------------------------------------------------------------- introspection
sd_status sd_net_tensor(sd_handle* h, sd_net net, const char* name, float* out, size_t cap_floats, int64_t* shape_out, void* stream) {
    if (!h || !name) return SD_ERR_INVALID;
    NetPlan& p = plan_of(h, net);
    auto it = p.tensor_by_name.find(name);
    if (it == p.tensor_by_name.end()) return fail(h, SD_ERR_NOTFOUND, std::string("unknown tensor ") + name);
    const TensorDesc& t = p.tensors[it->second];
    const int N = net == SD_NET_FCN8S ? h->last_fcn_images : h->last_mono_images;
    if (shape_out) { shape_out[0] = N; shape_out[1] = t.H; shape_out[2] = t.W; shape_out[3] = t.fmt != PL_F32 ? t.Ctf : t.C; }
    if (!out) return SD_OK;
    if (!h->bound) return fail(h, SD_ERR_STATE, "sd_bind_memory first");
    const size_t numel = (size_t)N * t.H * t.W * (t.fmt != PL_F32 ? t.Ctf : t.C);
    if (numel > cap_floats) return fail(h, SD_ERR_INVALID, "output buffer too small");
    const char* abase = act_base(h, net);
    if (t.fmt != PL_F32)      // split planes -> f32
        HIPCHK(h, launch_unsplit(reinterpret_cast<const float*>(abase + t.offset), out, (long)N * t.H * t.W, t.C, t.Ctf, (size_t)p.images * t.H * t.W * t.C,
                                 t.planar16 ? (size_t)p.images * t.H * t.W * 16 : 0, t.fmt, (hipStream_t)stream));
    else
        HIPCHK(h, hipMemcpyAsync(out, abase + t.offset, numel * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return SD_OK;
}

sd_status sd_profile(sd_handle* h, int enable) {
    if (!h) return SD_ERR_INVALID;
    h->prof = enable != 0;
    if (!h->prof) { h->prof_recs.clear(); h->prof_used = 0; h->prof_last = nullptr; }
    return SD_OK;
}

sd_status sd_profile_read(sd_handle* h, sd_profile_bucket* out, int cap_buckets, int* n_out) {
    if (!h || !out || !n_out || cap_buckets < 1) return SD_ERR_INVALID;
    HIPCHK(h, hipDeviceSynchronize());
    const bool verbose = (h->sw & SW_PROFILE_VERBOSE) != 0;
    int n = 0;
    for (auto& r : h->prof_recs) {
        float ms = 0.f;
        HIPCHK(h, hipEventElapsedTime(&ms, r.a, r.b));
        if (verbose)
            std::fprintf(stderr, "[sd_profile] %-28s M=%-8d N=%-5d K=%-6d %8.3f ms %7.2f TF/s  %s\n", r.op, r.M, r.N, r.K, ms,
                         r.flops / (ms * 1e-3) / 1e12, r.kernel.c_str());
        int b = 0;
        while (b < n && r.kernel != out[b].kernel) ++b;
        if (b == n) {
            if (n == cap_buckets) continue;
            std::memset(&out[n], 0, sizeof(out[n]));
            std::strncpy(out[n].kernel, r.kernel.c_str(), 63);
            ++n;
        }
        out[b].launches += 1;
        out[b].ms += ms;
        out[b].flops += r.flops;
        out[b].bytes += r.bytes;
    }
    *n_out = n;
    h->prof_recs.clear();
    h->prof_used = 0;
    h->prof_last = nullptr;
    return SD_OK;
}

double sd_net_flops_per_image(const sd_handle* h, sd_net net) { return h ? plan_of(h, net).flops_per_image : 0.0; }

int sd_pass_frames(const sd_handle* h) { return h ? h->chunk : 0; }

sd_status sd_saturation_count(sd_handle* h, uint64_t* count_out, int reset) {
    if (!h) return SD_ERR_INVALID;
    if (!h->bound) return fail(h, SD_ERR_STATE, "sd_bind_memory first");
    HIPCHK(h, hipDeviceSynchronize());
    unsigned long long v = 0;
    if (count_out) {
        HIPCHK(h, hipMemcpy(&v, sat_counter(h), sizeof(v), hipMemcpyDeviceToHost));
        *count_out = (uint64_t)v;
    }
    if (reset) {
        HIPCHK(h, hipMemset(sat_counter(h), 0, sizeof(v)));
        HIPCHK(h, hipMemset(sat_orphans(h), 0, sizeof(uint32_t)));      // (a part of the global count)
    }
    return SD_OK;
}

sd_status sd_set_small_batch(sd_handle* h, int on) {
    if (!h) return SD_ERR_INVALID;
    if (on > 2) return fail(h, SD_ERR_INVALID, "sd_set_small_batch: levels 0 (off), 1 (split-K GEMM layers) and 2 (1 + chunk-split direct 3x3 layers)");
    if (h->prec != (int)SD_PREC_F16X2) return fail(h, SD_ERR_INVALID, "sd_set_small_batch: the split-K forms exist for SD_PREC_F16X2 only");
    if (h->bound) return fail(h, SD_ERR_STATE, "sd_set_small_batch: call it before sd_bind_memory (the workspace changes)");
    if (on && !h->cus) {
        // the CU count the rule reads, latched once: the device's, or (no device: planning on a host) the MI355X's 256
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, h->device) != hipSuccess || n <= 0) { (void)hipGetLastError(); n = 256; }
        h->cus = n;
    }
    h->small_batch = on < 0 ? 1 : on;       // (any other non-zero value has always meant "on")
    resolve_forms(h);
    carve_workspace(h);
    return SD_OK;
}

int sd_small_batch_split(long rows, int cout, int kpad, int cus, int* k_tiles_per_slice_out) {
    const int S = conv_splitk_slices(rows, cout, kpad, cus);
    if (k_tiles_per_slice_out)
        for (int i = 0; i < S; ++i) {
            int first, count;
            conv_splitk_range(kpad / 32, S, i, first, count);
            k_tiles_per_slice_out[i] = S > 1 ? count : (kpad > 0 ? kpad / 32 : 0);
        }
    return S;
}

int sd_small_batch_split_direct(long items, int nchunks, int cus, int* chunks_per_slice_out) {
    const int S = conv_splitc_slices(items, nchunks, cus);
    if (chunks_per_slice_out)
        for (int i = 0; i < S; ++i) {
            int first, count;
            conv_splitk_range(nchunks, S, i, first, count);
            chunks_per_slice_out[i] = S > 1 ? count : (nchunks > 0 ? nchunks : 0);
        }
    return S;
}

sd_status sd_small_batch_plan(const sd_handle* h, sd_net net, char* layers_out, size_t cap) {
    if (!h || !layers_out || !cap) return SD_ERR_INVALID;
    const NetPlan& p = plan_of(h, net);
    std::string out;
    for (size_t i = 0; i < p.ops.size(); ++i)
        if (const int S = h->forms[net][i].slices; S > 1) out += (out.empty() ? "" : ",") + p.ops[i].name + ":" + std::to_string(S);
    std::strncpy(layers_out, out.c_str(), cap - 1);
    layers_out[cap - 1] = 0;
    return out.size() + 1 > cap ? SD_ERR_INVALID : SD_OK;
}

sd_status sd_conv_forms(const sd_handle* h, sd_net net, int frames, char* out, size_t cap) {
    if (!h || !out || !cap || frames < 0 || frames > h->chunk) return SD_ERR_INVALID;
    const NetPlan& p = plan_of(h, net);
    std::string text;
    for (size_t i = 0; i < p.ops.size(); ++i) {
        ConvForm called;
        const ConvForm& f = form_of(h, net, i, frames ? frames * (p.images / p.frames) : p.images, called);
        if (f.family != CF_NONE || f.error) text += p.ops[i].name + " " + (f.error ? std::string(f.error) : f.verbose) + " " + std::to_string(f.slices) + "\n";
    }
    std::strncpy(out, text.c_str(), cap - 1);
    out[cap - 1] = 0;
    return text.size() + 1 > cap ? SD_ERR_INVALID : SD_OK;
}

sd_status sd_set_reserved_cus(sd_handle* h, int n) {
    if (!h || n < 0 || n > 128) return SD_ERR_INVALID;
    h->reserve_cus = n;
    return SD_OK;
}

// the same counter without a device synchronisation: an 8-byte device-to-host copy enqueued on `stream` (host_dst: pinned memory of the caller; it
// holds the count once the work enqueued on the stream before this call has finished)
sd_status sd_saturation_count_async(sd_handle* h, uint64_t* host_dst, void* stream) {
    if (!h || !host_dst) return SD_ERR_INVALID;
    if (!h->bound) return fail(h, SD_ERR_STATE, "sd_bind_memory first");
    HIPCHK(h, hipMemcpyAsync(host_dst, sat_counter(h), sizeof(uint64_t), hipMemcpyDeviceToHost, (hipStream_t)stream));
    return SD_OK;
}

// the per-frame counts of the same clamps: frames 0..n-1 of the caller's batch, copied on `stream`; with reset the max_batch counters are then
// zeroed on the same stream (the global counter of sd_saturation_count is not touched)
sd_status sd_saturation_frames(sd_handle* h, uint32_t* dst, int n, int reset, void* stream) {
    if (!h || !dst || n < 1 || n > h->max_batch) return fail(h, SD_ERR_INVALID, "sd_saturation_frames: bad arguments");
    if (!h->bound) return fail(h, SD_ERR_STATE, "sd_bind_memory first");
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(h, hipMemcpyAsync(dst, sat_frames(h), (size_t)n * sizeof(uint32_t), hipMemcpyDefault, s));
    if (reset) HIPCHK(h, hipMemsetAsync(sat_frames(h), 0, (size_t)h->max_batch * sizeof(uint32_t), s));
    return SD_OK;
}

// the clamps of frames 0..n-1 and those no frame owns leave the global counter; the per-frame counts and the unowned count are zeroed.
// One single-workgroup kernel on `stream`, no synchronisation (the host-side recompute mode calls it once the flagged frames are recomputed)
sd_status sd_saturation_settle(sd_handle* h, int n, void* stream) {
    if (!h || n < 1 || n > h->max_batch) return fail(h, SD_ERR_INVALID, "sd_saturation_settle: bad arguments");
    if (!h->bound) return fail(h, SD_ERR_STATE, "sd_bind_memory first");
    HIPCHK(h, launch_sat_settle(sat_counter(h), sat_frames(h), sat_orphans(h), n, h->max_batch, (hipStream_t)stream));
    return SD_OK;
}

}  // extern "C"
