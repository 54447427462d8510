/*
 * semdepth.h — C ABI of libsemdepth.so, the MI355X (gfx950) implementation of semantic-depth's
 * per-frame hot path.  Plain pointers and sizes only; no torch / C++ types cross this boundary.
 *
 * The reference (pablopalafox/semantic-depth) has no FFI: its operator boundary is the Python
 * duck-type FrameProcessor consumes.  Every entry point below names the reference interface
 * it replaces (file:line relative to the reference tree; "seq" = semantic_depth_cityscapes_sequence.py).
 *
 * Conventions
 *   - every function returns sd_status (0 = OK, negative = error); sd_last_error() gives the text.
 *   - all data pointers are DEVICE pointers owned by the caller unless the name ends in _host.
 *   - every compute call takes a hipStream_t (passed as void*) and is asynchronous w.r.t. the host.
 *   - a handle is bound to one device, is not thread-safe, and owns no device memory: the caller
 *     (PyTorch-ROCm in the Python host) allocates the weight and workspace arenas whose sizes
 *     sd_query_memory() reports and binds them with sd_bind_memory().
 *   - images are NHWC, row-major, channel order as the caller supplies it (the reference feeds BGR).
 *
 * Streams
 *   Calls on one handle are enqueued from ONE host thread: the handle keeps host-side state (the camera stage, the look-back epoch
 *   of the one-pass fusion, the frame count of the last monodepth pass) that follows the order of the calls, not of the streams.
 *   Two streams of one handle may be in flight in exactly one arrangement, the one bench.py times: the NETWORK calls
 *   (sd_fcn8s_forward, sd_monodepth_forward) of a batch on one stream while the TAIL calls of the batch before it run on another.
 *   Tail calls are sd_postprocess_fuse_backproject / sd_fuse_backproject, sd_road_width, sd_fence_to_fence and the profile calls
 *   (sd_road_width_profile, sd_f2f_profile); all tail calls of all batches go to one stream.  The caller's only obligation: the
 *   fusion that reads the raw pair in the arena (sd_postprocess_fuse_backproject with disp_raw == NULL) is ordered AFTER the
 *   sd_monodepth_forward that wrote the pair and BEFORE the next sd_monodepth_forward (an event each way).  Tensors the caller owns
 *   (masks, frames, clouds, records) are the caller's to order.  Every other call (sd_resize_cubic_u8 aside, which touches only
 *   o_rsz) belongs on the stream of its family, or behind a synchronisation.
 *   The workspace regions (struct Arena in csrc/handle_arena.hpp: o_x is its field x, o_misc its fields scalar, zero, f2f_counts, f2f_planes and
 *   sat) and the call families that touch them -- net = network calls, tail = tail calls:
 *     o_fcn       FCN-8s activations                          net (sd_fcn8s_forward) reads + writes; sd_net_tensor reads
 *     o_mono      monodepth activations                       net (sd_monodepth_forward) reads + writes; sd_net_tensor reads
 *       raw pair  the plan's output tensor inside o_mono      net (sd_monodepth_forward) writes; tail (fusion from the arena) reads
 *     o_fuse      block counts / offsets of the fusion        tail (fusion, the count-scan-write forms) reads + writes
 *     o_fuse1     look-back words + tickets, one-pass fusion  tail (fusion) reads + writes; zeroed on its stream every 1023 launches
 *     o_cams      device copy of the cameras                  tail (fusion) writes when the cameras changed, reads
 *     o_bufA, o_bufB  point ping-pong of the chains           tail (sd_road_width, sd_fence_to_fence) reads + writes
 *     o_rgbA, o_rgbB  colour ping-pong of the chains          tail (sd_road_width, sd_fence_to_fence) reads + writes
 *     o_cnt       per-stage counts (slots 1-6 road, 8-14 fence)  tail (sd_road_width, sd_fence_to_fence) reads + writes
 *     o_plane     road plane coefficients                     tail (sd_road_width) reads + writes
 *     o_o3d       Open3D filter scratch / left fence cloud    tail (sd_road_width, sd_fence_to_fence) reads + writes
 *     o_cmp       ordered-compaction scratch                  tail (sd_road_width) reads + writes; the sd_pcl_* / sd_o3d_* calls too
 *     o_misc      +0     scalar slot                          the single-cloud sd_pcl_* / sd_o3d_* calls write + read; neither family
 *                 +256   zero page (to +4096)                 net reads; NOTHING writes after sd_bind_memory
 *                 +4096  f2f counts [7][B]                    tail (sd_fence_to_fence) reads + writes
 *                 then   f2f planes [3][B][4]                 tail (sd_fence_to_fence) reads + writes
 *                 then   clamp counters                       net reads + writes (atomics, the per-frame fold); the sd_saturation_* calls (net's stream)
 *     o_rsz       tap tables of sd_resize_cubic_u8            sd_resize_cubic_u8 only
 *     o_rsz_cmp   tap tables of sd_compose_result_frames      sd_compose_result_frames only
 *     o_splitk    partial sums of the split layers            net reads + writes (sd_set_small_batch handles)
 *   The profile calls use the caller's workspace and none of these regions.  The two families share the raw pair and nothing else;
 *   tests/two_stream_cases.py holds this table per call and checks the benchmark's event choreography against it.
 */
#ifndef SEMDEPTH_H
#define SEMDEPTH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int sd_status;
enum {
    SD_OK = 0,
    SD_ERR_INVALID = -1,   /* bad argument */
    SD_ERR_HIP = -2,       /* HIP runtime error (text in sd_last_error) */
    SD_ERR_STATE = -3,     /* call order violated (e.g. forward before weights are loaded) */
    SD_ERR_NOTFOUND = -4,  /* unknown weight / tensor name */
    SD_ERR_FORMAT = -5     /* sd_decode_files_jpeg_coef: the file is readable but not a JPEG -- decode it with sd_decode_files_bgr */
};

typedef enum { SD_ENC_VGG = 0, SD_ENC_RESNET50 = 1 } sd_encoder;      /* semantic_depth.py:721-722 --encoder */
typedef enum { SD_NET_FCN8S = 0, SD_NET_MONODEPTH = 1 } sd_net;
/* arithmetic of the conv stacks (f32 accumulate everywhere; gfx950 has no TF32):
 *   SD_PREC_F32    exact f32 MFMA;
 *   SD_PREC_BF16X2 every f32 operand split into two bf16 (hi + lo), THREE bf16 MFMA products per product (~1e-5 relative);
 *   2-product form: the activation rounded once to fp16 (one 16-bit plane: half the bytes of every tensor), the weight split into
 *                  two fp16 (22 bits), TWO fp16 MFMA products x*w_hi + x*w_lo; the only error is the 2^-12 rounding of the
 *                  activations (3e-5 .. 2e-4 on the outputs per layer, profiles/r02_precision_calibration.json);
 *   1-product form (":1"): the same one-plane fp16 activation times w_hi only: plain fp16 x fp16, adds the 2^-12 rounding of the weights;
 *   x2 form (":x"):  fp16 hi + lo ACTIVATION planes times w_hi: TWO products x_hi*w_hi + x_lo*w_hi, the error is the weight rounding
 *                  alone (for layers whose input tensor is precision-critical; direct 3x3 layers fed by direct 3x3 layers);
 *   SD_PREC_MIXED  FCN-8s as SD_PREC_BF16X2, every monodepth layer in the 2-product form;
 *   SD_PREC_PLAN   per-layer choice between these forms: the built-in plan (sd_default_plan) was calibrated on the MI355X against the
 *                  exact-f32 engine under an error budget; sd_create_with_plan takes any other choice
 *   SD_PREC_BF16X3 fp32-grade on the bf16 MFMA: every f32 operand (activations and weights) is carried as THREE bf16 planes whose sum is
 *                  the f32 value EXACTLY (8 + 8 + 8 significand bits, f32's exponent range); a product is SIX bf16 MFMA products
 *                  (hi*hi + hi*mid + mid*hi + mid*mid + hi*lo + lo*hi, each exact in the f32 accumulator); the dropped terms are below
 *                  2^-23 of the product, the size of the rounding an f32 FMA chain commits per accumulation.  Ceiling 2500 / 6 = 417
 *                  TFLOP/s of algorithmic work against 157.3 for the f32 MFMA;
 *   SD_PREC_F16X2  fp32-grade on THREE fp16 MFMA products (round 5): an activation is two fp16 planes, hi = RNE(v) and lo = RNE((v - hi) * 2^11)
 *                  -- the scaled residual stays in fp16's normal range wherever hi does, so v is carried to 22 significand bits for every
 *                  |v| in [1.2e-4, 65504] without any calibration (4 bytes per element); a weight is two fp16 planes of w * 2^k, the power of two k
 *                  chosen PER LAYER by sd_load_weight from the tensor it is given (largest stored |w'| in [2^12, 2^13): any finite f32
 *                  weight tensor loads); a product is x_hi*w_hi + x_hi*w_lo + x_lo*(w_hi * 2^-11) (the third weight operand formed in
 *                  registers), f32 accumulate, the accumulator times 2^-k in the epilogue.  Dropped: x_lo*w_lo and the representation error of each operand, 2^-23 ..
 *                  2^-24 of the product (an f32 FMA chain commits 2^-24 of the ACCUMULATOR per step).  Activations beyond +-65504 are clamped
 *                  and counted (sd_saturation_count; the host-side classes raise on a non-zero count).  Ceiling 2500 / 3 = 833 TFLOP/s of algorithmic work. */
typedef enum { SD_PREC_F32 = 0, SD_PREC_BF16X2 = 1, SD_PREC_MIXED = 2, SD_PREC_PLAN = 3, SD_PREC_BF16X3 = 4, SD_PREC_F16X2 = 5 } sd_precision;

typedef struct sd_handle sd_handle;

/* camera of DepthFrame.__init__, semantic_depth.py:592-607 (seq:500-508), plus the disparity
 * multiplier of semantic_depth.py:109,145 (seq:105,146).  Doubles: the library rounds the Q-matrix
 * entries to float32 exactly like np.float32([...]) at semantic_depth.py:691-694. */
typedef struct {
    double cx, cy, f, b, disp_mult;
} sd_camera;

/* every literal of the reference's road-width call sites (semantic_depth.py:206-259) */
typedef struct {
    double depth;         /* --depth, :754-756 (10.0) */
    double z_cut;         /* remove_from_to(..., 2, 0.0, 7.0)        :206 */
    double mad_y;         /* remove_noise_by_mad(..., 1, 15.0)       :209 */
    double mad_x;         /* remove_noise_by_mad(..., 0, 2.0)        :212 */
    double plane_thr;     /* remove_noise_by_fitting_plane(axis=1, threshold=5.0) :215-219 */
    int32_t sor_k;        /* statistical_outlier_removal nb_neighbors=10   :234-235 */
    double sor_ratio;     /*                              std_ratio=0.5 */
    int32_t ror_n;        /* radius_outlier_removal nb_points=80           :238-239 */
    double ror_r;         /*                         radius=0.5 */
    double window;        /* +-0.05 depth window, pcl.py:283 */
    double depth_offset;  /* depth-0.02, :254-255 */
    int32_t use_o3d;      /* 0 skips the two Open3D filters */
} sd_rw_params;

/* per-frame record: what the reference prints/draws (semantic_depth.py:259; seq:232-238) plus the
 * kept-point count after every stage.  This is the record the multi-GPU driver all-gathers. */
typedef struct {
    double width;          /* |x_left - x_right|, NaN when !found */
    float x_left, x_right; /* x of the first min-x / max-x point in the depth window */
    float left_pt[3], right_pt[3];
    int32_t found;         /* 0: no road point in the window ((None,None) of pcl.py:303-304) */
    int32_t n_road;        /* projected road points (points3D[road_mask]) */
    int32_t n_zcut, n_mad_y, n_mad_x, n_plane, n_sor, n_ror;
    double plane[4];       /* Cx,Cy,Cz,C of pcl.py:168 */
} sd_rw_result;

/* ---------------------------------------------------------------- lifecycle */
const char* sd_version(void);
const char* sd_status_string(sd_status s);
/* replaces DepthFrame.__init__ + SegmentFrame.__init__ (semantic_depth.py:464-469, :575-624):
 * fixes H, W, the largest batch a call may carry and the monodepth encoder; builds both layer plans.
 * Every kernel choice that changes the order of a sum is made here, on a full network pass of the handle (sd_pass_frames), not on the frames of a
 * call: on one handle a frame's outputs are the same bits whether it is submitted alone, with others, or at another batch position.
 * Environment read HERE and nowhere later: SEMDEPTH_DISABLE=name[,name...] (dma dma3 direct stem fold tail1 pool_fuse planar n16 fuse1 fuse4 flat rowskip
 * dma_big mfma16: the generic kernel instead of the named specialised one -- parity tests and A/B runs; an unknown name fails with SD_ERR_INVALID),
 * SEMDEPTH_CHUNK (frames per network pass, default 32), SEMDEPTH_RESERVE_CUS (sd_set_reserved_cus), SEMDEPTH_PROFILE_VERBOSE=1 (per-layer sd_profile labels),
 * SEMDEPTH_KEEP_ACTIVATIONS (no arena reuse: every intermediate tensor stays readable by sd_net_tensor). */
sd_status sd_create(sd_handle** out, int device, int H, int W, int max_batch, sd_encoder enc, sd_precision prec);
/* the same with an explicit precision plan for the split engine: per network a comma-separated list of conv layer names
 * (sd_net_tensor names, e.g. "fc6,fc7" / "enc/res4*,dec/upconv6"; a trailing '*' matches a prefix, "*" = all, "" = none) that run
 * the 2-product fp16 scheme -- or, with the suffix ":1" / ":x", the 1-product / x2 form; the rest run the 3-product bf16 one.  The
 * choice is closed under "one plane format per tensor" (sd_precision_plan returns what actually runs, with the suffixes).  ":x" on a
 * layer the geometry does not route to the direct 3x3 kernel (or whose producer is not one) keeps three products; on a layer that
 * is no 3x3 stride-1 convolution with a multiple of 64 output channels it is SD_ERR_INVALID, as is an unknown layer name.  A per-pixel
 * head (FCN score layers, dec/disp1) named exactly makes its INPUT tensor one fp16 plane (the producer writes, the head reads half the
 * bytes); heads otherwise follow the format the convolutions give their input. */
sd_status sd_create_with_plan(sd_handle** out, int device, int H, int W, int max_batch, sd_encoder enc, const char* fcn_f16_layers,
                              const char* mono_f16_layers);
const char* sd_default_plan(sd_net net);      /* (monodepth: the ResNet-50 plan; the vgg encoder's default plan is empty) */
/* layers_out (nullable): the 2-product layers of the handle's plan, comma-separated; flop_share_out (nullable): their share of
 * the network's algorithmic FLOPs */
sd_status sd_precision_plan(const sd_handle* h, sd_net net, char* layers_out, size_t cap, double* flop_share_out);
sd_status sd_destroy(sd_handle* h);
const char* sd_last_error(const sd_handle* h);

/* ---------------------------------------------------------------- memory + weights
 * replaces SegmentFrame.restore_model / DepthFrame.restore_model (semantic_depth.py:498-541, :627-653) */
sd_status sd_query_memory(const sd_handle* h, size_t* fcn_weight_bytes, size_t* mono_weight_bytes, size_t* workspace_bytes);
/* The arenas may hold anything when they are bound (fresh hipMalloc memory, the remains of another handle, NaN patterns): sd_bind_memory clears the
 * few regions the library reads before it writes them (a zero page, the clamp counters) and uploads the gather tables; every other byte a kernel reads
 * -- padded channels, rows of a partial tile, images beyond B, the padding of a weight slot, partial sums, halos -- was written by sd_load_weight or by
 * a kernel of the same call.  Results therefore depend neither on the arenas' contents at bind time nor on the calls made before
 * (tests/test_gpu_state_independence.py binds 0xFF- and 0x7B-filled arenas). */
sd_status sd_bind_memory(sd_handle* h, void* fcn_weights_dev, void* mono_weights_dev, void* workspace_dev);
int sd_weight_count(const sd_handle* h, sd_net net);
/* name_out: >= 64 bytes; shape_out: 4 x int64 in TensorFlow layout (conv HWIO, transposed conv HWOI, bias [C]) */
sd_status sd_weight_info(const sd_handle* h, sd_net net, int index, char* name_out, int64_t* shape_out, int* rank_out);
/* data_host: float32, TensorFlow layout; re-laid-out for the kernels and copied into the bound arena (synchronous) */
sd_status sd_load_weight(sd_handle* h, sd_net net, const char* name, const float* data_host, const int64_t* shape, int rank);

/* ---------------------------------------------------------------- the three operators + fused tail */
/* SegmentFrame.segment_frame, semantic_depth.py:544-571 (seq:459-485), for B frames at once.
 * frames: u8 [B,H,W,3].  Outputs (each nullable): logits f32 [B,H,W,3] ('logits:0', fcn8s/fcn.py:241),
 * road/fence u8 [B,H,W] = softmax > 0.5 (:555-556,:563-564), argmax u8 [B,H,W] (fcn8s/fcn.py:218-224). */
sd_status sd_fcn8s_forward(sd_handle* h, const uint8_t* frames, int B, float* logits, uint8_t* road_mask,
                           uint8_t* fence_mask, uint8_t* argmax, void* stream);

/* DepthFrame.compute_disparity, semantic_depth.py:667-678 (seq:568-579), for B frames: /255, (frame, fliplr(frame))
 * pair through monodepth, disp_left_est[0], post_processing (:656-664).  disp_pp: f32 [B,H,W] in fraction of
 * image width.  disp_raw (nullable): f32 [B,2,H,W] = the net's channel-0 output for frame and flipped frame.
 * disp_pp may be NULL when the post-processing is left to sd_postprocess_fuse_backproject (needs B <= the handle's pass size of
 * 32 frames, or disp_raw). */
sd_status sd_monodepth_forward(sd_handle* h, const uint8_t* frames, int B, float* disp_pp, float* disp_raw, void* stream);

/* Input stage, semantic_depth.py:111 / seq:128: cv2.resize(frame, (dst_w, dst_h), interpolation=cv2.INTER_CUBIC) for B
 * uint8 HWC frames already in device memory (OpenCV's scalar fixed-point path: A = -0.75, weights cvRound(w*2048), borders
 * replicated, (sum + 2^21) >> 22).  dst_h, dst_w at most 16384 (down- or up-scaling: semantic_depth.py:341 resizes the overlay back to
 * the original frame size the same way); equal sizes copy. */
sd_status sd_resize_cubic_u8(sd_handle* h, const uint8_t* src, int B, int src_h, int src_w, int channels, uint8_t* dst, int dst_h,
                             int dst_w, void* stream);

/* Output stage of the sequence tool, semantic_depth_cityscapes_sequence.py:303-336 (overlay of :463-485): the per-frame result image
 * for B frames in device memory, in one launch with no host synchronisation.  frames u8 [B,src_h,src_w,3] (the network-size BGR input),
 * road_mask / fence_mask u8 [B,src_h,src_w] (sd_fcn8s_forward; non-zero = set), records [B] (sd_road_width) -> dst u8 [B,dst_h,dst_w,3]:
 * PIL's Image.paste of road_color then fence_color (HOST pointers, 3 bytes each in the frame's channel order) with alpha on the masked
 * pixels (t = d*(255-a) + c*a + 128, ((t >> 8) + t) >> 8), cv2.resize INTER_CUBIC of that overlay to (dst_w, dst_h) with exactly the
 * integers of sd_resize_cubic_u8 (up-, down-scaling and equal sizes), then cv2.rectangle((0,0), (dst_w, int(0.25*dst_h)), (156,157,159), -1)
 * on the frames whose record has found != 0.  The sequence tool pastes (128,64,128) and (190,153,153) with alpha 64; semantic_depth.py:565
 * uses (160,10,10) for the fence.  dst_h, dst_w at most 16384. */
sd_status sd_compose_result_frames(sd_handle* h, const uint8_t* frames, const uint8_t* road_mask, const uint8_t* fence_mask,
                                   const sd_rw_result* records, int B, int src_h, int src_w, const uint8_t* road_color,
                                   const uint8_t* fence_color, int alpha, uint8_t* dst, int dst_h, int dst_w, void* stream);

/* HOST helper of the frame reader that replaces cv2.imread (semantic_depth.py:105; seq:123): reconstructs the scanlines of an
 * inflated 8-bit non-interlaced PNG (filter byte + width*channels bytes per row; channels 1 gray, 2 gray+alpha, 3 RGB, 4 RGBA)
 * and writes OpenCV's IMREAD_COLOR layout, u8 [height,width,3] BGR (alpha dropped, gray replicated).  Both pointers are HOST
 * memory; no handle, no GPU (semantic_depth_amd/frame_io.py inflates with zlib and calls this from a thread pool). */
sd_status sd_png_unfilter_bgr(const uint8_t* filtered_host, int height, int width, int channels, uint8_t* bgr_out_host);

/* HOST: a whole PNG file (8-bit, non-interlaced; gray, gray+alpha, RGB, RGBA, palette) -> cv2.imread(path) = u8 [height,width,3] BGR:
 * chunk walk, zlib inflate, scanline reconstruction, channel shuffle, palette expansion in one native call (no interpreter lock held).
 * bgr_out_host NULL: only *height_out / *width_out are written (size query).  SD_ERR_INVALID: not such a PNG / corrupt / buffer too small. */
sd_status sd_png_decode_bgr(const uint8_t* file_host, size_t len, uint8_t* bgr_out_host, size_t out_capacity, int* height_out, int* width_out);
/* HOST: a baseline / extended-sequential / progressive Huffman JPEG (SOF0 / SOF1 / SOF2, 8-bit; gray or YCbCr with 4:4:4, 4:2:2 or 4:2:0 chroma; restart intervals) ->
 * cv2.imread(path): libjpeg's default decode path restated (jidctint "ISLOW" inverse DCT, "fancy" triangle chroma upsampling, jdcolor's
 * fixed-point YCbCr -> RGB) followed by the EXIF orientation OpenCV's imread applies; u8 [height,width,3] BGR.  The reference's own example
 * frames are JPEGs (assets/images/test_munich/test_3.jpg, semantic_depth.py:105).  Same calling convention as sd_png_decode_bgr;
 * *height_out / *width_out are the dimensions AFTER the orientation.  Arithmetic-coded / lossless / 12-bit / CMYK files, Huffman tables that
 * are not a prefix code and files with more than one frame header: SD_ERR_INVALID. */
sd_status sd_jpeg_decode_bgr(const uint8_t* file_host, size_t len, uint8_t* bgr_out_host, size_t out_capacity, int* height_out, int* width_out);
/* HOST: either of the two, by file signature */
sd_status sd_image_decode_bgr(const uint8_t* file_host, size_t len, uint8_t* bgr_out_host, size_t out_capacity, int* height_out, int* width_out);
/* HOST: the batch reader behind frame_io.FrameFeeder (the loop over sorted(glob(...)) of seq:689-701, `cv2.imread` at seq:123): reads and
 * decodes n PNG / JPEG files of height x width on `threads` native threads (<= 0: one per host CPU) into out_host + i * frame_stride (e.g. a
 * pinned staging buffer).  status_out (nullable, int[n]): per-file sd_status (SD_ERR_NOTFOUND: unreadable file; SD_ERR_INVALID: not a
 * PNG of that shape).  Returns SD_OK when every file decoded. */
sd_status sd_decode_files_bgr(const char* const* paths, int n, int height, int width, uint8_t* out_host, size_t frame_stride, int threads,
                              int* status_out);
/* ---- JPEG frames, split route: entropy decoding on the host, everything behind it on the GPU ----
 * What the reconstruction of one JPEG frame needs besides its quantised coefficients, and nothing else.  height / width are the STORED
 * size (before the EXIF orientation); orientation is 1..8; adobe_transform is the APP14 flag (-1: no Adobe marker, 0: the components are
 * R, G, B).  Component 0 is sampled hmax x vmax, components 1 and 2 are sampled 1 x 1 (hmax x vmax is 1x1, 2x1 or 2x2; 1x1 for ncomp 1).
 * blocks_w / blocks_h: 8x8 blocks per row / column of the component's padded plane.  coef_offset: element (int16) offset of the
 * component's first block in the frame's coefficient buffer -- the components follow each other without gaps, component 0 at 0.
 * qt: the component's quantisation table in natural (row-major) order. */
typedef struct {
    int32_t height, width;
    int32_t ncomp, hmax, vmax;
    int32_t orientation, adobe_transform;
    int32_t reserved;                 /* 0 */
    int32_t blocks_w[3], blocks_h[3];
    int64_t coef_offset[3];
    uint16_t qt[3][64];
} sd_jpeg_frame_desc;
/* HOST: the front half of sd_jpeg_decode_bgr.  Huffman-decodes the file and writes the QUANTISED coefficients of every 8x8 block of the
 * padded component planes to coef_out_host: natural order inside a block, blocks row-major, components one after the other
 * (desc_out->coef_offset).  Baseline, extended-sequential and progressive files alike; no sample plane is allocated.
 * coef_out_host NULL: parses up to the first SOS and fills only *desc_out (its qt entries are final only after a full call); the full
 * call needs 2 * (coef_offset[ncomp-1] + 64 * blocks_w[ncomp-1] * blocks_h[ncomp-1]) bytes.  capacity_bytes below that: SD_ERR_INVALID
 * before anything is allocated or written.  Accepts exactly the files sd_jpeg_decode_bgr accepts, with the same status otherwise. */
sd_status sd_jpeg_decode_coefficients(const uint8_t* file_host, size_t len, int16_t* coef_out_host, size_t capacity_bytes,
                                      sd_jpeg_frame_desc* desc_out);
/* HOST: the back half of sd_jpeg_decode_bgr driven from a coefficient buffer (dequantise, ISLOW inverse DCT, fancy upsampling, colour,
 * orientation; the code the one-call decoder runs): sd_jpeg_reconstruct_bgr_host after sd_jpeg_decode_coefficients writes the bytes
 * of sd_jpeg_decode_bgr.  It is the CPU statement of sd_jpeg_reconstruct_bgr.  u8 [height,width,3] BGR AFTER the orientation;
 * SD_ERR_INVALID for a descriptor that is not self-consistent or out_capacity < height * width * 3. */
sd_status sd_jpeg_reconstruct_bgr_host(const int16_t* coef_host, const sd_jpeg_frame_desc* desc, uint8_t* bgr_out_host, size_t out_capacity);
/* HOST: the batch reader beside sd_decode_files_bgr for the split route: file i -> coefficients at coef_out_host + i * frame_stride_bytes
 * (e.g. a pinned staging buffer) and descs_out[i], on `threads` native threads (<= 0: one per host CPU).  height x width is the size
 * AFTER the orientation every frame must have.  status_out (nullable, int[n]): SD_ERR_NOTFOUND unreadable file; SD_ERR_FORMAT a readable
 * file that is not a JPEG (nothing written for it: send it down the BGR route); SD_ERR_INVALID a JPEG that is refused, has another
 * size or needs more than frame_stride_bytes.  Returns SD_OK when every status is SD_OK or SD_ERR_FORMAT, else SD_ERR_INVALID. */
sd_status sd_decode_files_jpeg_coef(const char* const* paths, int n, int height, int width, int16_t* coef_out_host, size_t frame_stride_bytes,
                                    sd_jpeg_frame_desc* descs_out, int threads, int* status_out);
/* bytes of device workspace sd_jpeg_reconstruct_bgr needs for these B frames (their padded u8 component planes) */
sd_status sd_jpeg_reconstruct_workspace(const sd_jpeg_frame_desc* descs_host, int B, size_t* bytes_out);
/* DEVICE: B frames' coefficients (frame b at coef_dev + b * frame_stride_bytes, laid out as sd_jpeg_decode_coefficients writes them) ->
 * u8 [height,width,3] BGR after the orientation at bgr_dev + b * bgr_frame_stride, the integers of sd_jpeg_decode_bgr for every stream it
 * accepts.  Two kernels per group of 8 frames (dequantise + inverse DCT into the padded planes of the workspace; upsample + colour +
 * orientation); the descriptors travel as kernel arguments, so descs_host may be reused when the call returns.  Enqueued on `stream`, no
 * synchronisation; the handle need not be bound.  SD_ERR_INVALID: a descriptor that is not self-consistent, coefficients beyond
 * frame_stride_bytes, a frame beyond bgr_frame_stride, workspace_bytes below sd_jpeg_reconstruct_workspace -- nothing is launched. */
sd_status sd_jpeg_reconstruct_bgr(sd_handle* h, const int16_t* coef_dev, size_t frame_stride_bytes, const sd_jpeg_frame_desc* descs_host, int B,
                                  uint8_t* bgr_dev, size_t bgr_frame_stride, void* workspace_dev, size_t workspace_bytes, void* stream);
/* ---- JPEG frames, entropy route: the host only finds the restart markers, the GPU decodes the Huffman code, one restart interval per lane ----
 * The Huffman recurrence is serial only inside a restart interval: at every RSTn marker the bit stream is byte-aligned and the DC
 * predictors are reset, so the intervals of a sequential scan are independent jobs once their byte ranges are known.  A file is ELIGIBLE
 * when all of this holds (anything else goes through sd_jpeg_decode_coefficients, whose marker hunting is not restated anywhere):
 *   - SOF0 or SOF1, 8-bit, and the header parse of sd_jpeg_decode_bgr accepts it (the scan's tables are defined before the scan);
 *   - exactly one SOS, covering all components (1 or 3) interleaved, in the frame header's order;
 *   - DRI > 0;
 *   - walking the scan data from its start, every 0xFF is followed by 0x00, by the expected RSTk (k counting 0..7 cyclically), or -- after
 *     exactly ceil(mcus / DRI) intervals -- by EOI as the last two bytes of the file.
 * Progressive, multi-scan, non-interleaved, DRI-less and truncated files, fill bytes and stray markers are ineligible.
 *
 * sd_jpeg_huff_table: one Huffman table in the decodable form of the host decoder (T.81 F.2.2.3 plus a 9-bit look-ahead): look[i] =
 * (length << 8) | symbol for the code that prefixes the 9 bits i, 0 when it is longer than 9 bits; mincode / maxcode / valptr per code
 * length 1..16 (maxcode -1: no code of that length), vals the symbols in code order.
 * sd_jpeg_entropy_frame: the scan of one file.  eligible 0: nothing else is promised.  mcus_x / mcus_y: MCUs per row / column;
 * restart_interval: DRI, MCUs per interval; n_intervals = ceil(mcus_x * mcus_y / DRI); per component the sampling factors and the
 * table ids Td / Ta (the frame's table array holds DC table Td in slot Td and AC table Ta in slot 4 + Ta; slots the scan does not name
 * are zero); scan_begin / scan_end: the file offsets of the first scan byte and of the 0xFF of EOI.
 * sd_jpeg_interval: the bytes [begin, end) of one restart interval as offsets FROM scan_begin; end is the 0xFF of the closing marker. */
#define SD_JPEG_ENTROPY_TABLES 8
typedef struct {
    uint16_t look[512];
    int32_t mincode[17], maxcode[18], valptr[17];
    uint8_t vals[256];
} sd_jpeg_huff_table;
typedef struct {
    int32_t eligible;
    int32_t ncomp;
    int32_t mcus_x, mcus_y;
    int32_t restart_interval;
    int32_t n_intervals;
    int32_t comp_h[3], comp_v[3], comp_dc[3], comp_ac[3];
    uint32_t scan_begin, scan_end;
} sd_jpeg_entropy_frame;
typedef struct {
    uint32_t begin, end;
} sd_jpeg_interval;
/* HOST: the plan of one file: a header parse and a byte scan for the markers, no bit work.  Writes *desc_out (for an eligible file every
 * byte of what sd_jpeg_decode_coefficients writes), *frame_out, tables_out[SD_JPEG_ENTROPY_TABLES] (built and validated as the host
 * decoder builds its own) and the first frame_out->n_intervals entries of intervals_out.  SD_OK with eligible 0 for a JPEG that is not
 * eligible; SD_ERR_FORMAT for a file that does not begin with SOI; SD_ERR_INVALID for NULL arguments, a file of 2 GiB or more, or an
 * eligible file with more than interval_cap intervals (n_intervals says how many it has).  *frame_out is cleared first: eligible is 0
 * on every return but SD_OK for an eligible file. */
sd_status sd_jpeg_entropy_plan(const uint8_t* file_host, size_t len, sd_jpeg_frame_desc* desc_out, sd_jpeg_entropy_frame* frame_out,
                               sd_jpeg_huff_table* tables_out, sd_jpeg_interval* intervals_out, size_t interval_cap);
/* HOST: the batch form beside sd_decode_files_jpeg_coef: reads n files on `threads` native threads (<= 0: one per host CPU), plans each
 * and copies the scan bytes [scan_begin, scan_end) of an eligible file to bytes_out_host + i * byte_stride (e.g. a pinned staging
 * buffer), its records to descs_out[i], frames_out[i], tables_out + i * SD_JPEG_ENTROPY_TABLES and intervals_out + i * interval_stride.
 * height x width is the size AFTER the orientation every frame must have.  status_out (nullable, int[n]): SD_ERR_NOTFOUND unreadable
 * file; SD_ERR_FORMAT a readable file that is not a JPEG; SD_ERR_INVALID an eligible JPEG of another size, with more scan bytes than
 * byte_stride or more intervals than interval_stride (eligible is 0 then); SD_OK otherwise, eligible or not.  Returns SD_OK when every
 * status is SD_OK or SD_ERR_FORMAT, else SD_ERR_INVALID. */
sd_status sd_plan_files_jpeg_entropy(const char* const* paths, int n, int height, int width, uint8_t* bytes_out_host, size_t byte_stride,
                                     sd_jpeg_frame_desc* descs_out, sd_jpeg_entropy_frame* frames_out, sd_jpeg_huff_table* tables_out,
                                     sd_jpeg_interval* intervals_out, size_t interval_stride, int threads, int* status_out);
/* HOST: the CPU statement of sd_jpeg_entropy_decode: the same checks, then a plain loop over the intervals calling the same function
 * (semantic_depth_amd/csrc/jpeg_entropy.hpp).  Frame b's scan bytes are at bytes_host + b * byte_stride.  For every eligible frame it
 * clears the frame's coefficients (the descriptor's element count, nothing behind them) at coef_out_host + b * coef_stride_bytes and
 * writes what sd_jpeg_decode_coefficients writes; status_out[b] = 0, or the refusal of the first refused interval (1 undecodable symbol,
 * 2 DC category above 15, 3 DC predictor outside +-32767, 4 run past coefficient 63) -- the frame is then to be decoded by
 * sd_jpeg_decode_coefficients, which refuses it as well.  Ineligible frames: status 0, coefficients untouched. */
sd_status sd_jpeg_entropy_decode_host(const uint8_t* bytes_host, size_t byte_stride, const sd_jpeg_frame_desc* descs, const sd_jpeg_entropy_frame* frames,
                                      const sd_jpeg_interval* intervals, size_t interval_stride, const sd_jpeg_huff_table* tables, int B,
                                      int16_t* coef_out_host, size_t coef_stride_bytes, int32_t* status_out);
/* bytes of device workspace sd_jpeg_entropy_decode needs (the uploaded records, tables and interval ranges) */
sd_status sd_jpeg_entropy_workspace(int B, size_t interval_stride, size_t* bytes_out);
/* DEVICE: B frames' scan bytes (frame b at bytes_dev + b * byte_stride) -> their quantised coefficients at coef_dev + b *
 * coef_stride_bytes as sd_jpeg_entropy_decode_host writes them, and status_dev[b]: 0 exactly where that function writes 0, otherwise
 * the refusal code of ONE of the frame's refused intervals (the lanes store without ordering; only non-zero is promised, not the first
 * interval's code); ineligible frames are skipped.  The records,
 * tables and ranges are HOST arrays: they are checked, then uploaded into workspace_dev by asynchronous copies on `stream` (pinned
 * arrays must stay unchanged until the stream has passed the call).  One kernel clears the eligible frames' coefficients, one decodes:
 * a lane per restart interval, 64 intervals of one frame per workgroup, the frame's named tables staged in LDS.  Enqueued on `stream`,
 * no synchronisation; the handle need not be bound.  SD_ERR_INVALID, and nothing is launched or copied: bytes_dev, byte_stride, coef_dev,
 * coef_stride_bytes or workspace_dev not multiples of 16; a record that disagrees with its descriptor; coefficients beyond
 * coef_stride_bytes; an interval range outside byte_stride; more intervals than interval_stride; a table not in decodable form;
 * workspace_bytes below sd_jpeg_entropy_workspace. */
sd_status sd_jpeg_entropy_decode(sd_handle* h, const uint8_t* bytes_dev, size_t byte_stride, const sd_jpeg_frame_desc* descs_host,
                                 const sd_jpeg_entropy_frame* frames_host, const sd_jpeg_interval* intervals_host, size_t interval_stride,
                                 const sd_jpeg_huff_table* tables_host, int B, int16_t* coef_dev, size_t coef_stride_bytes,
                                 int32_t* status_dev, void* workspace_dev, size_t workspace_bytes, void* stream);
/* ---- JPEG frames, sync route: the GPU decodes the Huffman code in short pieces that find the decoder's state by themselves ----
 * A sequential Huffman decoder at a bit position is in the state (p, u, k): bit position, data unit inside the MCU, zigzag index (k 0: a
 * DC symbol comes next).  Two decoders that meet in one state agree from there on, and a decoder started at a byte boundary in the
 * assumed state (u 0, k 0) nearly always falls into step with the true one within a few hundred bytes.  So an interval is cut into
 * PIECES of subseq_bytes (a power of two, 32..1024): a speculative pass finds every piece's end state, a write pass decodes every piece
 * from its predecessor's recorded end state and VERIFIES that it ends in its own; with the interval's true start that chain of
 * equalities proves the sequential decode.  A file without DRI is one interval of all its MCUs, so this route reaches it.
 * ELIGIBLE: the rule of sd_jpeg_entropy_plan with DRI = 0 admitted.
 * The plan writes the CLEAN stream: the scan bytes with FF 00 resolved to FF and the RSTk markers dropped, the intervals one behind the
 * other, so a bit position is a plain offset.
 * sd_jpeg_sync_frame: as sd_jpeg_entropy_frame, with restart_interval the MCUs of one interval (DRI, or mcus_x * mcus_y without DRI: a
 * field of 32 bits), clean_bytes the length of the clean stream, subseq_bytes the piece length the plan counted with and n_pieces the
 * pieces of the frame.  sd_jpeg_sync_interval: the bytes [begin, end) of the interval in the clean stream and the index of its first
 * piece; an interval of n bytes has max(1, ceil(n / subseq_bytes)) pieces, piece j covering [begin + j * subseq_bytes, ...) up to end. */
typedef struct {
    int32_t eligible;
    int32_t ncomp;
    int32_t mcus_x, mcus_y;
    int32_t restart_interval;
    int32_t n_intervals;
    int32_t comp_h[3], comp_v[3], comp_dc[3], comp_ac[3];
    uint32_t scan_begin, scan_end;
    uint32_t clean_bytes, subseq_bytes, n_pieces;
    uint32_t reserved;                /* 0 */
} sd_jpeg_sync_frame;
typedef struct {
    uint32_t begin, end;
    uint32_t first_piece;
    uint32_t reserved;                /* 0 */
} sd_jpeg_sync_interval;
/* per-frame status words of the sync route beyond the four refusals of the entropy route (1..4) */
#define SD_JPEG_SYNC_NOT_SYNCHRONISED 5   /* a piece did not end in its recorded state: the chain of equalities is broken */
#define SD_JPEG_SYNC_BITS_RAN_OUT 6       /* the interval's pieces hold fewer data units than the interval has */
#define SD_JPEG_SYNC_GROUP 256            /* pieces per workgroup of the speculative pass */
/* HOST: the plan of one file for the sync route: sd_jpeg_entropy_plan's header parse and byte walk, with DRI = 0 admitted.  Writes
 * *desc_out, *frame_out, tables_out[SD_JPEG_ENTROPY_TABLES], the first n_intervals entries of intervals_out and, when clean_out is not
 * NULL, the clean stream (frame_out->clean_bytes bytes; never more than scan_end - scan_begin; the walk of a file that turns out not to be
 * eligible may have written into clean_out as well, never beyond clean_capacity).  SD_OK with eligible 0 for a JPEG that is
 * not eligible; SD_ERR_FORMAT for a file without SOI; SD_ERR_INVALID for NULL arguments, subseq_bytes that is no power of two in
 * 32..1024, a file of 256 MiB or more, or an eligible file with more than interval_cap intervals or more than clean_capacity clean
 * bytes (n_intervals / clean_bytes say what it needs; eligible stays 0). */
sd_status sd_jpeg_sync_plan(const uint8_t* file_host, size_t len, int subseq_bytes, sd_jpeg_frame_desc* desc_out, sd_jpeg_sync_frame* frame_out,
                            sd_jpeg_huff_table* tables_out, sd_jpeg_sync_interval* intervals_out, size_t interval_cap, uint8_t* clean_out,
                            size_t clean_capacity);
/* HOST: the batch form, as sd_plan_files_jpeg_entropy: file i's clean stream goes to bytes_out_host + i * byte_stride, zero-filled up
 * to the next multiple of 16. */
sd_status sd_plan_files_jpeg_sync(const char* const* paths, int n, int height, int width, int subseq_bytes, uint8_t* bytes_out_host,
                                  size_t byte_stride, sd_jpeg_frame_desc* descs_out, sd_jpeg_sync_frame* frames_out, sd_jpeg_huff_table* tables_out,
                                  sd_jpeg_sync_interval* intervals_out, size_t interval_stride, int threads, int* status_out);
/* HOST: the CPU statement of sd_jpeg_sync_decode: the same checks, then the same passes (semantic_depth_amd/csrc/jpeg_sync.hpp) with the
 * lanes of the kernels run in a loop, in the kernels' schedule, so it predicts which frames the device flags.  For every eligible frame
 * it clears the frame's coefficients and writes what sd_jpeg_decode_coefficients writes; status_out[b] = 0, or the first code met (1..4
 * as sd_jpeg_entropy_decode_host, 5, 6 above).  Status 0 implies the sequential decode; a flagged frame is to be decoded by
 * sd_jpeg_decode_coefficients, which decides it.  Ineligible frames: status 0, coefficients untouched. */
sd_status sd_jpeg_sync_decode_host(const uint8_t* bytes_host, size_t byte_stride, const sd_jpeg_frame_desc* descs, const sd_jpeg_sync_frame* frames,
                                   const sd_jpeg_sync_interval* intervals, size_t interval_stride, const sd_jpeg_huff_table* tables, int B,
                                   int subseq_bytes, int16_t* coef_out_host, size_t coef_stride_bytes, int32_t* status_out);
/* bytes of device workspace sd_jpeg_sync_decode needs for B frames of at most max_pieces pieces each */
sd_status sd_jpeg_sync_workspace(int B, size_t interval_stride, size_t max_pieces, size_t* bytes_out);
/* DEVICE: B frames' clean streams (frame b at bytes_dev + b * byte_stride) -> coefficients and status words as
 * sd_jpeg_sync_decode_host writes them: status_dev[b] is 0 exactly where that function writes 0, otherwise one of the frame's codes.
 * The records, tables and ranges are HOST arrays: checked, then uploaded into workspace_dev by asynchronous copies on `stream`.  Six
 * kernels: clear; the speculative pass (a lane per piece, 256 pieces per workgroup, bounded rounds); the pass across workgroups (a lane
 * per workgroup, started from the previous workgroup's recorded end); the placement scan of the unit counts; the write pass with the
 * verification; the segmented scan of the DC differences.  No kernel waits for another workgroup, none uses atomics.  Enqueued on
 * `stream`, no synchronisation; the handle need not be bound.  SD_ERR_INVALID, and nothing is launched or copied: pointers or strides
 * that are not multiples of 16; subseq_bytes that is no power of two in 32..1024 or not the plan's; a record that disagrees with its
 * descriptor; coefficients beyond coef_stride_bytes; a range outside clean_bytes or byte_stride; piece indices that do not follow from
 * the ranges; more intervals than interval_stride; a table not in decodable form; workspace_bytes below sd_jpeg_sync_workspace of the
 * largest n_pieces. */
sd_status sd_jpeg_sync_decode(sd_handle* h, const uint8_t* bytes_dev, size_t byte_stride, const sd_jpeg_frame_desc* descs_host,
                              const sd_jpeg_sync_frame* frames_host, const sd_jpeg_sync_interval* intervals_host, size_t interval_stride,
                              const sd_jpeg_huff_table* tables_host, int B, int subseq_bytes, int16_t* coef_dev, size_t coef_stride_bytes,
                              int32_t* status_dev, void* workspace_dev, size_t workspace_bytes, void* stream);
/* ---- PNG frames, split route: the host only inflates, the GPU reconstructs the scanlines ----
 * What the reconstruction of one PNG frame needs besides its filtered scanlines.  channels is the bytes per pixel of the 8-bit colour type
 * (0 -> 1, 2 -> 3, 3 -> 1, 4 -> 2, 6 -> 4); palette holds the PLTE entries as the file has them (R, G, B), zero past palette_entries;
 * palette_entries is 0 for every colour type but 3. */
typedef struct {
    int32_t height, width;
    int32_t channels, color_type;
    int32_t palette_entries;
    int32_t reserved;                 /* 0 */
    uint8_t palette[256][3];
} sd_png_frame_desc;
/* HOST: the front half of sd_png_decode_bgr.  Walks the chunks and inflates the IDAT stream straight into rows_out_host: height rows of one
 * filter byte plus width * channels filtered bytes, exactly height * (1 + width * channels) bytes.  Checks that the stream has exactly
 * that length, that every row's filter byte is <= 4 and that a colour type 3 file has a PLTE chunk.  rows_out_host NULL: fills only
 * *desc_out from the header (palette_entries and palette are final only after a full call).  capacity below the byte count:
 * SD_ERR_INVALID before anything is written.  sd_png_unfilter_bgr on the rows (plus the palette lookup) gives the bytes of
 * sd_png_decode_bgr.  Accepts and refuses exactly the files sd_png_decode_bgr does, with one exception: a palette index beyond the
 * palette shows only after the reconstruction (sd_png_reconstruct_bgr flags it). */
sd_status sd_png_inflate_rows(const uint8_t* file_host, size_t len, uint8_t* rows_out_host, size_t capacity, sd_png_frame_desc* desc_out);
/* HOST: the batch reader beside sd_decode_files_bgr for the split PNG route: file i -> its filtered rows at rows_out_host + i * frame_stride
 * (e.g. a pinned staging buffer) and descs_out[i], on `threads` native threads (<= 0: one per host CPU).  status_out (nullable, int[n]):
 * SD_ERR_NOTFOUND unreadable file; SD_ERR_FORMAT a readable file without the PNG signature (nothing written for it: send it down the
 * other routes); SD_ERR_INVALID a PNG that is refused, has another size or needs more than frame_stride.  Returns SD_OK when every
 * status is SD_OK or SD_ERR_FORMAT, else SD_ERR_INVALID. */
sd_status sd_inflate_files_png(const char* const* paths, int n, int height, int width, uint8_t* rows_out_host, size_t frame_stride,
                               sd_png_frame_desc* descs_out, int threads, int* status_out);
/* bytes of device workspace sd_png_reconstruct_bgr needs for B frames (the uploaded descriptors) */
sd_status sd_png_reconstruct_workspace(int B, size_t* bytes_out);
/* DEVICE: B frames' filtered rows (frame b at rows_dev + b * frame_stride, laid out as sd_png_inflate_rows writes them) -> u8
 * [height,width,3] BGR at bgr_out_dev + b * out_stride, the bytes of sd_png_decode_bgr, and status_dev[b] (int32 [B], every word written
 * by the call): 0, or non-zero for a colour type 3 frame with an index beyond its palette (such a pixel takes palette entry 0).  The
 * frames share height x width (1..16384 each); channels, colour type and palette are per frame.  descs_host is a HOST array: checked, then
 * uploaded into workspace_dev by ONE asynchronous copy on `stream` (a pinned array must stay unchanged until the stream has passed the
 * call).  One kernel, one workgroup per frame: a lane per row of a 64-row band, the bands of a frame pipelined across the workgroup's
 * waves (semantic_depth_amd/csrc/png_in_gpu.hip).  Enqueued on `stream`, no synchronisation; the handle need not be bound.
 * SD_ERR_INVALID, and nothing is launched or copied: an extent outside 1..16384; rows_dev, frame_stride or workspace_dev not multiples
 * of 16; frame_stride below a frame's height * (1 + width * channels) rounded up to 16; out_stride below height * width * 3; a
 * descriptor of another size, with channels that are not its colour type's or more than 256 palette entries; workspace_bytes below
 * sd_png_reconstruct_workspace.  A filter byte above 4 is the host's to refuse (sd_png_inflate_rows does); the kernel reads it as 4. */
sd_status sd_png_reconstruct_bgr(sd_handle* h, const uint8_t* rows_dev, size_t frame_stride, const sd_png_frame_desc* descs_host, int B,
                                 int height, int width, uint8_t* bgr_out_dev, size_t out_stride, int32_t* status_dev, void* workspace_dev,
                                 size_t workspace_bytes, void* stream);
/* HOST: the writer behind the sequence tool's cv2.imwrite('<dir>/<name>.png', frame) (seq:336): encodes n u8 [height,width,3] BGR frames at
 * frames_host + i * frame_stride as 8-bit RGB PNGs (filter type 0 rows, one zlib stream at `level` 0..9) and writes them to paths[i], on
 * `threads` native threads (<= 0: one per host CPU).  Pixel-exact, not byte-identical to OpenCV's file: sd_png_decode_bgr reads each
 * file back as the input frame.  status_out (nullable, int[n]): per-file sd_status (SD_ERR_NOTFOUND: the file could not be written).
 * Returns SD_OK when every file was written. */
sd_status sd_png_encode_bgr_files(const char* const* paths, int n, int height, int width, const uint8_t* frames_host, size_t frame_stride,
                                  int level, int threads, int* status_out);

/* ---- result images, device route: the GPU makes each frame's complete zlib stream, the host wraps it in PNG chunks ----
 * The stream format, fixed here (C = 32768):
 *   filtered bytes   filtered row y is the byte 4 followed by the Paeth residuals (PNG filter type 4, bpp 3, pixels outside the image
 *                    count as 0) of the row's RGB bytes -- the BGR -> RGB swap is part of the read.  The filtered frame is the flat
 *                    sequence of height * (1 + 3 * width) bytes.
 *   chunks           the sequence is cut every C bytes, wherever that falls (inside a row, inside a pixel); the last chunk is shorter.
 *                    Chunks are coded independently: no token refers to a byte of another chunk, the first byte of a chunk is a literal.
 *   tokens           inside a chunk a maximal run of n >= 4 equal bytes is one literal followed by distance-1 matches over the other
 *                    n - 1 bytes: matches of 258 while more than 258 bytes remain or exactly 258 do, then one match of 3..257, or 1..2
 *                    literals when that few bytes remain.  Every other byte is a literal.
 *   a chunk          one non-final dynamic-Huffman block (BTYPE 10).  Literal/length code: Huffman lengths of the chunk's token histogram
 *                    (end-of-block counted once), limited to 15 bits; HLIT covers up to the last used symbol.  Two distance codes, 0 and
 *                    1, of length 1 each (a complete tree; a match sends the one bit of code 0).  The code lengths travel as plain
 *                    values 0..15 (no repeat codes 16/17/18) under a code-length code limited to 7 bits, all 19 of whose lengths are
 *                    sent.  Behind the end-of-block symbol an empty non-final stored block pads to a byte boundary: 000, zero bits,
 *                    00 00 FF FF.  When the dynamic block (header through end-of-block, in whole bytes) is not smaller than len + 5, the
 *                    chunk is instead one stored block 00 LEN NLEN bytes followed by the same empty stored block (00 00 00 FF FF).
 *                    The code construction (two-queue Huffman over the symbols sorted by (count, symbol), leaf before internal node at
 *                    equal weight; depths clamped to the limit and the Kraft sum repaired on the per-length counts; longest lengths to
 *                    the rarest symbols; canonical codes) is semantic_depth_amd/csrc/png_deflate.hpp, which host and device both run.
 *   the stream       78 01, the chunks in order, 01 00 00 FF FF (the final, empty stored block), the big-endian Adler-32 of the
 *                    filtered bytes.  At most 2 + sum(len_c + 16) + 16 bytes for any frame content.
 * sd_png_encode_workspace: the device workspace sd_png_encode_bgr needs for B frames of height x width and the smallest stream_stride it
 * accepts (that bound).  SD_ERR_INVALID for B < 1 or an extent outside 1..16384. */
sd_status sd_png_encode_workspace(int B, int height, int width, size_t* workspace_bytes, size_t* stream_stride);
/* DEVICE: frames u8 [B,height,width,3] BGR (frame b at frames_dev + b * frame_stride) -> frame b's stream at streams_dev + b * stream_stride,
 * its byte count in sizes_dev[b] (u64).  Bytes of a frame's slot behind its size are not written.  Three launches (one workgroup per
 * chunk; the layout of each frame; the chunks gathered) enqueued on `stream`, no synchronisation; the handle need not be bound.
 * SD_ERR_INVALID, nothing launched: an extent outside 1..16384, B < 1, frame_stride < height * width * 3, stream_stride below the bound,
 * workspace_bytes below sd_png_encode_workspace, a workspace that is not 16-byte aligned. */
sd_status sd_png_encode_bgr(sd_handle* h, const uint8_t* frames_dev, size_t frame_stride, int B, int height, int width, uint8_t* streams_dev,
                            size_t stream_stride, uint64_t* sizes_dev, void* workspace_dev, size_t workspace_bytes, void* stream);
/* HOST: the CPU statement of sd_png_encode_bgr for one frame: the same bytes.  *size_out = bytes written to out_host; SD_ERR_INVALID for an
 * extent outside 1..16384 or a stream larger than cap (the bound of sd_png_encode_workspace always suffices). */
sd_status sd_png_encode_zlib_host(const uint8_t* frame_host, int height, int width, uint8_t* out_host, size_t cap, size_t* size_out);
/* HOST: n finished streams (stream i at streams_host + i * stream_stride, sizes_host[i] bytes) -> the 8-bit RGB PNG files paths[i]:
 * signature, IHDR, the stream in IDAT chunks of at most 1 MiB, IEND, each with its CRC-32, on `threads` native threads (<= 0: one per host
 * CPU).  status_out and the return value as sd_png_encode_bgr_files (SD_ERR_NOTFOUND: the file could not be written); a size beyond
 * stream_stride is SD_ERR_INVALID before anything is written. */
sd_status sd_png_write_streams_files(const char* const* paths, int n, int height, int width, const uint8_t* streams_host, size_t stream_stride,
                                     const uint64_t* sizes_host, int threads, int* status_out);

/* ---- result video: every frame a complete baseline JPEG file made on the GPU, the host only concatenates them into a Motion-JPEG AVI ----
 * The file format, fixed here (the coder itself is semantic_depth_amd/csrc/jpeg_enc.hpp, integer arithmetic that host and device both run):
 *   the file         JFIF, baseline sequential (SOF0), 8 bits, three components Y Cb Cr, Y sampled 2x2 and the chroma 1x1 (4:2:0), one
 *                    interleaved scan.  Markers in order: SOI, APP0 (JFIF 1.01, density 1:1, no unit), DQT (tables 0 and 1), SOF0, DHT (DC 0,
 *                    AC 0, DC 1, AC 1), DRI, SOS, entropy-coded data, EOI.  The header is 613 bytes for every frame.
 *   colour           from the BGR bytes, 16-bit fixed point:  Y = (19595 R + 38470 G + 7471 B + 32768) >> 16,
 *                    Cb = (-11059 R - 21709 G + 32768 B + 8421375) >> 16,  Cr = (32768 R - 27439 G - 5329 B + 8421375) >> 16
 *                    (8421375 = (128 << 16) + 32767).
 *   planes           padded to a multiple of 16 by replicating the last column and the last row; the chroma planes are the 2x2 box
 *                    (a + b + c + d + 2) >> 2 of the padded planes.
 *   transform        samples - 128 through the separable integer forward DCT with 13-bit constants (rows first, 2 extra bits kept between
 *                    the passes); its outputs are the orthonormal DCT's coefficients times 8.
 *   quantisation     the ITU T.81 Annex K luminance / chrominance tables under the IJG quality rule: s = quality < 50 ? 5000 / quality :
 *                    200 - 2 quality, entry = (base s + 50) / 100 clamped to 1..255.  A coefficient c (times 8) and d = 8 entry give
 *                    (|c| + d / 2) / d with the sign of c: half away from zero.  Zigzag order.
 *   entropy coding   the four typical Huffman tables of Annex K, fixed.  DRI = the MCUs of one MCU row: every MCU row starts byte-aligned
 *                    with the DC predictors 0, ends padded with 1-bits and is followed by RSTm, m = row mod 8; the last row by EOI instead.
 *                    FF bytes of the coded data are followed by 00; runs of 16 zeros are ZRL; EOB is omitted when coefficient 63 is
 *                    non-zero.
 *   the bound        a block is at most 22 + 63 * 26 = 1660 bits (DC category <= 11: 11 + 11 bits; 63 AC symbols of category <= 10: 16 + 10
 *                    bits), counted as 208 bytes; an MCU row is at most 2 * 208 * 6 * ceil(width / 16) + 2 bytes (every byte stuffed, the
 *                    padding inside the last byte, the marker), a file at most 613 + ceil(height / 16) of those.
 * sd_jpeg_encode_workspace: the device workspace sd_jpeg_encode_bgr needs for B frames of height x width (12 bytes per MCU row) and that
 * bound, the largest stream_stride anyone needs.  SD_ERR_INVALID for B < 1 or an extent outside 1..16384. */
sd_status sd_jpeg_encode_workspace(int B, int height, int width, size_t* workspace_bytes, size_t* stream_bound);
/* DEVICE: frames u8 [B,height,width,3] BGR (frame b at frames_dev + b * frame_stride) -> frame b's file at streams_dev + b * stream_stride,
 * its byte count in sizes_dev[b] (u64), flags_dev[b] (i32) = 0.  Bytes of a frame's slot behind its size are not written.  A stream_stride
 * below the bound is legal: a frame whose file would pass it gets size 0 and flag 1 and nothing of its slot is written; the other frames
 * are unaffected.  Three launches (every MCU row coded for its size; the layout and header of each frame; every MCU row coded into place)
 * enqueued on `stream`, no synchronisation; the handle need not be bound.  SD_ERR_INVALID, nothing launched: an extent outside 1..16384,
 * B < 1, quality outside 1..100, frame_stride < height * width * 3, stream_stride < 613 (the header), workspace_bytes below
 * sd_jpeg_encode_workspace, a workspace that is not 16-byte aligned. */
sd_status sd_jpeg_encode_bgr(sd_handle* h, const uint8_t* frames_dev, size_t frame_stride, int B, int height, int width, int quality,
                             uint8_t* streams_dev, size_t stream_stride, uint64_t* sizes_dev, int32_t* flags_dev, void* workspace_dev,
                             size_t workspace_bytes, void* stream);
/* HOST: the CPU statement of sd_jpeg_encode_bgr for one frame: the same bytes, from one plain loop.  *size_out = bytes written to out_host;
 * SD_ERR_INVALID (nothing written) for a null pointer, an extent outside 1..16384, a quality outside 1..100 or a file larger than cap (the
 * bound of sd_jpeg_encode_workspace always suffices). */
sd_status sd_jpeg_encode_bgr_host(const uint8_t* frame_host, int height, int width, int quality, uint8_t* out_host, size_t cap, size_t* size_out);

/* HOST helper of the PLY writer that replaces semantic_depth_lib/point_cloud_2_ply.py:70 (numpy.savetxt(fh, rows, "%f %f %f %d %d %d")):
 * n vertex rows "x y z r g b\n" -- coordinates as "%f" % float(v) prints them (fixed, six decimals, correctly rounded; nan / inf /
 * -inf), colours as integers -- into out[0 .. cap).  xyz f64 [n,3], rgb int64 [n,3], HOST memory; threads <= 0: one per core, at most
 * 16.  Returns the number of bytes written, or SD_ERR_INVALID (bad argument, or cap too small: cap / n bytes must hold any row). */
int64_t sd_ply_format_rows(const double* xyz_host, const int64_t* rgb_host, int64_t n, char* out_host, int64_t cap, int threads);

/* ---- road PLYs, device route: the GPU writes the text of every frame's <name>_rw.ply, the host only writes the bytes to the files ----
 * The text of one frame is outputs.rw_ply_bytes(xyz as float64, rgb, left, right) byte for byte:
 *   rows      the n cloud points in order, then -- when record.found != 0 -- the 1001 points of the road-width line, in float64 without
 *             contraction: L = (double)left_pt, R = (double)right_pt, L.y += 0.01, R.y += 0.01, v = R - L; line row 0 is L, line row 1 + i
 *             is L + (i * 0.001) * v for i = 0..999 (a product, then a sum); colour 250 0 0.
 *   filter    zmin = the minimum z of all rows; a row is kept iff z > zmin (every row at the minimum goes; no row: no vertex).
 *   a row     "%f %f %f %d %d %d\n": "%f" of the double, six decimals, correctly rounded (half-even on the exact binary value), the sign
 *             printed whenever the sign bit is set; at most SD_PLY_ROW_CAP bytes.
 *   header    PointCloud2Ply.ply_header with the count of kept rows (four-space indents, four trailing spaces), at most SD_PLY_HEADER_CAP bytes.
 * The digits are semantic_depth_amd/csrc/ply_format.hpp (integer arithmetic only), which host and device both run.
 * flags      0: the frame's text was produced.  1: not formatted -- a cloud or line coordinate or an end point of a found record is not
 *            finite or has |v| >= 2^31, or n_dev[b] is outside 0..cap; the caller writes such a frame through the host route
 *            (sd_ply_format_rows).  2: the text would pass text_capacity.  A flagged frame has size 0. */
#define SD_PLY_ROW_CAP 69
#define SD_PLY_HEADER_CAP 209
#define SD_PLY_LINE_ROWS 1001
/* the device workspace sd_ply_format_rw needs for B frames of clouds of `cap` points, and the text capacity that holds any content:
 * B * (SD_PLY_HEADER_CAP + (cap + SD_PLY_LINE_ROWS) * SD_PLY_ROW_CAP).  SD_ERR_INVALID for B < 1, B > 65535 or cap < 0. */
sd_status sd_ply_format_workspace(int B, int cap, size_t* workspace_bytes, size_t* text_bound);
/* DEVICE: xyz f32 [B,cap,3], rgb u8 [B,cap,3], n i32 [B] (sd_road_width's final clouds) and records [B] -> the files PACKED back to back:
 * frame b's file is text_dev[offsets_dev[b] .. offsets_dev[b+1]), offsets_dev[0] = 0, so that offsets_dev[B] bytes cross to the host in one
 * copy.  text_capacity may be below the bound: a frame whose text would pass it gets flag 2 and size 0, and the frames behind it still
 * pack correctly.  Bytes at and behind offsets_dev[B] are never written.  The result does not depend on the workspace's contents or on the
 * order in which workgroups arrive (no floating-point atomics).  Five launches (minimum z and range test per 256-row block; per frame;
 * the kept rows' exact length per block; one workgroup that lays out blocks, frames, flags and headers; the rows) enqueued on `stream`,
 * no synchronisation; the handle need not be bound.  SD_ERR_INVALID, nothing launched: B < 1, cap < 0, a null pointer, workspace_bytes
 * below sd_ply_format_workspace, a workspace that is not 16-byte aligned, offsets_dev not 8-byte aligned. */
sd_status sd_ply_format_rw(sd_handle* h, const float* xyz_dev, const uint8_t* rgb_dev, const int32_t* n_dev, int B, int cap,
                           const sd_rw_result* records_dev, uint8_t* text_dev, size_t text_capacity, uint64_t* offsets_dev, int32_t* flags_dev,
                           void* workspace_dev, size_t workspace_bytes, void* stream);
/* HOST: the CPU statement of sd_ply_format_rw for one frame (xyz f32 [n,3], rgb u8 [n,3], one record): the same bytes into out_host[0 .. cap),
 * *size_out = their count, *flag_out = 0; or *flag_out = 1 and *size_out = 0 under the rule above.  SD_ERR_INVALID: n < 0, a null pointer,
 * or a text longer than cap (SD_PLY_HEADER_CAP + (n + SD_PLY_LINE_ROWS) * SD_PLY_ROW_CAP always suffices). */
sd_status sd_ply_format_rw_host(const float* xyz_host, const uint8_t* rgb_host, int n, const sd_rw_result* record, uint8_t* out_host, size_t cap,
                                size_t* size_out, int32_t* flag_out);

/* ---- result images, the banner text: rasterised on the GPU between sd_compose_result_frames and the PNG encoder (opt-in) ----
 * The reference draws its numbers with cv2.putText (fontFace 16 = italic | Hershey simplex; OpenCV ignores the italic bit for simplex).
 * OpenCV's glyph tables are not reproduced: the project draws a stroke font of its own (constructed by scripts/make_text_font.py from
 * straight strokes and sampled ellipse arcs; no vertex list of Hershey's or any other font) with a rule of its own, both stated once, for
 * host and device, in semantic_depth_amd/csrc/text_draw.hpp.  No pixel identity with OpenCV is claimed; no anti-aliasing.
 *   font      integer unit grid, baseline y = 0, y up, cap height 21, x-height 14, descenders to -7; every vertex of a glyph lies in
 *             [0, advance] x [-7, 21], advance <= 24; a glyph is at most SD_TEXT_MAX_SEGS straight segments.  Glyphs: space, 0-9, A-Z, a-z
 *             and . , : ; ' - + / ( ) % =; every other byte draws one box glyph.
 *   an item   text (len <= SD_TEXT_MAX_BYTES bytes), org = the baseline-left corner in pixels, scale_q8 = lround(fontScale * 256), the
 *             colour in the image's channel order, thickness.  Caps: 1 <= scale_q8 <= SD_TEXT_MAX_SCALE_Q8, 1 <= thickness <=
 *             SD_TEXT_MAX_THICKNESS, |org| <= SD_TEXT_MAX_ORG, image extents 1..16384.
 *   the rule  in 1/256 pixel: vertex (ux, uy) of the glyph at pen position p (the sum of the advances before it) is X = org_x * 256 +
 *             (p + ux) * scale_q8, Y = org_y * 256 - uy * scale_q8; pixel (px, py) has its centre at (px * 256, py * 256) and takes the
 *             item's colour iff its squared distance to some segment of the item is <= (thickness * 128)^2, decided in exact integer
 *             arithmetic (a degenerate segment is a disc).  Pixels outside the image are clipped, items are drawn in list order, and
 *             a pixel no item paints is never written.
 *   numbers   "%.2f" as Python's "{:.2f}".format(v): half-even on the exact binary value, the sign whenever the sign bit is set ("-0.00"),
 *             nan, inf, -inf; a finite |v| >= 2^31 draws inf / -inf (the _overlay.json keeps Python's string).
 *   sequence layout (outputs.overlay_items_sequence): found != 0 -- "At <depth> m depth:" at (int(0.36 w), int(0.05 h)), scale 2.2;
 *             "<-left_pt[0]>m to road's left end" at (int(0.05 w), int(0.13 h)), "<right_pt[0]>m to road's right end" at (int(0.5 w),
 *             int(0.13 h)), "Road's width: <width> m" at (int(0.35 w), int(0.22 h)), scale 2; white, thickness 2.  found == 0 -- "Cannot
 *             compute width of road at <depth> m depth:" at (int(0.28 w), int(0.035 h)), scale 2.2, green (0, 255, 0).  The origins are
 *             products in doubles, truncated.  <depth> is the caller's string, at most 23 bytes. */
#define SD_TEXT_MAX_BYTES 64
#define SD_TEXT_MAX_SEGS 32
#define SD_TEXT_MAX_ITEMS 4
#define SD_TEXT_MAX_SCALE_Q8 4096
#define SD_TEXT_MAX_THICKNESS 32
#define SD_TEXT_MAX_ORG 32768
typedef struct {
    uint8_t text[SD_TEXT_MAX_BYTES];
    int32_t len;
    int32_t org_x, org_y;
    int32_t scale_q8;
    int32_t thickness;
    uint8_t bgr[3];        /* the three bytes stored into a painted pixel, in the image's channel order */
    uint8_t reserved;      /* 0 */
} sd_text_item;
/* the device workspace sd_text_draw_rw needs for B frames; 0 for B < 1 or B > 65535 */
size_t sd_text_workspace_bytes(int B);
/* DEVICE: draws the sequence layout of records_dev[b] (B records, read on the device: no host synchronisation) into dst_dev u8
 * [B,dst_h,dst_w,3] IN PLACE; only painted pixels are written.  depth_text: the NUL-terminated "{:.2f}".format(depth) of the caller.  Two
 * launches on `stream` (one workgroup per frame formats the numbers and lays the items out in the workspace; 64 x 16 pixel tiles of every
 * item's box test their pixels against the segments of the glyphs in reach); every workspace byte that is read was written by the same call, so
 * the result does not depend on the workspace's contents.  The handle need not be bound.  SD_ERR_INVALID, nothing launched: a null pointer,
 * B < 1 or B > 65535, an extent outside 1..16384, depth_text longer than 23 bytes, workspace_bytes below sd_text_workspace_bytes(B), a
 * workspace that is not 16-byte aligned, records_dev not 8-byte aligned. */
sd_status sd_text_draw_rw(sd_handle* h, uint8_t* dst_dev, int B, int dst_h, int dst_w, const sd_rw_result* records_dev, const char* depth_text,
                          void* workspace_dev, size_t workspace_bytes, void* stream);
/* HOST: the items sd_text_draw_rw draws for one record on a dst_h x dst_w image, as data: items_out[0 .. *n_out), *n_out <= SD_TEXT_MAX_ITEMS;
 * every byte of a returned item is defined (text is zero-filled behind len).  SD_ERR_INVALID as above. */
sd_status sd_text_items_rw_host(const sd_rw_result* record, const char* depth_text, int dst_h, int dst_w, sd_text_item* items_out, int* n_out);
/* HOST: the same rule for any n >= 0 items on img_host u8 [h,w,3], in list order.  SD_ERR_INVALID, nothing drawn: a null pointer, an extent
 * outside 1..16384, an item outside the caps above. */
sd_status sd_text_draw_host(uint8_t* img_host, int h, int w, const sd_text_item* items, int n);
/* HOST: the font as data: the segments {x0, y0, x1, y1} of byte `code` (0..255) into segs_out[0 .. 4 * *n_out), *n_out <= SD_TEXT_MAX_SEGS,
 * and its advance.  SD_ERR_INVALID: a null pointer or a code outside 0..255. */
sd_status sd_text_glyph(int code, int8_t* segs_out, int* n_out, int* advance_out);

/* ---- rendered clouds: every frame's road cloud and road-width line drawn to a top-view image on the GPU (opt-in) ----
 * The reference renders each <name>_rw.ply with Open3D's OpenGL visualiser behind a saved pinhole camera (utils/render_ply.py).  Open3D's
 * pixels are not reproduced: the project draws z-buffered square points with a rule of its own, stated once, for host and device, in
 * semantic_depth_amd/csrc/render_rule.hpp.  No pixel identity with Open3D is claimed; no anti-aliasing.
 *   rows      the rows of the frame's _rw.ply before its filter: the n cloud points in order, then -- when record.found != 0 -- the 1001
 *             points of the road-width line (the device PLY route's rule above, the same function of ply_format.hpp), colour 250 0 0.  Row
 *             index i = the cloud index, or n + the line index.
 *   filter    zmin = the minimum world z over the rows whose three coordinates are all finite; a row is drawn iff its three coordinates are
 *             finite and z > zmin (every row at the minimum goes).  Non-finite rows are skipped and do not flag the frame.
 *   camera    sd_render_camera, Open3D's convention (x right, y down, z forward).  Caps: every double finite, z_near > 0, width and
 *             height 1..SD_RENDER_MAX_EXTENT, point_size 1..SD_RENDER_MAX_POINT.
 *   project   in doubles, no contraction, in this order: X = ((e00 x + e01 y) + e02 z) + e03, Y and Z likewise from rows 1 and 2 of ext;
 *             dropped unless Z >= z_near; u = fx (X / Z) + cx, v = fy (Y / Z) + cy; dropped unless -s <= u < width + s and
 *             -s <= v < height + s, s = point_size (a NaN fails the comparisons; the test comes before any cast); px = (int)floor(u),
 *             py = (int)floor(v).
 *   splat     columns px - (s - 1) / 2 .. px + s / 2 and the same range of rows around py (integer divisions), clipped to the image.
 *   depth     key = ((uint64)bits of (float)Z << 32) | row index.  Z > 0, so the float's bits order as an unsigned integer: a pixel takes
 *             the colour of the covering row with the smallest key -- the nearest row, and among equal depths the lowest row index.  A
 *             pixel no row covers takes `background`.
 *   output    u8 [height,width,3] in BGR, the channel order of sd_compose_result_frames: a cloud colour (r, g, b) is stored b, g, r.
 * flags      0: rendered.  1: n_dev[b] is outside 0..cap; the image is background only. */
#define SD_RENDER_MAX_EXTENT 16384
#define SD_RENDER_MAX_POINT 16
typedef struct {
    double ext[12];        /* world -> camera, row-major 3 x 4 */
    double fx, fy, cx, cy; /* pinhole intrinsics */
    double z_near;         /* finite, > 0 */
    int32_t width, height; /* 1..SD_RENDER_MAX_EXTENT */
    int32_t point_size;    /* 1..SD_RENDER_MAX_POINT */
    uint8_t background[3]; /* in the image's channel order */
    uint8_t reserved;      /* 0 */
} sd_render_camera;
/* the device workspace sd_render_rw needs for B frames of clouds of `cap` points behind this camera: the depth keys, 8 bytes per pixel per
 * frame, and the minimum-z slots.  SD_ERR_INVALID for B < 1, B > 65535, cap < 0, a null pointer or a camera outside the caps. */
sd_status sd_render_workspace(int B, int cap, const sd_render_camera* cam_host, size_t* workspace_bytes);
/* DEVICE: xyz f32 [B,cap,3], rgb u8 [B,cap,3], n i32 [B] (sd_road_width's final clouds) and records [B] -> dst_dev u8 [B,height,width,3] BGR,
 * every byte written, and flags_dev i32 [B].  The camera is read on the HOST and passed by value to the kernels.  Five launches on `stream`
 * (minimum z per 256-row block; per frame, with the flags; the keys cleared to all ones; one lane per row projects it once and issues a
 * 64-bit integer atomic minimum per covered pixel; one lane per four pixels resolves the keys to colours and stores three aligned words), no
 * host synchronisation, no floating-point atomics: the minimum of integers does not depend on the order in which workgroups arrive, and
 * every workspace byte that is read was written by the same call.  The handle need not be bound.  SD_ERR_INVALID, nothing launched: a null
 * pointer, B < 1, B > 65535, cap < 0, a camera outside the caps or with a non-finite field, workspace_bytes below sd_render_workspace, a
 * workspace that is not 16-byte aligned, records_dev not 8-byte aligned, xyz_dev, n_dev, flags_dev or dst_dev not 4-byte aligned. */
sd_status sd_render_rw(sd_handle* h, const float* xyz_dev, const uint8_t* rgb_dev, const int32_t* n_dev, int B, int cap,
                       const sd_rw_result* records_dev, const sd_render_camera* cam_host, uint8_t* dst_dev, int32_t* flags_dev,
                       void* workspace_dev, size_t workspace_bytes, void* stream);
/* HOST: the CPU statement of sd_render_rw for one frame (xyz f32 [n,3], rgb u8 [n,3], one record; the cloud's capacity is n): one plain loop
 * over the rows with a host key buffer -> out_host u8 [height,width,3], *flag_out = 0.  n < 0 stands for a count outside the cloud:
 * *flag_out = 1 and the image is background only.  SD_ERR_INVALID, nothing written: a null pointer (xyz_host and rgb_host may be null for
 * n <= 0) or a camera outside the caps. */
sd_status sd_render_rw_host(const float* xyz_host, const uint8_t* rgb_host, int n, const sd_rw_result* record, const sd_render_camera* cam,
                            uint8_t* out_host, int32_t* flag_out);

/* DepthFrame.post_processing alone, semantic_depth.py:656-664: disp_raw f32 [B,2,H,W] -> disp_pp f32 [B,H,W] */
sd_status sd_post_process(sd_handle* h, const float* disp_raw, int B, float* disp_pp, void* stream);

/* disparity scaling + DepthFrame.compute_3D_points + BGR->RGB + mask gather,
 * semantic_depth.py:145,160-161,183-187,686-697 (seq:146,152-153,170-174), for B frames.
 * disp_pp f32 [B,H,W]; masks u8 [B,H,W]; frames u8 [B,H,W,3]; cams[B] (HOST pointer).
 * points_dense (nullable) f32 [B,H,W,3] = cv2.reprojectImageTo3D(disp_pp*mult, Q).
 * road_xyz f32 [B,cap,3], road_rgb u8 [B,cap,3] (nullable), n_road i32 [B]; same for fence (all nullable as a group).
 * cap = per-frame capacity in points (H*W is always enough); order = row-major order of the True pixels. */
sd_status sd_fuse_backproject(sd_handle* h, const float* disp_pp, const uint8_t* road_mask, const uint8_t* fence_mask,
                              const uint8_t* frames, const sd_camera* cams_host, int B, int cap, float* points_dense,
                              float* road_xyz, uint8_t* road_rgb, int32_t* n_road, float* fence_xyz, uint8_t* fence_rgb,
                              int32_t* n_fence, void* stream);

/* DepthFrame.post_processing (:656-664) + the above in ONE pass over the pixels: the raw pair is read once, disp_pp_out
 * (f32 [B,H,W], required) is written once and never re-read, both clouds are gathered in the same launch (decoupled look-back
 * compaction).  disp_raw f32 [B,2,H,W], or NULL = the raw output of the handle's last sd_monodepth_forward (B <= 32 frames).
 * Same results as sd_post_process followed by sd_fuse_backproject, bit for bit. */
sd_status sd_postprocess_fuse_backproject(sd_handle* h, const float* disp_raw, float* disp_pp_out, const uint8_t* road_mask,
                                          const uint8_t* fence_mask, const uint8_t* frames, const sd_camera* cams_host, int B, int cap,
                                          float* road_xyz, uint8_t* road_rgb, int32_t* n_road, float* fence_xyz, uint8_t* fence_rgb,
                                          int32_t* n_fence, void* stream);

/* The calibration mode's inner loop, semantic_depth.py:854-906 (every frame once per trial focal length), behind ONE network pass:
 * sd_fuse_backproject for B frames under T trial cameras each, in one count + scan + write.  cams_host[t * B + b] is frame b's camera
 * of trial t (HOST pointer).  Slot s = t * B + b of road_xyz f32 [T*B,cap,3], road_rgb u8 [T*B,cap,3] (nullable) and n_road i32 [T*B]
 * receives, bit for bit, what sd_fuse_backproject writes for frame b with that camera: the full count (also when it passes cap), rows
 * [0, min(n, cap)); rows behind that are not written.  The fence outputs are nullable as a group (fence_rgb alone may be NULL too).
 * The masks are counted and scanned once per frame; a kept pixel loads its disparity and colour once and is projected through the
 * frame's T cameras.  The cameras, block counts and offsets live in workspace_dev (sd_fuse_sweep_workspace bytes for the handle's
 * H x W; 0 = bad arguments); every workspace byte that is read is written by the same call.  Enqueued on `stream`, no synchronisation;
 * the handle need not be bound.  SD_ERR_INVALID, nothing launched: a null disp_pp, road_mask, cams_host, road_xyz, n_road or
 * workspace_dev; B < 1, T < 1, T * B > 65535, cap < 1; fence_xyz without fence_mask or n_fence; a colour output without frames;
 * workspace_bytes below sd_fuse_sweep_workspace; a workspace that is not 16-byte aligned. */
size_t sd_fuse_sweep_workspace(int B, int T, int H, int W);
sd_status sd_fuse_backproject_sweep(sd_handle* h, const float* disp_pp, const uint8_t* road_mask, const uint8_t* fence_mask,
                                    const uint8_t* frames, const sd_camera* cams_host /* [T][B] */, int B, int T, int cap,
                                    float* road_xyz, uint8_t* road_rgb, int32_t* n_road,
                                    float* fence_xyz, uint8_t* fence_rgb, int32_t* n_fence,
                                    void* workspace_dev, size_t workspace_bytes, void* stream);

/* the road chain of FrameProcessor.process_frame, semantic_depth.py:203-259 (seq:180-238):
 * z-cut -> MAD(y) -> MAD(x) -> plane fit -> [Open3D statistical + radius] -> end points -> width.
 * road_xyz f32 [B,cap,3], n_road i32 [B] (device).  road_rgb (nullable) u8 [B,cap,3]: the colours the reference carries
 * through every filter (road_colors, :206-245).  results: DEVICE array of B sd_rw_result.
 * final_xyz (nullable) f32 [B,cap,3] receives the denoised cloud, final_rgb (nullable, needs road_rgb) its colours,
 * n_final i32 [B] its size. */
sd_status sd_road_width(sd_handle* h, const float* road_xyz, const uint8_t* road_rgb, const int32_t* n_road, int B, int cap,
                        const sd_rw_params* params_host, sd_rw_result* results, float* final_xyz, uint8_t* final_rgb,
                        int32_t* n_final, void* stream);

/* fence chain + fence-to-fence distance, semantic_depth.py:273-334 (seq:245-298), for B frames:
 * MAD(y, mad_y) -> |z| < z_max -> extract_pcls at mean x -> left: MAD(x, mad_left) + plane(axis 0, plane_thr);
 * right: MAD(x, mad_right) + plane(axis 0, plane_thr) -> both planes intersected with the road plane at z = -depth
 * -> Euclidean distance.  road: DEVICE array of B sd_rw_result (their .plane is the road plane, from sd_road_width). */
typedef struct {
    double depth;        /* :325 z=self.depth (10.0) */
    double mad_y;        /* remove_noise_by_mad(fence, 1, 5.0)      :279-280 */
    double z_max;        /* threshold_complete(fence, 2, 35.0)      :283-284 */
    double mad_left;     /* remove_noise_by_mad(left, 0, 5.0)       :291 */
    double mad_right;    /* remove_noise_by_mad(right, 0, 1.0)      :302 */
    double plane_thr;    /* remove_noise_by_fitting_plane(axis=0, threshold=1.0) :294-298, :305-309 */
} sd_f2f_params;
typedef struct {
    double dist;                       /* dist_f2f, :327 */
    double left_pt[3], right_pt[3];    /* plane intersections at z = -depth, :321-326 */
    double plane_left[4], plane_right[4];
    int32_t counts[7];                 /* n_fence, after MAD(y), after |z| cut, left, right, left final, right final */
    int32_t ok;                        /* 0 when a side is empty / the planes are degenerate (dist is NaN) */
} sd_f2f_result;
/* fence_rgb (nullable) u8 [B,cap,3]; left_* / right_* (nullable) receive the denoised left / right fence clouds the
 * reference writes to <name>_FENCE.ply (:412-415): xyz f32 [B,cap,3], rgb u8 [B,cap,3], sizes = results[b].counts[5], [6] */
sd_status sd_fence_to_fence(sd_handle* h, const float* fence_xyz, const uint8_t* fence_rgb, const int32_t* n_fence, int B, int cap,
                            const sd_rw_result* road, const sd_f2f_params* params_host, sd_f2f_result* results,
                            float* left_xyz, uint8_t* left_rgb, float* right_xyz, uint8_t* right_rgb, void* stream);

/* The bounding box of the cloud that ENTERS a plane fit -- what pcl.plane_grid lays its 5 cm lattice over (semantic_depth.py:215-219,
 * :294-309): the road cloud after z-cut, MAD(y), MAD(x); each fence side after its MAD(x).  n = that cloud's point count; a, b = the two
 * in-plane axes of pcl.plane_grid: road (x, z), fences (y, z); the bounds are the float32 np.amin / np.amax of those columns: a NaN in a
 * column makes both of its bounds NaN, between -0.0 and +0.0 the minimum is -0.0 and the maximum +0.0.  n == 0: the four floats are 0. */
typedef struct {
    float lo_a, hi_a, lo_b, hi_b;
    int32_t n;
    int32_t pad;                       /* 0 */
} sd_plane_box;                        /* 24 bytes */
/* sd_road_width / sd_fence_to_fence with the boxes: boxes_dev (DEVICE, nullable) receives [B] (road) or [B][2] (fence: left, right).
 * One more launch per plane fit (one workgroup per frame, wave shuffles, no floating-point atomics); every other output is bit-identical
 * with and without it.  The calls above forward here with boxes_dev = NULL. */
sd_status sd_road_width_boxes(sd_handle* h, const float* road_xyz, const uint8_t* road_rgb, const int32_t* n_road, int B, int cap,
                              const sd_rw_params* params_host, sd_rw_result* results, float* final_xyz, uint8_t* final_rgb,
                              int32_t* n_final, sd_plane_box* boxes_dev, void* stream);
sd_status sd_fence_to_fence_boxes(sd_handle* h, const float* fence_xyz, const uint8_t* fence_rgb, const int32_t* n_fence, int B, int cap,
                                  const sd_rw_result* road, const sd_f2f_params* params_host, sd_f2f_result* results,
                                  float* left_xyz, uint8_t* left_rgb, float* right_xyz, uint8_t* right_rgb, sd_plane_box* boxes_dev,
                                  void* stream);

/* ---- scene PLYs: the 3D products of semantic_depth.py:404-431 for every frame of a batch, formatted on the GPU ----
 * A file is the concatenation of the segments its mask selects, in the fixed order of semantic_depth.py:418-431:
 *   ROAD        the final road cloud (sd_road_width's final_xyz / final_rgb / n_final)
 *   ROAD_PLANE  the road plane lattice: pcl.plane_grid(axis 1) over the road box, lifted by record.plane, colour 200 200 200
 *   RW_LINE     the 1001 rows of the road-width line exactly as sd_ply_format_rw writes them, when record.found (colour 250 0 0)
 *   FENCE_L, FENCE_R   the denoised left / right fence clouds (sd_fence_to_fence's left_* / right_*; sizes f2f.counts[5], [6])
 *   PLANE_L, PLANE_R   the fence plane lattices: pcl.plane_grid(axis 0) over the fence boxes, lifted by f2f.plane_left / plane_right,
 *                      colour 40 70 40
 *   F2F_LINE    the same line rule on f2f.left_pt / right_pt (float64 already), when f2f.ok (colour 0 255 0)
 * The lattice (semantic_depth_amd/csrc/scene_format.hpp states it once for host and device) is np.arange's under numpy 2 for float32
 * bounds: n_a = max(0, ceil(fl32(fl32(hi_a - lo_a) / fl32(0.05)))), a_0 = lo_a, a_1 = fl32(lo_a + fl32(0.05)), a_i = lo_a + i * (a_1 - a_0)
 * in float64; row i is (a_{i mod n_a}, b_{i div n_a}); the lifted coordinate is (c_a * a + c_b * b) + C, without contraction.  A lattice is
 * absent when its box has n == 0 or n_a * n_b == 0.  The fence inputs (clouds, f2f, fence boxes) are nullable: their segments are absent.
 * Everything else is the contract of sd_ply_format_rw: zmin = the minimum z over ALL rows of the file, a row is kept iff z > zmin; rows
 * and header as there; the files PACKED, offsets[B+1], flags[B]; no synchronisation; the result depends neither on the workspace's
 * contents nor on the order of the workgroups.
 * flags  0: produced.  1: a coordinate of a selected segment (a NaN box, a lifted coordinate and the line end points among them) is not
 *        finite or has |v| >= 2^31, or a count is outside its capacity (n_road outside 0..cap_road, the two fence counts negative or
 *        together above cap_fence, a lattice axis of 2^31 samples or more).  2: the text would pass text_capacity; the frames behind it
 *        still pack.  3: a selected lattice has more than lattice_cap rows (0 on the host call: no cap).  A flagged frame has size 0. */
#define SD_SCENE_ROAD 1u
#define SD_SCENE_ROAD_PLANE 2u
#define SD_SCENE_RW_LINE 4u
#define SD_SCENE_FENCE_L 8u
#define SD_SCENE_FENCE_R 16u
#define SD_SCENE_PLANE_L 32u
#define SD_SCENE_PLANE_R 64u
#define SD_SCENE_F2F_LINE 128u
#define SD_SCENE_ALL 255u
/* the device workspace sd_scene_format needs for `mask`, and the text capacity that holds any content: B * (SD_PLY_HEADER_CAP + rows *
 * SD_PLY_ROW_CAP) with rows = the bound the grid is sized from, the sum over the SELECTED segments only: cap_road (ROAD), cap_fence
 * (FENCE_L and FENCE_R together), lattice_cap per lattice, SD_PLY_LINE_ROWS per line -- cap_road + cap_fence + 3 * lattice_cap + 2 *
 * SD_PLY_LINE_ROWS for SD_SCENE_ALL.  SD_ERR_INVALID for B outside 1..65535, a negative cap, a mask beyond SD_SCENE_ALL or rows of
 * 2^31 - 512 or more. */
sd_status sd_scene_workspace(int B, int cap_road, int cap_fence, uint32_t lattice_cap, uint32_t mask, size_t* workspace_bytes,
                             size_t* text_bound);
/* DEVICE: the road group (xyz f32 [B,cap_road,3], rgb u8, n i32 [B]), the fence group (left / right xyz f32 [B,cap_fence,3], rgb u8; all
 * four or none), records [B], f2f [B] (nullable; needed by the fence group), road_boxes [B] and fence_boxes [B][2] (nullable: no
 * lattice) -> the files of `mask` packed into text_dev as sd_ply_format_rw packs its files.  Six launches on `stream` (one thread per
 * frame makes the segment table: eight row counts, their prefix, n_a and the two steps per lattice, flag 3; then the five of
 * sd_ply_format_rw over the scene's rows; a workgroup whose 256 rows lie behind the frame's last row exits at once).  SD_ERR_INVALID,
 * nothing launched: as sd_ply_format_rw, and a fence group that is partly given or lacks f2f_dev, a mask beyond SD_SCENE_ALL. */
sd_status sd_scene_format(sd_handle* h, const float* road_xyz_dev, const uint8_t* road_rgb_dev, const int32_t* n_road_dev, int cap_road,
                          const float* left_xyz_dev, const uint8_t* left_rgb_dev, const float* right_xyz_dev, const uint8_t* right_rgb_dev,
                          int cap_fence, int B, const sd_rw_result* records_dev, const sd_f2f_result* f2f_dev,
                          const sd_plane_box* road_boxes_dev, const sd_plane_box* fence_boxes_dev, uint32_t mask, uint32_t lattice_cap,
                          uint8_t* text_dev, size_t text_capacity, uint64_t* offsets_dev, int32_t* flags_dev, void* workspace_dev,
                          size_t workspace_bytes, void* stream);
/* HOST: the CPU statement of sd_scene_format for one frame (clouds as long as n_road and f2f->counts[5], [6] say): the same bytes into
 * out_host[0 .. cap), *size_out = their count, *flag_out = 0; or *flag_out = 1 / 3 and *size_out = 0 under the rules above; or, when the
 * text is longer than cap, *flag_out = 2, *size_out = the size it needs and nothing written.  SD_ERR_INVALID: a null record, a negative
 * n_road, a fence cloud without its colours or without f2f, a mask beyond SD_SCENE_ALL. */
sd_status sd_scene_format_host(const float* road_xyz_host, const uint8_t* road_rgb_host, int n_road, const float* left_xyz_host,
                               const uint8_t* left_rgb_host, const float* right_xyz_host, const uint8_t* right_rgb_host,
                               const sd_rw_result* record, const sd_f2f_result* f2f, const sd_plane_box* road_box,
                               const sd_plane_box* fence_boxes, uint32_t mask, uint32_t lattice_cap, uint8_t* out_host, size_t cap,
                               size_t* size_out, int32_t* flag_out);
/* HOST: one lattice alone, by the same rule: box and plane (Cx, Cy, Cz, C) -> *n_a, *n_b and, when xyz_out is given, the n_a * n_b lattice
 * points f64 [rows,3] in file order (axis 1: the road's (x, z) lattice lifted in y; axis 0: a fence's (y, z) lattice lifted in x).
 * SD_ERR_INVALID: a null pointer, another axis, a box np.arange refuses, more rows than rows_cap. */
sd_status sd_scene_lattice_host(const sd_plane_box* box, const double* plane, int axis, uint32_t* n_a, uint32_t* n_b, double* xyz_out,
                                size_t rows_cap);

/* ---------------------------------------------------------------- depth profile
 * The depth (sd_rw_params.depth, sd_f2f_params.depth) enters the road chain only in its last step and the fence chain only in the two
 * plane intersections.  These calls take the ONE denoised cloud (sd_road_width's final_xyz / n_final) and the ONE set of planes per
 * frame and give the road record and the fence-to-fence distance at D depths, without running the chains again.
 *
 * sd_road_width_profile: results[b][i] holds, bit for bit, the width, x_left, x_right, left_pt, right_pt and found that sd_road_width's
 * last step writes for frame b's cloud with params.depth = depths[i] (the same window and depth_offset); n_window is the number of rows
 * inside that window.  depths_host may come in any order and may repeat.  Two launches on `stream`, no global atomics and no
 * synchronisation; every byte of every record is written, and every workspace byte that is read is written by the same call
 * (sd_rw_profile_workspace bytes; 0 = bad arguments).  The handle need not be bound and its max_batch / cap do not matter.
 * SD_ERR_INVALID, nothing launched: a null pointer; B < 1 or B > 65535; cap < 1; D outside 1..SD_PROFILE_MAX_DEPTHS; a non-finite depth,
 * window or depth_offset; window <= 0; workspace_bytes below sd_rw_profile_workspace; a workspace that is not 16-byte aligned, float /
 * counter arrays that are not 4-byte or results that are not 8-byte aligned.
 * sd_road_width_profile_host: the same records for one HOST cloud of n >= 0 rows (xyz_host may be NULL when n == 0).
 *
 * sd_f2f_profile: results[b][i] holds the dist, left_pt, right_pt and ok that sd_fence_to_fence gives frame b with params.depth =
 * depths[i] (z = -depths[i]; no depth_offset there), from road[b].plane and f2f[b].plane_left / plane_right / counts[5], counts[6].
 * A NaN in these records is the quiet NaN 0x7ff8000000000000 whatever the processor's own 0 / 0 looks like.  One launch, every byte
 * written.  SD_ERR_INVALID: a null pointer, B < 1 or B > 65535, D outside 1..SD_PROFILE_MAX_DEPTHS, a non-finite depth, records that are
 * not 8-byte aligned.  sd_f2f_profile_host: the same records for ONE frame's two HOST records. */
#define SD_PROFILE_MAX_DEPTHS 256
typedef struct {
    double width;                      /* as sd_rw_result */
    float x_left, x_right;
    float left_pt[3], right_pt[3];
    int32_t found;
    int32_t n_window;                  /* rows inside the window of this depth */
} sd_rw_depth_result;                  /* 48 bytes */
typedef struct {
    double dist;                       /* as sd_f2f_result */
    double left_pt[3], right_pt[3];
    int32_t ok, reserved;              /* reserved = 0 */
} sd_f2f_depth_result;                 /* 64 bytes */
size_t sd_rw_profile_workspace(int B, int cap, int D);
sd_status sd_road_width_profile(sd_handle* h, const float* xyz_dev /* [B,cap,3] */, const int32_t* n_dev /* [B] */, int B, int cap,
                                const double* depths_host, int D, double window, double depth_offset,
                                sd_rw_depth_result* results_dev /* [B][D] */, void* workspace_dev, size_t workspace_bytes, void* stream);
sd_status sd_road_width_profile_host(const float* xyz_host, int n, const double* depths, int D, double window, double depth_offset,
                                     sd_rw_depth_result* results_host /* [D] */);
sd_status sd_f2f_profile(sd_handle* h, const sd_rw_result* road_dev, const sd_f2f_result* f2f_dev, int B, const double* depths_host, int D,
                         sd_f2f_depth_result* results_dev /* [B][D] */, void* stream);
sd_status sd_f2f_profile_host(const sd_rw_result* road, const sd_f2f_result* f2f, const double* depths, int D,
                              sd_f2f_depth_result* results_host /* [D] */);

/* ---------------------------------------------------------------- measurement lines in the result images (opt-in)
 * seq:330-333, step "8.A Project the 3D points that define the line to the image plane": two calls of print_line_on_image, commented out
 * because the function was never written.  The project draws them -- the measured road-width line, the fence-to-fence line and, with a
 * depth profile, the road's left and right edge along the profile and a rung per depth -- with a rule of its own, stated once, for host and
 * device, in semantic_depth_amd/csrc/overlay_rule.hpp.  The reference gives only the two colours (0,0,255) and (0,255,0); the edge colour and
 * the thicknesses are the project's choice.  No pixel identity with cv2.line is claimed; no anti-aliasing; a segment is not clipped at the
 * near plane but skipped.
 *   project   the inverse of make_Q / reprojectImageTo3D, in doubles, no contraction, in this order: cx, cy, f rounded to float32 (as the
 *             Q matrix rounds them) and promoted; zn = -Z, the point is dropped unless zn > 0 (a NaN fails); s = f / zn; xn = cx + X s,
 *             yn = cy - Y s (network pixels, centres at integers); xo = (xn + 0.5) ((double)dst_w / net_w) - 0.5 and yo likewise with the
 *             heights (the pixel-centre alignment of cv2.resize); dropped unless |xo| <= SD_OVERLAY_MAX_COORD and |yo| <=
 *             SD_OVERLAY_MAX_COORD (before any cast); q = (int32)floor(v * 256 + 0.5), in 1/256 pixel.
 *   slots     a frame with D profile depths has 4 D + 2 slots (at most SD_OVERLAY_MAX_SEGS); slot order is paint order, the highest valid
 *             slot that covers a pixel gives its colour.  Slot i (i < D - 1): the left edge, profile[i].left_pt -> profile[i + 1].left_pt in
 *             the order the depths were given, when both entries are found (slot D - 1 is never valid).  Slot D + i: the same on right_pt.
 *             Slot 2 D + i: the road rung of depth i, left_pt -> right_pt, when found.  Slot 3 D + i: the fence rung of depth i from the
 *             sd_f2f_depth_result points, when ok (only with fence profile records).  Slot 4 D: the record's road-width line, when found.
 *             Slot 4 D + 1: the fence record's line, when ok (only with fence records).  A slot whose segment exists but has a dropped end
 *             point is not drawn and sets bit 0 of the frame's flag.
 *   style     sd_overlay_style: rw_bgr colours the road rungs and the road-width line, f2f_bgr the fence rungs and the fence line, edge_bgr
 *             the two edges (the image's channel order); thickness 1..SD_OVERLAY_MAX_THICKNESS for the two record lines,
 *             profile_thickness likewise for everything from the profile; clip_top 0..dst_h: rows above it are never painted (the banner
 *             stays clean); reserved = 0.
 *   paint     sd_text_draw_host's rule on the segment: pixel (px, py), centre (256 px, 256 py), is painted iff its squared distance to the
 *             segment is <= (128 thickness)^2, in exact integers; a zero-length segment is a disc.  A pixel no slot paints is never written.
 * flags      bit 0: a segment of the frame was skipped for a dropped end point. */
#define SD_OVERLAY_MAX_SEGS (4 * SD_PROFILE_MAX_DEPTHS + 2)
#define SD_OVERLAY_MAX_COORD 32768
#define SD_OVERLAY_MAX_THICKNESS 32
typedef struct {
    uint8_t rw_bgr[3], f2f_bgr[3], edge_bgr[3];
    uint8_t reserved[3];               /* 0 */
    int32_t thickness, profile_thickness, clip_top;
} sd_overlay_style;                    /* 24 bytes */
typedef struct {
    int32_t ax, ay, bx, by;            /* the end points in 1/256 pixel */
    uint8_t bgr[3];
    uint8_t thickness;
} sd_overlay_segment;                  /* 20 bytes */
/* the device workspace sd_overlay_draw needs for B frames with D profile depths; 0 for B outside 1..65535 or D outside
 * 0..SD_PROFILE_MAX_DEPTHS */
size_t sd_overlay_workspace_bytes(int B, int D);
/* DEVICE: draws the slots of frame b -- from records_dev[b], f2f_dev[b] (nullable: no slot 4 D + 1), rw_profile_dev[b][0 .. D) (needed when
 * D > 0) and f2f_profile_dev[b][0 .. D) (nullable: no fence rungs), all read on the device -- into dst_dev u8 [B,dst_h,dst_w,3] IN PLACE; only
 * painted pixels are written; flags_dev i32 [B] receives every frame's flag.  cams_host[b] (HOST pointer; cx, cy and f are used) is
 * frame b's camera at the network size net_h x net_w; the cameras are staged through the workspace.  Two launches on `stream` (one
 * workgroup per frame projects the end points and writes every slot, its clipped pixel box and the union of the boxes; 64 x 16 pixel
 * tiles inside that union keep the slots whose box meets them and test their pixels from the last slot to the first), no atomics, no host
 * synchronisation; every workspace byte that is read was written by the same call.  The handle need not be bound.  SD_ERR_INVALID, nothing
 * launched: a null pointer (but the three nullable ones), B outside 1..65535, an extent outside 1..16384, D outside
 * 0..SD_PROFILE_MAX_DEPTHS, D > 0 without rw_profile_dev, a style outside its caps, a camera whose cx, cy or f is not finite in float32,
 * workspace_bytes below sd_overlay_workspace_bytes(B, D), a workspace that is not 16-byte aligned, records that are not 8-byte or flags
 * that are not 4-byte aligned. */
sd_status sd_overlay_draw(sd_handle* h, uint8_t* dst_dev, int B, int dst_h, int dst_w, int net_h, int net_w, const sd_camera* cams_host,
                          const sd_rw_result* records_dev, const sd_f2f_result* f2f_dev, const sd_rw_depth_result* rw_profile_dev,
                          const sd_f2f_depth_result* f2f_profile_dev, int D, const sd_overlay_style* style_host, int32_t* flags_dev,
                          void* workspace_dev, size_t workspace_bytes, void* stream);
/* HOST: the valid segments of one frame in slot order, as data: segs_out[0 .. *n_out), *n_out <= 4 D + 2 (segs_out holds that many), and the
 * frame's flag.  SD_ERR_INVALID, nothing written: as above. */
sd_status sd_overlay_segments_host(const sd_rw_result* record, const sd_f2f_result* f2f, const sd_rw_depth_result* rw_profile,
                                   const sd_f2f_depth_result* f2f_profile, int D, const sd_camera* cam, int net_h, int net_w, int dst_h, int dst_w,
                                   const sd_overlay_style* style, sd_overlay_segment* segs_out, int* n_out, int32_t* flag_out);
/* HOST: the paint rule for any n >= 0 segments on img_host u8 [h,w,3], in list order (a later segment paints over an earlier one), rows
 * above clip_top untouched.  SD_ERR_INVALID, nothing drawn: a null pointer, an extent outside 1..16384, clip_top outside 0..h, a segment
 * with a thickness outside 1..SD_OVERLAY_MAX_THICKNESS or a coordinate beyond 256 SD_OVERLAY_MAX_COORD in magnitude. */
sd_status sd_overlay_draw_host(uint8_t* img_host, int h, int w, const sd_overlay_segment* segs, int n, int clip_top);

/* ---------------------------------------------------------------- scoring the segmentation (fcn8s/fcn.py test mode, FCN.inference :384-492)
 * The test mode resizes the frame AND the label image with scipy.misc.imresize(img, image_shape) (:408, :412), which for uint8 input is
 * PIL.Image.resize((W, H), BILINEAR) -- not the cv2.resize cubic of sd_resize_cubic_u8 -- and scores argmax against
 * helper.prepare_ground_truth (:149-177) with tf.metrics.mean_iou, whose state is a count matrix.
 *
 * sd_resize_pil_bilinear_u8: Pillow's ImagingResample for 8-bit images with the bilinear filter, bit for bit (csrc/pil_resample.hpp states
 * the rule: a window that grows with the downscale factor, 22-bit fixed-point weights made on the host in double, horizontal then vertical
 * pass with the uint8 rounding between them).  src_dev: B frames of src_h x src_w pixels whose first bytes lie pixel_stride bytes apart
 * (rows and frames packed: src_w * pixel_stride and src_h * src_w * pixel_stride bytes); `channels` (1 or 3, <= pixel_stride <= 4) bytes
 * are taken per pixel, so channel 0 of a [H,W,3] label frame is read in place with pixel_stride 3, channels 1.  dst_dev: u8
 * [B,dst_h,dst_w,channels]; reverse != 0 stores the channels in reverse order (the readers deliver BGR, the test mode feeds RGB).
 * Two launches on `stream` (one when dst_h == src_h), no synchronisation, integer arithmetic only.  Every workspace byte the result depends on
 * is written by the same call (sd_resize_pil_workspace bytes, 16-byte aligned); the handle need not be bound.
 * SD_ERR_INVALID, nothing launched: a null pointer; B < 1 or B > 65535; channels not 1 or 3; pixel_stride < channels or > 4; a source or
 * destination extent outside 1..16384; a downscale factor above 32 on an axis (src > 32 * dst; the window would pass 65 taps); a
 * workspace that is too small or not 16-byte aligned.  Upscaling (windows of 1 or 2 taps) is accepted.
 * sd_resize_pil_bilinear_u8_host: the same bytes for HOST arrays (no B limit).
 *
 * sd_seg_confusion: counts_dev int64 [B][10] += per frame b the 3 x 3 matrix [label class][predicted class] in cells 0..8, where the
 * label class is table_host[labels[b][y][x]] (256 bytes, values 0..2: road 0, fence 1, everything else 2 -- prepare_ground_truth as a
 * table) and the predicted class pred[b][y][x] (the argmax of sd_fcn8s_forward).  A prediction above 2 is counted in no cell of the matrix
 * but in cell 9 of its frame, for the caller to turn into an error.  The caller zeroes counts_dev or keeps accumulating into it.  One
 * launch: ballots and population counts per wave, one sum per workgroup, at most ten 64-bit atomic adds per workgroup; integer sums, so
 * the result does not depend on their order.  The handle need not be bound.
 * SD_ERR_INVALID: a null pointer; B < 1 or B > 65535; height or width outside 1..16384; a table value above 2; counts_dev not 8-byte
 * aligned.  sd_seg_confusion_host: the same counts for HOST arrays (no B limit). */
sd_status sd_resize_pil_workspace(int B, int src_h, int src_w, int dst_h, int dst_w, int channels, size_t* bytes_out);
sd_status sd_resize_pil_bilinear_u8(sd_handle* h, const uint8_t* src_dev, int B, int src_h, int src_w, int pixel_stride, int channels, int reverse,
                                    uint8_t* dst_dev /* [B,dst_h,dst_w,channels] */, int dst_h, int dst_w, void* workspace_dev,
                                    size_t workspace_bytes, void* stream);
sd_status sd_resize_pil_bilinear_u8_host(const uint8_t* src, int B, int src_h, int src_w, int pixel_stride, int channels, int reverse,
                                         uint8_t* dst, int dst_h, int dst_w);
sd_status sd_seg_confusion(sd_handle* h, const uint8_t* pred_dev /* [B,height,width] */, const uint8_t* labels_dev /* [B,height,width] */, int B,
                           int height, int width, const uint8_t* table_host /* [256] */, int64_t* counts_dev /* [B][10] */, void* stream);
sd_status sd_seg_confusion_host(const uint8_t* pred, const uint8_t* labels, int B, int height, int width, const uint8_t* table /* [256] */,
                                int64_t* counts /* [B][10] */);

/* ---------------------------------------------------------------- the disparity image of a frame (semantic_depth.py:681-683)
 * DepthFrame.disp_to_image is scipy.misc.imresize(disp_pp, [h, w]) followed by plt.imsave(name + "_disp.png", img, cmap='gray')
 * (cmap='plasma' commented out beside it).  The rule, per frame b of a float32 [B, height, width] map (csrc/disp_image_rule.hpp states it
 * for host and device); mult[b] is the frame's disparity multiplier (:145), 1.0 when the pointer is NULL:
 *   1. v = d * mult[b] in float32.
 *   2. lo, hi = minimum and maximum of the FINITE v of the frame; cs = hi - lo in float32; cs == 0, or a frame with no finite value, means
 *      cs = 1 (and lo = 0 when nothing is finite); scale = (float)(255.0 / (double)cs).
 *   3. byte = (int)(clip((v - lo) * scale, 0, 255) + 0.5f), the difference and the product each rounded to float32 and never contracted into
 *      an fma: scipy's bytescale with the arithmetic of the numpy of the reference's time (an f32 array against a scalar stays f32)
 *      [UPSTREAM, unpinned].  A non-finite v gives byte 0 and sets flags[b] = 1; otherwise flags[b] = 0.  (hi - lo beyond the float32
 *      range makes scale 0 and the product of an infinite difference not a number: byte 0.)
 *   4. Pillow's bilinear resample of the [height, width] byte image to [out_h, out_w] (sd_resize_pil_bilinear_u8's arithmetic, one
 *      channel, shrinking and its support included); equal sizes mean a copy.
 *   5. lo8, hi8 = minimum and maximum of the RESIZED byte image of the frame; hi8 == lo8 gives index 0 for every pixel, otherwise
 *      idx = min(255, 256 * (p - lo8) / (hi8 - lo8)) in integers (floor).  This is matplotlib's float32 Normalize followed by int(x * 256)
 *      with 256 mapped to 255, for every (p, lo8, hi8): 256 a / b with b <= 255 is never within a float32 rounding of an integer it does
 *      not hit.  A constant image leaves as entry 0 of the table: black for gray, (12, 7, 134) for plasma.
 *   6. colour = table[cmap][idx], table = matplotlib.colormaps[cmap](np.arange(256), bytes=True)[:, :3], kept as data.  gray is NOT the
 *      identity: it is trunc(i / 255 * 255) in double, one below i at 24 entries (33, 37, 41, ..., 244).
 *   7. out: u8 [B, out_h, out_w, 3] in the channel order the PNG routes take (BGR).  imsave writes RGBA with alpha 255; the files here are
 *      8-bit RGB: pixels are pinned, not file bytes.
 * sd_disp_image: disp_dev f32 [B,height,width] (4-byte aligned; 16-byte aligned maps with height * width % 4 == 0 are read four floats per
 * lane), mult_host NULL or B floats on the HOST, out_bgr_dev any alignment (4-byte aligned with out_h * out_w % 4 == 0: dword stores),
 * flags_dev i32 [B].  Five launches on `stream` plus the resample's (none when the sizes agree), no synchronisation, no allocation: a
 * per-frame minimum / maximum over several workgroups combined by 32-bit integer atomics on an order-preserving key (no dependence on
 * grid size or arrival order), the byte pass, the resample, the minimum / maximum of the resized bytes, the colour pass.  Every workspace
 * byte the result depends on is written by the same call (sd_disp_image_workspace bytes, 16-byte aligned); the handle need not be bound.
 * SD_ERR_INVALID, nothing launched: a null pointer (mult_host excepted); B < 1 or B > 65535; a cmap that is not one of the two; an extent
 * below 1 or beyond what the resample accepts (1..16384, a downscale factor of at most 32 per axis); a workspace that is too small or not
 * 16-byte aligned; disp_dev or flags_dev not 4-byte aligned.
 * sd_disp_image_host: the same bytes and flags for HOST arrays (no B limit, no handle, no GPU).
 * sd_disp_colormap: the 256 entries of a map as R, G, B bytes. */
#define SD_CMAP_GRAY 0
#define SD_CMAP_PLASMA 1
sd_status sd_disp_image_workspace(int B, int height, int width, int out_h, int out_w, size_t* bytes_out);
sd_status sd_disp_image(sd_handle* h, const float* disp_dev, const float* mult_host /* nullable */, int B, int height, int width, int out_h,
                        int out_w, int cmap, uint8_t* out_bgr_dev /* [B,out_h,out_w,3] */, int32_t* flags_dev /* [B] */, void* workspace_dev,
                        size_t workspace_bytes, void* stream);
sd_status sd_disp_image_host(const float* disp, const float* mult /* nullable */, int B, int height, int width, int out_h, int out_w, int cmap,
                             uint8_t* out_bgr /* [B,out_h,out_w,3] */, int32_t* flags /* [B] */);
sd_status sd_disp_colormap(int cmap, uint8_t* rgb_out /* [768] */);

/* ---------------------------------------------------------------- pcl.py, function by function
 * (semantic_depth_lib/pcl.py; one cloud per call: xyz f32 [n,3], rgb u8 [n,3] nullable, n on the host).
 * Outputs keep the input row order.  *n_out is a DEVICE int32. */
/* pcl.remove_from_to, pcl.py:30-43 (keeps coord[axis] < -to_meter) */
sd_status sd_pcl_remove_from_to(sd_handle* h, const float* xyz, const uint8_t* rgb, int n, int axis, double to_meter,
                                float* xyz_out, uint8_t* rgb_out, int32_t* n_out, void* stream);
/* pcl.remove_noise_by_mad + mad, pcl.py:46-81.  stats_out (nullable, device f32[2]) = {median, MAD} */
sd_status sd_pcl_remove_noise_by_mad(sd_handle* h, const float* xyz, const uint8_t* rgb, int n, int axis, double threshold,
                                     float* xyz_out, uint8_t* rgb_out, int32_t* n_out, float* stats_out, void* stream);
/* pcl.remove_noise_by_fitting_plane, pcl.py:84-209 (without the visualisation grid).  coeff_out: device f64[4] = Cx,Cy,Cz,C */
sd_status sd_pcl_remove_noise_by_fitting_plane(sd_handle* h, const float* xyz, const uint8_t* rgb, int n, int axis,
                                               double threshold, float* xyz_out, uint8_t* rgb_out, int32_t* n_out,
                                               double* coeff_out, void* stream);
/* pcl.threshold_complete, pcl.py:240-250 (keeps |coord[axis]| < threshold) */
sd_status sd_pcl_threshold_complete(sd_handle* h, const float* xyz, const uint8_t* rgb, int n, int axis, double threshold,
                                    float* xyz_out, uint8_t* rgb_out, int32_t* n_out, void* stream);
/* pcl.extract_pcls, pcl.py:253-268: split at np.mean(coord[axis]) (reproduced bit for bit): left = coord < mean,
 * right = coord > mean.  mean_out (nullable): device f32[1] */
sd_status sd_pcl_extract_pcls(sd_handle* h, const float* xyz, const uint8_t* rgb, int n, int axis, float* left_xyz,
                              uint8_t* left_rgb, int32_t* n_left, float* right_xyz, uint8_t* right_rgb, int32_t* n_right,
                              float* mean_out, void* stream);
/* pcl.get_end_points_of_road, pcl.py:271-313: first min-x and max-x rows of the depth window.
 * out: device sd_rw_result (only found, x_left, x_right, left_pt, right_pt, width are written) */
sd_status sd_pcl_get_end_points_of_road(sd_handle* h, const float* xyz, int n, double depth, double window,
                                        sd_rw_result* out, void* stream);
/* Open3D statistical_outlier_removal / radius_outlier_removal as called at semantic_depth.py:234-241 */
sd_status sd_o3d_statistical_outlier_removal(sd_handle* h, const float* xyz, const uint8_t* rgb, int n, int nb_neighbors,
                                             double std_ratio, float* xyz_out, uint8_t* rgb_out, int32_t* n_out,
                                             double* mean_dist_out /* nullable, device f64[n] */, void* stream);
sd_status sd_o3d_radius_outlier_removal(sd_handle* h, const float* xyz, const uint8_t* rgb, int n, int nb_points,
                                        double radius, float* xyz_out, uint8_t* rgb_out, int32_t* n_out, void* stream);

/* ---------------------------------------------------------------- introspection (tests / profiling) */
/* copy an intermediate activation of the last forward (e.g. "layer3_out", "conv5") to out (device f32);
 * numel_out receives its element count; shape_out 4 x int64 [N,H,W,C] */
sd_status sd_net_tensor(sd_handle* h, sd_net net, const char* name, float* out, size_t out_capacity_floats,
                        int64_t* shape_out, void* stream);
/* per-kernel timing of the conv engine with HIP events on the launch stream (bench.py roofline).
 * sd_profile(h,1) starts recording an event pair around every conv launch; sd_profile_read synchronises the
 * device, sums elapsed time / algorithmic FLOPs (2*M*N*K) / launches per kernel instantiation into out[0..*n),
 * and clears the recording.  out: HOST array of capacity cap_buckets. */
typedef struct {
    char kernel[64];
    int64_t launches;
    double ms;
    double flops;
    double bytes;      /* algorithmic HBM bytes of those launches: every source tensor, the weights and the output tensor ONCE, in the
                          formats the engine stores them in (what a launch cannot avoid moving; the PMC traffic is compared with it) */
} sd_profile_bucket;
sd_status sd_profile(sd_handle* h, int enable);
sd_status sd_profile_read(sd_handle* h, sd_profile_bucket* out_host, int cap_buckets, int* n_out);

/* number of conv-engine FLOPs (2*M*N*K over all layers, per image) of a plan — for roofline accounting */
double sd_net_flops_per_image(const sd_handle* h, sd_net net);

/* frames of one network pass (the chunk size latched at sd_create: min(max_batch, SEMDEPTH_CHUNK or 32)); a batch of at most this many
 * frames leaves its raw disparity pair in the arena for sd_postprocess_fuse_backproject(disp_raw = NULL) */
int sd_pass_frames(const sd_handle* h);

/* fp16 range guard of the reduced-precision plans: the conv epilogues that write fp16 planes clamp at +-65504 and COUNT the values
 * they clamped (and NaNs) in a device counter.  *count_out = values clamped since the handle was bound or the counter last reset
 * (synchronises the device); reset != 0 clears it.  A non-zero count means the plan does not fit these weights / inputs: run the
 * layer's producer with more products, or the exact engine (the reference has no such failure mode: it computes in f32). */
sd_status sd_saturation_count(sd_handle* h, uint64_t* count_out, int reset);
/* Tail overlap: the conv kernels of the 3x3 layers are persistent workgroups that fill every CU's register file, so work on a second stream
 * (the per-frame tail of the previous batch: back-projection, road chain) finds no CU while they run.  n > 0 makes those launches use
 * (CUs - n) workgroups; the n CUs left free take the side stream's kernels.  0 (default, or SEMDEPTH_RESERVE_CUS at sd_create) = every CU.
 * Results do not depend on it (the tiles a workgroup walks change, not their arithmetic). */
sd_status sd_set_reserved_cus(sd_handle* h, int n);

/* Small-batch forms (SD_PREC_F16X2 only, opt-in).  Every GEMM block is chosen from the output tiles of a FULL pass of the handle, so that a
 * frame's bits do not depend on the call it is computed in.  On a handle whose full pass is one or two frames the deep GEMM layers (FCN-8s fc6 /
 * fc7, the res5 1x1 layers of monodepth-resnet50) have 16-32 tiles for 256 CUs.  on != 0 runs such a layer split along K: S slices per
 * output tile (the k-range form of the LDS-DMA ring, f32 partial sums in the workspace) and one reduce launch that adds the slices in ascending
 * order and applies the layer's epilogue.  The order of summation changes, so the last bits differ from the default handle's (same error
 * against a float64 reference); results stay deterministic and independent of the call size.  On a handle where no layer qualifies nothing changes.
 * Call it before sd_bind_memory (SD_ERR_STATE afterwards): sd_query_memory then reports the workspace with the partial-sum scratch.
 * SD_ERR_INVALID on a handle of another precision. */
sd_status sd_set_small_batch(sd_handle* h, int on);
/* The rule, device-free: the slice count S (1 = not split) of a GEMM with `rows` output pixels in a full pass, `cout` output channels and a
 * padded K axis of `kpad` on a chip of `cus` CUs.  tiles = ceil(rows / 256) * (cout / 256); a layer with cout % 256 != 0 or 8 * tiles > cus is not
 * split (measured: every layer that gained covers at most an eighth of the CUs; at a quarter and above the unsplit launch is as fast); S is the smallest value with tiles * S >= cus, capped at 16 and at (kpad / 32) / 8 (a slice keeps at least 8 k-tiles of 32);
 * a layer the caps leave below S = 4 is not split either (measured as well).
 * k_tiles_per_slice_out (nullable, int[16]): the S slice lengths in k-tiles -- contiguous ranges in this order, sum = kpad / 32. */
int sd_small_batch_split(long rows, int cout, int kpad, int cus, int* k_tiles_per_slice_out);
/* Level 2 (sd_set_small_batch(h, 2); 0 = off and 1 = the GEMM layers above stay what they are, a value above 2 is SD_ERR_INVALID; same guards): level 1 plus
 * the under-filled 3x3 DIRECT conv layers.  The direct kernel walks work items = (16 x 32-pixel tile) x (pass of 64 output channels), each over the layer's whole
 * chunk axis (a chunk = 16 input channels x 9 taps); at one frame conv5_x has 8-32 items for 256 CUs.  Level 2 runs such a layer as S contiguous chunk ranges per
 * item (conv_direct_splitc_hs_kernel, f32 partial sums at conv resolution in the same workspace region) and one reduce launch (splitc_reduce_kernel) that adds
 * the slices in ascending order and applies the layer's epilogue -- alpha, bias, activation, the fused 2x2 max pool, the HS split with the per-frame clamp
 * attribution.  Candidates: the 64-channel-pass HS form, not upsample-folded, not the all-upsampled instantiation, no padded channels.
 * The rule, device-free: S (1 = not split) of a layer with `items` work items in a FULL pass -- (W / 32) * ceil(H / 16) * images * passes at conv resolution --
 * and `nchunks` chunks on a chip of `cus` CUs.  S = 1 when items >= cus; otherwise S is the smallest value with items * S >= cus, capped at 16 and at
 * nchunks / 4 (a slice keeps at least 4 chunks).  Measured (profiles/latency_b1_direct.json; the table is in DESIGN section 4): a layer is admitted when
 * 2 * items <= cus, and above a quarter of the chip (4 * items > cus) only with nchunks >= 16 -- every admitted layer gained more than its default launch's
 * spread (conv5_x of one frame: 0.13 -> 0.04 ms), the two half-filled layers with 4-5 chunks per slice did not and left the rule.
 * chunks_per_slice_out (nullable, int[16]): the S slice lengths in chunks -- contiguous ranges in this order, longer ones first, sum = nchunks. */
int sd_small_batch_split_direct(long items, int nchunks, int cus, int* chunks_per_slice_out);
/* the layers of `net` this handle runs split, as "layer:S,layer:S" (empty: none); SD_ERR_INVALID when cap is too small */
sd_status sd_small_batch_plan(const sd_handle* h, sd_net net, char* layers_out, size_t cap);
/* which kernel runs every conv layer of `net` in a call of `frames` frames (0 = a full pass): one line "layer label slices\n" per layer, in launch order.
 * `label` is the per-layer profile label (the one SEMDEPTH_PROFILE_VERBOSE prints), `slices` the small-batch split (1 = one launch; above it the layer's reduce
 * launch follows).  A layer nothing can run is listed with the text of the error its call fails with in place of the label.  Needs no bound memory and no
 * device.  SD_ERR_INVALID when cap is too small (the text is cut at cap - 1) */
sd_status sd_conv_forms(const sd_handle* h, sd_net net, int frames, char* out, size_t cap);

/* the same count without a device synchronisation: an 8-byte device-to-host copy enqueued on `stream` behind the work already on it
 * (host_dst = pinned host memory of the caller).  The host-side classes use it to turn a range violation into an ERROR of the call that
 * produced it instead of a counter somebody has to poll (semantic_depth_amd/engine.py Engine.check_range). */
sd_status sd_saturation_count_async(sd_handle* h, uint64_t* host_dst, void* stream);

/* the same clamps attributed to frames: dst[i] = values clamped in frame i of the caller's batch (a monodepth frame's fliplr copy counts
 * toward the frame; every network pass adds at the frame's position in the batch) since the handle was bound or the counts last reset.
 * Copied on `stream` behind the work already on it (dst = pinned host or device memory, n uint32 values); reset != 0 then zeroes the
 * max_batch counters on the same stream.  The global counter of sd_saturation_count is not changed.  SD_ERR_INVALID for a NULL dst,
 * n < 1 or n > max_batch. */
sd_status sd_saturation_frames(sd_handle* h, uint32_t* dst, int n, int reset, void* stream);
/* after the frames 0..n-1 of the last calls have been dealt with (recomputed on an engine without the fp16 limit): their clamps, and those of
 * the rows no frame owns (the zero-padded rows of a partial last GEMM tile, which write no output), leave the global counter of
 * sd_saturation_count; the per-frame counts are zeroed.  Enqueued on `stream`, no synchronisation.  SD_ERR_INVALID for n < 1 or
 * n > max_batch. */
sd_status sd_saturation_settle(sd_handle* h, int n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SEMDEPTH_H */
