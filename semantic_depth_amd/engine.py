"""Engine: one libsemdepth handle + the torch-allocated device arenas it runs in.

PyTorch-ROCm is plumbing here (device memory, streams); every op on the hot path is a HIP kernel behind the
C ABI of include/semdepth.h.  One Engine per process / per GPU.
"""
from __future__ import annotations

import ctypes as C
import os
import warnings
from dataclasses import dataclass, asdict

import numpy as np
import torch

from . import _lib as L
from . import recompute as RC

RW_DTYPE = np.dtype([("width", "<f8"), ("x_left", "<f4"), ("x_right", "<f4"), ("left_pt", "<f4", 3), ("right_pt", "<f4", 3),
                     ("found", "<i4"), ("n_road", "<i4"), ("n_zcut", "<i4"), ("n_mad_y", "<i4"), ("n_mad_x", "<i4"),
                     ("n_plane", "<i4"), ("n_sor", "<i4"), ("n_ror", "<i4"), ("plane", "<f8", 4)])
assert RW_DTYPE.itemsize == C.sizeof(L.sd_rw_result)
F2F_DTYPE = np.dtype([("dist", "<f8"), ("left_pt", "<f8", 3), ("right_pt", "<f8", 3), ("plane_left", "<f8", 4), ("plane_right", "<f8", 4),
                      ("counts", "<i4", 7), ("ok", "<i4")])
assert F2F_DTYPE.itemsize == C.sizeof(L.sd_f2f_result)
# the depth profile's records (sd_rw_depth_result, sd_f2f_depth_result): one per (frame, depth)
RWP_DTYPE = np.dtype([("width", "<f8"), ("x_left", "<f4"), ("x_right", "<f4"), ("left_pt", "<f4", 3), ("right_pt", "<f4", 3),
                      ("found", "<i4"), ("n_window", "<i4")])
assert RWP_DTYPE.itemsize == C.sizeof(L.sd_rw_depth_result) == 48
F2FP_DTYPE = np.dtype([("dist", "<f8"), ("left_pt", "<f8", 3), ("right_pt", "<f8", 3), ("ok", "<i4"), ("reserved", "<i4")])
assert F2FP_DTYPE.itemsize == C.sizeof(L.sd_f2f_depth_result) == 64
# the box of the cloud that enters a plane fit (sd_plane_box): what the plane lattices of the scene files are laid over
BOX_DTYPE = np.dtype([("lo_a", "<f4"), ("hi_a", "<f4"), ("lo_b", "<f4"), ("hi_b", "<f4"), ("n", "<i4"), ("pad", "<i4")])
assert BOX_DTYPE.itemsize == 24


@dataclass
class RoadWidthParams:
    """literals of the reference's road chain, semantic_depth.py:206-259 (defaults = the reference's)."""
    depth: float = 10.0
    z_cut: float = 7.0
    mad_y: float = 15.0
    mad_x: float = 2.0
    plane_thr: float = 5.0
    sor_k: int = 10
    sor_ratio: float = 0.5
    ror_n: int = 80
    ror_r: float = 0.5
    window: float = 0.05
    depth_offset: float = 0.02
    use_o3d: bool = True

    def to_c(self) -> L.sd_rw_params:
        d = asdict(self)
        d["use_o3d"] = int(d["use_o3d"])
        return L.sd_rw_params(**d)


@dataclass
class FenceParams:
    """literals of the reference's fence chain, semantic_depth.py:273-334 (defaults = the reference's)."""
    depth: float = 10.0
    mad_y: float = 5.0
    z_max: float = 35.0
    mad_left: float = 5.0
    mad_right: float = 1.0
    plane_thr: float = 1.0

    def to_c(self) -> L.sd_f2f_params:
        return L.sd_f2f_params(**asdict(self))


@dataclass
class Camera:
    """DepthFrame intrinsics (semantic_depth.py:592-607) + disparity multiplier (:109,:145 / seq:105)."""
    cx: float
    cy: float
    f: float
    b: float
    disp_mult: float


def sweep_chunks(B: int, T: int, max_batch: int) -> list:
    """the trial ranges [(t0, t1), ...] Engine.sweep_tail walks: max(1, max_batch // B) trials per chunk, so that no chain call
    carries more than max_batch (trial, frame) slots.  B > max_batch is refused: a chain call takes at most max_batch slots."""
    if B < 1 or T < 1:
        raise ValueError(f"a sweep needs at least one frame and one trial, got B={B}, T={T}")
    if B > max_batch:
        raise ValueError(f"a sweep of B={B} frames needs max_batch >= B, the engine has {max_batch}")
    per = max(1, max_batch // B)
    return [(t0, min(T, t0 + per)) for t0 in range(0, T, per)]


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _raw(a):
    """the address of a ctypes array"""
    return C.cast(a, C.c_void_p)


class RangeError(L.SdError):
    """an activation left the range of the fp16 planes of a reduced-plane engine (|v| > 65504, or NaN): the outputs of the call are not the
    network's.  The fp32 reference has no such failure mode; run these weights with precision='bf16x3' or 'f32'."""


# engines whose activation planes are fp16: their conv epilogues clamp at +-65504 and count what they clamped
FP16_PLANE_ENGINES = ("f16x2", "f16x2x2", "mixed", "plan")


class Engine:
    def __init__(self, H: int, W: int, max_batch: int = 1, encoder: str = "resnet50", device: int = 0, precision: str = "f32",
                 plan: tuple[str, str] | None = None, range_check: bool = True, on_range: str = "raise", small_batch: bool | int = False,
                 arena_fill: int = 0):
        """precision: 'f32' (exact f32 MFMA), 'bf16x3' (fp32-grade on the bf16 MFMA: every f32 operand as three bf16 planes that sum to it
        exactly, 6 MFMA products), 'f16x2' (fp32-grade on 3 fp16 MFMA products: activations as fp16 hi + 2^11-scaled lo planes, weights as fp16 hi + lo of
        w * 2^k, k per layer), 'bf16x2' (3 bf16 MFMA products, ~1e-5), 'mixed' (monodepth on 2 fp16 products), 'plan' (per-layer
        choice; ``plan`` = (fcn8s layers, monodepth layers) that run the 2-product scheme, default = the calibrated built-in).
        range_check (engines with fp16 planes): a value beyond the fp16 range is an ERROR -- every network call enqueues an 8-byte read of
        the device's saturation counter behind its launches and the next call / ``check_range()`` raises RangeError on a non-zero count
        (no device synchronisation on the launch path).
        on_range: 'raise' (default): as above.  'recompute' (engines with fp16 planes): every network call (fcn8s_forward,
        monodepth_forward, process_batch) reads and resets the per-frame clamp counts behind its launches (one small synchronising read),
        recomputes the frames that left the fp16 range on a companion 'bf16x3' engine (built on first need, same geometry, encoder,
        device and weights) and splices their results into the outputs on the device; the other frames keep this engine's results.
        ``last_recomputed`` lists the frames of the last call that were recomputed.
        small_batch ('f16x2' only; sd_set_small_batch): the GEMM layers whose full pass has at most an eighth as many 256 x 256 output tiles as the chip has
        CUs (fc6 / fc7 and the res5 1x1 layers of a max_batch = 1 handle; sd_small_batch_split is the rule) run split along K, S slices per tile plus a reduce launch
        (``small_batch_plan()`` lists layer -> S).  Their sums are formed in another order, so the last bits differ from the default
        handle's; on a handle where no layer qualifies nothing changes.  The 'bf16x3' companion of on_range='recompute' is not split.
        small_batch=2 (level 2; True means 1): level 1 plus the under-filled 3x3 direct conv layers (conv4_x / conv5_x of FCN-8s, the deep encoder and iconv layers
        of monodepth; sd_small_batch_split_direct is the rule) split along their input-channel chunks, S contiguous chunk ranges per tile plus a reduce launch
        that applies the layer's epilogue, fused 2x2 pool included.  ``small_batch_level`` holds the level, ``small_batch`` stays its truth value.
        arena_fill: the byte (0..255) the three arenas hold when they are bound; 0 is the zero fill this class has always used.  Results must not depend on
        it (sd_bind_memory: "the arenas may hold anything"): tests/test_gpu_state_independence.py binds NaN- and huge-valued arenas through it."""
        RC.check_mode(on_range)
        if not 0 <= int(arena_fill) <= 255:
            raise ValueError("arena_fill is a byte, 0..255")
        if int(small_batch) not in (0, 1, 2):
            raise ValueError("small_batch is False / True or the level 0, 1 or 2")
        if small_batch and precision not in ("f16x2", "f16x2x2"):
            raise ValueError("small_batch needs precision='f16x2'")
        if not torch.cuda.is_available():
            raise RuntimeError("semantic_depth_amd.Engine needs a GPU (MI355X); there is no CPU fallback")
        self.lib = L.load()
        self.H, self.W, self.max_batch, self.encoder = H, W, max_batch, encoder
        self.device = torch.device("cuda", device)
        torch.cuda.set_device(self.device)
        h = C.c_void_p()
        enc = {"vgg": L.SD_ENC_VGG, "resnet50": L.SD_ENC_RESNET50}[encoder]
        self.precision = precision
        prec = {"f32": L.SD_PREC_F32, "bf16x2": L.SD_PREC_BF16X2, "mixed": L.SD_PREC_MIXED, "plan": L.SD_PREC_PLAN, "bf16x3": L.SD_PREC_BF16X3,
                "f16x2": L.SD_PREC_F16X2, "f16x2x2": L.SD_PREC_F16X2}[precision]      # ("f16x2x2": VERDICT r4's name for the same engine)
        if plan is not None:
            if precision != "plan":
                raise ValueError("an explicit plan needs precision='plan'")
            st = self.lib.sd_create_with_plan(C.byref(h), device, H, W, max_batch, enc, plan[0].encode(), plan[1].encode())
        else:
            st = self.lib.sd_create(C.byref(h), device, H, W, max_batch, enc, prec)
        L.check(self.lib, None, st, f"sd_create(H={H}, W={W}, max_batch={max_batch}, {encoder}, {precision}, plan={plan})")
        self.h = h
        self.small_batch, self.small_batch_level = bool(small_batch), int(small_batch)
        if small_batch:
            L.check(self.lib, h, self.lib.sd_set_small_batch(h, int(small_batch)), "sd_set_small_batch")
        fw, mw, ws = C.c_size_t(), C.c_size_t(), C.c_size_t()
        L.check(self.lib, h, self.lib.sd_query_memory(h, C.byref(fw), C.byref(mw), C.byref(ws)), "sd_query_memory")
        self.bytes = dict(fcn_weights=fw.value, mono_weights=mw.value, workspace=ws.value)
        # arenas: torch owns the memory; every byte holds arena_fill when they are bound (0: never-written padding is finite)
        self._wf = torch.full((fw.value,), int(arena_fill), dtype=torch.uint8, device=self.device)
        self._wm = torch.full((mw.value,), int(arena_fill), dtype=torch.uint8, device=self.device)
        self._ws = torch.full((ws.value,), int(arena_fill), dtype=torch.uint8, device=self.device)
        L.check(self.lib, h, self.lib.sd_bind_memory(h, _ptr(self._wf), _ptr(self._wm), _ptr(self._ws)), "sd_bind_memory")
        self.cap = H * W
        self.pass_frames = int(self.lib.sd_pass_frames(h))        # frames per network pass, as the handle latched it at sd_create
        self._sat_host = torch.zeros(1, dtype=torch.int64).pin_memory() if (range_check and precision in FP16_PLANE_ENGINES) else None
        self._sat_pending = None                                  # event behind the counter read in flight
        # per-frame clamp counts (sd_saturation_frames): pinned uint32 [max_batch]
        self._satf_host = torch.zeros(max_batch, dtype=torch.int32).pin_memory()
        self.on_range = on_range                                  # (as asked: the registry keys of api.py use it)
        self._recompute = on_range == "recompute" and precision in FP16_PLANE_ENGINES      # (the other engines cannot leave the range)
        self._kept_weights: dict = {}                             # recompute: net -> {name: the caller's host array} for the companion
        self._companion = None
        self._warned = False
        self.last_recomputed: list[int] = []
        self._profile_ws: dict = {}                               # road_width_profile: (B, cap, D) -> workspace tensor

    def close(self):
        if getattr(self, "_companion", None) is not None:
            self._companion.close()
            self._companion = None
        if getattr(self, "h", None):
            torch.cuda.synchronize(self.device)
            self.lib.sd_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ weights
    def weight_table(self, net: int):
        out = {}
        name = C.create_string_buffer(64)
        shape = (C.c_int64 * 4)()
        rank = C.c_int()
        for i in range(self.lib.sd_weight_count(self.h, net)):
            L.check(self.lib, self.h, self.lib.sd_weight_info(self.h, net, i, name, shape, C.byref(rank)), "sd_weight_info")
            out[name.value.decode()] = tuple(shape[j] for j in range(rank.value))
        return out

    def load_weights(self, net: int, weights: dict):
        for name, arr in weights.items():
            a = np.ascontiguousarray(arr, dtype=np.float32)
            shape = (C.c_int64 * 4)(*a.shape)
            st = self.lib.sd_load_weight(self.h, net, name.encode(), a.ctypes.data_as(C.c_void_p), shape, a.ndim)
            L.check(self.lib, self.h, st, f"sd_load_weight({name})")
        if self._recompute:
            self._kept_weights.setdefault(net, {}).update(weights)
            if self._companion is not None:
                self._companion.load_weights(net, weights)

    # ------------------------------------------------------------------ fp16 range guard
    def _resolve_range(self, block: bool):
        ev = self._sat_pending
        if ev is None:
            return
        if block:
            ev.synchronize()
        elif not ev.query():
            return
        self._sat_pending = None
        n = int(self._sat_host[0])
        if n:
            raise RangeError(f"{n} activation values left the fp16 range (+-65504) of the '{self.precision}' engine's planes since the arenas were bound: "
                             "the outputs are not the network's.  Use precision='bf16x3' or 'f32' for these weights (Engine.saturation_count(reset=True) clears the count)")

    def _post_range_check(self):
        """behind the launches of a network call: raise for a finished counter read, then (if none is in flight) enqueue the next one"""
        if self._sat_host is None:
            return
        self._resolve_range(block=False)
        if self._sat_pending is None:
            L.check(self.lib, self.h, self.lib.sd_saturation_count_async(self.h, C.c_void_p(self._sat_host.data_ptr()), self._stream()),
                    "sd_saturation_count_async")
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self.device))
            self._sat_pending = ev

    def check_range(self):
        """wait for the work enqueued so far and raise RangeError if any conv epilogue had to clamp a value to the fp16 range (no-op for the
        engines without fp16 planes).  The api classes call it where they bring results to the host."""
        if self._sat_host is None:
            return
        self._sat_pending = None
        self._post_range_check()
        self._resolve_range(block=True)

    def _frame_counts(self, n: int, reset: bool) -> np.ndarray:
        """clamp counts of frames 0..n-1 of the calls since the last reset (sd_saturation_frames; synchronises the stream)"""
        L.check(self.lib, self.h, self.lib.sd_saturation_frames(self.h, C.c_void_p(self._satf_host.data_ptr()), int(n), int(reset), self._stream()),
                "sd_saturation_frames")
        torch.cuda.current_stream(self.device).synchronize()
        return self._satf_host[:n].numpy().view(np.uint32).copy()

    def saturated_frames(self, reset: bool = False, n: int | None = None) -> np.ndarray:
        """bool [n]: which frames of the batch (position in the caller's batch; a monodepth frame's fliplr copy counts toward the frame)
        had a value clamped to the fp16 range since the arenas were bound / the last reset (synchronises).  ``n`` defaults to max_batch.
        The engines without fp16 planes report no frame."""
        return self._frame_counts(self.max_batch if n is None else n, reset) > 0

    def _companion_engine(self) -> "Engine":
        if self._companion is None:
            comp = Engine(self.H, self.W, self.max_batch, self.encoder, self.device.index or 0, precision="bf16x3")
            for net, w in self._kept_weights.items():
                comp.load_weights(net, w)
            self._companion = comp
        return self._companion

    def _settle(self, frames: torch.Tensor, out, rerun):
        """behind the launches of a network call: 'raise' mode -> the counter read of _post_range_check; 'recompute' mode -> read the
        per-frame counts, rerun(companion, flagged frames), splice its results over those frames of ``out`` and settle the counters"""
        if self._recompute:
            B = frames.shape[0]
            counts = self._frame_counts(B, reset=False)
            idx = RC.flagged_frames(counts)
            self.last_recomputed = idx
            if idx:
                sel = torch.tensor(idx, dtype=torch.int64, device=self.device)
                sub = rerun(self._companion_engine(), frames.index_select(0, sel).contiguous())
                out = RC.splice(out, sub, sel)
                if not self._warned:
                    self._warned = True
                    warnings.warn(f"frames {idx} left the fp16 range of the '{self.precision}' engine and were recomputed on 'bf16x3' "
                                  "(further recomputes of this engine are listed in Engine.last_recomputed only)", RuntimeWarning, stacklevel=3)
            # every clamp of this call is now dealt with: those of the recomputed frames, and those of the zero-padded GEMM rows that no
            # frame owns and nothing reads -- both leave the global counter (on the stream), so check_range stays quiet
            L.check(self.lib, self.h, self.lib.sd_saturation_settle(self.h, B, self._stream()), "sd_saturation_settle")
        self._post_range_check()
        return out

    # ------------------------------------------------------------------ operators
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _frames(self, frames):
        assert frames.dtype == torch.uint8 and frames.is_cuda and frames.is_contiguous()
        assert tuple(frames.shape[1:]) == (self.H, self.W, 3), frames.shape
        return frames.shape[0]

    def fcn8s_forward(self, frames: torch.Tensor, want_logits: bool = False):
        out = self._fcn8s(frames, want_logits)
        return self._settle(frames, out, lambda e, f: e.fcn8s_forward(f, want_logits))

    def _fcn8s(self, frames: torch.Tensor, want_logits: bool = False):
        B = self._frames(frames)
        dev = self.device
        logits = torch.empty((B, self.H, self.W, 3), dtype=torch.float32, device=dev) if want_logits else None
        road = torch.empty((B, self.H, self.W), dtype=torch.uint8, device=dev)
        fence = torch.empty_like(road)
        amax = torch.empty_like(road)
        st = self.lib.sd_fcn8s_forward(self.h, _ptr(frames), B, _ptr(logits), _ptr(road), _ptr(fence), _ptr(amax), self._stream())
        L.check(self.lib, self.h, st, "sd_fcn8s_forward")
        return dict(logits=logits, road=road, fence=fence, argmax=amax)

    def monodepth_forward(self, frames: torch.Tensor, want_raw: bool = False, post_process: bool = True):
        """post_process=False: leave the flip-pair post-processing to fuse_from_raw (one pass); returns None (B <= 32 frames).
        In 'recompute' mode the raw pair in the arena cannot be spliced: post_process=False is refused there (process_batch does it)."""
        if not post_process:
            if self._recompute:
                raise ValueError("monodepth_forward(post_process=False) leaves the disparity in the arena, where on_range='recompute' cannot "
                                 "splice it: use post_process=True or process_batch")
            self._mono(frames, False, False)
            self._post_range_check()
            return None
        out = self._mono(frames, want_raw, True)
        return self._settle(frames, out, lambda e, f: e.monodepth_forward(f, want_raw))

    def _mono(self, frames: torch.Tensor, want_raw: bool, post_process: bool):
        B = self._frames(frames)
        if not post_process:
            st = self.lib.sd_monodepth_forward(self.h, _ptr(frames), B, None, None, self._stream())
            L.check(self.lib, self.h, st, "sd_monodepth_forward")
            return None
        pp = torch.empty((B, self.H, self.W), dtype=torch.float32, device=self.device)
        raw = torch.empty((B, 2, self.H, self.W), dtype=torch.float32, device=self.device) if want_raw else None
        st = self.lib.sd_monodepth_forward(self.h, _ptr(frames), B, _ptr(pp), _ptr(raw), self._stream())
        L.check(self.lib, self.h, st, "sd_monodepth_forward")
        return (pp, raw) if want_raw else pp

    def resize_cubic(self, frames: torch.Tensor, out_h: int | None = None, out_w: int | None = None) -> torch.Tensor:
        """cv2.resize(frame, (out_w, out_h), interpolation=cv2.INTER_CUBIC) for u8 [B,h,w,C] device frames (semantic_depth.py:111)"""
        out_h, out_w = out_h or self.H, out_w or self.W
        assert frames.dtype == torch.uint8 and frames.is_cuda and frames.is_contiguous() and frames.dim() == 4
        B, sh, sw, ch = frames.shape
        out = torch.empty((B, out_h, out_w, ch), dtype=torch.uint8, device=self.device)
        st = self.lib.sd_resize_cubic_u8(self.h, _ptr(frames), B, sh, sw, ch, _ptr(out), out_h, out_w, self._stream())
        L.check(self.lib, self.h, st, "sd_resize_cubic_u8")
        return out

    def resize_pil(self, frames: torch.Tensor, out_h: int | None = None, out_w: int | None = None, channels: int | None = None,
                   pixel_stride: int | None = None, reverse: bool = False) -> torch.Tensor:
        """scipy.misc.imresize(frame, (out_h, out_w)) of the FCN test mode (fcn8s/fcn.py:408,412) = PIL.Image.resize((out_w, out_h), BILINEAR)
        for u8 [B,h,w,S] (or [B,h,w], S = 1) device frames, bit for bit (sd_resize_pil_bilinear_u8) -> u8 [B,out_h,out_w,channels].
        ``pixel_stride`` (default S) bytes lie between pixels and ``channels`` (1 or 3, default S) of them are taken: channel 0 of a
        reader's [B,h,w,3] label frame is resampled in place with channels=1.  ``reverse`` stores the channels in reverse order (the
        readers deliver BGR, the test mode feeds RGB).  Two launches on the current stream, no synchronisation; the workspace (the windows
        and the uint8 intermediate between the passes) is a torch allocation."""
        out_h, out_w = out_h or self.H, out_w or self.W
        assert frames.dtype == torch.uint8 and frames.is_cuda and frames.is_contiguous() and frames.dim() in (3, 4)
        B, sh, sw = (int(v) for v in frames.shape[:3])
        S = int(frames.shape[3]) if frames.dim() == 4 else 1
        pixel_stride = pixel_stride or S
        channels = channels or S
        if pixel_stride != S:
            raise ValueError(f"resize_pil: pixel_stride {pixel_stride} is not the frames' last extent {S}")
        need = C.c_size_t()
        st = self.lib.sd_resize_pil_workspace(B, sh, sw, out_h, out_w, channels, C.byref(need))
        L.check(self.lib, None, st, f"sd_resize_pil_workspace({B}, {sh}x{sw} -> {out_h}x{out_w}, channels={channels})")
        out = torch.empty((B, out_h, out_w, channels), dtype=torch.uint8, device=self.device)
        ws = torch.empty((need.value,), dtype=torch.uint8, device=self.device)
        st = self.lib.sd_resize_pil_bilinear_u8(self.h, _ptr(frames), B, sh, sw, pixel_stride, channels, int(bool(reverse)), _ptr(out), out_h, out_w,
                                                _ptr(ws), need.value, self._stream())
        L.check(self.lib, self.h, st, "sd_resize_pil_bilinear_u8")
        return out

    def seg_confusion(self, pred: torch.Tensor, labels: torch.Tensor, table, out: torch.Tensor | None = None) -> torch.Tensor:
        """the state of tf.metrics.mean_iou per frame (sd_seg_confusion): ``pred`` u8 [B,h,w] (fcn8s_forward's argmax, 0..2) against
        ``labels`` u8 [B,h,w] label ids through ``table`` (256 bytes, label id -> class 0..2; evaluate.label_table) ADDED into ``out``
        int64 [B,10] (zeros when None): cells 0..8 are the 3 x 3 matrix [label class][predicted class], cell 9 counts the predictions
        above 2, which enter no cell of the matrix.  One launch on the current stream, no synchronisation."""
        for t in (pred, labels):
            assert t.dtype == torch.uint8 and t.is_cuda and t.is_contiguous() and t.dim() == 3, t.shape
        assert pred.shape == labels.shape, (pred.shape, labels.shape)
        B, h, w = (int(v) for v in pred.shape)
        tab = np.ascontiguousarray(table, dtype=np.uint8)
        if tab.shape != (256,):
            raise ValueError("seg_confusion: the table holds 256 bytes")
        if out is None:
            out = torch.zeros((B, L.SD_SEG_CELLS), dtype=torch.int64, device=self.device)
        assert out.dtype == torch.int64 and out.is_cuda and out.is_contiguous() and tuple(out.shape) == (B, L.SD_SEG_CELLS), out.shape
        st = self.lib.sd_seg_confusion(self.h, _ptr(pred), _ptr(labels), B, h, w, tab.ctypes.data_as(C.c_void_p), _ptr(out), self._stream())
        L.check(self.lib, self.h, st, "sd_seg_confusion")
        return out

    def jpeg_reconstruct(self, coef: torch.Tensor, descs, out: torch.Tensor | None = None) -> torch.Tensor:
        """the device half of the split JPEG route (sd_jpeg_reconstruct_bgr): ``coef`` int16 [B, stride] device tensor of quantised
        coefficients as sd_jpeg_decode_coefficients / sd_decode_files_jpeg_coef lay them out, ``descs`` a ctypes array of B
        _lib.sd_jpeg_frame_desc -> u8 [B,h,w,3] BGR after the EXIF orientation, the bytes of frame_io.decode_jpeg.  Two kernels per eight
        frames on the current stream, no synchronisation; the workspace (the padded component planes) is a torch allocation."""
        assert coef.dtype == torch.int16 and coef.is_cuda and coef.is_contiguous() and coef.dim() == 2
        B = coef.shape[0]
        if B < 1 or len(descs) < B:
            raise ValueError("jpeg_reconstruct: one descriptor per frame")
        h, w = descs[0].oriented_size()
        if any(descs[i].oriented_size() != (h, w) for i in range(B)):
            raise ValueError("jpeg_reconstruct: the frames of a batch share one size after the orientation")
        if out is None:
            out = torch.empty((B, h, w, 3), dtype=torch.uint8, device=self.device)
        assert out.dtype == torch.uint8 and out.is_cuda and out.is_contiguous() and tuple(out.shape) == (B, h, w, 3)
        need = C.c_size_t()
        st = self.lib.sd_jpeg_reconstruct_workspace(descs, B, C.byref(need))
        L.check(self.lib, None, st, "sd_jpeg_reconstruct_workspace")
        ws = torch.empty((max(need.value, 16),), dtype=torch.uint8, device=self.device)
        st = self.lib.sd_jpeg_reconstruct_bgr(self.h, _ptr(coef), coef.shape[1] * 2, descs, B, _ptr(out), h * w * 3, _ptr(ws), need.value,
                                              self._stream())
        L.check(self.lib, self.h, st, "sd_jpeg_reconstruct_bgr")
        return out

    def png_reconstruct(self, rows: torch.Tensor, descs, out: torch.Tensor | None = None, status: torch.Tensor | None = None):
        """the device half of the split PNG route (sd_png_reconstruct_bgr): ``rows`` u8 [B, frame_stride] device tensor of the frames'
        filtered scanlines as sd_png_inflate_rows / sd_inflate_files_png lay them out (frame_stride a multiple of 16 that holds the
        widest frame's rows rounded up to 16), ``descs`` a HOST ctypes array of B _lib.sd_png_frame_desc of one height x width ->
        (frames u8 [B,h,w,3] BGR, status int32 [B]) device tensors: the bytes of frame_io.decode_png, and a non-zero status word for a
        palette frame with an index beyond its palette (such pixels take entry 0).  One kernel, one workgroup per frame, on the current
        stream, no synchronisation: a pinned ``descs`` must stay unchanged until the stream has passed the call."""
        assert rows.dtype == torch.uint8 and rows.is_cuda and rows.is_contiguous() and rows.dim() == 2
        B = rows.shape[0]
        if B < 1 or len(descs) < B:
            raise ValueError("png_reconstruct: one descriptor per frame")
        h, w = descs[0].height, descs[0].width
        if any((descs[i].height, descs[i].width) != (h, w) for i in range(B)):
            raise ValueError("png_reconstruct: the frames of a batch share one size")
        if out is None:
            out = torch.empty((B, h, w, 3), dtype=torch.uint8, device=self.device)
        if status is None:
            status = torch.empty((B,), dtype=torch.int32, device=self.device)
        assert out.dtype == torch.uint8 and out.is_cuda and out.is_contiguous() and tuple(out.shape) == (B, h, w, 3)
        assert status.dtype == torch.int32 and status.is_cuda and status.is_contiguous() and status.numel() >= B
        need = C.c_size_t()
        st = self.lib.sd_png_reconstruct_workspace(B, C.byref(need))
        L.check(self.lib, None, st, "sd_png_reconstruct_workspace")
        ws = torch.empty((need.value,), dtype=torch.uint8, device=self.device)
        st = self.lib.sd_png_reconstruct_bgr(self.h, _ptr(rows), rows.shape[1], descs, B, h, w, _ptr(out), h * w * 3, _ptr(status), _ptr(ws),
                                             need.value, self._stream())
        L.check(self.lib, self.h, st, "sd_png_reconstruct_bgr")
        return out, status

    def jpeg_entropy_decode(self, scan: torch.Tensor, descs, frames, tables, intervals, interval_stride: int, coef_stride: int | None = None,
                            out: torch.Tensor | None = None, status: torch.Tensor | None = None):
        """the device half of the entropy JPEG route (sd_jpeg_entropy_decode): ``scan`` u8 [B, byte_stride] device tensor of the frames'
        scan bytes (byte_stride a multiple of 16) plus the plan records of sd_jpeg_entropy_plan / sd_plan_files_jpeg_entropy -- ``descs``
        B _lib.sd_jpeg_frame_desc, ``frames`` B _lib.sd_jpeg_entropy_frame, ``tables`` B * 8 _lib.sd_jpeg_huff_table, ``intervals``
        B * interval_stride _lib.sd_jpeg_interval, all HOST ctypes arrays -> (coef int16 [B, coef_stride], status int32 [B]) device
        tensors: the coefficients sd_jpeg_decode_coefficients writes for every eligible frame (Engine.jpeg_reconstruct takes them as they
        are) and a non-zero status word for a frame whose stream was refused; ineligible frames keep what ``out`` held.  One lane per
        restart interval, on the current stream, no synchronisation: the host arrays must stay unchanged until the stream has passed
        the call when they are pinned.  ``coef_stride`` (int16 elements, a multiple of 8) defaults to the largest frame's need."""
        assert scan.dtype == torch.uint8 and scan.is_cuda and scan.is_contiguous() and scan.dim() == 2
        B = scan.shape[0]
        if B < 1 or len(descs) < B or len(frames) < B:
            raise ValueError("jpeg_entropy_decode: one descriptor and one record per frame")
        if coef_stride is None:
            coef_stride = out.shape[1] if out is not None else max(-(-descs[i].coef_elems() // 8) * 8 for i in range(B))
        if out is None:
            out = torch.empty((B, coef_stride), dtype=torch.int16, device=self.device)
        if status is None:
            status = torch.empty((B,), dtype=torch.int32, device=self.device)
        assert out.dtype == torch.int16 and out.is_cuda and out.is_contiguous() and tuple(out.shape) == (B, coef_stride)
        assert status.dtype == torch.int32 and status.is_cuda and status.is_contiguous() and status.numel() >= B
        need = C.c_size_t()
        st = self.lib.sd_jpeg_entropy_workspace(B, interval_stride, C.byref(need))
        L.check(self.lib, None, st, "sd_jpeg_entropy_workspace")
        ws = torch.empty((need.value,), dtype=torch.uint8, device=self.device)
        st = self.lib.sd_jpeg_entropy_decode(self.h, _ptr(scan), scan.shape[1], _raw(descs), _raw(frames), _raw(intervals), interval_stride,
                                             _raw(tables), B, _ptr(out), coef_stride * 2, _ptr(status), _ptr(ws), need.value, self._stream())
        L.check(self.lib, self.h, st, "sd_jpeg_entropy_decode")
        return out, status

    def jpeg_sync_decode(self, clean: torch.Tensor, descs, frames, tables, intervals, interval_stride: int, subseq_bytes: int,
                         coef_stride: int | None = None, out: torch.Tensor | None = None, status: torch.Tensor | None = None):
        """the device half of the sync JPEG route (sd_jpeg_sync_decode): ``clean`` u8 [B, byte_stride] device tensor of the frames' clean
        streams (byte_stride a multiple of 16) plus the plan records of sd_jpeg_sync_plan / sd_plan_files_jpeg_sync at ``subseq_bytes``
        -- ``descs`` B _lib.sd_jpeg_frame_desc, ``frames`` B _lib.sd_jpeg_sync_frame, ``tables`` B * 8 _lib.sd_jpeg_huff_table,
        ``intervals`` B * interval_stride _lib.sd_jpeg_sync_interval, all HOST ctypes arrays -> (coef int16 [B, coef_stride], status
        int32 [B]) device tensors: the coefficients sd_jpeg_decode_coefficients writes for every eligible frame whose status word is 0
        (1..4: the stream was refused; 5: the pieces did not synchronise; 6: the bits ran out -- the host decoder decides those
        frames); ineligible frames keep what ``out`` held.  A lane per piece of subseq_bytes, files without DRI included, on the current
        stream, no synchronisation: the host arrays must stay unchanged until the stream has passed the call when they are pinned."""
        assert clean.dtype == torch.uint8 and clean.is_cuda and clean.is_contiguous() and clean.dim() == 2
        B = clean.shape[0]
        if B < 1 or len(descs) < B or len(frames) < B:
            raise ValueError("jpeg_sync_decode: one descriptor and one record per frame")
        if coef_stride is None:
            coef_stride = out.shape[1] if out is not None else max(-(-descs[i].coef_elems() // 8) * 8 for i in range(B))
        if out is None:
            out = torch.empty((B, coef_stride), dtype=torch.int16, device=self.device)
        if status is None:
            status = torch.empty((B,), dtype=torch.int32, device=self.device)
        assert out.dtype == torch.int16 and out.is_cuda and out.is_contiguous() and tuple(out.shape) == (B, coef_stride)
        assert status.dtype == torch.int32 and status.is_cuda and status.is_contiguous() and status.numel() >= B
        most = max([1] + [frames[i].n_pieces for i in range(B) if frames[i].eligible])
        need = C.c_size_t()
        st = self.lib.sd_jpeg_sync_workspace(B, interval_stride, most, C.byref(need))
        L.check(self.lib, None, st, "sd_jpeg_sync_workspace")
        ws = torch.empty((need.value,), dtype=torch.uint8, device=self.device)
        st = self.lib.sd_jpeg_sync_decode(self.h, _ptr(clean), clean.shape[1], _raw(descs), _raw(frames), _raw(intervals), interval_stride,
                                          _raw(tables), B, subseq_bytes, _ptr(out), coef_stride * 2, _ptr(status), _ptr(ws), need.value,
                                          self._stream())
        L.check(self.lib, self.h, st, "sd_jpeg_sync_decode")
        return out, status

    def compose_result_frames(self, frames: torch.Tensor, road: torch.Tensor, fence: torch.Tensor, records: torch.Tensor, out_h: int, out_w: int,
                              road_color=(128, 64, 128), fence_color=(190, 153, 153), alpha: int = 64, out: torch.Tensor | None = None) -> torch.Tensor:
        """the sequence tool's result image (semantic_depth_cityscapes_sequence.py:303-336) for B device frames in one launch
        (sd_compose_result_frames): PIL paste of the road, then the fence colour on the network-size u8 [B,h,w,3] ``frames`` where the
        u8 [B,h,w] masks are set, INTER_CUBIC resize to (out_h, out_w), the 25 % grey banner on frames whose record (u8 [B,104] device
        buffer of road_width) has found != 0.  Colours are in the frames' channel order; semantic_depth.py:565 pastes (160,10,10) on fences."""
        assert frames.dtype == torch.uint8 and frames.is_cuda and frames.is_contiguous() and frames.dim() == 4 and frames.shape[3] == 3
        B, sh, sw = frames.shape[:3]
        for m in (road, fence):
            assert m.dtype == torch.uint8 and m.is_cuda and m.is_contiguous() and tuple(m.shape) == (B, sh, sw), m.shape
        assert records.dtype == torch.uint8 and records.is_cuda and records.is_contiguous() and tuple(records.shape) == (B, RW_DTYPE.itemsize)
        if out is None:
            out = torch.empty((B, out_h, out_w, 3), dtype=torch.uint8, device=self.device)
        assert out.dtype == torch.uint8 and out.is_cuda and out.is_contiguous() and tuple(out.shape) == (B, out_h, out_w, 3), out.shape
        rc, fc = (C.c_uint8 * 3)(*road_color), (C.c_uint8 * 3)(*fence_color)
        st = self.lib.sd_compose_result_frames(self.h, _ptr(frames), _ptr(road), _ptr(fence), _ptr(records), B, sh, sw, rc, fc, int(alpha),
                                               _ptr(out), out_h, out_w, self._stream())
        L.check(self.lib, self.h, st, "sd_compose_result_frames")
        return out

    def draw_result_text(self, images: torch.Tensor, records: torch.Tensor, depth: float) -> torch.Tensor:
        """the text of the sequence tool's result images (seq:303-336: "At 10.00 m depth:", the two distances to the road's ends and "Road's
        width: 4.41 m", or the green "Cannot compute ..." line) drawn IN PLACE into u8 [B,h,w,3] device ``images`` (compose_result_frames'
        output) from ``records`` u8 [B,104] (sd_rw_result), read on the device; ``depth`` is formatted here as "{:.2f}".  The strokes are the
        project's own font and raster rule (include/semdepth.h; not cv2.putText's pixels), the same pixels outputs.draw_text paints for
        overlay_items_sequence's items.  Two launches on the current stream, no synchronisation; the workspace is a torch allocation.
        Returns ``images``."""
        assert images.dtype == torch.uint8 and images.is_cuda and images.is_contiguous() and images.dim() == 4 and images.shape[3] == 3
        B, h, w = (int(v) for v in images.shape[:3])
        assert records.dtype == torch.uint8 and records.is_cuda and records.is_contiguous() and tuple(records.shape) == (B, RW_DTYPE.itemsize)
        need = self.lib.sd_text_workspace_bytes(B)
        ws = torch.empty((max(need, 16),), dtype=torch.uint8, device=self.device)
        st = self.lib.sd_text_draw_rw(self.h, _ptr(images), B, h, w, _ptr(records), "{:.2f}".format(depth).encode(), _ptr(ws), need, self._stream())
        L.check(self.lib, self.h, st, "sd_text_draw_rw")
        return images

    def draw_result_lines(self, images: torch.Tensor, records: torch.Tensor, cams, lines, f2f: torch.Tensor | None = None,
                          profile: torch.Tensor | None = None, f2f_profile: torch.Tensor | None = None, clip_top: int = 0):
        """the measurement lines of the result images (seq:330-333, the print_line_on_image calls the reference never wrote) drawn IN PLACE
        into u8 [B,h,w,3] device ``images`` (compose_result_frames' output): the road-width line of ``records`` u8 [B,104], the fence line of
        ``f2f`` u8 [B,152] (sd_f2f_result; None: none) and -- with ``profile`` u8 [B,D,48] (road_width_profile) -- the road's left and right
        edge along the profile and a rung per depth, the fence rungs with ``f2f_profile`` u8 [B,D,64]; all read on the device.  ``cams``: the
        frames' Camera at the network size (this engine's H x W); ``lines``: an outputs.OverlayLines; rows above ``clip_top`` are never
        painted.  The rule is the project's own (include/semdepth.h; not cv2.line's pixels), the same pixels outputs.draw_lines paints for
        outputs.overlay_segments' segments.  Two launches on the current stream, no synchronisation; the workspace is a torch allocation.
        Returns (``images``, ``flags`` i32 [B]; bit 0: a segment of the frame was skipped because an end point does not project)."""
        assert images.dtype == torch.uint8 and images.is_cuda and images.is_contiguous() and images.dim() == 4 and images.shape[3] == 3
        B, h, w = (int(v) for v in images.shape[:3])
        assert records.dtype == torch.uint8 and records.is_cuda and records.is_contiguous() and tuple(records.shape) == (B, RW_DTYPE.itemsize)
        cams = list(cams)
        if len(cams) != B:
            raise ValueError(f"draw_result_lines: {len(cams)} cameras for {B} frames")
        D = 0
        if profile is not None:
            D = int(profile.shape[1])
            assert profile.dtype == torch.uint8 and profile.is_cuda and profile.is_contiguous() and tuple(profile.shape) == (B, D, RWP_DTYPE.itemsize)
        if f2f is not None:
            assert f2f.dtype == torch.uint8 and f2f.is_cuda and f2f.is_contiguous() and tuple(f2f.shape) == (B, F2F_DTYPE.itemsize)
        if f2f_profile is not None:
            if profile is None:
                raise ValueError("draw_result_lines: f2f_profile needs profile")
            assert f2f_profile.dtype == torch.uint8 and f2f_profile.is_cuda and f2f_profile.is_contiguous() and \
                tuple(f2f_profile.shape) == (B, D, F2FP_DTYPE.itemsize)
        carr = (L.sd_camera * B)(*[L.sd_camera(c.cx, c.cy, c.f, c.b, c.disp_mult) for c in cams])
        style = lines.struct(clip_top)
        flags = torch.empty((B,), dtype=torch.int32, device=self.device)
        need = self.lib.sd_overlay_workspace_bytes(B, D)
        ws = torch.empty((max(need, 16),), dtype=torch.uint8, device=self.device)
        st = self.lib.sd_overlay_draw(self.h, _ptr(images), B, h, w, self.H, self.W, carr, _ptr(records), _ptr(f2f), _ptr(profile) if D else None,
                                      _ptr(f2f_profile) if D else None, D, C.byref(style), _ptr(flags), _ptr(ws), need, self._stream())
        L.check(self.lib, self.h, st, "sd_overlay_draw")
        return images, flags

    def encode_png(self, images: torch.Tensor):
        """the device half of the result-image writer (sd_png_encode_bgr): u8 [B,h,w,3] BGR device ``images`` -> (``streams`` u8 [B,stride],
        ``sizes`` i64 [B]) device tensors: frame b's complete zlib stream (Paeth rows, run matches, one dynamic-Huffman block per 32 KiB chunk;
        include/semdepth.h) is ``streams[b, :sizes[b]]``, the bytes behind it are not written.  outputs.write_png_streams wraps the streams in
        PNG chunks.  Three launches on the current stream, no synchronisation; the workspace is a torch allocation."""
        assert images.dtype == torch.uint8 and images.is_cuda and images.is_contiguous() and images.dim() == 4 and images.shape[3] == 3
        B, h, w = (int(v) for v in images.shape[:3])
        need, stride = C.c_size_t(), C.c_size_t()
        st = self.lib.sd_png_encode_workspace(B, h, w, C.byref(need), C.byref(stride))
        L.check(self.lib, None, st, "sd_png_encode_workspace")
        streams = torch.empty((B, stride.value), dtype=torch.uint8, device=self.device)
        sizes = torch.empty((B,), dtype=torch.int64, device=self.device)
        ws = torch.empty((need.value,), dtype=torch.uint8, device=self.device)
        st = self.lib.sd_png_encode_bgr(self.h, _ptr(images), h * w * 3, B, h, w, _ptr(streams), stride.value, _ptr(sizes), _ptr(ws), need.value,
                                        self._stream())
        L.check(self.lib, self.h, st, "sd_png_encode_bgr")
        return streams, sizes

    def encode_jpeg(self, images: torch.Tensor, quality: int = 90, stream_stride: int | None = None):
        """the device half of the result video (sd_jpeg_encode_bgr): u8 [n,h,w,3] BGR device ``images`` -> (``streams`` u8 [n,stride], ``sizes``
        i64 [n], ``flags`` i32 [n]) device tensors: frame b's complete baseline JPEG file (4:2:0, the Annex K tables at the IJG ``quality``
        1..100, one restart interval per MCU row; include/semdepth.h) is ``streams[b, :sizes[b]]``, the bytes behind it are not written.
        ``stream_stride`` None: the bound for any content (about 10 bytes per pixel); a smaller one is legal: a frame whose file would pass it
        has size 0 and flag 1 (encode it with outputs.encode_jpeg_host).  Three launches on the current stream, no synchronisation; the
        workspace is a torch allocation."""
        assert images.dtype == torch.uint8 and images.is_cuda and images.is_contiguous() and images.dim() == 4 and images.shape[3] == 3
        B, h, w = (int(v) for v in images.shape[:3])
        need, bound = C.c_size_t(), C.c_size_t()
        st = self.lib.sd_jpeg_encode_workspace(B, h, w, C.byref(need), C.byref(bound))
        L.check(self.lib, None, st, "sd_jpeg_encode_workspace")
        stride = bound.value if stream_stride is None else int(stream_stride)
        streams = torch.empty((B, stride), dtype=torch.uint8, device=self.device)
        sizes = torch.empty((B,), dtype=torch.int64, device=self.device)
        flags = torch.empty((B,), dtype=torch.int32, device=self.device)
        ws = torch.empty((need.value,), dtype=torch.uint8, device=self.device)
        st = self.lib.sd_jpeg_encode_bgr(self.h, _ptr(images), h * w * 3, B, h, w, int(quality), _ptr(streams), stride, _ptr(sizes), _ptr(flags),
                                         _ptr(ws), need.value, self._stream())
        L.check(self.lib, self.h, st, "sd_jpeg_encode_bgr")
        return streams, sizes, flags

    def format_rw_ply(self, final: dict, records: torch.Tensor, capacity: int | None = None, out: torch.Tensor | None = None):
        """the device half of the road PLY writer (sd_ply_format_rw): ``final`` = process_batch(want_final=True)'s road_final (xyz f32 [B,cap,3],
        rgb u8 [B,cap,3], n i32 [B]) and ``records`` u8 [B,104] (sd_rw_result) -> (``text`` u8 [capacity], ``offsets`` i64 [B+1], ``flags`` i32 [B])
        device tensors: frame b's ``<name>_rw.ply`` is ``text[offsets[b]:offsets[b+1]]``, the bytes of outputs.rw_ply_bytes; the files are packed
        back to back and nothing at or behind ``offsets[B]`` is written.  flags[b] = 1: the frame holds a non-finite value or |v| >= 2^31 and
        was not formatted (write it through rw_ply_bytes); 2: its text would pass ``capacity``; both have size 0.
        ``capacity`` None: the bound for the clouds' ``cap`` dimension, B * (209 + (cap + 1001) * 69) bytes -- about 1.2 GB at B = 32 and
        512 x 1024 -- unless ``out`` (a u8 device tensor to write into) gives it; a smaller capacity is legal (flag 2).  Five launches on the
        current stream, no synchronisation; the workspace is a torch allocation."""
        xyz, rgb, n = final["xyz"], final.get("rgb"), final["n"]
        if rgb is None:
            raise ValueError("format_rw_ply needs the colours of the road cloud (final['rgb'] is None)")
        assert xyz.dtype == torch.float32 and xyz.is_cuda and xyz.is_contiguous() and xyz.dim() == 3 and xyz.shape[2] == 3
        B, cap = int(xyz.shape[0]), int(xyz.shape[1])
        assert rgb.dtype == torch.uint8 and rgb.is_cuda and rgb.is_contiguous() and tuple(rgb.shape) == (B, cap, 3)
        assert n.dtype == torch.int32 and n.is_cuda and n.is_contiguous() and tuple(n.shape) == (B,)
        assert records.dtype == torch.uint8 and records.is_cuda and records.is_contiguous() and tuple(records.shape) == (B, RW_DTYPE.itemsize)
        need, bound = C.c_size_t(), C.c_size_t()
        st = self.lib.sd_ply_format_workspace(B, cap, C.byref(need), C.byref(bound))
        L.check(self.lib, None, st, "sd_ply_format_workspace")
        if out is not None:
            assert out.dtype == torch.uint8 and out.is_cuda and out.is_contiguous() and out.dim() == 1
            capacity = int(out.numel()) if capacity is None else int(capacity)
            assert capacity <= out.numel()
        else:
            capacity = bound.value if capacity is None else int(capacity)
            out = torch.empty((max(capacity, 1),), dtype=torch.uint8, device=self.device)
        offsets = torch.empty((B + 1,), dtype=torch.int64, device=self.device)
        flags = torch.empty((B,), dtype=torch.int32, device=self.device)
        ws = torch.empty((need.value,), dtype=torch.uint8, device=self.device)
        st = self.lib.sd_ply_format_rw(self.h, _ptr(xyz), _ptr(rgb), _ptr(n), B, cap, _ptr(records), _ptr(out), capacity, _ptr(offsets), _ptr(flags),
                                       _ptr(ws), need.value, self._stream())
        L.check(self.lib, self.h, st, "sd_ply_format_rw")
        return out[:capacity], offsets, flags

    def format_scene_ply(self, final: dict, fence_final: dict | None, records: torch.Tensor, f2f: torch.Tensor | None, boxes: dict | None,
                         mask: int = L.SD_SCENE_ALL, lattice_cap: int = 1 << 18, capacity: int | None = None, out: torch.Tensor | None = None):
        """the device half of the scene PLY writer (sd_scene_format): ``final`` / ``fence_final`` = process_batch(want_final=True)'s
        road_final and fence_final (None with approach 'rw': the fence segments are absent), ``records`` u8 [B,104], ``f2f`` u8 [B,152] (None
        likewise) and ``boxes`` = process_batch(want_boxes=True)'s plane_boxes (None: no lattice) -> (``text`` u8 [capacity], ``offsets`` i64
        [B+1], ``flags`` i32 [B]) device tensors packed as format_rw_ply packs them; ``mask`` selects the segments (L.SD_SCENE_*): all eight
        for the scene file, ROAD for ``_ROAD.ply``, FENCE_L | FENCE_R for ``_FENCE.ply``.  The bytes are outputs.scene_ply_bytes'.
        flags[b] = 1: a non-finite or |v| >= 2^31 coordinate, a NaN box, a count outside its capacity (write the frame through
        scene_ply_bytes); 2: its text would pass ``capacity``; 3: a lattice has more than ``lattice_cap`` rows (both: sd_scene_format_host);
        all have size 0.  ``capacity`` None: the bound of the mask, B * (209 + rows * 69) with rows = cap + cap_fence + 3 lattice_cap + 2002 for all
        eight segments and only the selected ones' share otherwise, unless ``out`` gives it; a larger ``capacity`` is cut to that bound.
        Six launches on the current stream, no synchronisation; the workspace is a torch allocation."""
        xyz, rgb, n = final["xyz"], final.get("rgb"), final["n"]
        if rgb is None:
            raise ValueError("format_scene_ply needs the colours of the road cloud (final['rgb'] is None)")
        assert xyz.dtype == torch.float32 and xyz.is_cuda and xyz.is_contiguous() and xyz.dim() == 3 and xyz.shape[2] == 3
        B, cap = int(xyz.shape[0]), int(xyz.shape[1])
        assert rgb.dtype == torch.uint8 and rgb.is_cuda and rgb.is_contiguous() and tuple(rgb.shape) == (B, cap, 3)
        assert n.dtype == torch.int32 and n.is_cuda and n.is_contiguous() and tuple(n.shape) == (B,)
        assert records.dtype == torch.uint8 and records.is_cuda and records.is_contiguous() and tuple(records.shape) == (B, RW_DTYPE.itemsize)
        fence = [None] * 4
        cap_f = 0
        if fence_final is not None:
            if f2f is None or any(fence_final.get(k) is None for k in ("left_xyz", "left_rgb", "right_xyz", "right_rgb")):
                raise ValueError("format_scene_ply: the fence clouds need their colours and the f2f records")
            fence = [fence_final[k] for k in ("left_xyz", "left_rgb", "right_xyz", "right_rgb")]
            cap_f = int(fence[0].shape[1])
            for t, dt in zip(fence, (torch.float32, torch.uint8) * 2):
                assert t.dtype == dt and t.is_cuda and t.is_contiguous() and tuple(t.shape) == (B, cap_f, 3), t.shape
        if f2f is not None:
            assert f2f.dtype == torch.uint8 and f2f.is_cuda and f2f.is_contiguous() and tuple(f2f.shape) == (B, F2F_DTYPE.itemsize)
        rbox = fbox = None
        if boxes is not None:
            rbox, fbox = boxes.get("road"), boxes.get("fence")
            for t, shape in ((rbox, (B, BOX_DTYPE.itemsize)), (fbox, (B, 2, BOX_DTYPE.itemsize))):
                assert t is None or (t.dtype == torch.uint8 and t.is_cuda and t.is_contiguous() and tuple(t.shape) == shape), shape
        need, bound = C.c_size_t(), C.c_size_t()
        st = self.lib.sd_scene_workspace(B, cap, cap_f, int(lattice_cap), int(mask), C.byref(need), C.byref(bound))
        L.check(self.lib, None, st, "sd_scene_workspace")
        if out is not None:
            assert out.dtype == torch.uint8 and out.is_cuda and out.is_contiguous() and out.dim() == 1
            capacity = int(out.numel()) if capacity is None else int(capacity)
            assert capacity <= out.numel()
        else:
            # (never more than the mask's own bound: the _ROAD and _FENCE files, without lattices and lines, need a fraction of the scene file's)
            capacity = bound.value if capacity is None else min(int(capacity), bound.value)
            out = torch.empty((max(capacity, 1),), dtype=torch.uint8, device=self.device)
        offsets = torch.empty((B + 1,), dtype=torch.int64, device=self.device)
        flags = torch.empty((B,), dtype=torch.int32, device=self.device)
        ws = torch.empty((need.value,), dtype=torch.uint8, device=self.device)
        st = self.lib.sd_scene_format(self.h, _ptr(xyz), _ptr(rgb), _ptr(n), cap, _ptr(fence[0]), _ptr(fence[1]), _ptr(fence[2]), _ptr(fence[3]), cap_f,
                                      B, _ptr(records), _ptr(f2f), _ptr(rbox), _ptr(fbox), int(mask), int(lattice_cap), _ptr(out), capacity,
                                      _ptr(offsets), _ptr(flags), _ptr(ws), need.value, self._stream())
        L.check(self.lib, self.h, st, "sd_scene_format")
        return out[:capacity], offsets, flags

    def render_rw(self, final: dict, records: torch.Tensor, camera, out: torch.Tensor | None = None):
        """the rendered view of every frame's ``_rw.ply`` (sd_render_rw): ``final`` = process_batch(want_final=True)'s road_final (xyz f32
        [B,cap,3], rgb u8 [B,cap,3], n i32 [B]), ``records`` u8 [B,104] (sd_rw_result) and ``camera`` (outputs.RenderCamera) -> (``images`` u8
        [B,height,width,3] BGR, ``flags`` i32 [B]) device tensors: the n cloud points and, on a found frame, the 1001 points of the road-width
        line, behind the file's minimum-z filter, as z-buffered squares of ``camera.point_size`` pixels (the rule of include/semdepth.h; the
        bytes of outputs.render_rw, not Open3D's pixels).  flags[b] = 1: n[b] is outside 0..cap and the image is background only.  Five
        launches on the current stream, no synchronisation; the workspace (8 bytes per pixel per frame) is a torch allocation."""
        xyz, rgb, n = final["xyz"], final.get("rgb"), final["n"]
        if rgb is None:
            raise ValueError("render_rw needs the colours of the road cloud (final['rgb'] is None)")
        assert xyz.dtype == torch.float32 and xyz.is_cuda and xyz.is_contiguous() and xyz.dim() == 3 and xyz.shape[2] == 3
        B, cap = int(xyz.shape[0]), int(xyz.shape[1])
        assert rgb.dtype == torch.uint8 and rgb.is_cuda and rgb.is_contiguous() and tuple(rgb.shape) == (B, cap, 3)
        assert n.dtype == torch.int32 and n.is_cuda and n.is_contiguous() and tuple(n.shape) == (B,)
        assert records.dtype == torch.uint8 and records.is_cuda and records.is_contiguous() and tuple(records.shape) == (B, RW_DTYPE.itemsize)
        cam = camera.struct()
        need = C.c_size_t()
        st = self.lib.sd_render_workspace(B, cap, C.byref(cam), C.byref(need))
        L.check(self.lib, None, st, "sd_render_workspace")
        if out is None:
            out = torch.empty((B, cam.height, cam.width, 3), dtype=torch.uint8, device=self.device)
        assert out.dtype == torch.uint8 and out.is_cuda and out.is_contiguous() and tuple(out.shape) == (B, cam.height, cam.width, 3), out.shape
        flags = torch.empty((B,), dtype=torch.int32, device=self.device)
        ws = torch.empty((need.value,), dtype=torch.uint8, device=self.device)
        st = self.lib.sd_render_rw(self.h, _ptr(xyz), _ptr(rgb), _ptr(n), B, cap, _ptr(records), C.byref(cam), _ptr(out), _ptr(flags), _ptr(ws), need.value,
                                   self._stream())
        L.check(self.lib, self.h, st, "sd_render_rw")
        return out, flags

    def disparity_image(self, disp: torch.Tensor, out_h: int, out_w: int, cmap: str = "gray", mults=None, out: torch.Tensor | None = None):
        """DepthFrame.disp_to_image (semantic_depth.py:681-683: scipy.misc.imresize(disp, [h, w]) then plt.imsave(cmap=)) for f32
        [B,h,w] device ``disp`` (process_batch's ``disp_pp``) -> (``images`` u8 [B,out_h,out_w,3] BGR, ``flags`` i32 [B]) device tensors
        (sd_disp_image: the rule of include/semdepth.h, the bytes of outputs.disparity_image): per frame the map times ``mults[b]`` (host
        numbers, the frames' Camera.disp_mult; None: 1) is byte-scaled over its finite range, resampled with Pillow's bilinear filter,
        normalised over the range of the resized bytes and looked up in matplotlib's ``cmap`` table ("gray" or "plasma").  flags[b] = 1:
        frame b holds a non-finite value, which became byte 0.  ``out``: a contiguous u8 tensor of that shape to write into (any byte
        offset: a base that is not 4-byte aligned takes the byte-store form of the colour pass).  Five launches plus the resample's on the
        current stream, no synchronisation; the workspace is a torch allocation."""
        from .outputs import DISP_MAPS
        if cmap not in DISP_MAPS:
            raise ValueError(f"cmap must be 'gray' or 'plasma', got {cmap!r}")
        assert disp.dtype == torch.float32 and disp.is_cuda and disp.is_contiguous() and disp.dim() == 3, (disp.dtype, disp.shape)
        B, h, w = (int(v) for v in disp.shape)
        out_h, out_w = int(out_h), int(out_w)
        m = None
        if mults is not None:
            m = np.ascontiguousarray(mults, dtype=np.float32).reshape(-1)
            if m.shape != (B,):
                raise ValueError(f"disparity_image: {m.size} multipliers for {B} frames")
        need = C.c_size_t()
        st = self.lib.sd_disp_image_workspace(B, h, w, out_h, out_w, C.byref(need))
        L.check(self.lib, None, st, f"sd_disp_image_workspace({B}, {h}x{w} -> {out_h}x{out_w})")
        if out is None:
            out = torch.empty((B, out_h, out_w, 3), dtype=torch.uint8, device=self.device)
        assert out.dtype == torch.uint8 and out.is_cuda and out.is_contiguous() and tuple(out.shape) == (B, out_h, out_w, 3), out.shape
        flags = torch.empty((B,), dtype=torch.int32, device=self.device)
        ws = torch.empty((need.value,), dtype=torch.uint8, device=self.device)
        st = self.lib.sd_disp_image(self.h, _ptr(disp), None if m is None else m.ctypes.data_as(C.c_void_p), B, h, w, out_h, out_w,
                                    DISP_MAPS.index(cmap), _ptr(out), _ptr(flags), _ptr(ws), need.value, self._stream())
        L.check(self.lib, self.h, st, "sd_disp_image")
        return out, flags

    def post_process(self, disp_raw: torch.Tensor):
        B = disp_raw.shape[0]
        assert disp_raw.dtype == torch.float32 and tuple(disp_raw.shape[1:]) == (2, self.H, self.W) and disp_raw.is_contiguous()
        pp = torch.empty((B, self.H, self.W), dtype=torch.float32, device=self.device)
        L.check(self.lib, self.h, self.lib.sd_post_process(self.h, _ptr(disp_raw), B, _ptr(pp), self._stream()), "sd_post_process")
        return pp

    def fuse_backproject(self, disp_pp, road, fence, frames, cams, dense: bool = False, cap: int | None = None,
                         want_rgb: bool = True, want_fence: bool = True):
        B = disp_pp.shape[0]
        cap = cap or self.cap
        dev = self.device
        carr = (L.sd_camera * B)(*[L.sd_camera(c.cx, c.cy, c.f, c.b, c.disp_mult) for c in cams])
        out = {}
        out["dense"] = torch.empty((B, self.H, self.W, 3), dtype=torch.float32, device=dev) if dense else None
        if road is not None:
            out["road_xyz"] = torch.empty((B, cap, 3), dtype=torch.float32, device=dev)
            out["road_rgb"] = torch.empty((B, cap, 3), dtype=torch.uint8, device=dev) if (want_rgb and frames is not None) else None
            out["n_road"] = torch.empty((B,), dtype=torch.int32, device=dev)
        else:
            out["road_xyz"] = out["road_rgb"] = out["n_road"] = None
        if want_fence and fence is not None:
            out["fence_xyz"] = torch.empty((B, cap, 3), dtype=torch.float32, device=dev)
            out["fence_rgb"] = torch.empty((B, cap, 3), dtype=torch.uint8, device=dev) if (want_rgb and frames is not None) else None
            out["n_fence"] = torch.empty((B,), dtype=torch.int32, device=dev)
        else:
            out["fence_xyz"] = out["fence_rgb"] = out["n_fence"] = None
        st = self.lib.sd_fuse_backproject(self.h, _ptr(disp_pp), _ptr(road), _ptr(fence), _ptr(frames), carr, B, cap,
                                          _ptr(out["dense"]), _ptr(out["road_xyz"]), _ptr(out["road_rgb"]), _ptr(out["n_road"]),
                                          _ptr(out["fence_xyz"]), _ptr(out["fence_rgb"]), _ptr(out["n_fence"]), self._stream())
        L.check(self.lib, self.h, st, "sd_fuse_backproject")
        return out

    def fuse_from_raw(self, road, fence, frames, cams, disp_raw=None, cap: int | None = None, want_rgb: bool = True):
        """post-processing + back-projection + gather in ONE launch (sd_postprocess_fuse_backproject).  ``disp_raw`` None = the raw
        pair of the last monodepth_forward on this engine.  Returns the fuse dict plus 'disp_pp'."""
        B = road.shape[0]
        cap = cap or self.cap
        dev = self.device
        carr = (L.sd_camera * B)(*[L.sd_camera(c.cx, c.cy, c.f, c.b, c.disp_mult) for c in cams])
        out = dict(dense=None, disp_pp=torch.empty((B, self.H, self.W), dtype=torch.float32, device=dev))
        for k, m in (("road", road), ("fence", fence)):
            out[f"{k}_xyz"] = torch.empty((B, cap, 3), dtype=torch.float32, device=dev) if m is not None else None
            out[f"{k}_rgb"] = torch.empty((B, cap, 3), dtype=torch.uint8, device=dev) if (m is not None and want_rgb and frames is not None) else None
            out[f"n_{k}"] = torch.empty((B,), dtype=torch.int32, device=dev) if m is not None else None
        st = self.lib.sd_postprocess_fuse_backproject(self.h, _ptr(disp_raw), _ptr(out["disp_pp"]), _ptr(road), _ptr(fence), _ptr(frames), carr, B,
                                                      cap, _ptr(out["road_xyz"]), _ptr(out["road_rgb"]), _ptr(out["n_road"]),
                                                      _ptr(out["fence_xyz"]), _ptr(out["fence_rgb"]), _ptr(out["n_fence"]), self._stream())
        L.check(self.lib, self.h, st, "sd_postprocess_fuse_backproject")
        return out

    def _sweep_buffers(self, slots: int, B: int, T: int, cap: int, rgb: bool, fence_group: bool) -> dict:
        """the fuse dict of ``slots`` (trial, frame) slots plus the workspace of a T-trial launch over B frames"""
        dev = self.device
        out = dict(dense=None)
        for k, on in (("road", True), ("fence", fence_group)):
            out[f"{k}_xyz"] = torch.empty((slots, cap, 3), dtype=torch.float32, device=dev) if on else None
            out[f"{k}_rgb"] = torch.empty((slots, cap, 3), dtype=torch.uint8, device=dev) if (on and rgb) else None
            out[f"n_{k}"] = torch.empty((slots,), dtype=torch.int32, device=dev) if on else None
        nbytes = int(self.lib.sd_fuse_sweep_workspace(B, T, self.H, self.W))
        if nbytes == 0:
            raise ValueError(f"sd_fuse_sweep_workspace refuses B={B}, T={T} (T * B is at most 65535)")
        out["workspace"] = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        return out

    def _fuse_sweep_into(self, buf: dict, disp_pp, road, fence, frames, cams) -> dict:
        """one sd_fuse_backproject_sweep launch of len(cams) trials into the first T * B slots of ``buf`` (_sweep_buffers); returns views"""
        B, T = disp_pp.shape[0], len(cams)
        if any(len(row) != B for row in cams):
            raise ValueError(f"cams must be T lists of B={B} cameras")
        n = T * B
        cap = buf["road_xyz"].shape[1]
        if n > buf["road_xyz"].shape[0]:
            raise ValueError(f"{T} trials of {B} frames do not fit buffers of {buf['road_xyz'].shape[0]} slots")
        assert disp_pp.dtype == torch.float32 and disp_pp.is_contiguous() and tuple(disp_pp.shape) == (B, self.H, self.W), disp_pp.shape
        for m in (road, fence):
            assert m is None or (m.dtype == torch.uint8 and m.is_contiguous() and tuple(m.shape) == (B, self.H, self.W)), m.shape
        assert frames is None or self._frames(frames) == B
        carr = (L.sd_camera * n)(*[L.sd_camera(c.cx, c.cy, c.f, c.b, c.disp_mult) for row in cams for c in row])
        out = {k: (v[:n] if v is not None else None) for k, v in buf.items() if k != "workspace"}
        ws = buf["workspace"]
        st = self.lib.sd_fuse_backproject_sweep(self.h, _ptr(disp_pp), _ptr(road), _ptr(fence if out["fence_xyz"] is not None else None),
                                                _ptr(frames), carr, B, T, cap, _ptr(out["road_xyz"]), _ptr(out["road_rgb"]), _ptr(out["n_road"]),
                                                _ptr(out["fence_xyz"]), _ptr(out["fence_rgb"]), _ptr(out["n_fence"]), _ptr(ws), ws.numel(),
                                                self._stream())
        L.check(self.lib, self.h, st, "sd_fuse_backproject_sweep")
        return out

    def fuse_backproject_sweep(self, disp_pp, road, fence, frames, cams, cap: int | None = None, want_rgb: bool = True, want_fence: bool = True):
        """fuse_backproject for B frames under T trial cameras each, behind ONE compaction (sd_fuse_backproject_sweep): ``cams`` is a list
        of T lists of B Camera.  Returns the fuse dict with a leading T * B axis: slot t * B + b holds, bit for bit, what fuse_backproject
        gives frame b with cams[t][b]."""
        B, T = disp_pp.shape[0], len(cams)
        buf = self._sweep_buffers(T * B, B, T, cap or self.cap, want_rgb and frames is not None, want_fence and fence is not None)
        return self._fuse_sweep_into(buf, disp_pp, road, fence, frames, cams)

    def road_width(self, road_xyz, n_road, params: RoadWidthParams = RoadWidthParams(), want_final: bool = False, road_rgb=None,
                   boxes: torch.Tensor | None = None):
        """road chain (semantic_depth.py:203-259).  ``road_rgb`` (u8 [B,cap,3], optional): the colours the reference carries
        through every filter.  want_final: also return the denoised cloud -> (records, xyz, n) or, with colours,
        (records, xyz, rgb, n).  ``boxes`` (a device u8 [B,24] tensor to fill, optional): the sd_plane_box of the cloud that enters the
        plane fit (sd_road_width_boxes: one more launch, every other output bit-identical)."""
        B, cap = road_xyz.shape[0], road_xyz.shape[1]
        res = torch.empty((B, RW_DTYPE.itemsize), dtype=torch.uint8, device=self.device)    # (every byte of a record is written by the tail kernels)
        fin = torch.empty_like(road_xyz) if want_final else None
        frgb = torch.empty_like(road_rgb) if (want_final and road_rgb is not None) else None
        nfin = torch.empty((B,), dtype=torch.int32, device=self.device) if want_final else None
        prm = params.to_c()
        if boxes is None:
            st = self.lib.sd_road_width(self.h, _ptr(road_xyz), _ptr(road_rgb), _ptr(n_road), B, cap, C.byref(prm), _ptr(res), _ptr(fin),
                                        _ptr(frgb), _ptr(nfin), self._stream())
        else:
            assert boxes.dtype == torch.uint8 and boxes.is_cuda and boxes.is_contiguous() and tuple(boxes.shape) == (B, BOX_DTYPE.itemsize), boxes.shape
            st = self.lib.sd_road_width_boxes(self.h, _ptr(road_xyz), _ptr(road_rgb), _ptr(n_road), B, cap, C.byref(prm), _ptr(res), _ptr(fin),
                                              _ptr(frgb), _ptr(nfin), _ptr(boxes), self._stream())
        L.check(self.lib, self.h, st, "sd_road_width")
        if not want_final:
            return res
        return (res, fin, nfin) if road_rgb is None else (res, fin, frgb, nfin)

    def fence_to_fence(self, fence_xyz, n_fence, road_records: torch.Tensor, params: FenceParams = FenceParams(), fence_rgb=None,
                       want_clouds: bool = False, boxes: torch.Tensor | None = None):
        """fence chain + fence-to-fence distance (semantic_depth.py:273-334) for B frames; ``road_records`` is the device
        buffer returned by road_width (its plane is the road plane).  Returns a device buffer of sd_f2f_result; with
        want_clouds also the denoised left / right fence clouds (dict; sizes = counts[5], counts[6] of the records).
        ``boxes`` (a device u8 [B,2,24] tensor to fill, optional): the sd_plane_box of the left and the right cloud that enter their
        plane fits (sd_fence_to_fence_boxes: two more launches, every other output bit-identical)."""
        B, cap = fence_xyz.shape[0], fence_xyz.shape[1]
        res = torch.zeros((B, F2F_DTYPE.itemsize), dtype=torch.uint8, device=self.device)
        prm = params.to_c()
        cl = {k: None for k in ("left_xyz", "left_rgb", "right_xyz", "right_rgb")}
        if want_clouds:
            cl["left_xyz"], cl["right_xyz"] = torch.empty_like(fence_xyz), torch.empty_like(fence_xyz)
            if fence_rgb is not None:
                cl["left_rgb"], cl["right_rgb"] = torch.empty_like(fence_rgb), torch.empty_like(fence_rgb)
        if boxes is None:
            st = self.lib.sd_fence_to_fence(self.h, _ptr(fence_xyz), _ptr(fence_rgb), _ptr(n_fence), B, cap, _ptr(road_records), C.byref(prm),
                                            _ptr(res), _ptr(cl["left_xyz"]), _ptr(cl["left_rgb"]), _ptr(cl["right_xyz"]), _ptr(cl["right_rgb"]),
                                            self._stream())
        else:
            assert boxes.dtype == torch.uint8 and boxes.is_cuda and boxes.is_contiguous() and tuple(boxes.shape) == (B, 2, BOX_DTYPE.itemsize), boxes.shape
            st = self.lib.sd_fence_to_fence_boxes(self.h, _ptr(fence_xyz), _ptr(fence_rgb), _ptr(n_fence), B, cap, _ptr(road_records), C.byref(prm),
                                                  _ptr(res), _ptr(cl["left_xyz"]), _ptr(cl["left_rgb"]), _ptr(cl["right_xyz"]),
                                                  _ptr(cl["right_rgb"]), _ptr(boxes), self._stream())
        L.check(self.lib, self.h, st, "sd_fence_to_fence")
        return (res, cl) if want_clouds else res

    @staticmethod
    def _depth_array(depths):
        d = np.ascontiguousarray(np.asarray(depths, dtype=np.float64).reshape(-1))
        if not 1 <= d.size <= L.SD_PROFILE_MAX_DEPTHS:
            raise ValueError(f"a depth profile takes 1..{L.SD_PROFILE_MAX_DEPTHS} depths, got {d.size}")
        return d

    def road_width_profile(self, xyz: torch.Tensor, n: torch.Tensor, depths, params: RoadWidthParams = RoadWidthParams(),
                           out: torch.Tensor | None = None) -> torch.Tensor:
        """the road record at D depths from ONE cloud per frame (sd_road_width_profile): ``xyz`` f32 [B,cap,3] and ``n`` i32 [B] are any
        device cloud, normally road_width(want_final=True)'s denoised one; ``depths`` in any order, repeats allowed.  Returns a device u8
        [B, D, 48] buffer of sd_rw_depth_result: entry [b, i] holds the width, x_left, x_right, end points and found that road_width gives
        frame b with ``params.depth = depths[i]`` (window and depth_offset come from ``params``) plus n_window, the rows inside that
        window.  Two launches on the current stream, no synchronisation; the workspace is cached per (B, cap, D)."""
        assert xyz.dtype == torch.float32 and xyz.is_cuda and xyz.is_contiguous() and xyz.dim() == 3 and xyz.shape[2] == 3, xyz.shape
        B, cap = int(xyz.shape[0]), int(xyz.shape[1])
        assert n.dtype == torch.int32 and n.is_cuda and n.is_contiguous() and tuple(n.shape) == (B,)
        d = self._depth_array(depths)
        D = int(d.size)
        need = int(self.lib.sd_rw_profile_workspace(B, cap, D))
        if need == 0:
            raise ValueError(f"sd_rw_profile_workspace refuses B={B}, cap={cap}, D={D}")
        ws = self._profile_ws.get((B, cap, D))
        if ws is None:
            ws = self._profile_ws[(B, cap, D)] = torch.empty((need,), dtype=torch.uint8, device=self.device)
        if out is None:
            out = torch.empty((B, D, RWP_DTYPE.itemsize), dtype=torch.uint8, device=self.device)     # (every byte of a record is written)
        assert out.dtype == torch.uint8 and out.is_cuda and out.is_contiguous() and tuple(out.shape) == (B, D, RWP_DTYPE.itemsize), out.shape
        prm = params.to_c()
        st = self.lib.sd_road_width_profile(self.h, _ptr(xyz), _ptr(n), B, cap, d.ctypes.data_as(C.c_void_p), D, prm.window, prm.depth_offset,
                                            _ptr(out), _ptr(ws), need, self._stream())
        L.check(self.lib, self.h, st, "sd_road_width_profile")
        return out

    def f2f_profile(self, road_records: torch.Tensor, f2f_records: torch.Tensor, depths, out: torch.Tensor | None = None) -> torch.Tensor:
        """the fence-to-fence distance at D depths from ONE set of planes per frame (sd_f2f_profile): ``road_records`` u8 [B,104]
        (road_width) and ``f2f_records`` u8 [B,168] (fence_to_fence) device buffers -> device u8 [B, D, 64] of sd_f2f_depth_result:
        entry [b, i] holds the dist, points and ok fence_to_fence gives frame b with ``FenceParams(depth=depths[i])``.  One launch."""
        B = int(road_records.shape[0])
        for t, sz in ((road_records, RW_DTYPE.itemsize), (f2f_records, F2F_DTYPE.itemsize)):
            assert t.dtype == torch.uint8 and t.is_cuda and t.is_contiguous() and tuple(t.shape) == (B, sz), t.shape
        d = self._depth_array(depths)
        D = int(d.size)
        if out is None:
            out = torch.empty((B, D, F2FP_DTYPE.itemsize), dtype=torch.uint8, device=self.device)
        assert out.dtype == torch.uint8 and out.is_cuda and out.is_contiguous() and tuple(out.shape) == (B, D, F2FP_DTYPE.itemsize), out.shape
        st = self.lib.sd_f2f_profile(self.h, _ptr(road_records), _ptr(f2f_records), B, d.ctypes.data_as(C.c_void_p), D, _ptr(out), self._stream())
        L.check(self.lib, self.h, st, "sd_f2f_profile")
        return out

    @staticmethod
    def profile_records(res: torch.Tensor) -> np.ndarray:
        """device [B, D, 48] profile buffer -> structured array [B, D] (synchronises)."""
        return res.cpu().numpy().view(RWP_DTYPE).reshape(res.shape[0], res.shape[1])

    @staticmethod
    def f2f_profile_records(res: torch.Tensor) -> np.ndarray:
        return res.cpu().numpy().view(F2FP_DTYPE).reshape(res.shape[0], res.shape[1])

    @staticmethod
    def f2f_records(res: torch.Tensor) -> np.ndarray:
        return res.cpu().numpy().view(F2F_DTYPE).reshape(-1)

    @staticmethod
    def records(res: torch.Tensor) -> np.ndarray:
        """device record buffer -> numpy structured array (synchronises)."""
        return res.cpu().numpy().view(RW_DTYPE).reshape(-1)

    # ------------------------------------------------------------------ whole path
    def process_batch(self, frames: torch.Tensor, cams, params: RoadWidthParams = RoadWidthParams(), approach: str = "rw",
                      fence_params: FenceParams | None = None, colours: bool = True, want_final: bool = False, depths=None,
                      want_boxes: bool = False):
        """FrameProcessor.process_frame for B frames at once (semantic_depth.py:98-334; seq:117-298): seg + depth + fusion +
        road chain (+ the fence chain and fence-to-fence distance when ``approach == 'both'``, :273-334).  ``colours``: carry
        the RGB of every point through the filters like the reference does (they feed only the PLY outputs).
        ``depths`` (None = off): also the depth profile of every frame, from the one denoised cloud and the one set of planes the chains
        leave: ``profile`` u8 [B, D, 48] (road_width_profile) and, with approach 'both', ``f2f_profile`` u8 [B, D, 64] (f2f_profile).
        ``want_boxes``: also ``plane_boxes`` = dict(road u8 [B,24], fence u8 [B,2,24] or None without the fence chain): the sd_plane_box
        (BOX_DTYPE) of the cloud that entered each plane fit, which the plane lattices of the scene files are laid over (format_scene_ply).
        Returns device tensors: seg, disp_pp, fuse, records (sd_rw_result), f2f (sd_f2f_result or None) [, final clouds]."""
        if approach not in ("rw", "both"):
            raise ValueError("approach must be 'rw' or 'both' (semantic_depth.py:743-745)")
        cams = list(cams)
        if depths is not None:
            depths = self._depth_array(depths)
        out = self._process_batch(frames, cams, params, approach, fence_params, colours, want_final, depths, want_boxes)
        # ('recompute': ONE per-frame read behind both networks and the tail; the companion reruns the whole path on the flagged frames)
        return self._settle(frames, out, lambda e, f: e.process_batch(f, [cams[i] for i in self.last_recomputed], params, approach,
                                                                      fence_params, colours, want_final, depths, want_boxes))

    def _process_batch(self, frames, cams, params, approach, fence_params, colours, want_final, depths=None, want_boxes=False):
        seg = self._fcn8s(frames)
        if frames.shape[0] <= self.pass_frames:
            # the raw disparity pair stays in the activation arena: post-processing, back-projection and both gathers in ONE launch
            self._mono(frames, False, False)
            fz = self.fuse_from_raw(seg["road"], seg["fence"], frames, cams, want_rgb=colours)
            disp_pp = fz["disp_pp"]
        else:
            disp_pp = self._mono(frames, False, True)
            fz = self.fuse_backproject(disp_pp, seg["road"], seg["fence"], frames, cams, want_rgb=colours)
        out = dict(seg=seg, disp_pp=disp_pp, fuse=fz, f2f=None)
        # (a depth profile reads the denoised cloud: the chain runs once and keeps it, whether or not the caller asked for it)
        keep = want_final or depths is not None
        B = int(frames.shape[0])
        if want_boxes:
            out["plane_boxes"] = dict(road=torch.empty((B, BOX_DTYPE.itemsize), dtype=torch.uint8, device=self.device), fence=None)
        rw = self.road_width(fz["road_xyz"], fz["n_road"], params, want_final=keep, road_rgb=fz["road_rgb"] if colours else None,
                             boxes=out["plane_boxes"]["road"] if want_boxes else None)
        if keep:
            out["records"] = rw[0]
            if want_final:
                out["road_final"] = dict(xyz=rw[1], rgb=rw[2] if colours else None, n=rw[-1])
            if depths is not None:
                out["profile"] = self.road_width_profile(rw[1], rw[-1], depths, params)
        else:
            out["records"] = rw
        if approach == "both":
            fp = fence_params or FenceParams(depth=params.depth)
            if want_boxes:
                out["plane_boxes"]["fence"] = torch.empty((B, 2, BOX_DTYPE.itemsize), dtype=torch.uint8, device=self.device)
            f2 = self.fence_to_fence(fz["fence_xyz"], fz["n_fence"], out["records"], fp, fence_rgb=fz["fence_rgb"] if colours else None,
                                     want_clouds=want_final, boxes=out["plane_boxes"]["fence"] if want_boxes else None)
            if want_final:
                out["f2f"], out["fence_final"] = f2
            else:
                out["f2f"] = f2
            if depths is not None:
                out["f2f_profile"] = self.f2f_profile(out["records"], out["f2f"], depths)
        return out

    # ------------------------------------------------------------------ camera sweep (the calibration mode, semantic_depth.py:843-944)
    def sweep_tail(self, disp_pp, road, fence, frames, cams, params: RoadWidthParams = RoadWidthParams(), approach: str = "rw",
                   fence_params: FenceParams | None = None, colours: bool = False):
        """everything behind the networks for B frames under T trial cameras each (``cams``: T lists of B Camera): the trials are walked in
        chunks of max(1, max_batch // B) (sweep_chunks), per chunk one sweep launch, one road_width and -- approach == 'both' -- one
        fence_to_fence over the chunk's (trial, frame) slots, all into one set of buffers.  One RoadWidthParams / FenceParams per sweep.
        Returns dict(records, f2f): DEVICE buffers of T * B sd_rw_result / sd_f2f_result (f2f None unless 'both'), slot t * B + b, the bytes
        fuse_backproject + road_width + fence_to_fence give frame b with cams[t][b]; nothing is read back here (Engine.records /
        f2f_records read them, once)."""
        if approach not in ("rw", "both"):
            raise ValueError("approach must be 'rw' or 'both' (semantic_depth.py:743-745)")
        B, T = disp_pp.shape[0], len(cams)
        chunks = sweep_chunks(B, T, self.max_batch)
        per = chunks[0][1] - chunks[0][0]
        both = approach == "both"
        rgb = colours and frames is not None
        buf = self._sweep_buffers(per * B, B, per, self.cap, rgb, both)
        records = torch.empty((T * B, RW_DTYPE.itemsize), dtype=torch.uint8, device=self.device)
        f2f = torch.empty((T * B, F2F_DTYPE.itemsize), dtype=torch.uint8, device=self.device) if both else None
        fp = fence_params or FenceParams(depth=params.depth)
        for t0, t1 in chunks:
            fz = self._fuse_sweep_into(buf, disp_pp, road, fence, frames if rgb else None, cams[t0:t1])
            rw = self.road_width(fz["road_xyz"], fz["n_road"], params, road_rgb=fz["road_rgb"])
            records[t0 * B:t1 * B].copy_(rw)
            if both:
                f2f[t0 * B:t1 * B].copy_(self.fence_to_fence(fz["fence_xyz"], fz["n_fence"], rw, fp, fence_rgb=fz["fence_rgb"]))
        return dict(records=records, f2f=f2f)

    def camera_sweep(self, frames: torch.Tensor, cams, params: RoadWidthParams = RoadWidthParams(), approach: str = "rw",
                     fence_params: FenceParams | None = None, colours: bool = False):
        """process_batch for B frames under T trial cameras each with ONE pass of each network: the cameras enter the path only behind the
        networks, so fcn8s_forward and monodepth_forward run once (the public methods: on_range and the range check as everywhere else)
        and sweep_tail does the rest.  Returns dict(seg, disp_pp, records, f2f); records / f2f as sweep_tail."""
        seg = self.fcn8s_forward(frames)
        disp_pp = self.monodepth_forward(frames)
        tail = self.sweep_tail(disp_pp, seg["road"], seg["fence"], frames, cams, params, approach, fence_params, colours)
        return dict(seg=seg, disp_pp=disp_pp, records=tail["records"], f2f=tail["f2f"])

    # ------------------------------------------------------------------ introspection
    def net_tensor(self, net: int, name: str) -> torch.Tensor:
        shape = (C.c_int64 * 4)()
        L.check(self.lib, self.h, self.lib.sd_net_tensor(self.h, net, name.encode(), None, 0, shape, None), "sd_net_tensor")
        out = torch.empty(tuple(shape), dtype=torch.float32, device=self.device)
        L.check(self.lib, self.h, self.lib.sd_net_tensor(self.h, net, name.encode(), _ptr(out), out.numel(), shape, self._stream()),
                "sd_net_tensor")
        return out

    def profile(self, enable: bool):
        L.check(self.lib, self.h, self.lib.sd_profile(self.h, int(enable)), "sd_profile")

    def profile_read(self):
        """[{kernel, launches, ms, flops}] per conv-engine instantiation since the last read (synchronises)."""
        buf = (L.sd_profile_bucket * 32)()
        n = C.c_int()
        L.check(self.lib, self.h, self.lib.sd_profile_read(self.h, buf, 32, C.byref(n)), "sd_profile_read")
        return [dict(kernel=b.kernel.decode(), launches=int(b.launches), ms=float(b.ms), flops=float(b.flops), bytes=float(b.bytes)) for b in buf[:n.value]]

    def precision_plan(self) -> dict:
        """{net: (layers that run the 2-product fp16 scheme, their share of the net's FLOPs)} after the consistency closure"""
        out = {}
        for name, net in (("fcn8s", L.SD_NET_FCN8S), ("monodepth", L.SD_NET_MONODEPTH)):
            buf = C.create_string_buffer(8192)
            share = C.c_double()
            L.check(self.lib, self.h, self.lib.sd_precision_plan(self.h, net, buf, 8192, C.byref(share)), "sd_precision_plan")
            out[name] = ([s for s in buf.value.decode().split(",") if s], share.value)
        return out

    def small_batch_plan(self) -> dict:
        """{net: {layer: S}}: the GEMM layers a small_batch handle runs split along K -- at level 2 also the direct 3x3 layers it runs split along
        their chunk axis -- and their slice counts (empty without the switch, or where every layer's full pass already fills the chip)"""
        out = {}
        for name, net in (("fcn8s", L.SD_NET_FCN8S), ("monodepth", L.SD_NET_MONODEPTH)):
            buf = C.create_string_buffer(8192)
            L.check(self.lib, self.h, self.lib.sd_small_batch_plan(self.h, net, buf, 8192), "sd_small_batch_plan")
            out[name] = {k: int(v) for k, v in (s.rsplit(":", 1) for s in buf.value.decode().split(",") if s)}
        return out

    def conv_forms(self, net, frames=None) -> dict:
        """{conv layer: (kernel label, slices)} of ``net`` (L.SD_NET_*) in a call of ``frames`` frames (None: a full pass), in launch order: what the
        handle resolved, read without a device.  The label is the per-layer profile label; slices > 1 means the layer's reduce launch follows."""
        return L.conv_forms(self.lib, self.h, net, frames or 0)

    def saturation_count(self, reset: bool = False) -> int:
        """values the fp16 output formats of the reduced-precision plans had to clamp at +-65504 (or that were NaN) since the arenas were
        bound / the last reset (synchronises).  Non-zero = the plan does not fit these weights: use more products or precision='f32'."""
        n = C.c_uint64()
        L.check(self.lib, self.h, self.lib.sd_saturation_count(self.h, C.byref(n), int(reset)), "sd_saturation_count")
        if reset:
            self._sat_pending = None
        return int(n.value)

    def reserve_cus(self, n: int):
        """persistent conv launches leave ``n`` CUs free for work on another stream (the tail of the previous batch under the networks of this
        one: sd_set_reserved_cus); 0 = use every CU"""
        L.check(self.lib, self.h, self.lib.sd_set_reserved_cus(self.h, int(n)), "sd_set_reserved_cus")

    def flops_per_image(self, net: int) -> float:
        return float(self.lib.sd_net_flops_per_image(self.h, net))
