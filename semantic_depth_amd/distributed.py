"""Multi-GPU driver pieces: frames are independent, so they are sharded over ranks with no data-path
collective; the only exchange is one all_gather of the per-frame road-width records (104 B each).

One process per GPU, `torch.distributed` backend "nccl" (= RCCL over xGMI) on GPUs, "gloo" in the CPU tests.
This replaces the reference's strictly serial driver loop (semantic_depth_cityscapes_sequence.py:689-701).
"""
from __future__ import annotations

import numpy as np
import torch
import torch.distributed as dist

RECORD_BYTES = 104      # sizeof(sd_rw_result)
_gather_bufs: dict = {}  # (device, world, bmax) -> (send, recv): the staging buffers of gather_records, allocated once


def shard_range(n_frames: int, rank: int, world: int) -> tuple[int, int]:
    """contiguous block [lo, hi) of the frame list owned by ``rank`` (sizes differ by at most one)."""
    base, rem = divmod(n_frames, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def gather_records(local: torch.Tensor, n_frames: int | None = None, group=None, force_collective: bool = False) -> torch.Tensor:
    """all_gather of the per-frame record buffers.  ``local``: uint8 [B_local, 104] on the rank's device.
    Returns uint8 [n_frames, 104] in global frame order on every rank (shards may be ragged: padded to the
    largest shard for the collective, then trimmed).  ``force_collective``: run the collective in a group of one rank too
    (the single-GPU test of the RCCL call)."""
    assert local.dtype == torch.uint8 and local.dim() == 2 and local.shape[1] == RECORD_BYTES
    if not dist.is_initialized() or (dist.get_world_size(group) == 1 and not force_collective):
        return local
    world = dist.get_world_size(group)
    if n_frames is None:
        n_frames = local.shape[0] * world
    sizes = [shard_range(n_frames, r, world) for r in range(world)]
    bmax = max(hi - lo for lo, hi in sizes)
    # RCCL ("nccl") gathers device buffers in place; a gloo group (CPU tests, or ranks sharing one GPU) stages through the host
    via_host = local.is_cuda and dist.get_backend(group) == "gloo"
    dev = torch.device("cpu") if via_host else local.device
    even = all(hi - lo == bmax for lo, hi in sizes)
    if even and not via_host and local.shape[0] == bmax:
        # equal shards on the device (the benchmarked case): the local buffer IS the send buffer, the result is the receive buffer --
        # one collective, no staging copy, nothing allocated besides the [n_frames, 104] result the caller keeps
        out = torch.empty((world * bmax, RECORD_BYTES), dtype=torch.uint8, device=dev)
        dist.all_gather_into_tensor(out, local.contiguous(), group=group)
        return out
    key = (str(dev), world, bmax)
    if key not in _gather_bufs:                                    # ragged shards / host staging: buffers allocated once per geometry
        _gather_bufs[key] = (torch.zeros((bmax, RECORD_BYTES), dtype=torch.uint8, device=dev),
                             torch.empty((world * bmax, RECORD_BYTES), dtype=torch.uint8, device=dev))
    pad, out = _gather_bufs[key]
    pad[: local.shape[0]].copy_(local)
    dist.all_gather_into_tensor(out, pad, group=group)
    if even:
        return out.to(local.device, copy=True)
    parts = [out[r * bmax: r * bmax + (hi - lo)] for r, (lo, hi) in enumerate(sizes)]
    return torch.cat(parts, 0).to(local.device)


def records_view(buf: torch.Tensor) -> np.ndarray:
    from .engine import RW_DTYPE
    return buf.cpu().numpy().view(RW_DTYPE).reshape(-1)


def run_sequence(load_frames, n_frames: int, step, batch: int = 32, group=None, device=None) -> torch.Tensor:
    """The multi-frame driver: replaces the reference's strictly serial loop over ``sorted(glob(input_folder))``
    (semantic_depth_cityscapes_sequence.py:689-701; the frames carry no state between iterations).

    Rank r owns the contiguous block ``shard_range(n_frames, r, world)`` of the frame list, walks it in chunks of ``batch``
    frames and runs the whole per-frame path locally; the only exchange is ONE all_gather of the per-frame records at the end
    (104 B per frame, RCCL over xGMI on GPUs).

      load_frames(lo, hi) -> frames lo..hi-1 of the (sorted) list, in whatever form ``step`` consumes (e.g. u8 [n,h,w,3])
      step(frames, lo)    -> uint8 [n, 104] record buffer (sd_rw_result per frame) on this rank's device
                             (``make_engine_step`` wraps Engine.process_batch; the CPU tests pass a stub)

    Returns uint8 [n_frames, 104] in global frame order on every rank."""
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    rank = dist.get_rank(group) if dist.is_initialized() else 0
    lo, hi = shard_range(n_frames, rank, world)
    parts = []
    for a in range(lo, hi, batch):
        b = min(a + batch, hi)
        rec = step(load_frames(a, b), a)
        assert rec.dtype == torch.uint8 and tuple(rec.shape) == (b - a, RECORD_BYTES), (rec.dtype, rec.shape)
        parts.append(rec)
    if parts:
        local = torch.cat(parts, 0)
    else:
        local = torch.zeros((0, RECORD_BYTES), dtype=torch.uint8, device=device or "cpu")
    out = gather_records(local, n_frames, group)
    if getattr(step, "finish", None) is not None:
        step.finish()              # (make_engine_step: the engine's fp16 range check -- a violation is an error of the sequence)
    return out


def run_sequence_files(paths, step, batch: int = 32, group=None, device="cuda", workers: int = 0, outputs=None, jpeg: str = "host",
                       engine=None, png: str | None = None, ply: str | None = None, text: str | None = None, render=None, video=None,
                       png_in: str | None = None, disp: str | None = None, lines=None, scene=None) -> torch.Tensor:
    """run_sequence on FILES (semantic_depth_cityscapes_sequence.py:689-701 reads ``sorted(glob(input_folder))`` frame by frame): rank r
    decodes ONLY its shard of the sorted list -- frame_io.FrameFeeder: one native call per batch into pinned staging, upload one batch
    ahead, ``workers`` decode threads (default: this rank's share of the node's CPUs, frame_io.default_decode_workers) -- and hands every
    batch to ``step(frames_on_device, first_global_index)``; one all_gather of the records at the end.
    ``outputs`` (default: ``step.outputs``, set by ``make_engine_step(..., outputs=)``): an outputs.SequenceOutputs the step feeds; this
    rank writes the files of its shard only, and the manifest last -- 'ok', or 'range_error' / 'error' when the run raised (the files
    written before are then not valid outputs; the exception still propagates).
    ``jpeg`` ("host" | "device" | "device_entropy" | "device_sync") and ``engine`` go to the feeder: with "device" the JPEG frames are only entropy-decoded on
    the host and reconstructed on the GPU by ``engine`` (default: ``step.engine``, set by make_engine_step); with "device_entropy" the files
    that have restart intervals (one interleaved sequential scan, DRI > 0, nothing but stuffed bytes and the expected RSTk markers in it) are
    entropy-decoded on the GPU as well, the host only finds their markers, and every other JPEG falls back to the host decoder
    (FrameFeeder.entropy_fallback names them); with "device_sync" the files without restart intervals are entropy-decoded on the GPU too,
    in short pieces that find the decoder's state by themselves (FrameFeeder.sync_fallback names the frames that took the host decoder);
    the frames are the same bytes on all four.
    ``png_in`` (None = "host" | "device") is the feeder's ``png=`` (``png`` here already names the output writer): with "device" the PNG
    frames are only inflated on the host and their scanlines reconstructed on the GPU by ``engine``; the frames are the same bytes.
    ``png``, ``ply``, ``text``, ``render``, ``video``, ``disp``, ``lines``, ``scene`` (None = what the SequenceOutputs was built with) go to
    SequenceOutputs.configure before the first batch: its class docstring describes the choices, make_engine_step's what the step launches
    for each."""
    from .frame_io import FrameFeeder
    engine = engine if engine is not None else getattr(step, "engine", None)
    paths = sorted(paths)
    n_frames = len(paths)
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    rank = dist.get_rank(group) if dist.is_initialized() else 0
    lo, hi = shard_range(n_frames, rank, world)
    outputs = outputs if outputs is not None else getattr(step, "outputs", None)
    if outputs is not None:
        if len(outputs.names) != n_frames:
            raise ValueError(f"SequenceOutputs has {len(outputs.names)} names for {n_frames} frames")
        outputs.configure(png, ply, text, render, video, disp, lines, scene)
        outputs.begin(rank, world, lo, hi)
    try:
        parts = []
        if hi > lo:
            png_in = png_in if png_in is not None else "host"
            with FrameFeeder(paths[lo:hi], batch, device=device, workers=workers, jpeg=jpeg,
                             engine=engine if jpeg != "host" or png_in != "host" else None, png=png_in) as feeder:
                for frames, first in feeder:
                    rec = step(frames, lo + first)
                    assert rec.dtype == torch.uint8 and tuple(rec.shape) == (frames.shape[0], RECORD_BYTES), (rec.dtype, rec.shape)
                    parts.append(rec)
        local = torch.cat(parts, 0) if parts else torch.zeros((0, RECORD_BYTES), dtype=torch.uint8, device=device)
        out = gather_records(local, n_frames, group)
        if getattr(step, "finish", None) is not None:
            step.finish()
    except BaseException as e:
        if outputs is not None:
            from .engine import RangeError
            try:
                outputs.close("range_error" if isinstance(e, RangeError) else "error")
            except Exception:
                pass                      # (the run's own exception is the one reported)
        raise
    if outputs is not None:
        outputs.close("ok")
    return out


def make_engine_step(engine, camera_of, params=None, approach: str = "rw", outputs=None, on_range: str | None = None, png: str | None = None,
                     ply: str | None = None, text: str | None = None, render=None, video=None, depths=None, disp: str | None = None, lines=None,
                     scene=None):
    """``step`` for run_sequence on a real Engine: host or device u8 frames of any size -> (cubic resize to the network shape on
    the GPU, semantic_depth_cityscapes_sequence.py:123-130) -> Engine.process_batch -> record buffer.
    ``camera_of(global_frame_index) -> engine.Camera`` (the sequence tool: cx = 1048.64/4·s, cy = 519.277/4·s, disp_mult = 3800).
    ``outputs`` (outputs.SequenceOutputs, None = records only): also the sequence tool's files -- the batch goes to ``outputs.submit``
    (copies on a side stream, written on host threads); the records are the same either way.
    ``on_range`` (None = the engine's own mode; else it must match Engine(on_range=)): with 'recompute' the frames that left the fp16 range
    are recomputed on bf16x3 inside process_batch, so every batch's records, images and PLYs are final before gather_records and no rank
    raises from ``step.finish`` for them; ``step.recomputed`` (and the manifest's 'recomputed' names) lists those frames.
    ``png``, ``ply``, ``text``, ``render``, ``video``, ``disp``, ``lines``, ``scene`` (None = what ``outputs`` was built with) go to
    SequenceOutputs.configure, whose class docstring describes the choices.  ``depths`` (None likewise) becomes the outputs' profile, and
    must agree with one already chosen; without ``outputs`` it asks for nothing.
    What the step launches for them, all on its own stream and in this order (a choice that is off launches nothing):
      1. Engine.process_batch -- with want_final when PLYs, renders or scene files are on, so that it keeps the final road (and fence)
         clouds, with depths= for a profile (two launches behind the road chain, one more with approach 'both') and with want_boxes for
         scene= (one launch beside each plane fit).
      2. ply="device": Engine.format_rw_ply, the text of the ``_rw.ply`` files from the final clouds and the records.
         scene= on its "device" route: Engine.format_scene_ply once per file of Scene.files (six launches each; the ``_FENCE`` file only
         with approach 'both'), with Scene.capacity_per_frame bytes per frame of the batch as the text capacity.
      3. render=: Engine.render_rw behind that camera, then on the device PNG route Engine.encode_png of the renders.
      4. disp=: Engine.disparity_image of ``disp_pp`` at the original frame size with the frames' Camera.disp_mult as multipliers (five
         launches plus the resample's two), then on the device PNG route Engine.encode_png of the images.
      5. ``outputs.images`` or video=: Engine.compose_result_frames, the result images at the original frame size; then, on those images:
         a. lines=: Engine.draw_result_lines (two launches), right behind the compose launch;
         b. text="draw": Engine.draw_result_text, before anything reads the images;
         c. video route "device": Engine.encode_jpeg behind the text, with a stream stride of 1024 bytes plus half the raw image;
         d. ``outputs.images`` on the device PNG route: Engine.encode_png, last.
    The step hands ``outputs.submit`` exactly what those made, the flags of 4 and 5a among them, and with lines= the cameras, the network
    size and the fence records (SequenceOutputs.submit lists the keywords)."""
    from .engine import RoadWidthParams
    from .recompute import check_mode

    if on_range is not None and check_mode(on_range) != getattr(engine, "on_range", "raise"):
        raise ValueError(f"make_engine_step(on_range={on_range!r}) on an engine built with on_range={getattr(engine, 'on_range', 'raise')!r}")
    prm = params or RoadWidthParams()
    if outputs is not None:
        outputs.configure(png, ply, text, render, video, disp, lines, scene)
        if depths is not None:
            want = [float(d) for d in np.asarray(depths, dtype=np.float64).reshape(-1)]
            if outputs.profile is None:
                outputs.set_profile(want)
            elif list(outputs.profile) != want:
                raise ValueError("make_engine_step(depths=) disagrees with SequenceOutputs(profile=)")
    recomputed: list[int] = []

    def note(lo):
        idx = [lo + i for i in getattr(engine, "last_recomputed", [])]
        recomputed.extend(idx)
        if outputs is not None and idx:
            outputs.mark_recomputed(idx)

    def png_keyword(raw: str, streams: str, images):
        """a batch of images of one PNG family as its keyword of outputs.submit: ``raw``, or ``streams`` = Engine.encode_png of them on the
        device PNG route"""
        return {streams: engine.encode_png(images)} if outputs.device_png else {raw: images}

    def step(frames, lo):
        fr = frames if isinstance(frames, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(frames))
        fr = fr.to(engine.device, non_blocking=True)
        size = tuple(fr.shape[1:3])
        if size != (engine.H, engine.W):
            fr = engine.resize_cubic(fr)
        cams = [camera_of(lo + i) for i in range(fr.shape[0])]
        if outputs is None:
            rec = engine.process_batch(fr, cams, prm, approach=approach)["records"]
            note(lo)
            return rec
        # (depths=None is process_batch's default: no profile)
        want_scene = outputs.scene is not None
        out = engine.process_batch(fr, cams, prm, approach=approach, want_final=outputs.wants_final, depths=outputs.profile,
                                   **(dict(want_boxes=True) if want_scene else {}))
        note(lo)
        rec = out["records"]
        more = dict(images=None, final=out.get("road_final") if outputs.ply or want_scene else None)
        if outputs.profile is not None:
            more.update(profile=out["profile"], f2f_profile=out.get("f2f_profile"))
        if outputs.device_ply:                                     # the text of the PLY files
            more["ply_text"] = engine.format_rw_ply(out["road_final"], rec)
        if want_scene:                                             # the scene files: their inputs and, on the device route, their text
            from .outputs import SCENE_FILES
            sc = more["scene"] = dict(fence_final=out.get("fence_final"), f2f=out.get("f2f"), boxes=out["plane_boxes"], text=None)
            if outputs.device_scene:
                sc["text"] = {key: engine.format_scene_ply(out["road_final"], sc["fence_final"], rec, sc["f2f"], sc["boxes"], SCENE_FILES[key][1],
                                                           outputs.scene.lattice_cap, capacity=fr.shape[0] * outputs.scene.capacity_per_frame)
                              for key in outputs.scene.files if key != "fence" or sc["fence_final"] is not None}
        if outputs.render is not None:                             # the rendered clouds, behind the road chain
            more.update(png_keyword("renders", "render_streams", engine.render_rw(out["road_final"], rec, outputs.render)[0]))
        if outputs.disp is not None:                               # the disparity images, behind the networks
            dimg, more["disp_flags"] = engine.disparity_image(out["disp_pp"], size[0], size[1], outputs.disp, mults=[c.disp_mult for c in cams])
            more.update(png_keyword("disp_images", "disp_streams", dimg))
        if outputs.wants_composed:
            images = more["images"] = engine.compose_result_frames(fr, out["seg"]["road"], out["seg"]["fence"], rec, size[0], size[1],
                                                                   outputs.road_color, outputs.fence_color, outputs.alpha)
            if outputs.lines is not None:                          # the measurement lines, below the banner rows
                more["lines_flags"] = engine.draw_result_lines(images, rec, cams, outputs.lines, f2f=out.get("f2f"), profile=more.get("profile"),
                                                               f2f_profile=more.get("f2f_profile"), clip_top=int(0.25 * size[0]))[1]
            if outputs.text == "draw":                             # the banner text, before anything reads the images
                engine.draw_result_text(images, rec, outputs.depth)
            if outputs.device_video:                               # the frames of the video, behind the text
                more["video_streams"] = engine.encode_jpeg(images, outputs.video.quality, stream_stride=1024 + size[0] * size[1] * 3 // 2)
            if outputs.images:                                     # (the zlib streams last)
                more.update(png_keyword("images", "png_streams", images))
        if outputs.lines is not None:
            more.update(f2f=out.get("f2f"), cams=cams, net_size=(engine.H, engine.W))
        outputs.submit(lo, rec, size, **more)
        return rec

    # ('recompute': every clamp in a stored output is attributed to its frame and that frame recomputed, so the step has no verdict left
    # to give at the end -- no rank can raise alone here and leave the others in the all_gather)
    step.finish = None if getattr(engine, "on_range", "raise") == "recompute" else getattr(engine, "check_range", None)
    step.outputs = outputs
    step.engine = engine
    step.recomputed = recomputed
    return step
