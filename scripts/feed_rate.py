"""Input-stage feed rate (dev tool, run on the GPU box): can the host keep the GPU supplied at the benchmarked
frames/s?  Measures, for frames of one size (default: generated Cityscapes-sized 1024 x 2048 PNGs):
  decode    one thread per frame (whole decode; for JPEG also the coefficient-only half of the split route) and the native batch reader
  upload    pinned host -> HBM copy of decoded frames
  resize    Engine.resize_cubic to 512 x 1024 on the GPU
  feeder    frame_io.FrameFeeder end to end (decode + pinned upload + resize, one batch ahead), best and median of --repeats passes
    python scripts/feed_rate.py [--frames 256] [--workers N] [--format png|jpeg] [--jpeg host|device|device_entropy|device_sync] [--frames-dir DIR] [--out FILE]
                                [--size HxW] [--restart-rows N] [--encoder pillow|own] [--compare]
--frames-dir times the *.png / *.jpg files of a directory instead of generating frames (JPEG frames cannot be written here without
Pillow, which a GPU box may lack: write them elsewhere and ship them).  --jpeg device feeds through FrameFeeder(jpeg="device"): Huffman
decoding on the host, reconstruction on the GPU; the script passes jpeg= only then, so --jpeg host also runs in a tree that lacks the
split route (the parent commit's, for an A/B of the host route).  --jpeg device_entropy feeds through FrameFeeder(jpeg="device_entropy"):
the host only finds the restart markers, the GPU decodes the Huffman code; it needs files with restart intervals: --restart-rows 1 makes
Pillow write them, --encoder own writes the frames with the project's encoder (one interval per MCU row).  --jpeg device_sync feeds
through FrameFeeder(jpeg="device_sync"), which also takes files without restart intervals (--sync-piece: its piece length).  --compare
runs the four JPEG routes on the same files in one process, interleaved pass by pass, and adds the plans' single-thread times and the
HIP-event times of Engine.jpeg_entropy_decode (files with restart intervals only) and of Engine.jpeg_sync_decode at 64, 128 and 256 bytes
per piece.  Nothing is written unless --out is given.
"""
import argparse
import ctypes as C
import glob
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from semantic_depth_amd import _lib as L                    # noqa: E402
from semantic_depth_amd import frame_io, outputs            # noqa: E402
from semantic_depth_amd.engine import Engine                # noqa: E402


def _generate(td, n, fmt, size=(1024, 2048), restart_rows=0, encoder="pillow"):
    H, W = size
    rng = np.random.default_rng(0)
    # street-like content: smooth gradients + texture noise (PNG of pure noise does not compress; real frames do, ~2.2 MB each)
    yy, xx = np.mgrid[0:H, 0:W]
    paths = []
    for i in range(n):
        base = np.stack([(yy // 3 + xx // 5 + 7 * i) % 256, (xx // 4 + 3 * i) % 256, (yy // 2 + xx // 7) % 256], -1).astype(np.uint8)
        img = base ^ rng.integers(0, 4, (H, W, 3), dtype=np.uint8)
        if fmt == "png":
            paths.append(outputs.write_png(os.path.join(td, f"f{i:05d}.png"), img, level=6))
        else:
            p = os.path.join(td, f"f{i:05d}.jpg")
            if encoder == "own":
                open(p, "wb").write(outputs.encode_jpeg_host(img, 90))
            else:
                from PIL import Image
                kw = {"restart_marker_rows": restart_rows} if restart_rows else {}
                Image.fromarray(img[..., ::-1]).save(p, "JPEG", quality=90, subsampling=2, **kw)
            paths.append(p)
    return paths


def _single_thread_ms(paths, res):
    """whole decode of one frame on one thread; for JPEG files, where the library has the split route, also its host half alone"""
    lib = L.load()
    bufs = [open(p, "rb").read() for p in paths[:8]]
    frame_io.decode_image(bufs[0])
    t0 = time.perf_counter()
    for b in bufs:
        frame_io.decode_image(b)
    res["decode_ms_per_frame_1_thread"] = (time.perf_counter() - t0) / len(bufs) * 1e3
    if "sd_jpeg_decode_coefficients" in L.SIGNATURES and all(b[:2] == b"\xff\xd8" for b in bufs):
        d = L.sd_jpeg_frame_desc()
        assert lib.sd_jpeg_decode_coefficients(bufs[0], len(bufs[0]), None, 0, C.byref(d)) == L.SD_OK
        h, w = d.oriented_size()
        coef = np.empty(frame_io.FrameFeeder.coef_stride_bytes(h, w) // 2, np.int16)
        lib.sd_jpeg_decode_coefficients(bufs[0], len(bufs[0]), coef.ctypes.data_as(C.c_void_p), coef.nbytes, C.byref(d))
        t0 = time.perf_counter()
        for b in bufs:
            assert lib.sd_jpeg_decode_coefficients(b, len(b), coef.ctypes.data_as(C.c_void_p), coef.nbytes, C.byref(d)) == L.SD_OK
        res["coefficients_ms_per_frame_1_thread"] = (time.perf_counter() - t0) / len(bufs) * 1e3


def _kernel_ms_per_batch(eng, paths, workers, res):
    """HIP-event time of Engine.jpeg_reconstruct (the two kernels, four launches each for 32 frames) on one resident batch"""
    lib = L.load()
    n = min(32, len(paths))
    with open(paths[0], "rb") as f:
        h, w = frame_io.image_size(f.read())
    stride = frame_io.FrameFeeder.coef_stride_bytes(h, w)
    coef = torch.empty((n, stride // 2), dtype=torch.int16, pin_memory=True)
    descs = (L.sd_jpeg_frame_desc * n)()
    arr = (C.c_char_p * n)(*[os.fsencode(p) for p in paths[:n]])
    t0 = time.perf_counter()
    assert lib.sd_decode_files_jpeg_coef(arr, n, h, w, C.c_void_p(coef.data_ptr()), stride, descs, workers, None) == L.SD_OK
    res["coefficients_ms_per_batch_native"] = (time.perf_counter() - t0) * 1e3
    cdev = coef.cuda()
    out = eng.jpeg_reconstruct(cdev, descs)
    torch.cuda.synchronize()
    times = []
    for _ in range(7):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        eng.jpeg_reconstruct(cdev, descs, out=out)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    res["reconstruct_kernels_ms_per_batch"] = {"frames": n, "median": float(np.median(times)), "min": float(min(times)), "max": float(max(times))}


def _staged_plan(feeder, n):
    """the host half of the feeder's plan stage on its first n files -> (the plan, the stage's pinned staging, (h, w))"""
    stage, batch = feeder.stages[0], feeder._decode_into(0, 0, n)
    return batch.payload[stage.name], batch.pinned[stage.name], batch.size


def _entropy_measurements(eng, paths, workers, res):
    """the plan's host time per frame on one thread (against coefficients_ms_per_frame_1_thread on the same files) and the HIP-event
    time of Engine.jpeg_entropy_decode on one resident batch: the uploads of the records, the clearing kernel and the decoding kernel"""
    lib = L.load()
    bufs = [open(p, "rb").read() for p in paths[:8]]
    cap = 1 << 16
    d, fr = L.sd_jpeg_frame_desc(), L.sd_jpeg_entropy_frame()
    tables, iv = (L.sd_jpeg_huff_table * L.SD_JPEG_ENTROPY_TABLES)(), (L.sd_jpeg_interval * cap)()
    for rep in range(2):
        t0 = time.perf_counter()
        for b in bufs:
            assert lib.sd_jpeg_entropy_plan(b, len(b), C.byref(d), C.byref(fr), tables, iv, cap) == L.SD_OK and fr.eligible
        res["plan_ms_per_frame_1_thread"] = (time.perf_counter() - t0) / len(bufs) * 1e3
    res["intervals_per_frame"] = int(fr.n_intervals)
    n = min(32, len(paths))
    feeder = frame_io.FrameFeeder(paths[:n], n, "cuda", workers, jpeg="device_entropy", engine=eng)
    t0 = time.perf_counter()
    plan, staged, (h, w) = _staged_plan(feeder, n)
    res["plan_ms_per_batch_native"] = (time.perf_counter() - t0) * 1e3
    assert len(plan.eligible) == n
    used = max(int(plan.frames[i].scan_end - plan.frames[i].scan_begin) for i in range(n))
    used = -(-used // 16) * 16
    res["scan_bytes_per_frame_max"] = used
    sdev = staged.bytes[:n, :used].cuda()
    out = torch.empty((n, frame_io.FrameFeeder.coef_stride_bytes(h, w) // 2), dtype=torch.int16, device="cuda")
    args = (sdev, plan.descs, plan.frames, plan.tables, plan.intervals, plan.ivs)
    _, status = eng.jpeg_entropy_decode(*args, out=out)
    torch.cuda.synchronize()
    assert int(status.abs().sum()) == 0
    times = []
    for _ in range(7):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        eng.jpeg_entropy_decode(*args, out=out, status=status)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    res["entropy_decode_ms_per_batch"] = {"frames": n, "median": float(np.median(times)), "min": float(min(times)), "max": float(max(times))}
    feeder.close()


def _sync_measurements(eng, paths, workers, res):
    """the sync plan's host time per frame on one thread and the HIP-event time of Engine.jpeg_sync_decode on one resident batch (the
    uploads of the records and the six kernels) at 64, 128 and 256 bytes per piece, with the frames each flags"""
    lib = L.load()
    bufs = [open(p, "rb").read() for p in paths[:8]]
    cap = 1 << 16
    d, fr = L.sd_jpeg_frame_desc(), L.sd_jpeg_sync_frame()
    tables, iv = (L.sd_jpeg_huff_table * L.SD_JPEG_ENTROPY_TABLES)(), (L.sd_jpeg_sync_interval * cap)()
    clean = np.empty(max(len(b) for b in bufs), np.uint8)
    for rep in range(2):
        t0 = time.perf_counter()
        for b in bufs:
            assert lib.sd_jpeg_sync_plan(b, len(b), 128, C.byref(d), C.byref(fr), tables, iv, cap, clean.ctypes.data_as(C.c_void_p), clean.nbytes) == L.SD_OK
        res["sync_plan_ms_per_frame_1_thread"] = (time.perf_counter() - t0) / len(bufs) * 1e3
    n = min(32, len(paths))
    res["sync_decode_ms_per_batch"] = {}
    for piece in (64, 128, 256):
        feeder = frame_io.FrameFeeder(paths[:n], n, "cuda", workers, jpeg="device_sync", engine=eng, sync_piece=piece)
        t0 = time.perf_counter()
        plan, staged, (h, w) = _staged_plan(feeder, n)
        plan_ms = (time.perf_counter() - t0) * 1e3
        if len(plan.eligible) != n:
            res["sync_decode_ms_per_batch"][str(piece)] = {"eligible": len(plan.eligible)}
            feeder.close()
            continue
        used = -(-max(int(plan.frames[i].clean_bytes) for i in range(n)) // 16) * 16
        sdev = staged.bytes[:n, :used].cuda()
        out = torch.empty((n, frame_io.FrameFeeder.coef_stride_bytes(h, w) // 2), dtype=torch.int16, device="cuda")
        args = (sdev, plan.descs, plan.frames, plan.tables, plan.intervals, plan.ivs, piece)
        _, status = eng.jpeg_sync_decode(*args, out=out)
        torch.cuda.synchronize()
        times = []
        for _ in range(7):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            eng.jpeg_sync_decode(*args, out=out, status=status)
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b))
        res["sync_decode_ms_per_batch"][str(piece)] = {
            "frames": n, "median": float(np.median(times)), "min": float(min(times)), "max": float(max(times)), "plan_ms_per_batch_native": plan_ms,
            "clean_bytes_per_batch": int(sum(int(plan.frames[i].clean_bytes) for i in range(n))),
            "pieces_per_frame_max": int(max(int(plan.frames[i].n_pieces) for i in range(n))),
            "intervals_per_frame": int(plan.frames[0].n_intervals), "flagged_frames": int((status != 0).sum())}
        feeder.close()


def _feeder_pass(eng, paths, workers, route, sync_piece=None):
    kw = {"jpeg": route, "engine": eng} if route != "host" else {}
    if route == "device_sync" and sync_piece:
        kw["sync_piece"] = sync_piece
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 0
    with frame_io.FrameFeeder(paths, 32, "cuda", workers, **kw) as feeder:
        for fr, lo in feeder:
            eng.resize_cubic(fr)
            n += fr.shape[0]
        fallbacks = len(feeder.sync_fallback if route == "device_sync" else feeder.entropy_fallback)
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t0), fallbacks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--workers", type=int, default=frame_io.default_decode_workers())
    ap.add_argument("--format", choices=("png", "jpeg"), default="png")
    ap.add_argument("--jpeg", choices=("host", "device", "device_entropy", "device_sync"), default="host")
    ap.add_argument("--sync-piece", type=int, default=frame_io.SYNC_PIECE_BYTES, help="--jpeg device_sync / --compare: bytes of the clean stream per lane")
    ap.add_argument("--size", default="1024x2048", help="HxW of the generated frames")
    ap.add_argument("--restart-rows", type=int, default=0, help="generated JPEG frames: Pillow's restart_marker_rows (0: no restart intervals)")
    ap.add_argument("--encoder", choices=("pillow", "own"), default="pillow", help="generated JPEG frames: Pillow, or the project's encoder")
    ap.add_argument("--compare", action="store_true", help="JPEG frames: the four routes interleaved in this process, plan and kernel times")
    ap.add_argument("--frames-dir", default=None, help="time the *.png / *.jpg / *.jpeg files of this directory (one size) instead of generating frames")
    ap.add_argument("--repeats", type=int, default=3, help="timed passes of the feeder after one warm pass")
    ap.add_argument("--out", default=None, help="write the JSON record here (default: print only)")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as td:
        if a.frames_dir:
            paths = sorted(p for e in ("*.png", "*.jpg", "*.jpeg") for p in glob.glob(os.path.join(a.frames_dir, e)))
            if not paths:
                raise SystemExit(f"no frames in {a.frames_dir}")
            paths = (paths * (-(-a.frames // len(paths))))[:a.frames]      # (cycled to --frames: the page cache holds them either way)
        else:
            distinct = min(a.frames, 32) if a.compare else a.frames           # (--compare cycles 32 distinct files)
            paths = _generate(td, distinct, a.format, tuple(int(v) for v in a.size.split("x")), a.restart_rows, a.encoder)
            paths = (paths * (-(-a.frames // len(paths))))[:a.frames]
        with open(paths[0], "rb") as f:
            H, W = frame_io.image_size(f.read())
        res = {"frame": [H, W, 3], "frames": len(paths), "distinct_files": len(set(paths)), "host_cpus": os.cpu_count(), "workers": a.workers,
               "format": "dir" if a.frames_dir else a.format, "jpeg": a.jpeg, "file_bytes_mean": float(np.mean([os.path.getsize(p) for p in set(paths)]))}
        all_png = all(p.lower().endswith(".png") for p in paths)
        if all_png:
            res["png_bytes_mean"] = res["file_bytes_mean"]                  # (the key of the earlier PNG records)
        _single_thread_ms(paths, res)
        if all_png:                                                         # the Python-level pool of the earlier PNG records
            from concurrent.futures import ThreadPoolExecutor
            with ThreadPoolExecutor(a.workers) as ex:
                list(ex.map(frame_io.imread, paths[:a.workers]))            # warm
                t0 = time.perf_counter()
                list(ex.map(frame_io.imread, paths))
                res["decode_fps_python_thread_pool"] = len(paths) / (time.perf_counter() - t0)
        # the native batch reader (what FrameFeeder calls): files -> one host buffer, `workers` C++ threads (PNG: all frames, as the
        # earlier records; JPEG frames may be 36 MB each decoded, so at most 64 of them)
        lib = L.load()
        nb = len(paths) if all_png else min(len(paths), 64)
        hostbuf = np.empty((nb, H, W, 3), np.uint8)
        arr = (C.c_char_p * nb)(*[os.fsencode(p) for p in paths[:nb]])
        for _ in range(2):
            t0 = time.perf_counter()
            st = lib.sd_decode_files_bgr(arr, nb, H, W, hostbuf.ctypes.data_as(C.c_void_p), H * W * 3, a.workers, None)
            dt = time.perf_counter() - t0
        assert st == 0
        res["decode_fps_native_batch"] = nb / dt
        del hostbuf
        if torch.cuda.is_available():
            host = torch.empty((32, H, W, 3), dtype=torch.uint8, pin_memory=True)
            dev = torch.empty((32, H, W, 3), dtype=torch.uint8, device="cuda")
            dev.copy_(host, non_blocking=True); torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(5):
                dev.copy_(host, non_blocking=True)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / 5
            res["upload_gb_per_s"] = host.numel() / dt / 1e9
            res["upload_fps"] = 32 / dt
            eng = Engine(512, 1024, 32, "resnet50", precision="bf16x2")
            eng.resize_cubic(dev); torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(5):
                eng.resize_cubic(dev)
            torch.cuda.synchronize()
            res["resize_fps"] = 32 * 5 / (time.perf_counter() - t0)
            del host, dev
            kw = {"jpeg": a.jpeg, "engine": eng} if a.jpeg != "host" else {}          # (nothing the parent commit's feeder lacks in host mode)
            if a.jpeg == "device_sync":
                kw["sync_piece"] = a.sync_piece
            with open(paths[0], "rb") as f:
                has_dri = b"\xff\xdd" in f.read(4096)                                 # (the DRI segment comes before the scan)
            if a.jpeg != "host" or a.compare:
                _kernel_ms_per_batch(eng, paths, a.workers, res)
            if a.jpeg == "device_entropy" or (a.compare and has_dri):
                _entropy_measurements(eng, paths, a.workers, res)
            if a.jpeg == "device_sync" or a.compare:
                _sync_measurements(eng, paths, a.workers, res)
            if a.compare:                                                             # the four routes, pass by pass, in this process
                routes = ("host", "device", "device_entropy", "device_sync")
                res["restart_intervals_in_files"], res["sync_piece"] = bool(has_dri), a.sync_piece
                rates = {r: [] for r in routes}
                for rep in range(a.repeats + 1):
                    for r in routes:
                        fps, fb = _feeder_pass(eng, paths if rep else paths[:64], a.workers, r, a.sync_piece)
                        if rep:
                            rates[r].append(fps)
                        if r == "device_entropy":
                            res["entropy_fallback_frames"] = fb
                        if r == "device_sync":
                            res["sync_fallback_frames"] = fb
                res["compare_feeder_fps"] = {r: {"median": float(np.median(v)), "passes": v} for r, v in rates.items()}
            rates = []
            for rep in range(a.repeats + 1):                                          # pass 0 warms (pinned staging allocation, page cache)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                n = 0
                with frame_io.FrameFeeder(paths if rep else paths[:64], 32, "cuda", a.workers, **kw) as feeder:
                    for fr, lo in feeder:
                        eng.resize_cubic(fr)
                        n += fr.shape[0]
                torch.cuda.synchronize()
                if rep:
                    rates.append(n / (time.perf_counter() - t0))
            res["feeder_fps_decode_upload_resize"] = float(np.median(rates))
            res["feeder_fps_passes"] = rates
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
