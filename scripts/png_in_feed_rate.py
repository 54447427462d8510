"""PNG input route, host against device (dev tool, run on the GPU box; the sibling of feed_rate.py for FrameFeeder(png=...)):
  feed rate    FrameFeeder end to end (decode / inflate, pinned upload, reconstruction, GPU cubic resize; batch 32), png="host" and
               png="device" interleaved pass by pass in ONE process: one warm pass and --repeats timed passes per route and size.  The
               device route counts as faster only when median(host time) - median(device time) > max(host time) - min(host time).
  kernel time  HIP events around Engine.png_reconstruct at B = 32, 1024 x 2048 RGB, 20 calls after 3; the shipped 16-wave workgroup and the
               one-wave form (SEMDEPTH_DISABLE=png_waves)
  host split   sd_decode_files_bgr against sd_inflate_files_png on ONE thread, ms per frame: the share of the host's PNG work that the
               device route takes off the host
    python scripts/png_in_feed_rate.py [--workers 16] [--repeats 3] [--out profiles/png_in_feed_rate.json]
The frames are generated: street-like gradients xor noise, written as RGB PNGs with the adaptive (minimum sum of absolute residuals)
filter choice per row.  Generated frames compress unlike photographs, so the inflate share differs from real Cityscapes frames.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import struct
import sys
import tempfile
import time
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from semantic_depth_amd import _lib as L                    # noqa: E402
from semantic_depth_amd import frame_io                     # noqa: E402
from semantic_depth_amd.engine import Engine                # noqa: E402


def _chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def _adaptive_png(img):
    """RGB u8 [h,w,3] -> (file bytes, rows per filter type): every row takes the filter with the smallest sum of |signed residual|"""
    h, w, ch = img.shape
    cur = img.reshape(h, w * ch).astype(np.int32)
    a = np.zeros_like(cur)
    a[:, ch:] = cur[:, :-ch]
    b = np.zeros_like(cur)
    b[1:] = cur[:-1]
    c = np.zeros_like(cur)
    c[1:, ch:] = cur[:-1, :-ch]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    res = [((cur - q) & 255).astype(np.uint8) for q in (np.zeros_like(cur), a, b, (a + b) >> 1, paeth)]
    cost = np.stack([np.abs(r.astype(np.int8).astype(np.int32)).sum(1) for r in res])
    ft = cost.argmin(0)
    rows = np.empty((h, 1 + w * ch), np.uint8)
    rows[:, 0] = ft
    for t in range(5):
        rows[ft == t, 1:] = res[t][ft == t]
    buf = (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) + _chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) +
           _chunk(b"IEND", b""))
    return buf, np.bincount(ft, minlength=5).tolist()


def _generate(td, n, size):
    H, W = size
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:H, 0:W]
    paths, hist, nbytes = [], np.zeros(5, np.int64), 0
    for i in range(n):
        base = np.stack([(yy // 3 + xx // 5 + 7 * i) % 256, (xx // 4 + 3 * i) % 256, (yy // 2 + xx // 7) % 256], -1).astype(np.uint8)
        buf, ft = _adaptive_png(base ^ rng.integers(0, 4, (H, W, 3), dtype=np.uint8))
        p = os.path.join(td, f"f{H}_{i:03d}.png")
        open(p, "wb").write(buf)
        paths.append(p)
        hist += ft
        nbytes += len(buf)
    return paths, hist.tolist(), nbytes / n


def _feeder_pass(eng, paths, workers, route):
    kw = {"png": "device", "engine": eng} if route == "device" else {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 0
    with frame_io.FrameFeeder(paths, 32, "cuda", workers, **kw) as feeder:
        for fr, lo in feeder:
            eng.resize_cubic(fr)
            n += fr.shape[0]
    torch.cuda.synchronize()
    return time.perf_counter() - t0, n


def _host_split(paths, size):
    lib = L.load()
    h, w = size
    n = len(paths)
    arr = (C.c_char_p * n)(*[p.encode() for p in paths])
    status = (C.c_int * n)()
    bgr = np.zeros((n, h * w * 3), np.uint8)
    stride = frame_io.FrameFeeder.png_rows_stride(h, w)
    rows = np.zeros((n, stride), np.uint8)
    descs = (L.sd_png_frame_desc * n)()
    out = {}
    for name, call in (("decode_bgr", lambda: lib.sd_decode_files_bgr(arr, n, h, w, bgr.ctypes.data_as(C.c_void_p), h * w * 3, 1, status)),
                       ("inflate_rows", lambda: lib.sd_inflate_files_png(arr, n, h, w, rows.ctypes.data_as(C.c_void_p), stride, descs, 1, status))):
        assert call() == L.SD_OK
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            call()
            ts.append((time.perf_counter() - t0) * 1e3 / n)
        out[name + "_ms_per_frame_one_thread"] = statistics.median(ts)
    out["host_share_left"] = out["inflate_rows_ms_per_frame_one_thread"] / out["decode_bgr_ms_per_frame_one_thread"]
    return out


def _kernel_ms(eng, paths, size):
    lib = L.load()
    h, w = size
    B = 32
    stride = -(-(h * (1 + 3 * w)) // 16) * 16
    rows = np.zeros((B, stride), np.uint8)
    descs = (L.sd_png_frame_desc * B)()
    for i in range(B):
        buf = open(paths[i % len(paths)], "rb").read()
        assert lib.sd_png_inflate_rows(buf, len(buf), rows[i].ctypes.data_as(C.c_void_p), stride, C.byref(descs[i])) == L.SD_OK
    rdev = torch.from_numpy(rows).cuda()
    out = torch.empty((B, h, w, 3), dtype=torch.uint8, device="cuda")
    status = torch.empty((B,), dtype=torch.int32, device="cuda")
    ms = []
    for k in range(23):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        eng.png_reconstruct(rdev, descs, out=out, status=status)
        e1.record()
        e1.synchronize()
        if k >= 3:
            ms.append(e0.elapsed_time(e1))
    ref = frame_io.decode_png(open(paths[0], "rb").read())
    assert np.array_equal(out[0].cpu().numpy(), ref) and not status.cpu().numpy().any()
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "calls": len(ms), "B": B}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--distinct", type=int, default=8, help="distinct generated files per size, cycled")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    eng = Engine(512, 1024, 32, "resnet50")
    os.environ["SEMDEPTH_DISABLE"] = "png_waves"
    eng1 = Engine(128, 256, 1, "resnet50")
    del os.environ["SEMDEPTH_DISABLE"]
    rec = {"what": "scripts/png_in_feed_rate.py: FrameFeeder(png='host') against FrameFeeder(png='device') on generated adaptive-filter RGB PNGs, one "
                   "process, routes interleaved pass by pass; kernel time by HIP events; host split on one thread",
           "workers": args.workers, "host_cpus": os.cpu_count(), "repeats": args.repeats, "rows": []}
    with tempfile.TemporaryDirectory() as td:
        for size, frames in (((512, 1024), 512), ((1024, 2048), 256)):
            paths, hist, mean_bytes = _generate(td, args.distinct, size)
            seq = [paths[i % len(paths)] for i in range(frames)]
            times = {"host": [], "device": []}
            for route in ("host", "device"):
                _feeder_pass(eng, seq, args.workers, route)                     # warm: page cache, pinned buffers, kernels
            for _ in range(args.repeats):
                for route in ("host", "device"):
                    t, n = _feeder_pass(eng, seq, args.workers, route)
                    assert n == frames
                    times[route].append(t)
            th, tdv = times["host"], times["device"]
            row = {"size": list(size), "frames": frames, "distinct_files": len(paths), "mean_file_bytes": mean_bytes, "rows_per_filter_type": hist,
                   "host_pass_s": th, "device_pass_s": tdv, "host_fps_median": frames / statistics.median(th),
                   "device_fps_median": frames / statistics.median(tdv),
                   "median_gain_s": statistics.median(th) - statistics.median(tdv), "host_spread_s": max(th) - min(th)}
            row["device_counts_as_faster"] = row["median_gain_s"] > row["host_spread_s"]
            row["host_split"] = _host_split(paths, size)
            if size == (1024, 2048):
                row["kernel_b32_rgb"] = _kernel_ms(eng, paths, size)
                row["kernel_b32_rgb_one_wave"] = _kernel_ms(eng1, paths, size)
            rec["rows"].append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
