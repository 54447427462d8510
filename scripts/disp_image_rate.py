#!/usr/bin/env python3
"""dev tool: what the disparity images cost (one GPU, one process, the compared things interleaved).

    python scripts/disp_image_rate.py [--batch 32] [--calls 20] [--frames 128] [--repeats 3] [--threads 16] [--out FILE]
    python scripts/disp_image_rate.py --kernels-only --shape 256x512          # under rocprofv3 --kernel-trace --stats, a run of its own
    python scripts/disp_image_rate.py --merge FILE --stats 256x512=CSV --stats 512x1024=CSV

Part 1: Engine.disparity_image (time between device events around the whole call: five launches plus the resample's two) against the host
twin, outputs.disparity_image, on --threads threads (the batch split into that many parts; the native call holds no interpreter lock), at
256 x 512 -> 1024 x 2048 and 512 x 1024 -> 1024 x 2048, B = --batch, both maps; the two are checked to give the same bytes.
Part 2: frames/s of distributed.run_sequence_files on 1024 x 2048 PNG frames (the setup of scripts/sequence_outputs_rate.py: a
512 x 1024 f16x2 engine, result images on, PLYs off) with disp off, "gray" and "plasma" on both PNG routes, --repeats runs each,
interleaved; the cost of the option per frame is 1 / fps(on) - 1 / fps(off) of the medians.
Per-pass kernel times are not taken by events: --kernels-only runs only the calls of one shape for a rocprofv3 --kernel-trace --stats run,
and --merge puts the average time of every kernel from its kernel_stats CSV into the JSON file under "per_pass_us"."""
import argparse
import csv
import json
import os
import re
import shutil
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"256x512": (256, 512), "512x1024": (512, 1024)}
OUT_H, OUT_W = 1024, 2048


def disparity_like(seed, B, h, w):
    """smooth positive maps with a different range per frame, like a post-processed disparity"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    out = np.empty((B, h, w), np.float32)
    for b in range(B):
        out[b] = (0.01 + 0.08 * (yy / h) ** 2 + 0.004 * np.sin(xx / (17.0 + b)) + 0.002 * rng.random((h, w), dtype=np.float32)) * (1.0 + 0.1 * b)
    return out


def merge(path, stats):
    res = json.load(open(path))
    res["per_pass_us"] = {}
    for item in stats:
        shape, file = item.split("=", 1)
        rows = {}
        for r in csv.DictReader(open(file)):
            m = re.search(r"\b((?:disp|pil)_\w+_kernel(?:<\d+>)?)", r["Name"])
            if m:
                rows[m.group(1)] = dict(calls=int(r["Calls"]), average_us=round(float(r["AverageNs"]) / 1e3, 2))
        res["per_pass_us"][shape] = rows
    res["per_pass_source"] = "rocprofv3 --kernel-trace --stats -- python scripts/disp_image_rate.py --kernels-only --shape <shape> (a run of its own per shape)"
    json.dump(res, open(path, "w"), indent=1)
    print(json.dumps(res["per_pass_us"], indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--precision", default="f16x2")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--shape", default="256x512", choices=sorted(SHAPES))
    ap.add_argument("--skip-step", action="store_true", help="part 1 only")
    ap.add_argument("--merge", default=None)
    ap.add_argument("--stats", action="append", default=[])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.merge:
        return merge(a.merge, a.stats)

    import torch

    import __graft_entry__ as graft
    graft.build()
    from semantic_depth_amd import _lib as L
    from semantic_depth_amd import outputs
    from semantic_depth_amd import weights as Wt
    from semantic_depth_amd.distributed import make_engine_step, run_sequence_files
    from semantic_depth_amd.engine import Camera, Engine, RoadWidthParams

    B = a.batch
    mults = [3800.0] * B
    if a.kernels_only:
        eng = Engine(128, 256, 1, "resnet50")
        h, w = SHAPES[a.shape]
        d = torch.from_numpy(disparity_like(1, B, h, w)).cuda()
        out = torch.empty((B, OUT_H, OUT_W, 3), dtype=torch.uint8, device="cuda")
        for _ in range(a.calls + 3):
            eng.disparity_image(d, OUT_H, OUT_W, "plasma", mults=mults, out=out)
        torch.cuda.synchronize()
        eng.close()
        return

    res = dict(batch=B, calls=a.calls, out_size=[OUT_H, OUT_W], host_threads=a.threads, host_cpus=len(os.sched_getaffinity(0)), shapes={})
    eng = Engine(128, 256, 1, "resnet50")
    pool = ThreadPoolExecutor(max_workers=a.threads)
    try:
        for shape, (h, w) in SHAPES.items():
            disp = disparity_like(1, B, h, w)
            d = torch.from_numpy(disp).cuda()
            out = torch.empty((B, OUT_H, OUT_W, 3), dtype=torch.uint8, device="cuda")
            parts = [p for p in np.array_split(np.arange(B), a.threads) if len(p)]

            def host_call(cmap):
                t0 = time.perf_counter()
                imgs = list(pool.map(lambda p: outputs.disparity_image(disp[p[0]:p[-1] + 1], OUT_H, OUT_W, cmap, mults[p[0]:p[-1] + 1])[0], parts))
                return (time.perf_counter() - t0) * 1e3, imgs

            entry = {}
            for cmap in outputs.DISP_MAPS:
                for _ in range(3):
                    eng.disparity_image(d, OUT_H, OUT_W, cmap, mults=mults, out=out)
                dev_ms, host_ms, imgs = [], [], None
                for k in range(a.calls):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    eng.disparity_image(d, OUT_H, OUT_W, cmap, mults=mults, out=out)
                    e1.record()
                    e1.synchronize()
                    dev_ms.append(e0.elapsed_time(e1))
                    if k % 5 == 0:                                   # the host twin in between, a quarter as often (it takes far longer)
                        t, imgs = host_call(cmap)
                        host_ms.append(t)
                assert np.array_equal(out.cpu().numpy(), np.concatenate(imgs)), (shape, cmap)
                px = B * OUT_H * OUT_W
                hbm = B * (2 * 4 * h * w + h * w + (h * w + h * OUT_W) + (h * OUT_W + OUT_H * OUT_W) + 2 * OUT_H * OUT_W + 3 * OUT_H * OUT_W)
                entry[cmap] = dict(device_ms_per_batch=dict(median=round(float(np.median(dev_ms)), 3), min=round(min(dev_ms), 3), max=round(max(dev_ms), 3)),
                                   device_us_per_frame=round(float(np.median(dev_ms)) * 1e3 / B, 1),
                                   host_twin_ms_per_batch=dict(median=round(float(np.median(host_ms)), 1), min=round(min(host_ms), 1), max=round(max(host_ms), 1)),
                                   algorithmic_bytes_per_output_pixel=round(hbm / px, 2),
                                   achieved_GBps_over_the_call=round(hbm / (float(np.median(dev_ms)) * 1e-3) / 1e9, 1),
                                   equals_host_twin=True)
            res["shapes"][f"{shape} -> {OUT_H}x{OUT_W}"] = entry
    finally:
        pool.shutdown()
        eng.close()

    if not a.skip_step:
        H, W = 512, 1024
        cam = Camera(1048.64 / 2, 519.277 / 2, 1000.0, 1.0, 3800.0)
        prm = RoadWidthParams()
        rng = np.random.default_rng(1000)
        base = rng.integers(0, 256, (B, 2 * H // 8, 2 * W // 8, 3), dtype=np.uint8)
        frames = np.repeat(np.repeat(base, 8, axis=1), 8, axis=2)
        frames = (frames.astype(np.int16) + rng.integers(-16, 17, frames.shape, dtype=np.int16)).clip(0, 255).astype(np.uint8)
        work = tempfile.mkdtemp(prefix="sd_disp_rate_")
        try:
            src = os.path.join(work, "in")
            os.makedirs(src)
            paths = [os.path.join(src, f"frame_{i:06d}.png") for i in range(a.frames)]
            outputs.write_png_batch(paths, frames[np.arange(a.frames) % B], level=1)
            eng = Engine(H, W, B, "resnet50", precision=a.precision, range_check=False)
            eng.load_weights(L.SD_NET_FCN8S, Wt.make_fcn8s_weights(1, decoder_std=0.05))
            eng.load_weights(L.SD_NET_MONODEPTH, Wt.make_monodepth_weights("resnet50", 2))
            configs = [(png, disp) for png in ("host", "device") for disp in (None, "gray", "plasma")]

            def run(png, disp, frame_paths):
                tag = f"{png}_{disp}"
                shutil.rmtree(os.path.join(work, tag), ignore_errors=True)
                outs = outputs.SequenceOutputs(os.path.join(work, tag), outputs.sequence_names(frame_paths), depth=prm.depth, level=1, threads=a.threads,
                                               ply=False, png=png, disp=disp)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run_sequence_files(frame_paths, make_engine_step(eng, lambda i: cam, prm, outputs=outs), batch=B, device="cuda")
                torch.cuda.synchronize()
                return time.perf_counter() - t0

            for c in configs:
                run(*c, paths[:B])                                   # warm-up: tables, pinned staging, allocator
            times = {c: [] for c in configs}
            for _ in range(a.repeats):
                for c in configs:
                    times[c].append(run(*c, paths))
            step = {}
            for png in ("host", "device"):
                off = a.frames / float(np.median(times[(png, None)]))
                step[png] = {}
                for disp in (None, "gray", "plasma"):
                    fps = sorted(a.frames / t for t in times[(png, disp)])
                    e = dict(fps=[round(v, 1) for v in fps], median=round(float(np.median(fps)), 1))
                    if disp is not None:
                        e["cost_us_per_frame"] = round((1.0 / float(np.median(fps)) - 1.0 / off) * 1e6, 1)
                        d = os.path.join(work, f"{png}_{disp}", outputs.SEQ_DISP_DIR)
                        e["disp_png_bytes_per_frame"] = sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) // a.frames
                    step[png][str(disp)] = e
            res["sequence_step"] = dict(frames=a.frames, frame_size=[2 * H, 2 * W], engine=[H, W], precision=a.precision, repeats=a.repeats,
                                        result_images=True, ply=False, writer_threads=a.threads, routes=step)
            eng.close()
        finally:
            shutil.rmtree(work, ignore_errors=True)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
