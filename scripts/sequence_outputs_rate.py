"""frames/s of distributed.run_sequence_files on 1024 x 2048 PNG frames with the sequence tool's files off and on (one GPU).

    python scripts/sequence_outputs_rate.py [--frames 128] [--batch 32] [--precision f16x2] [--level 1] [--threads 0]
                                            [--png host|device|both] [--ply host|device|both] [--repeats 5] [--no-ply]
                                            [--video off|device|host] [--scene host,device [--out profiles/scene_ply_rate.json]]

Setup as bench.py --config 5 (smooth random frames, seeded weights, the monodepth bias calibrated so that the median depth is the
measuring depth); the frames are written once, untimed.  Each run is timed from the first decode to the last file written
(SequenceOutputs.close).  Prints one JSON line: both rates, whether the records agree, the bytes written and the host threads of
the writer and of the decoder.  --png chooses where the result images are compressed (SequenceOutputs(png=)); with "both" the two
routes are timed interleaved, --repeats times each, and the line also carries each route's rates (median, min, max), the image bytes
copied device-to-host per frame, the PNG bytes per frame, and whether the device route is faster by the rule of DESIGN section 4
(median(device) - median(host) > max(host) - min(host)).  --ply chooses where the road PLYs are formatted (SequenceOutputs(ply=)) in the
same way: with "both" (and one --png route) the two PLY routes are timed interleaved, and the line carries each route's rates, the PLY
bytes per frame (on the device route: the text copied device-to-host) and the raw cloud bytes per frame (15 B per point, the host route's copy).
--video device|host also writes the result video (SequenceOutputs(video=outputs.Video(route=...))) in every run with files on; the line then
carries the route and the bytes of the AVI files per frame.  Compare against the same command without it.
--scene host,device times the scene PLY files (SequenceOutputs(scene=outputs.Scene(route=...)), approach 'both') and nothing else: every
other file of the tool is off, the listed routes are timed interleaved in one process, --repeats times each.  The line (also written to
--out) carries each route's frames/s and time per batch (median, min, max), the bytes copied device-to-host per frame, the scene bytes
written per frame, how many frames of the device route fell back to the host formatter, the time of the new kernels on one batch (device
events around process_batch with and without want_boxes, and around Engine.format_scene_ply per file) and whether the device route is
faster by the rule above, in time per batch: median(host) - median(device) > max(host) - min(host).
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--precision", default="f16x2")
    ap.add_argument("--level", type=int, default=1)
    ap.add_argument("--threads", type=int, default=0)
    ap.add_argument("--png", choices=("host", "device", "both"), default="host", help="where the result images are compressed")
    ap.add_argument("--ply", dest="ply_route", choices=("host", "device", "both"), default="host", help="where the road PLYs are formatted")
    ap.add_argument("--repeats", type=int, default=5, help="timed runs per route with --png both / --ply both")
    ap.add_argument("--no-ply", dest="ply", action="store_false", help="no road PLYs (images and overlay items only)")
    ap.add_argument("--video", choices=("off", "device", "host"), default="off", help="also write the result video (Motion-JPEG AVI) on this route")
    ap.add_argument("--scene", default="", help="comma-separated Scene routes to time (host,device): the scene PLY files alone, approach 'both'")
    ap.add_argument("--out", default="", help="with --scene: also write the JSON line to this file")
    ap.add_argument("--keep", action="store_true", help="keep the written files (default: removed)")
    args = ap.parse_args()
    if args.png == "both" and args.ply_route == "both":
        ap.error("--png both and --ply both: vary one route at a time")
    if args.ply_route != "host" and not args.ply:
        ap.error("--ply device / both with --no-ply")
    vary_ply = args.ply_route == "both"

    import torch

    import __graft_entry__ as graft
    graft.build()
    from semantic_depth_amd import _lib as L
    from semantic_depth_amd import outputs
    from semantic_depth_amd import weights as Wt
    from semantic_depth_amd.distributed import make_engine_step, run_sequence_files
    from semantic_depth_amd.engine import RW_DTYPE, Camera, Engine, RoadWidthParams
    from semantic_depth_amd.frame_io import default_decode_workers

    H, W, B = 512, 1024, args.batch
    cam = Camera(1048.64 / 2, 519.277 / 2, 1000.0, 1.0, 3800.0)
    prm = RoadWidthParams()
    rng = np.random.default_rng(1000)
    base = rng.integers(0, 256, (B, 2 * H // 8, 2 * W // 8, 3), dtype=np.uint8)
    frames = np.repeat(np.repeat(base, 8, axis=1), 8, axis=2)
    frames = (frames.astype(np.int16) + rng.integers(-16, 17, frames.shape, dtype=np.int16)).clip(0, 255).astype(np.uint8)
    work = tempfile.mkdtemp(prefix="sd_seq_rate_")
    try:
        src = os.path.join(work, "in")
        os.makedirs(src)
        paths = [os.path.join(src, f"frame_{i:06d}.png") for i in range(args.frames)]
        outputs.write_png_batch(paths, frames[np.arange(args.frames) % B], level=1)

        wf = Wt.make_fcn8s_weights(1, decoder_std=0.05)
        wm = Wt.make_monodepth_weights("resnet50", 2)
        eng = Engine(H, W, B, "resnet50", precision=args.precision, range_check=False)
        eng.load_weights(L.SD_NET_FCN8S, wf)
        eng.load_weights(L.SD_NET_MONODEPTH, wm)
        fr = eng.resize_cubic(torch.from_numpy(frames).cuda())
        d0 = float(eng.monodepth_forward(fr).median().item())
        target = cam.f * cam.b / prm.depth / cam.disp_mult
        logit = lambda p: float(np.log(p / (1.0 - p)))
        bias = round((logit(target / 0.3) - logit(min(max(d0, 1e-4), 0.2999) / 0.3)) * 64.0) / 64.0
        eng.load_weights(L.SD_NET_MONODEPTH, {"dec/disp1/biases": (wm["dec/disp1/biases"] + np.float32(bias)).astype(np.float32)})

        threads = args.threads if args.threads > 0 else default_decode_workers()

        if args.scene:
            line = scene_rates(args, eng, cam, prm, paths, work, threads, B)
            print(json.dumps(line))
            if args.out:
                with open(args.out, "w") as f:
                    json.dump(line, f, indent=1)
                    f.write("\n")
            eng.close()
            return

        def run(with_outputs, frame_paths, tag, route="host"):
            outs = None
            if with_outputs:
                png, ply = (args.png, route) if vary_ply else (route, args.ply_route)
                outs = outputs.SequenceOutputs(os.path.join(work, tag), outputs.sequence_names(frame_paths), depth=prm.depth, level=args.level,
                                               threads=threads, ply=ply if args.ply else False, png=png,
                                               video=None if args.video == "off" else outputs.Video(route=args.video))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rec = run_sequence_files(frame_paths, make_engine_step(eng, lambda i: cam, prm, outputs=outs), batch=B, device="cuda")
            torch.cuda.synchronize()
            return time.perf_counter() - t0, rec

        def png_bytes(tag):
            d = os.path.join(work, tag, outputs.SEQ_IMG_DIR)
            return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d) if f.endswith(".png"))

        def stream_bytes(tag):
            """bytes of the zlib streams inside the device route's files: a file is signature (8), IHDR (25), IEND (12) and one 12-byte
            IDAT frame per MiB of its stream"""
            d = os.path.join(work, tag, outputs.SEQ_IMG_DIR)
            total = 0
            for f in os.listdir(d):
                if f.endswith(".png"):
                    body, k = os.path.getsize(os.path.join(d, f)) - 45, 1
                    while body - 12 * k > k << 20:
                        k += 1
                    total += body - 12 * k
            return total

        def ply_bytes(tag):
            d = os.path.join(work, tag, outputs.SEQ_PLY_DIR)
            return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d) if f.endswith(".ply"))

        both = args.png == "both" or vary_ply
        routes = ("host", "device") if both else (args.png,)
        for r in routes:
            run(True, paths[:B], "warm_on_" + r, r)      # (warm-up: tables, pinned staging, allocator)
        run(False, paths[:B], "warm_off")
        t_off, rec_off = run(False, paths, "off")
        times = {r: [] for r in routes}
        same = True
        for k in range(args.repeats if both else 1):
            for r in routes:
                tag = "on_" + r
                shutil.rmtree(os.path.join(work, tag), ignore_errors=True)
                t, rec_on = run(True, paths, tag, r)
                times[r].append(t)
                same = same and bool(torch.equal(rec_on.cpu(), rec_off.cpu()))
        found = int(rec_on.cpu().numpy().view(RW_DTYPE)["found"].sum())
        out_dir = os.path.join(work, "on_" + routes[-1])
        nbytes = sum(os.path.getsize(os.path.join(dp, f)) for dp, _, fs in os.walk(out_dir) for f in fs)
        line = dict(frames=args.frames, batch=B, precision=args.precision, png_level=args.level, png=args.png, ply=args.ply, ply_route=args.ply_route,
                    fps_outputs_off=round(args.frames / t_off, 1), fps_outputs_on=round(args.frames / float(np.median(times[routes[-1]])), 1),
                    records_identical=same, found=found, bytes_written=nbytes,
                    writer_threads=threads, decode_threads=default_decode_workers(), host_cpus=len(os.sched_getaffinity(0)))
        if args.png == "both":
            fps = {r: sorted(args.frames / t for t in times[r]) for r in routes}
            line["routes"] = {r: dict(fps=[round(v, 1) for v in fps[r]], median=round(float(np.median(fps[r])), 1), min=round(fps[r][0], 1),
                                      max=round(fps[r][-1], 1), png_bytes_per_frame=png_bytes("on_" + r) // args.frames) for r in routes}
            line["routes"]["host"]["d2h_image_bytes_per_frame"] = 2 * H * 2 * W * 3
            line["routes"]["device"]["d2h_image_bytes_per_frame"] = stream_bytes("on_device") // args.frames + 8      # (+ the u64 size)
            h_, d_ = line["routes"]["host"], line["routes"]["device"]
            line["device_faster"] = bool(d_["median"] - h_["median"] > h_["max"] - h_["min"])
            line["png_size_device_over_host"] = round(d_["png_bytes_per_frame"] / h_["png_bytes_per_frame"], 4)
        if vary_ply:
            fps = {r: sorted(args.frames / t for t in times[r]) for r in routes}
            line["routes"] = {r: dict(fps=[round(v, 1) for v in fps[r]], median=round(float(np.median(fps[r])), 1), min=round(fps[r][0], 1),
                                      max=round(fps[r][-1], 1), ply_bytes_per_frame=ply_bytes("on_" + r) // args.frames) for r in routes}
            n_final = rec_on.cpu().numpy().view(RW_DTYPE)["n_ror"].astype(np.int64)
            line["routes"]["host"]["d2h_ply_bytes_per_frame"] = int(n_final.sum()) * 15 // args.frames + 4            # (+ the i32 count)
            line["routes"]["device"]["d2h_ply_bytes_per_frame"] = line["routes"]["device"]["ply_bytes_per_frame"] + 12  # (+ offset and flag)
            line["ply_fallback"] = len(json.load(open(os.path.join(work, "on_device", "manifest_rank0.json")))["ply_fallback"])
            h_, d_ = line["routes"]["host"], line["routes"]["device"]
            line["device_faster"] = bool(d_["median"] - h_["median"] > h_["max"] - h_["min"])
            line["files_identical"] = all(
                open(os.path.join(work, "on_host", outputs.SEQ_PLY_DIR, f), "rb").read() == open(os.path.join(work, "on_device", outputs.SEQ_PLY_DIR, f), "rb").read()
                for f in sorted(os.listdir(os.path.join(work, "on_host", outputs.SEQ_PLY_DIR))))
        if args.video != "off":
            tags = [d for d in sorted(os.listdir(work)) if d.startswith("on")]
            avi = [os.path.join(work, tags[-1], f) for f in sorted(os.listdir(os.path.join(work, tags[-1]))) if f.endswith(".avi")]
            line["video"] = dict(route=args.video, files=len(avi), avi_bytes_per_frame=sum(os.path.getsize(f) for f in avi) // args.frames)
        print(json.dumps(line))
        eng.close()
    finally:
        if args.keep:
            print("files kept in", work)
        else:
            shutil.rmtree(work, ignore_errors=True)


def scene_rates(args, eng, cam, prm, paths, work, threads, B):
    """the --scene mode: see the module docstring"""
    import torch

    from semantic_depth_amd import outputs
    from semantic_depth_amd.distributed import make_engine_step, run_sequence_files
    from semantic_depth_amd.engine import BOX_DTYPE, F2F_DTYPE, RW_DTYPE
    from semantic_depth_amd.frame_io import FrameFeeder
    routes = tuple(r for r in args.scene.split(",") if r)
    assert routes and all(r in ("host", "device") for r in routes), routes
    nb = -(-len(paths) // B)

    def run(route, frame_paths, tag):
        shutil.rmtree(os.path.join(work, tag), ignore_errors=True)
        outs = outputs.SequenceOutputs(os.path.join(work, tag), outputs.sequence_names(frame_paths), depth=prm.depth, threads=threads,
                                       images=False, items=False, ply=False, scene=outputs.Scene(route=route))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rec = run_sequence_files(frame_paths, make_engine_step(eng, lambda i: cam, prm, approach="both", outputs=outs), batch=B, device="cuda")
        torch.cuda.synchronize()
        return time.perf_counter() - t0, rec, json.load(open(outs.manifest))

    for r in routes:
        run(r, paths[:B], "warm_" + r)
        shutil.rmtree(os.path.join(work, "warm_" + r), ignore_errors=True)
    times, man, rec = {r: [] for r in routes}, {}, None
    for _ in range(args.repeats):
        for r in routes:
            t, rec, man[r] = run(r, paths, "on_" + r)
            times[r].append(t)

    def size(tag, rel):
        return os.path.getsize(os.path.join(work, tag, rel))

    line = dict(frames=len(paths), batch=B, precision=args.precision, writer_threads=threads, host_cpus=len(os.sched_getaffinity(0)),
                repeats=args.repeats, routes={})
    recs = rec.cpu().numpy().view(RW_DTYPE).reshape(-1)
    line["found"] = int(recs["found"].sum())
    for r in routes:
        per_batch = sorted(t / nb for t in times[r])
        written = sum(size("on_" + r, f) for f in man[r]["scene"])
        line["routes"][r] = dict(fps_median=round(len(paths) / float(np.median(times[r])), 1), s_per_batch=[round(v, 4) for v in per_batch],
                                 s_per_batch_median=round(float(np.median(per_batch)), 4), s_per_batch_min=round(per_batch[0], 4),
                                 s_per_batch_max=round(per_batch[-1], 4), scene_bytes_per_frame=written // len(paths),
                                 fallback_frames=len(man[r]["scene_fallback"]))
    # bytes copied device-to-host per frame, and the new kernels' time, from one batch processed here
    feeder = FrameFeeder(paths[:B], B, device="cuda")
    with feeder:
        frames = next(iter(feeder))[0]
    fr = eng.resize_cubic(frames)
    cams = [cam] * B
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def timed(fn, n=3):
        out, ms = None, []
        for _ in range(n + 1):
            a, b = ev(), ev()
            a.record()
            out = fn()
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return out, round(float(np.median(ms[1:])), 3)

    _, ms_plain = timed(lambda: eng.process_batch(fr, cams, prm, approach="both", want_final=True))
    out, ms_boxes = timed(lambda: eng.process_batch(fr, cams, prm, approach="both", want_final=True, want_boxes=True))
    sc = outputs.Scene()
    kernels = dict(process_batch_ms=ms_plain, process_batch_with_boxes_ms=ms_boxes)
    d2h_device = 0
    for key in sc.files:
        (text, offsets, flags), ms = timed(lambda: eng.format_scene_ply(out["road_final"], out["fence_final"], out["records"], out["f2f"],
                                                                          out["plane_boxes"], outputs.SCENE_FILES[key][1], sc.lattice_cap,
                                                                          capacity=B * sc.capacity_per_frame))
        kernels["format_" + key + "_ms"] = ms
        kernels["format_" + key + "_flags"] = [int(v) for v in np.bincount(flags.cpu().numpy(), minlength=4)]
        d2h_device += int(offsets[-1].item()) + 12 * B + 8
    f2 = out["f2f"].cpu().numpy().view(F2F_DTYPE).reshape(-1)
    points = int(out["road_final"]["n"].sum().item()) + int(f2["counts"][:, 5].sum()) + int(f2["counts"][:, 6].sum())
    small = B * (RW_DTYPE.itemsize + F2F_DTYPE.itemsize + 3 * BOX_DTYPE.itemsize + 4)
    if "host" in line["routes"]:
        line["routes"]["host"]["d2h_bytes_per_frame"] = (points * 15 + small) // B
    if "device" in line["routes"]:
        line["routes"]["device"]["d2h_bytes_per_frame"] = (d2h_device + small) // B     # (a batch without fallback frames)
    line["new_kernels_one_batch"] = kernels
    if len(routes) == 2:
        h_, d_ = line["routes"]["host"], line["routes"]["device"]
        line["device_faster"] = bool(h_["s_per_batch_median"] - d_["s_per_batch_median"] > h_["s_per_batch_max"] - h_["s_per_batch_min"])
        line["files_identical"] = all(open(os.path.join(work, "on_host", f), "rb").read() == open(os.path.join(work, "on_device", f), "rb").read()
                                      for f in man["host"]["scene"])
    return line


if __name__ == "__main__":
    main()
