#!/usr/bin/env python3
"""dev tool: what the measurement lines cost (one GPU, one process, the compared things interleaved).

    python scripts/overlay_lines_rate.py [--batch 32] [--calls 20] [--out profiles/overlay_lines_rate.json]

Engine.draw_result_lines (time between device events around the whole call: the camera upload and the two launches) on B = --batch result
images of 1024 x 2048 behind a 512 x 1024 network, without a profile (D = 0: the two measured lines) and with a 32-depth profile (D = 32: 130
slots per frame), beside Engine.compose_result_frames and Engine.draw_result_text on the same images in the same process: --calls timed
calls after 3 warm-ups each, median and minimum in milliseconds.  The device result is checked against the host statement once."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NET_H, NET_W, OUT_H, OUT_W = 512, 1024, 1024, 2048


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--depths", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "overlay_lines_rate.json"))
    a = ap.parse_args()

    import torch

    import __graft_entry__ as graft
    graft.build()
    from semantic_depth_amd import outputs
    from semantic_depth_amd.engine import F2F_DTYPE, F2FP_DTYPE, RW_DTYPE, RWP_DTYPE, Camera, Engine

    B, D = a.batch, a.depths
    cam = Camera(1048.64 / 2, 519.277 / 2, 1000.0, 1.0, 3800.0)          # the sequence tool's camera at 512 x 1024

    def point(fx, fy, zn):
        """the 3D point that lands near output pixel (fx * w, fy * h) at depth zn"""
        xn, yn = (fx * OUT_W + 0.5) * NET_W / OUT_W - 0.5, (fy * OUT_H + 0.5) * NET_H / OUT_H - 0.5
        return [(xn - cam.cx) * zn / cam.f, (cam.cy - yn) * zn / cam.f, -zn]

    rng = np.random.default_rng(0)
    recs, f2 = np.zeros((B,), RW_DTYPE), np.zeros((B,), F2F_DTYPE)
    prof, fprof = np.zeros((B, D), RWP_DTYPE), np.zeros((B, D), F2FP_DTYPE)
    for b in range(B):
        j = float(rng.uniform(-0.02, 0.02))
        recs[b]["found"], recs[b]["width"] = 1, 4.41
        recs[b]["left_pt"], recs[b]["right_pt"] = point(0.3 + j, 0.8, 10.0), point(0.7 + j, 0.8, 10.0)
        f2[b]["ok"], f2[b]["dist"] = 1, 9.0
        f2[b]["left_pt"], f2[b]["right_pt"] = point(0.2 + j, 0.8, 10.0), point(0.8 + j, 0.8, 10.0)
        for i, d in enumerate(np.linspace(5.0, 40.0, D)):
            t = (d - 5.0) / 35.0
            half, y = 0.45 * (1.0 - t) + 0.02, 0.95 - 0.6 * t
            prof[b, i]["found"], fprof[b, i]["ok"] = 1, 1
            prof[b, i]["left_pt"], prof[b, i]["right_pt"] = point(0.5 - half + j, y, d), point(0.5 + half + j, y, d)
            fprof[b, i]["left_pt"], fprof[b, i]["right_pt"] = point(0.5 - half - 0.04 + j, y, d), point(0.5 + half + 0.04 + j, y, d)

    def dev(arr):
        return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(arr.shape + (arr.dtype.itemsize,)).copy()).cuda()

    eng = Engine(NET_H, NET_W, B, "resnet50", precision="f16x2")
    try:
        frames = torch.from_numpy(rng.integers(0, 256, (B, NET_H, NET_W, 3), dtype=np.uint8)).cuda()
        road = torch.from_numpy((rng.random((B, NET_H, NET_W)) < 0.3).astype(np.uint8)).cuda()
        fence = torch.from_numpy((rng.random((B, NET_H, NET_W)) < 0.1).astype(np.uint8)).cuda()
        drec, df2, dprof, dfprof = dev(recs), dev(f2), dev(prof), dev(fprof)
        images = torch.empty((B, OUT_H, OUT_W, 3), dtype=torch.uint8, device="cuda")
        lines, cams, clip = outputs.OverlayLines(), [cam] * B, int(0.25 * OUT_H)
        calls = {
            "compose_result_frames": lambda: eng.compose_result_frames(frames, road, fence, drec, OUT_H, OUT_W, out=images),
            "draw_result_text": lambda: eng.draw_result_text(images, drec, 10.0),
            "draw_result_lines_D0": lambda: eng.draw_result_lines(images, drec, cams, lines, f2f=df2, clip_top=clip),
            f"draw_result_lines_D{D}": lambda: eng.draw_result_lines(images, drec, cams, lines, f2f=df2, profile=dprof, f2f_profile=dfprof, clip_top=clip),
        }
        # once: the device result is the host statement's
        calls["compose_result_frames"]()
        base = images[0].cpu().numpy()
        flags = calls[f"draw_result_lines_D{D}"]()[1]
        segs, flag = outputs.overlay_segments(recs[0], cam, (NET_H, NET_W), (OUT_H, OUT_W), lines, f2f=f2[0], profile=prof[0], f2f_profile=fprof[0], clip_top=clip)
        want = outputs.draw_lines(base, segs, clip)
        assert np.array_equal(images[0].cpu().numpy(), want) and int(flags[0]) == flag, "the device lines are not the host statement's"
        painted = int((want != base).any(-1).sum())
        res = dict(batch=B, calls=a.calls, warmups=3, out_size=[OUT_H, OUT_W], net_size=[NET_H, NET_W], depths=D, segments_per_frame=len(segs),
                   painted_pixels_frame0=painted, painted_share_frame0=round(painted / (OUT_H * OUT_W), 5), device=torch.cuda.get_device_name(0), ms={})
        times = {k: [] for k in calls}
        for it in range(a.calls + 3):
            for name, fn in calls.items():                                # interleaved: every call sees the same clocks
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                fn()
                t1.record()
                t1.synchronize()
                if it >= 3:
                    times[name].append(t0.elapsed_time(t1))
        for name, v in times.items():
            res["ms"][name] = dict(median=round(float(np.median(v)), 4), min=round(float(np.min(v)), 4), max=round(float(np.max(v)), 4))
    finally:
        eng.close()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
