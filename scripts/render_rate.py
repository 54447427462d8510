#!/usr/bin/env python3
"""dev tool: kernel time of the rendered clouds (Engine.render_rw, five launches) between device events, and the host statement's time per
frame on one core, for the same road-like cloud under outputs.top_camera().
usage: python scripts/render_rate.py [--host-only] [--batch 32] [--cap 524288] [--points 150000] [--sizes 512,1024] [--calls 20] [--out FILE]
Prints one JSON object; per-kernel times are not taken here (they need a rocprofv3 --kernel-trace --stats run of their own)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def road_cloud(seed, n):
    rng = np.random.default_rng(seed)
    return (rng.random((n, 3)) * [12.0, 0.4, 30.0] + [-6.0, 1.3, 5.0]).astype(np.float32), rng.integers(0, 250, (n, 3), dtype=np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--cap", type=int, default=512 * 1024, help="the bench shape's capacity, H * W of a 512 x 1024 engine")
    ap.add_argument("--points", type=int, default=150000)
    ap.add_argument("--sizes", default="512,1024")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import __graft_entry__ as graft
    graft.build()
    from semantic_depth_amd import outputs
    from semantic_depth_amd.engine import RW_DTYPE
    xyz, rgb = road_cloud(1, a.points)
    left, right = np.float32([-3.7, 1.5, 19.9]), np.float32([4.1, 1.5, 20.1])
    res = dict(batch=a.batch, cap=a.cap, points_per_frame=a.points, calls=a.calls, sizes={})
    for size in (int(s) for s in a.sizes.split(",")):
        cam = outputs.top_camera(size, size)
        t = []
        for _ in range(3):
            t0 = time.perf_counter()
            img = outputs.render_rw(xyz, rgb, left, right, cam)
            t.append((time.perf_counter() - t0) * 1e3)
        entry = dict(host_statement_ms_per_frame_one_core=round(min(t), 2), drawn_pixels_per_frame=int((img != 255).any(-1).sum()))
        if not a.host_only:
            import torch
            from semantic_depth_amd.engine import Engine
            eng = Engine(128, 256, 1, "resnet50")
            try:
                fx = torch.zeros((a.batch, a.cap, 3), dtype=torch.float32, device="cuda")
                fc = torch.zeros((a.batch, a.cap, 3), dtype=torch.uint8, device="cuda")
                fx[:, :a.points] = torch.from_numpy(xyz).cuda()
                fc[:, :a.points] = torch.from_numpy(rgb).cuda()
                final = dict(xyz=fx, rgb=fc, n=torch.full((a.batch,), a.points, dtype=torch.int32, device="cuda"))
                rec = np.zeros(a.batch, RW_DTYPE)
                rec["found"], rec["left_pt"], rec["right_pt"] = 1, left, right
                records = torch.from_numpy(rec.view(np.uint8).reshape(a.batch, -1).copy()).cuda()
                out = torch.empty((a.batch, size, size, 3), dtype=torch.uint8, device="cuda")
                for _ in range(3):
                    eng.render_rw(final, records, cam, out=out)
                ms = []
                for _ in range(a.calls):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    eng.render_rw(final, records, cam, out=out)
                    e1.record()
                    e1.synchronize()
                    ms.append(e0.elapsed_time(e1))
                assert np.array_equal(out[0].cpu().numpy(), img) and np.array_equal(out[-1].cpu().numpy(), img)
                entry.update(kernel_ms_per_batch=dict(median=round(float(np.median(ms)), 3), min=round(min(ms), 3), max=round(max(ms), 3)),
                             equals_host_statement=True)
            finally:
                eng.close()
        res["sizes"][f"{size}x{size}"] = entry
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
