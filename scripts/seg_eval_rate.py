#!/usr/bin/env python3
"""dev tool: evaluate.evaluate_files through its two routes in one process -- route="device" (Engine.resize_pil and Engine.seg_confusion
around the network call, one read of the counts at the end) against route="host" (the host twins around the same network call) -- on a
synthetic Cityscapes-layout tree of N 1200 x 1600 frames (block noise) with label images of the ids 0 / 7 / 13 (blocks), written to a
temporary folder by the project's PNG writers.  One f16x2 engine at 256 x 512 with seeded FCN-8s weights, batches of 8.  1 warm pass and
--passes timed passes per route, interleaved; a pass ends with the counts on the host.  In the warm pass the two routes' matrices must
be equal.  Both routes read and decode the same files on the same host threads and run the same network: the difference is the resample
of frame and labels and the counting.
The device route counts as faster only under the project's rule median(host) - median(device) > max(host) - min(host).
Beside the rates: the time of the new calls alone by device events (median of 20; a call = the upload of its windows plus its one or two
launches): resize_pil of 8 frames 1200 x 1600 x 3 -> 256 x 512 RGB, of 8 label frames (channel 0 of [.., 3]) -> 256 x 512, seg_confusion of
8 frames 256 x 512.  These are call times on an otherwise idle stream, not kernel times from a trace.
usage: python scripts/seg_eval_rate.py [--frames 32] [--passes 5] [--out profiles/seg_eval_rate.json] [--counts-only]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, SRC_H, SRC_W, BATCH = 256, 512, 1200, 1600, 8


def static_fields(n):
    src_bytes = SRC_H * SRC_W * 3
    return dict(network_size=[H, W], source_size=[SRC_H, SRC_W], frames=n, batch=BATCH, precision="f16x2",
                bytes_per_frame=dict(frame_read=src_bytes, labels_read=src_bytes, intermediate_written_and_read=2 * (SRC_H * W * 3 + SRC_H * W),
                                     resampled_written=H * W * 3 + H * W, confusion_read=2 * H * W))


def write_tree(root, n):
    from semantic_depth_amd import outputs
    rng = np.random.default_rng(5)
    gt, im = os.path.join(root, "gtFine", "test", "synth"), os.path.join(root, "leftImg8bit", "test", "synth")
    os.makedirs(gt)
    os.makedirs(im)
    ids = np.array([0, 7, 13, 7, 23], np.uint8)
    frames = np.stack([np.kron(rng.integers(0, 256, (SRC_H // 8, SRC_W // 8, 3), dtype=np.uint8), np.ones((8, 8, 1), np.uint8)) for _ in range(n)])
    outputs.write_png_batch([os.path.join(im, f"synth_{i:05d}_leftImg8bit.png") for i in range(n)], frames)
    for i in range(n):
        lab = np.kron(ids[rng.integers(0, len(ids), (SRC_H // 40, SRC_W // 40))], np.ones((40, 40), np.uint8))
        outputs.write_png(os.path.join(gt, f"synth_{i:05d}_gtFine_labelIds.png"), lab)
    return os.path.dirname(gt), os.path.dirname(im)


def call_ms(torch, fn, reps=20):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return dict(min=round(min(ms), 4), median=round(float(np.median(ms)), 4), max=round(max(ms), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seg_eval_rate.json"))
    ap.add_argument("--counts-only", action="store_true", help="no GPU: write the static fields with empty times")
    a = ap.parse_args()
    res = static_fields(a.frames)
    if a.counts_only:
        res.update(measured=False, seconds=dict(device=[], host=[]), stats=None, call_ms=None, verdict="NOT MEASURED")
        return finish(res, a.out)
    import torch

    import __graft_entry__ as graft
    graft.build()
    from semantic_depth_amd import _lib as L
    from semantic_depth_amd import evaluate as E
    from semantic_depth_amd import weights as Wt
    from semantic_depth_amd.engine import Engine
    from semantic_depth_amd.frame_io import default_decode_workers

    eng = Engine(H, W, BATCH, "resnet50", precision="f16x2")
    eng.load_weights(L.SD_NET_FCN8S, Wt.make_fcn8s_weights(1))
    t = dict(device=[], host=[])
    with tempfile.TemporaryDirectory() as root:
        gt, im = write_tree(root, a.frames)
        for p in range(1 + a.passes):                                      # pass 0 warms both routes and compares them
            got = {}
            for route in ("host", "device") if p % 2 else ("device", "host"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                got[route] = E.evaluate_files(gt, im, eng, route=route, batch=BATCH)
                torch.cuda.synchronize()
                if p:
                    t[route].append(time.perf_counter() - t0)
            if p == 0:
                assert np.array_equal(got["device"]["per_frame"], got["host"]["per_frame"]), "the two routes' matrices differ"
                res["mean_iou_seeded_weights"] = float(got["device"]["mean_iou"])
    st = {r: dict(min=round(min(v), 4), median=round(float(np.median(v)), 4), max=round(max(v), 4)) for r, v in t.items()}
    host, dev = st["host"], st["device"]
    rng = np.random.default_rng(6)
    frames = torch.from_numpy(rng.integers(0, 256, (BATCH, SRC_H, SRC_W, 3), dtype=np.uint8)).cuda()
    pred = torch.from_numpy(rng.integers(0, 3, (BATCH, H, W), dtype=np.uint8)).cuda()
    lab = torch.from_numpy(np.array([0, 7, 13], np.uint8)[rng.integers(0, 3, (BATCH, H, W))]).cuda()
    counts = torch.zeros((BATCH, L.SD_SEG_CELLS), dtype=torch.int64, device="cuda")
    table = E.label_table("robo")
    calls = dict(resize_pil_b8_frames_rgb=call_ms(torch, lambda: eng.resize_pil(frames, H, W, channels=3, reverse=True)),
                 resize_pil_b8_labels=call_ms(torch, lambda: eng.resize_pil(frames, H, W, channels=1, pixel_stride=3)),
                 seg_confusion_b8=call_ms(torch, lambda: eng.seg_confusion(pred, lab, table, out=counts)))
    res.update(measured=True, passes=a.passes, decode_workers=default_decode_workers(), seconds={r: [round(x, 4) for x in v] for r, v in t.items()},
               stats=st, frames_per_s={r: round(a.frames / st[r]["median"], 1) for r in st}, matrices_equal=True, call_ms=calls,
               verdict=("device route faster" if host["median"] - dev["median"] > host["max"] - host["min"]
                        else "no difference beyond the host route's own spread"))
    eng.close()
    return finish(res, a.out)


def finish(res, out):
    text = json.dumps(res, indent=1)
    print(text)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
