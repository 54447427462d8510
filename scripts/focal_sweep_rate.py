#!/usr/bin/env python3
"""dev tool: the focal-length sweep (semantic_depth.py:843-944) through its two routes in one process -- outputs.focal_sweep over
FrameProcessor.process_frame (both networks once per (focal length, frame)) against the batched route (outputs.focal_sweep_batched:
both networks once per frame, the trial cameras as a batch axis of the tail).  One engine at 256 x 512 (the sweep mode's own geometry),
vgg, f16x2, max_batch 32, synthetic weights, 5 synthetic frames, focal lengths range(380, 580, 10).  1 warm pass and 5 timed passes per
route, interleaved, each ended by a device synchronise; the two result dicts must be equal.  Network calls are counted per route.
The batched route counts as faster only under the project's rule median(old) - median(new) > max(old) - min(old).

Synthetic weights segment and range arbitrarily, so a (focal length, frame) may have no distance; both drivers refuse such a sweep
(TypeError / ValueError).  The script then carries the missing distances as NaN through both routes -- focal_sweep over a
process_frame wrapper, and focal_sweep fed from sweep_distances_batched -- and says so in the output (missing_distances).
usage: python scripts/focal_sweep_rate.py [--passes 5] [--out profiles/focal_sweep_rate.json] [--counts-only]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, MAX_BATCH, N_FRAMES = 256, 512, 32, 5
FOCAL = list(range(380, 580, 10))


def static_fields():
    from semantic_depth_amd.engine import sweep_chunks
    chunks = sweep_chunks(N_FRAMES, len(FOCAL), MAX_BATCH)
    return dict(geometry=[H, W], encoder="vgg", precision="f16x2", max_batch=MAX_BATCH, frames=N_FRAMES, focal_lengths=FOCAL,
                network_calls_expected=dict(per_frame_loop=dict(fcn8s=len(FOCAL) * N_FRAMES, monodepth=len(FOCAL) * N_FRAMES),
                                            batched=dict(fcn8s=1, monodepth=1)),
                trial_slots_per_chain_call=[(t1 - t0) * N_FRAMES for t0, t1 in chunks])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "focal_sweep_rate.json"))
    ap.add_argument("--counts-only", action="store_true", help="no GPU: write the counted fields with empty times")
    a = ap.parse_args()
    res = static_fields()
    if a.counts_only:
        res.update(measured=False, seconds=dict(per_frame_loop=[], batched=[]), network_calls=None, verdict="NOT MEASURED")
        return finish(res, a.out)
    import torch

    import __graft_entry__ as graft
    graft.build()
    from oracle import pipeline
    from semantic_depth_amd import api, outputs
    from semantic_depth_amd import weights as Wt
    from semantic_depth_amd.engine import Engine

    eng = Engine(H, W, MAX_BATCH, "vgg", precision="f16x2")
    seg = api.SegmentFrame((H, W), Wt.make_fcn8s_weights(1, decoder_std=0.05), engine=eng)
    dep = api.DepthFrame(encoder="vgg", input_height=H, input_width=W, checkpoint_path=Wt.make_monodepth_weights("vgg", 2), engine=eng)
    proc = api.FrameProcessor(seg, dep, depth=10.0, approach="both")
    frames = {f"frame_{i}": pipeline.synthetic_scene(H, W, seed=40 + i)[3] for i in range(N_FRAMES)}
    gt = {name: 7.0 + 0.1 * i for i, name in enumerate(sorted(frames))}
    nan = float("nan")
    calls = dict(fcn8s=0, monodepth=0)
    fcn, mono = Engine._fcn8s, Engine._mono

    def count_fcn(self, *args, **kw):
        calls["fcn8s"] += 1
        return fcn(self, *args, **kw)

    def count_mono(self, *args, **kw):
        calls["monodepth"] += 1
        return mono(self, *args, **kw)

    Engine._fcn8s, Engine._mono = count_fcn, count_mono

    def process(name):
        r = proc.process_frame(frames[name])
        return (nan if r["dist_rw"] is None else r["dist_rw"]), (nan if r["dist_f2f"] is None else r["dist_f2f"])

    def old_route(directory):
        f0 = dep.f
        try:
            return outputs.focal_sweep(process, gt, dep, FOCAL, directory)
        finally:
            dep.f = f0

    # decided once, outside the timed passes: does this sweep have every distance?
    probe = outputs.sweep_distances_batched(frames, gt, seg, dep, FOCAL, depth=10.0, approach="both")
    missing = sum(v is None for pair in probe.values() for v in pair)

    def new_route(directory):
        if not missing:
            return outputs.focal_sweep_batched(frames, gt, seg, dep, FOCAL, directory, depth=10.0, approach="both")
        dists = outputs.sweep_distances_batched(frames, gt, seg, dep, FOCAL, depth=10.0, approach="both")

        class Trial:
            f = None

        trial = Trial()
        table = {k: tuple(nan if v is None else v for v in pair) for k, pair in dists.items()}
        return outputs.focal_sweep(lambda name: table[(trial.f, name)], gt, trial, FOCAL, directory)

    secs = dict(per_frame_loop=[], batched=[])
    counted = {}
    with tempfile.TemporaryDirectory() as tmp:
        for p in range(1 + a.passes):                                  # pass 0 warms both routes
            for route in ("per_frame_loop", "batched"):
                d = os.path.join(tmp, f"{route}_{p}")
                calls.update(fcn8s=0, monodepth=0)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                got = new_route(d) if route == "batched" else old_route(d)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if p:
                    secs[route].append(dt)
                counted[route] = dict(calls)
                if route == "per_frame_loop":
                    want = got
                else:
                    assert json.dumps(got, sort_keys=True) == json.dumps(want, sort_keys=True), "the two routes' result dicts differ"
                    for f in FOCAL:
                        assert open(os.path.join(tmp, f"per_frame_loop_{p}", str(f), "data.txt")).read() == open(os.path.join(d, str(f), "data.txt")).read()
    Engine._fcn8s, Engine._mono = fcn, mono
    stats = {r: dict(min=round(min(v), 4), median=round(float(np.median(v)), 4), max=round(max(v), 4)) for r, v in secs.items()}
    old, new = stats["per_frame_loop"], stats["batched"]
    faster = old["median"] - new["median"] > old["max"] - old["min"]
    res.update(measured=True, passes=a.passes, seconds={r: [round(x, 4) for x in v] for r, v in secs.items()}, stats=stats, network_calls=counted,
               missing_distances=missing, results_equal=True,
               verdict="batched faster" if faster else "no difference beyond the per-frame loop's own spread")
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
