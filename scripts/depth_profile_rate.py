#!/usr/bin/env python3
"""dev tool: the road width at D depths through its two batched routes in one process -- D calls of Engine.road_width with depth = d
(the whole chain per depth: the only batched route before the depth profile) against one Engine.road_width(want_final=True) plus one
Engine.road_width_profile on the denoised cloud it keeps.  One engine at 512 x 1024 (no weights: the tail alone), B = 32 crafted road
clouds of 40 000 rows each (a 7 m wide patch from 8.2 m on, 300 points per square metre, 1 % outliers in y and in x, 2 000 rows in front
of the z-cut), D = 16 and D = 64 depths spread over the patch.  1 warm pass and 5 timed passes per route, interleaved, each ended by a
device synchronise; in the warm pass the shared fields of the two routes' records must be equal bytes.
The new route counts as faster only under the project's rule median(old) - median(new) > max(old) - min(old).
usage: python scripts/depth_profile_rate.py [--passes 5] [--out profiles/depth_profile_rate.json] [--counts-only]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, B, ROWS, REJECTS = 512, 1024, 32, 40_000, 2_000
DEPTH_SETS = {16: (8.5, 16.0), 64: (8.5, 24.0)}


def static_fields():
    return dict(geometry=[H, W], frames=B, rows_per_cloud=ROWS + REJECTS, depths={str(D): [lo, hi] for D, (lo, hi) in DEPTH_SETS.items()},
                launches_expected=dict(per_depth_chain="D chains", profile="1 chain + 2 launches"))


def road_cloud(rng, n, rejects):
    length = n / 300.0 / 7.0
    x = rng.uniform(-3.5, 3.5, n)
    z = rng.uniform(-8.2 - length, -8.2, n)
    y = -1.5 + rng.standard_normal(n) * 0.02
    k = n // 100
    i = rng.choice(n, k, replace=False)
    y[i] += rng.choice([-1.0, 1.0], k) * rng.uniform(0.5, 1.5, k)
    i = rng.choice(n, k, replace=False)
    x[i] = rng.choice([-1.0, 1.0], k) * rng.uniform(6.0, 7.0, k)
    kept = np.stack([x, y, z], 1)
    front = np.stack([rng.uniform(-4, 4, rejects), rng.uniform(-2, -1, rejects), rng.uniform(-6.9, -1.0, rejects)], 1)
    return rng.permutation(np.concatenate([kept, front])).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_profile_rate.json"))
    ap.add_argument("--counts-only", action="store_true", help="no GPU: write the static fields with empty times")
    a = ap.parse_args()
    res = static_fields()
    if a.counts_only:
        res.update(measured=False, seconds={str(D): dict(per_depth_chain=[], profile=[]) for D in DEPTH_SETS}, stats=None, verdict="NOT MEASURED")
        return finish(res, a.out)
    import torch

    import __graft_entry__ as graft
    graft.build()
    from semantic_depth_amd.engine import RW_DTYPE, RWP_DTYPE, Engine, RoadWidthParams

    eng = Engine(H, W, B, "vgg", precision="f32")
    rng = np.random.default_rng(77)
    xyz = torch.zeros((B, eng.cap, 3), dtype=torch.float32, device=eng.device)
    for b in range(B):
        xyz[b, :ROWS + REJECTS] = torch.from_numpy(road_cloud(rng, ROWS, REJECTS)).to(eng.device)
    n = torch.full((B,), ROWS + REJECTS, dtype=torch.int32, device=eng.device)
    shared = RWP_DTYPE.fields["found"][1] + 4
    assert RW_DTYPE.fields["found"][1] + 4 == shared

    def old_route(depths):
        return torch.stack([eng.road_width(xyz, n, RoadWidthParams(depth=float(d))) for d in depths], 1)          # [B, D, 104]

    def new_route(depths):
        rec, fin, nfin = eng.road_width(xyz, n, RoadWidthParams(depth=float(depths[0])), want_final=True)
        return eng.road_width_profile(fin, nfin, depths)                                                         # [B, D, 48]

    secs, stats, verdicts, found = {}, {}, {}, {}
    for D, (lo, hi) in DEPTH_SETS.items():
        depths = np.linspace(lo, hi, D)
        t = dict(per_depth_chain=[], profile=[])
        for p in range(1 + a.passes):                                      # pass 0 warms both routes and compares them
            got = {}
            for route, fn in (("per_depth_chain", old_route), ("profile", new_route)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                got[route] = fn(depths)
                torch.cuda.synchronize()
                if p:
                    t[route].append(time.perf_counter() - t0)
            if p == 0:
                o, nw = got["per_depth_chain"].cpu().numpy(), got["profile"].cpu().numpy()
                assert o[:, :, :shared].tobytes() == nw[:, :, :shared].tobytes(), "the two routes' records differ"
                found[str(D)] = int(nw.view(RWP_DTYPE)["found"].sum())
        secs[str(D)] = {r: [round(x, 5) for x in v] for r, v in t.items()}
        st = {r: dict(min=round(min(v), 5), median=round(float(np.median(v)), 5), max=round(max(v), 5)) for r, v in t.items()}
        stats[str(D)] = st
        old, new = st["per_depth_chain"], st["profile"]
        verdicts[str(D)] = ("profile faster" if old["median"] - new["median"] > old["max"] - old["min"]
                            else "no difference beyond the per-depth chains' own spread")
    res.update(measured=True, passes=a.passes, seconds=secs, stats=stats, records_equal=True, found=found, verdict=verdicts)
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
