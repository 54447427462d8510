"""One-frame latency of the f16x2 engine on a max_batch = 1 handle, default against small_batch (Engine(small_batch=True): split-K forms of the
under-filled GEMM layers), in ONE process on ONE box, the two handles interleaved.

    python scripts/latency_b1.py [--repeats 20] [--warmup 3] [--out profiles/latency_b1.json] [--level 1]

--level 2 (Engine(small_batch=2): level 1 plus the chunk-split 3x3 direct layers): THREE handles interleaved -- default, level 1 ("level1") and level 2
("small_batch") --, the watched layers are every layer either plan lists plus conv3_x / conv4_x / conv5_x, every record carries the level-1 time beside the
default's and level 2's, and the output goes to profiles/latency_b1_direct.json.

Configurations: 256 x 512 with the vgg encoder (the reference's defaults) and 512 x 1024 with resnet50.  Each runs in a child process of its
own under `timeout -k 10`; a configuration that fails ends the run (nothing is retried).  Reported per configuration, for both handles:
  * per-layer HIP-event times (sd_profile, verbose names) of every layer the rule split, plus fc6 and fc7: median / min / max over the
    repeats; a split layer's time is its GEMM launch + its reduce launch;
  * one fcn8s_forward, one monodepth_forward and one process_batch of a single frame, device input to record (torch events);
  * beside each layer the floors from the layer's own figures: weight bytes / 8 TB/s and flops / 833 TF/s;
  * the verdicts of the rule: a layer `keeps` its split when default median - split median > the default's spread (max - min)."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CONFIGS = [(256, 512, "vgg"), (512, 1024, "resnet50")]
HBM_BPS, MFMA_FLOPS = 8.0e12, 833.0e12      # the floors' denominators (include/semdepth.h: 2500 / 3 TFLOP/s of algorithmic work on three products)


def stat(v):
    v = sorted(v)
    n = len(v)
    return dict(median=(v[n // 2] + v[(n - 1) // 2]) / 2, min=v[0], max=v[-1])


class StderrCapture:
    """the [sd_profile] lines are written by the library to fd 2"""
    def __enter__(self):
        sys.stderr.flush()
        self.tmp = tempfile.TemporaryFile(mode="w+b")
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *a):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode(errors="replace")
        self.tmp.close()


LINE = re.compile(r"\[sd_profile\]\s+(\S+)\s+M=(\d+)\s+N=(\d+)\s+K=(\d+)\s+([\d.]+) ms\s+[\d.]+ TF/s\s+(\S.*)$")


def layer_records(text):
    """{layer: dict(ms, kernels, M, N, K)}: the launches of one layer added up"""
    out = {}
    for line in text.splitlines():
        m = LINE.match(line.strip())
        if not m:
            continue
        r = out.setdefault(m.group(1), dict(ms=0.0, kernels=[], M=int(m.group(2)), N=int(m.group(3)), K=int(m.group(4))))
        r["ms"] += float(m.group(5))
        r["kernels"].append(m.group(6).strip())
    return out


VGG_DIRECT = {f"conv{b}_{i}" for b in (3, 4, 5) for i in (1, 2, 3)}


def run_config(idx, repeats, warmup, level=1):
    os.environ["SEMDEPTH_PROFILE_VERBOSE"] = "1"
    import numpy as np
    import torch
    from semantic_depth_amd import _lib as L, weights as Wt
    from semantic_depth_amd.engine import Camera, Engine
    H, W, enc = CONFIGS[idx]
    rng = np.random.default_rng(7)
    base = rng.integers(0, 256, (1, H // 8, W // 8, 3), dtype=np.uint8)
    fr = np.repeat(np.repeat(base, 8, axis=1), 8, axis=2)
    fr = (fr.astype(np.int16) + rng.integers(-16, 17, fr.shape, dtype=np.int16)).clip(0, 255).astype(np.uint8)
    frame = torch.from_numpy(fr).cuda()
    cams = [Camera(W / 2, H / 2, 1000.0, 1.0, float(W))]
    wf, wm = Wt.make_fcn8s_weights(1, decoder_std=0.05, bias_std=0.1), Wt.make_monodepth_weights(enc, 2, bias_std=0.05)
    engines = {}
    for name, sb in (("default", False), ("small_batch", True)) if level == 1 else (("default", False), ("level1", 1), ("small_batch", level)):
        e = Engine(H, W, 1, enc, precision="f16x2", small_batch=sb)
        e.load_weights(L.SD_NET_FCN8S, wf)
        e.load_weights(L.SD_NET_MONODEPTH, wm)
        engines[name] = e
    plan = engines["small_batch"].small_batch_plan()
    watched = set(plan["fcn8s"]) | set(plan["monodepth"]) | {"fc6", "fc7"}
    if level > 1:
        plan1 = engines["level1"].small_batch_plan()
        watched |= set(plan1["fcn8s"]) | set(plan1["monodepth"]) | VGG_DIRECT
    calls = {"fcn8s_forward": lambda e: e.fcn8s_forward(frame), "monodepth_forward": lambda e: e.monodepth_forward(frame),
             "process_batch": lambda e: e.process_batch(frame, cams)}
    for _ in range(warmup):
        for e in engines.values():
            for f in calls.values():
                f(e)
    torch.cuda.synchronize()
    # end to end: device input to result, one call at a time, the two handles alternating
    e2e = {n: {c: [] for c in calls} for n in engines}
    for _ in range(repeats):
        for cname, f in calls.items():
            for n, e in engines.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                f(e)
                b.record()
                b.synchronize()
                e2e[n][cname].append(a.elapsed_time(b))
    # per layer: HIP events around every conv launch
    layers = {n: {} for n in engines}
    meta = {}
    for _ in range(repeats):
        for n, e in engines.items():
            e.profile(True)
            e.fcn8s_forward(frame)
            e.monodepth_forward(frame)
            with StderrCapture() as cap:
                e.profile_read()
            e.profile(False)
            for layer, r in layer_records(cap.text).items():
                if layer in watched:
                    layers[n].setdefault(layer, []).append(r["ms"])
                    meta.setdefault(layer, {}).setdefault(n, r)
    for e in engines.values():
        e.check_range()
    table = []
    for layer in sorted(watched & set(layers["default"])):
        d, s = stat(layers["default"][layer]), stat(layers["small_batch"][layer])
        r = meta[layer]["default"]
        flops, wbytes = 2.0 * r["M"] * r["N"] * r["K"], 4.0 * r["N"] * r["K"]       # (fp16 hi + lo plane of every weight)
        S = {**plan["fcn8s"], **plan["monodepth"]}.get(layer, 1)
        if level > 1:
            # the criterion is level 2's gain over the handle WITHOUT the direct split where that is what changed the layer: a GEMM layer level 1 already split
            # is judged against the default as before, and its level-1 time shows that level 2 left it alone
            l1 = stat(layers["level1"][layer])
            direct = layer not in plan1["fcn8s"] and layer not in plan1["monodepth"]
            table.append(dict(layer=layer, S=S, direct=bool(direct and S > 1), M=r["M"], N=r["N"], K=r["K"], default_ms=d, level1_ms=l1, small_batch_ms=s,
                              default_kernels=meta[layer]["default"]["kernels"], small_batch_kernels=meta[layer]["small_batch"]["kernels"],
                              floor_weights_ms=wbytes / HBM_BPS * 1e3, floor_mfma_ms=flops / MFMA_FLOPS * 1e3,
                              keeps=bool(S > 1 and d["median"] - s["median"] > d["max"] - d["min"])))
            continue
        table.append(dict(layer=layer, S=S, M=r["M"], N=r["N"], K=r["K"], default_ms=d, small_batch_ms=s,
                          default_kernels=meta[layer]["default"]["kernels"], small_batch_kernels=meta[layer]["small_batch"]["kernels"],
                          floor_weights_ms=wbytes / HBM_BPS * 1e3, floor_mfma_ms=flops / MFMA_FLOPS * 1e3,
                          keeps=bool(S > 1 and d["median"] - s["median"] > d["max"] - d["min"])))
    res = dict(H=H, W=W, encoder=enc, precision="f16x2", max_batch=1, level=level, repeats=repeats, warmup=warmup, device=torch.cuda.get_device_name(0),
               split_plan=plan, layers=table, end_to_end_ms={n: {c: stat(v) for c, v in per.items()} for n, per in e2e.items()})
    d, s = res["end_to_end_ms"]["default"]["fcn8s_forward"], res["end_to_end_ms"]["small_batch"]["fcn8s_forward"]
    res["fcn8s_forward_faster"] = bool(d["median"] - s["median"] > d["max"] - d["min"])
    for e in engines.values():
        e.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="default profiles/latency_b1.json; required with --config")
    ap.add_argument("--config", type=int, default=None, help="run ONE configuration in this process (what the parent starts)")
    ap.add_argument("--step-timeout", type=int, default=420)
    ap.add_argument("--level", type=int, default=1, choices=(1, 2), help="the small_batch level of the second handle; 2 adds a level-1 handle beside the default")
    a = ap.parse_args()
    if a.repeats < 20:
        ap.error("at least 20 timed repeats")
    if a.config is not None and a.out is None:
        ap.error("--config writes ONE configuration's record: name its file with --out")
    a.out = a.out or os.path.join(ROOT, "profiles", "latency_b1.json" if a.level == 1 else "latency_b1_direct.json")
    if a.config is not None:
        json.dump(run_config(a.config, a.repeats, a.warmup, a.level), open(a.out, "w"), indent=1)
        return 0
    results = []
    for i in range(len(CONFIGS)):
        with tempfile.TemporaryDirectory() as td:
            part = os.path.join(td, "part.json")
            cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--config", str(i), "--repeats", str(a.repeats),
                   "--warmup", str(a.warmup), "--out", part, "--level", str(a.level)]
            rc = subprocess.run(cmd).returncode
            if rc != 0:          # a fault, an abort or the time limit: nothing more is started on the GPU
                print(f"configuration {CONFIGS[i]} ended with status {rc}: stopping", file=sys.stderr)
                return rc
            results.append(json.load(open(part)))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(dict(tool="scripts/latency_b1.py", floors=dict(hbm_bytes_per_s=HBM_BPS, mfma_flops_per_s=MFMA_FLOPS), configurations=results),
              open(a.out, "w"), indent=1)
    for r in results:
        print(f"{r['H']}x{r['W']} {r['encoder']}: " + ", ".join(
            f"{c} " + " -> ".join(f"{per[c]['median']:.3f}" for per in r["end_to_end_ms"].values()) + " ms" for c in r["end_to_end_ms"]["default"]))
        for t in r["layers"]:
            print(f"   {t['layer']:22s} S={t['S']:<2d} {t['default_ms']['median']:.4f} (spread {t['default_ms']['max'] - t['default_ms']['min']:.4f}) -> {t['small_batch_ms']['median']:.4f} ms  "
                  f"(floors: weights {t['floor_weights_ms']:.4f}, mfma {t['floor_mfma_ms']:.4f})  {'keeps' if t['keeps'] else ('-' if t['S'] == 1 else 'NO GAIN')}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
