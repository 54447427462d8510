"""CPU: bench.py's own multi-GPU launcher.  `python bench.py --gpus N` with no WORLD_SIZE starts N fresh rank processes (before
anything touches a GPU); under a launcher the world size must equal --gpus.  No GPU here, so the ranks stop at their first
check — which is exactly what this pins: N ranks were started with the right environment, and a mismatch is refused."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra=None, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True, timeout=timeout)


def test_gpus_n_spawns_n_ranks():
    r = _run(["--gpus", "2", "--steps", "1", "--warmup", "0", "--no-cpu-baseline"])
    assert r.returncode != 0                                   # no GPU in this container: both ranks refuse to run
    assert r.stderr.count("--gpus 2 but only 0 GPU(s) visible") == 2, r.stderr[-2000:]
    assert r.stdout.strip() == ""                              # and nobody printed a result line


def test_world_size_must_equal_gpus():
    r = _run(["--gpus", "4"], {"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "world size 2 (WORLD_SIZE) != --gpus 4" in r.stderr
    r = _run(["--gpus", "1"], {"WORLD_SIZE": "8", "RANK": "3", "LOCAL_RANK": "3"})
    assert r.returncode != 0 and "world size 8 (WORLD_SIZE) != --gpus 1" in r.stderr


def test_a_rank_that_dies_takes_its_siblings_down():
    """VERDICT r2 / ADVICE r2: one rank exiting early (OOM, HIP error, failed GPU check) must not leave the launcher waiting for the
    others' rendezvous timeout: wait_ranks polls every child, stops the siblings on the first failure and returns THAT exit code."""
    import importlib.util
    import time
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    t0 = time.time()
    procs = [subprocess.Popen([sys.executable, "-c", "import time; time.sleep(120)"]),
             subprocess.Popen([sys.executable, "-c", "import sys, time; time.sleep(0.5); sys.exit(7)"]),
             subprocess.Popen([sys.executable, "-c", "import signal, time; signal.signal(signal.SIGTERM, signal.SIG_IGN); time.sleep(120)"])]
    rc = bench.wait_ranks(procs, poll_s=0.05, grace_s=1.0)
    assert rc == 7
    assert time.time() - t0 < 30                               # not the sleepers' 120 s
    assert all(p.poll() is not None for p in procs)            # the sibling that ignored SIGTERM was killed
    # every rank fine -> 0; a rank killed by a signal -> 128 + n
    assert bench.wait_ranks([subprocess.Popen([sys.executable, "-c", "pass"]) for _ in range(3)]) == 0
    p = subprocess.Popen([sys.executable, "-c", "import os, signal; os.kill(os.getpid(), signal.SIGKILL)"])
    assert bench.wait_ranks([p]) == 128 + 9


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_the_stdout_line_of_a_full_size_record_stays_under_8_kb():
    """round 5's 22.8-KB bench line was not parsed by the driver.  The stdout line is now `compact_line(full record)`;
    the full record of round 5's default run (profiles/r05_bench_default.json: headline + f32_exact + two legs with their by_kernel lists
    and the plan's 90-layer list), widened to the FOUR legs of the present default, must give a line under bench.LINE_LIMIT that still
    carries every key of the contract."""
    import json
    bench = _bench_module()
    full = json.load(open(os.path.join(ROOT, "profiles", "r05_bench_default.json")))
    assert len(json.dumps(full)) > 20000                      # the mock is the real 22.8-KB record
    full["legs"]["bf16x3"] = json.loads(json.dumps(full["legs"]["f16x2"]))
    full["legs"]["mixed"] = json.loads(json.dumps(full["legs"]["plan"]))
    full["dtype"] = bench.DTYPE["f16x2"]
    for k, v in full["legs"].items():
        v["dtype"] = bench.DTYPE.get(k, v["dtype"])
    line = bench.compact_line(full)
    text = json.dumps(line)
    assert len(text) < bench.LINE_LIMIT, len(text)
    assert "\n" not in text
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
              "config", "roofline", "cpu_baseline"):
        assert k in line, k
    assert "workload" in line["config"] and "model" not in line["config"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in line["roofline"], k
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in line["cpu_baseline"], k
    assert set(line["legs"]) == {"f16x2", "plan", "bf16x3", "mixed"}
    for leg in line["legs"].values():
        assert {"value", "ms_per_step", "dtype", "roofline", "fp16_saturated_values", "vs_f32_engine"} <= set(leg), leg.keys()
    assert line["f32_exact"]["value"] == full["f32_exact"]["value"]
    assert line["parity"]["vs_cpu_oracle"]["logits_max_rel"] < 1e-3
    # every dtype string of the line is a short one
    assert all(len(s_) < 160 for s_ in bench.DTYPE.values())


def test_a_plain_record_gives_a_line_with_the_contract_keys():
    """a run without --full measures no roofline region, no legs, no parity and no CPU baseline: the record then carries those as null
    and no stage split or tail-overlap figures, and compact_line must still give the contract's keys with the headline's numbers."""
    import json
    bench = _bench_module()
    full = json.load(open(os.path.join(ROOT, "profiles", "r05_bench_default.json")))
    for k in ("roofline", "fusion_roofline", "f32_exact", "legs", "parity", "cpu_baseline"):
        full[k] = None
    for k in ("stage_ms_last_step", "tail_overlap", "road_fraction", "n_road_mean", "n_after_chain_mean", "found"):
        full["config"].pop(k, None)
    full["config"]["full"] = False
    line = bench.compact_line(full)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert line[k] == full[k], k
    for k in ("roofline", "fusion_roofline", "f32_exact", "legs", "parity", "cpu_baseline"):
        assert line[k] is None, k
    assert line["config"]["full"] is False and "stage_ms_last_step" not in line["config"]


def test_legs_need_full():
    r = _run(["--legs", "f32"])
    assert r.returncode != 0 and "--legs needs --full" in r.stderr
    assert r.stdout.strip() == ""
