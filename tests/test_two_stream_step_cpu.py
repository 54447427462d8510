"""CPU: the event choreography of bench.py's two-stream step against the hand-written table of what every engine call of the step reads and
writes in the handle's workspace (tests/two_stream_cases.py).  Nothing here runs a kernel: the step's stream operations are taken from the source
of `instrumented_step` with `ast`, unrolled over several steps and checked for a pair of accesses to one region, at least one a write, that no
stream order and no event orders.  tests/test_gpu_two_stream_step.py runs the same step on a GPU."""
import copy

import pytest

import two_stream_cases as T

STEPS = 5


def test_the_restated_step_is_the_benchmarks_step():
    """drift guard: pipelined_steps makes the engine calls, event records, event waits, record_stream calls and stream-context entries of
    bench.py's instrumented_step, in its order (bench.py's config-5 resize aside)"""
    bench = T.bench_choreography()
    mine = T.choreography(T.__file__, "pipelined_steps")
    assert mine == bench, (mine, bench)
    # ... and the extraction saw the step: both networks, the three tail stages, all seven events, both waits, the side context
    assert [op[1] for op in bench if op[0] == "eng"] == ["fcn8s_forward", "monodepth_forward", "fuse_from_raw", "road_width", "fence_to_fence"]
    assert [op[1] for op in bench if op[0] == "record"] == list(range(7))
    assert [op for op in bench if op[0] == "wait"] == [("wait", "main", 4), ("wait", "side", 3)]
    assert bench.count(("record_stream", "side")) == 1 and bench.count(("stream", "side")) == 1 and bench.count(("with",)) == 1


def test_every_carved_region_is_in_the_table_and_in_the_header():
    carved = T.carved_regions()
    assert len(carved) >= 17 and len(set(carved)) == len(carved), carved
    tabled = {r.split(".")[0] for r in T.REGIONS}
    assert set(carved) == tabled, (set(carved) ^ tabled)
    # o_misc by its parts, the raw pair on its own
    assert {"o_misc.scalar", "o_misc.zero_page", "o_misc.f2f_counts", "o_misc.f2f_planes", "o_misc.clamp_counters", "o_mono.raw_pair"} <= set(T.REGIONS)
    assert "o_misc" not in T.REGIONS
    header = open(T.HEADER).read()
    streams = header[header.index(" * Streams"):header.index("#ifndef SEMDEPTH_H")]
    for name in carved:
        assert name in streams, name
    for call, a in T.ACCESS.items():
        assert a["cite"] and (a["reads"] | a["writes"]) <= set(T.REGIONS), call


def test_the_table_covers_every_engine_call_of_the_step():
    calls = {op[1] for op in T.bench_choreography() if op[0] == "eng"}
    assert calls == set(T.ACCESS), calls ^ set(T.ACCESS)


@pytest.mark.parametrize("approach", ["both", "rw"])
def test_the_benchmarks_choreography_has_no_unordered_conflict(approach):
    ops = T.unroll(T.bench_choreography(), STEPS, approach)
    calls = [o for o in ops if o["kind"] == "call"]
    assert len(calls) == STEPS * (5 if approach == "both" else 4)
    assert {o["stream"] for o in calls if o["name"] in ("fcn8s_forward", "monodepth_forward")} == {"main"}
    assert {o["stream"] for o in calls if o["name"] in ("fuse_from_raw", "road_width", "fence_to_fence")} == {"side"}
    assert T.conflicts(ops) == []
    # the two families share one region, and it is the one the two events order
    net = set().union(*[T.ACCESS[c]["reads"] | T.ACCESS[c]["writes"] for c in ("fcn8s_forward", "monodepth_forward")])
    tail = set().union(*[T.ACCESS[c]["reads"] | T.ACCESS[c]["writes"] for c in ("fuse_from_raw", "road_width", "fence_to_fence")])
    assert net & tail == {"o_mono.raw_pair"}


def test_the_overlap_is_real():
    """not vacuous: the checker does see the networks of step i+1 unordered against the tail of step i (otherwise nothing could conflict)"""
    ops = T.unroll(T.bench_choreography(), 2, "both")
    everything = {c: dict(cite="x", reads={"r"}, writes={"r"}) for c in T.ACCESS}
    pairs = {(a[1], b[1]) for _, a, b in T.conflicts(ops, everything) if a[0] == 0 and b[0] == 1}
    assert ("road_width", "fcn8s_forward") in pairs and ("fence_to_fence", "monodepth_forward") in pairs and ("fuse_from_raw", "fcn8s_forward") in pairs
    assert ("fuse_from_raw", "monodepth_forward") not in pairs            # ev[4]
    assert not [1 for _, a, b in T.conflicts(ops, everything) if a[0] == b[0]]      # within a step everything is ordered (ev[3])


@pytest.mark.parametrize("approach", ["both", "rw"])
def test_dropping_the_main_streams_wait_on_ev4_is_caught(approach):
    chor = [op for op in T.bench_choreography() if op != ("wait", "main", 4)]
    bad = T.conflicts(T.unroll(chor, STEPS, approach))
    # the fusion of step i reads the raw pair while the monodepth of step i+1 (and later) writes it
    assert bad and {b[0] for b in bad} == {"o_mono.raw_pair"}
    assert ("o_mono.raw_pair", (0, "fuse_from_raw", "side"), (1, "monodepth_forward", "main")) in bad
    assert all(a[1] == "fuse_from_raw" and b[1] == "monodepth_forward" and b[0] > a[0] for _, a, b in bad)


@pytest.mark.parametrize("approach", ["both", "rw"])
def test_dropping_the_side_streams_wait_on_ev3_is_caught(approach):
    chor = [op for op in T.bench_choreography() if op != ("wait", "side", 3)]
    bad = T.conflicts(T.unroll(chor, STEPS, approach))
    assert bad and {b[0] for b in bad} == {"o_mono.raw_pair"}
    for step in range(STEPS):           # the fusion of a step no longer waits for its own monodepth pass
        assert ("o_mono.raw_pair", (step, "monodepth_forward", "main"), (step, "fuse_from_raw", "side")) in bad


@pytest.mark.parametrize("call", ["fuse_from_raw", "road_width", "fence_to_fence"])
def test_a_tail_write_into_the_zero_page_is_caught(call):
    access = copy.deepcopy(T.ACCESS)
    access[call]["writes"] = access[call]["writes"] | {"o_misc.zero_page"}
    bad = T.conflicts(T.unroll(T.bench_choreography(), STEPS, "both"), access)
    assert bad and {b[0] for b in bad} == {"o_misc.zero_page"}
    assert ("o_misc.zero_page", (0, call, "side"), (1, "fcn8s_forward", "main")) in bad
    assert T.ACCESS[call]["writes"].isdisjoint({"o_misc.zero_page"})       # (the real table was not touched)


def test_a_wait_on_an_event_never_recorded_orders_nothing():
    """the step-0 wait the benchmark skips with `fused_once`: harmless to the checker either way"""
    ops = T.unroll([("wait", "main", 4), ("eng", "monodepth_forward")], 1)
    assert ops[0]["preds"] == [] and ops[1]["preds"] == [0]
