"""CPU: the crafted clouds of tests/pcl_chain_cases.py do what tests/test_gpu_pcl_chains.py relies on -- each reaches the median
branches it claims (through a model of the kernels' decision whose constants are parsed from csrc/pcl.hip), the oracle keeps a
non-trivial cloud through every stage, and six seeded mistakes restated in numpy each change a field the GPU test compares."""
import numpy as np
import pytest

import pcl_chain_cases as cc

ROAD = [n for n in cc.ROAD_CASES if n != "mixed_reversed"]
FENCE = [n for n in cc.FENCE_CASES if n != "main_reversed"]
ROAD_STAGES = ("n_zcut", "n_mad_y", "n_mad_x", "n_plane", "n_sor", "n_ror")
FENCE_STAGES = ("mad_y", "thr", "mad_left", "mad_right", "plane_left", "plane_right")


def _oracle_as_compared(o):
    """an oracle.pipeline.road_width_tail record in the shape road_diff reads"""
    r = dict(o)
    r.setdefault("points", np.zeros((0, 3)))
    r.setdefault("colors", np.zeros((0, 3), np.uint8))
    r["n_road"] = None
    return r


def test_constants_parsed_from_the_kernels():
    assert cc.K == dict(MED_S=cc.MED_S, MED_D=cc.MED_D, MED_CAP=cc.MED_CAP, CMP_G=cc.CMP_G, TB=cc.TB)
    assert cc.SWITCH == 4 * cc.MED_S and all(v > 0 for v in cc.K.values())
    # the shapes of the cases are written for these relations; a retune that breaks one must revisit the cases
    assert cc.MED_CAP < 0.45 * 42_000 and 2 * cc.MED_D < cc.MED_S and cc.CMP_G * 256 == cc.SWITCH


def test_median_route_model():
    rng = np.random.default_rng(0)
    v = rng.standard_normal(70_000).astype(np.float32)
    assert cc.median_route(v[:0]) == "empty" and cc.median_route(v[:cc.SWITCH - 1]) == "small"
    assert cc.median_route(v[:cc.SWITCH]) == "hit" and cc.median_route(v) == "hit"
    w = v.copy(); w[5] = np.nan
    assert cc.median_route(w) == "nan" and cc.median_route(w[:100]) == "small"
    w = v.copy(); w[(np.arange(cc.MED_S, dtype=np.int64) * len(w)) // cc.MED_S] = 1e6
    assert cc.median_route(w) == "miss"
    w = v.copy(); w[: len(w) // 2 + 5] = 0.25
    assert cc.median_route(w) == "overflow"
    b = cc.median_bracket(v)
    assert 0.05 * len(v) < b["cnt"] < 0.11 * len(v)          # 2 * MED_D / MED_S = 7.8 % of the column
    assert np.array_equal(cc.key2f(cc.f2key(v)), v) and np.all(np.diff(cc.f2key(np.sort(v)).astype(np.int64)) >= 0)


@pytest.mark.parametrize("name", ROAD)
def test_staged_road_chain_is_the_oracle(name):
    """the stage-by-stage restatement the mistakes are seeded into equals oracle.pipeline.road_width_tail, field for field"""
    c = cc.road_cases()[name]
    ref, model = cc.road_expected(name)
    for fr, o, m in zip(c.frames, ref, model):
        d = cc.road_diff(dict(m, n_road=None), _oracle_as_compared(o))
        assert d is None, (name, fr.label, d)
        assert m["n_road"] == fr.n_passed >= o["n_in"]


def test_routes(capsys):
    """every frame reaches the routes it claims; each chain's cases reach all six routes.  Prints case x frame x stage x route."""
    lines, seen_road, seen_fence = [], set(), set()
    for name in ROAD:
        for fr, m in zip(cc.road_cases()[name].frames, cc.road_expected(name)[1]):
            lines.append(f"road  {name:15s} {fr.label:18s} " + "  ".join(f"{s}.{w}={r}" for (s, w), r in m["routes"].items()))
            seen_road.update(m["routes"].values())
            for k, want in fr.claims.items():
                assert m["routes"][k] == want, (name, fr.label, k, m["routes"][k], want)
    for name in FENCE:
        for fr, m in zip(cc.fence_cases()[name].frames, cc.fence_expected(name)):
            lines.append(f"fence {name:15s} {fr.label:18s} " + "  ".join(f"{s}.{w}={r}" for (s, w), r in m["routes"].items()))
            seen_fence.update(m["routes"].values())
            for k, want in fr.claims.items():
                assert m["routes"][k] == want, (name, fr.label, k, m["routes"][k], want)
    with capsys.disabled():
        print("\nroute table (case, frame, stage.median = route)\n" + "\n".join(lines))
    assert seen_road == set(cc.ROUTES), seen_road
    assert seen_fence == set(cc.ROUTES), seen_fence


def test_mixed_batch_shape():
    """the sizes after the z-cut are the ones the batch is built for, and the two slice sizes of cmp_slice both occur"""
    model = cc.road_expected("mixed")[1]
    assert sorted(m["n_zcut"] for m in model) == [0, 1, cc.SWITCH - 1, cc.SWITCH, cc.SWITCH + 1, 70_001]
    assert [m["n_zcut"] for m in model] != sorted(m["n_zcut"] for m in model)          # shuffled batch positions
    by = {fr.label: m for fr, m in zip(cc.road_cases()["mixed"].frames, model)}
    assert by["hit16384_nanx"]["n_mad_y"] == cc.SWITCH and by["hit16384_nanx"]["n_mad_x"] == 0      # all rows, then the NaN exit
    assert by["overflow70001"]["n_mad_y"] < 70_001 and by["overflow70001"]["found"]
    cap_frames = cc.road_cases()["capacity"]
    assert cap_frames.frames[1].n_passed > cap_frames.cap == len(cap_frames.frames[1].xyz)


def test_end_point_and_fence_patterns():
    tied, nowin = cc.road_expected("end_points")[1]
    assert tied["found"] and min(tied["ties"]) >= 3, tied.get("ties")
    assert not nowin["found"] and nowin["n_ror"] > 0
    main = {fr.label: m for fr, m in zip(cc.fence_cases()["main"].frames, cc.fence_expected("main"))}
    z = main["straddle9000"]["thr_in_z"]
    assert tuple(np.nonzero(~(abs(z) < 35.0))[0]) == cc.STRADDLE and len(z) == 9000
    assert 4 * cc.TB - 6 in cc.STRADDLE and 4 * cc.TB + 6 in cc.STRADDLE and 8 * cc.TB in cc.STRADDLE
    sw = main["switch_l"]
    assert sw["counts"][3:5] == (cc.SWITCH, cc.SWITCH - 1)
    sw = cc.fence_expected("even")[1]
    assert sw["counts"][3:5] == (cc.SWITCH - 1, cc.SWITCH)
    ev = cc.fence_expected("even")[0]
    assert ev["counts"][3] % 2 == 0 and ev["counts"][3] >= cc.SWITCH
    assert main["right_const"]["counts"][4] > 0 and main["right_const"]["counts"][6] == 0 and not main["right_const"]["ok"]
    assert main["no_fence"]["counts"] == (0,) * 7 and main["nan_row"]["counts"][1] == 0
    for name, frac in (("keep_all", 1.0), ("keep_none", 0.0)):
        for m in cc.fence_expected(name):
            kept, n = m["kept"]["thr"]
            assert kept == frac * n and n > 0


def test_stage_liveness():
    """the oracle alone: every stage keeps more than nothing and fewer than all rows on some non-degenerate frame (a filter that
    keeps everything, or nothing, cannot pass), and the end points are found on at least half of those frames"""
    live = {s: [] for s in ROAD_STAGES}
    found = []
    for name in ROAD:
        for fr, m in zip(cc.road_cases()[name].frames, cc.road_expected(name)[1]):
            if fr.degenerate:
                continue
            found.append(m["found"])
            for s in ROAD_STAGES:
                if s in m["kept"] and 0 < m["kept"][s][0] < m["kept"][s][1]:
                    live[s].append((name, fr.label))
    assert all(live.values()), {s: len(v) for s, v in live.items()}
    assert sum(found) * 2 >= len(found), found
    live = {s: [] for s in FENCE_STAGES}
    ok = []
    for name in FENCE:
        for fr, m in zip(cc.fence_cases()[name].frames, cc.fence_expected(name)):
            if fr.degenerate or name == "keep_none":
                continue
            ok.append(m["ok"])
            assert not (m["rank_deficient_left"] or m["rank_deficient_right"])
            for s in FENCE_STAGES:
                if s in m["kept"] and 0 < m["kept"][s][0] < m["kept"][s][1]:
                    live[s].append((name, fr.label))
    assert all(live.values()), {s: len(v) for s, v in live.items()}
    assert all(ok), ok


# where each mistake is looked for first (any case may catch it; these are the ones built for it)
_ROAD_ORDER = {"a_upper_middle": ["even_ties"], "b_miss_nearest": ["mixed"], "c_frame0_median": ["even_ties", "mixed"],
               "d_slice_last_row": ["small_pair", "capacity"], "e_overflow_truncate": ["mixed"], "f_last_tied": ["end_points"]}
_FENCE_ORDER = {"a_upper_middle": ["even"], "b_miss_nearest": ["main"], "c_frame0_median": ["even"], "e_overflow_truncate": ["main"]}


@pytest.mark.parametrize("mistake", list(cc.MISTAKES))
def test_seeded_mistake_is_caught(mistake, capsys):
    """each mistake, seeded into the numpy restatement of the chain, changes a field that test_gpu_pcl_chains.py compares"""
    hits = []
    for name in _ROAD_ORDER[mistake]:
        c = cc.road_cases()[name]
        good = cc.road_expected(name)[1]
        bad = cc.road_chain(c.frames, c.params, c.cap, mistake=mistake)
        for fr, g, b in zip(c.frames, good, bad):
            d = cc.road_diff(g, b)
            if d is not None and not fr.rank_deficient:
                hits.append(f"road {name}/{fr.label}: {d}")
    for name in _FENCE_ORDER.get(mistake, []):
        c = cc.fence_cases()[name]
        good = cc.fence_expected(name)
        planes = [None] * len(c.frames)
        bad = cc.fence_chain(c.frames, planes, c.params, mistake=mistake)
        for fr, g, b in zip(c.frames, good, bad):
            d = cc.fence_diff(dict(g, ok=False), b)
            if d is not None:
                hits.append(f"fence {name}/{fr.label}: {d}")
    with capsys.disabled():
        print(f"\nmistake {mistake} ({cc.MISTAKES[mistake]}): " + ("; ".join(hits) if hits else "NOT CAUGHT"))
    assert any(h.startswith("road") for h in hits), mistake
    if mistake in _FENCE_ORDER:
        assert any(h.startswith("fence") for h in hits), mistake
