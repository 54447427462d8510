"""GPU parity of the two batched chains the pipeline runs, Engine.road_width (sd_road_width: the multi-block forms at B > 1) and
Engine.fence_to_fence (sd_fence_to_fence: the only caller of the single-workgroup, in-place forms -- mad_filter_kernel<true>,
plane_filter_kernel<true>, filter_coord_kernel, block_median_fast, block_compact with input and output aliased), on the crafted
clouds of tests/pcl_chain_cases.py against the oracle.  tests/test_pcl_chain_cases_cpu.py shows on the CPU that these clouds reach
every branch of the medians and that six seeded mistakes each change a field compared here.

Rank-deficient plane fits (fewer than three points, or all points collinear in (u, v)) are outside the parity contract: the kernel
solves centred normal equations (det == 0 or rounding noise), the oracle's scipy.linalg.lstsq returns the minimum-norm solution.
Such frames are compared up to the stage before the fit and held to invariants after it."""
from dataclasses import asdict

import numpy as np
import pytest

import pcl_chain_cases as cc
from gpu_common import RoadWidthParams, dev, engine
from semantic_depth_amd.engine import FenceParams

pytestmark = pytest.mark.gpu

ROAD = [n for n in cc.ROAD_CASES if n not in ("mixed_reversed", "rank_deficient")]
FENCE = [n for n in cc.FENCE_CASES if n != "main_reversed"]
PLANE_TOL = dict(rtol=1e-8, atol=1e-10)          # as in test_gpu_pcl.py


@pytest.fixture(scope="module")
def eng():
    e = engine(256, 512, 8, "resnet50", load=())[0]
    assert e.cap == 131072
    return e


def _pack(frames, cap):
    """(B, cap, 3) tensors; the rows past a frame's count hold a sentinel no filter would keep silently"""
    B = len(frames)
    xyz = np.full((B, cap, 3), 777.0, np.float32)
    rgb = np.full((B, cap, 3), 201, np.uint8)
    for b, fr in enumerate(frames):
        assert len(fr.xyz) <= cap
        xyz[b, :len(fr.xyz)], rgb[b, :len(fr.rgb)] = fr.xyz, fr.rgb
    return dev(xyz), dev(rgb), dev(np.int32([fr.n_passed for fr in frames]))


def _run_road(eng, frames, params, cap=None):
    xyz, rgb, n = _pack(frames, cap or eng.cap)
    res, fin, frgb, nfin = eng.road_width(xyz, n, RoadWidthParams(**asdict(params)), want_final=True, road_rgb=rgb)
    nfin = nfin.cpu().numpy()
    fin, frgb = fin.cpu().numpy(), frgb.cpu().numpy()
    return eng.records(res), [fin[b, :nfin[b]] for b in range(len(frames))], [frgb[b, :nfin[b]] for b in range(len(frames))], res


def _check_road_frame(tag, fr, rec, fin, frgb, ref, upto=len(cc.ROAD_COUNTS)):
    """one frame against oracle.pipeline.road_width_tail: the seven counts, the final cloud and its colours in full, the end points
    and the plane.  ``upto`` < 7: only the counts before that stage (a rank-deficient fit follows)."""
    got = tuple(int(rec[k]) for k in cc.ROAD_COUNTS)
    want = (fr.n_passed,) + tuple(int(ref[k]) for k in cc.ROAD_COUNTS[1:])
    print(tag, fr.label, "counts", got, "oracle", want)
    assert got[:upto] == want[:upto], (tag, fr.label, got, want)
    if upto < len(cc.ROAD_COUNTS):
        return
    assert len(fin) == got[-1]
    assert np.array_equal(fin.astype(np.float64), ref.get("points", np.zeros((0, 3))), equal_nan=True), (tag, fr.label, "final xyz")
    assert np.array_equal(frgb.astype(np.float64), np.asarray(ref.get("colors", np.zeros((0, 3))), np.float64)), (tag, fr.label, "final rgb")
    assert bool(rec["found"]) == ref["found"], (tag, fr.label, rec["found"], ref["found"])
    if ref["found"]:
        assert float(rec["x_left"]) == ref["x_left"] and float(rec["x_right"]) == ref["x_right"] and float(rec["width"]) == ref["width"], \
            (tag, fr.label, rec["x_left"], rec["x_right"], rec["width"], ref["x_left"], ref["x_right"], ref["width"])
        assert np.array_equal(rec["left_pt"].astype(np.float64), ref["left_pt"]), (tag, fr.label, rec["left_pt"], ref["left_pt"])
        assert np.array_equal(rec["right_pt"].astype(np.float64), ref["right_pt"]), (tag, fr.label, rec["right_pt"], ref["right_pt"])
    else:
        assert np.isnan(rec["width"]) and np.isnan(rec["x_left"]) and np.isnan(rec["x_right"])
    if ref["plane"] is not None:
        assert np.allclose(rec["plane"], cc.plane_vec(ref["plane"]), **PLANE_TOL), (tag, fr.label, rec["plane"], ref["plane"])


def _same_frame(a, b, ia, ib):
    """frame ia of run a and frame ib of run b are the same bytes: record, final cloud, colours"""
    return (a[0][ia].tobytes() == b[0][ib].tobytes() and np.array_equal(a[1][ia], b[1][ib], equal_nan=True)
            and np.array_equal(a[2][ia], b[2][ib]))


@pytest.mark.parametrize("name", ROAD)
def test_road_chain_vs_oracle(eng, name):
    c = cc.road_cases()[name]
    assert not any(fr.rank_deficient for fr in c.frames)
    recs, fins, rgbs, _ = _run_road(eng, c.frames, c.params, c.cap)
    for b, (fr, ref) in enumerate(zip(c.frames, cc.road_expected(name)[0])):
        _check_road_frame(name, fr, recs[b], fins[b], rgbs[b], ref)


def test_road_reversed_batch_is_the_same_frames(eng):
    """the mixed batch in reversed order: every frame's record, cloud and colours are the forward batch's, permuted (per-frame
    state -- MedG[b], blk_cnt[b*CMP_G+g], params[b*CMP_PARAMS], the grid meta -- indexed by the right b), and equal the oracle"""
    fwd, rev = cc.road_cases()["mixed"], cc.road_cases()["mixed_reversed"]
    a = _run_road(eng, fwd.frames, fwd.params)
    r = _run_road(eng, rev.frames, rev.params)
    B = len(fwd.frames)
    for b, (fr, ref) in enumerate(zip(rev.frames, cc.road_expected("mixed_reversed")[0])):
        _check_road_frame("mixed_reversed", fr, r[0][b], r[1][b], r[2][b], ref)
        assert _same_frame(a, r, B - 1 - b, b), (fr.label, a[0][B - 1 - b], r[0][b])


def test_road_call_history(eng):
    """the mixed batch, a B = 2 batch of small clouds, the mixed batch again on one handle: all three equal their oracles, the first
    and the third are the same bytes (nothing of a launch survives in MedG / blk_cnt / the arenas)"""
    mixed, small = cc.road_cases()["mixed"], cc.road_cases()["small_pair"]
    first = _run_road(eng, mixed.frames, mixed.params)
    mid = _run_road(eng, small.frames, small.params)
    third = _run_road(eng, mixed.frames, mixed.params)
    for tag, case, run in (("first", mixed, first), ("small_pair", small, mid), ("third", mixed, third)):
        for b, (fr, ref) in enumerate(zip(case.frames, cc.road_expected(case.name)[0])):
            _check_road_frame(tag, fr, run[0][b], run[1][b], run[2][b], ref)
    for b in range(len(mixed.frames)):
        assert _same_frame(first, third, b, b), mixed.frames[b].label


def test_road_rank_deficient_frames(eng):
    """two rows / a cloud collinear in (x, z) reach the plane fit: compared with the oracle up to the stage before it, then only
    invariants; the ordinary frame between them is the same bytes as in a launch without them"""
    c = cc.road_cases()["rank_deficient"]
    refs = cc.road_expected("rank_deficient")[0]
    recs, fins, rgbs, _ = _run_road(eng, c.frames, c.params)
    normal = [b for b, fr in enumerate(c.frames) if not fr.rank_deficient]
    alone = _run_road(eng, [c.frames[b] for b in normal], c.params)
    for b, (fr, ref) in enumerate(zip(c.frames, refs)):
        if not fr.rank_deficient:
            _check_road_frame("rank_deficient", fr, recs[b], fins[b], rgbs[b], ref)
            assert _same_frame((recs, fins, rgbs), alone, b, normal.index(b)), fr.label
            continue
        assert ref["n_mad_x"] >= 2                                   # the fit does see the degenerate cloud
        _check_road_frame("rank_deficient", fr, recs[b], fins[b], rgbs[b], ref, upto=cc.ROAD_COUNTS.index("n_plane"))
        got = [int(recs[b][k]) for k in cc.ROAD_COUNTS]
        assert all(x >= y for x, y in zip(got, got[1:])), got       # counts never increase along the chain
        assert len(fins[b]) == got[-1]
        if got[-1] == 0:
            assert recs[b]["found"] == 0 and np.isnan(recs[b]["width"])
    # one row after the z-cut: MAD = 0 ends the frame before the fit; the fit of one row would have det == 0 exactly
    one = next(b for b, fr in enumerate(cc.road_cases()["mixed"].frames) if fr.label == "zcut1")
    r = _run_road(eng, cc.road_cases()["mixed"].frames, cc.road_cases()["mixed"].params)[0][one]
    assert r["n_zcut"] == 1 and r["n_plane"] == 0 and r["found"] == 0


# ------------------------------------------------------------------------------------------ fence chain
def _run_fence(eng, frames, params, roads):
    rx, _, rn = _pack(roads, eng.cap)
    rw = eng.road_width(rx, rn, RoadWidthParams(**asdict(cc.FENCE_ROAD_PARAMS)))
    xyz, rgb, n = _pack(frames, eng.cap)
    res, cl = eng.fence_to_fence(xyz, n, rw, FenceParams(**asdict(params)), fence_rgb=rgb, want_clouds=True)
    rec = eng.f2f_records(res)
    out = []
    for b in range(len(frames)):
        nl, nr = int(rec[b]["counts"][5]), int(rec[b]["counts"][6])
        out.append(dict(rec=rec[b], left=cl["left_xyz"][b, :nl].cpu().numpy(), left_rgb=cl["left_rgb"][b, :nl].cpu().numpy(),
                        right=cl["right_xyz"][b, :nr].cpu().numpy(), right_rgb=cl["right_rgb"][b, :nr].cpu().numpy()))
    return out


def _check_fence_frame(tag, fr, got, ref):
    """all seven counts, both final clouds and their colours in full, both planes, ok, dist and left_pt"""
    rec = got["rec"]
    counts = tuple(int(v) for v in rec["counts"])
    print(tag, fr.label, "counts", counts, "oracle", ref["counts"])
    assert not (ref["rank_deficient_left"] or ref["rank_deficient_right"])
    assert counts == ref["counts"], (tag, fr.label, counts, ref["counts"])
    for side in ("left", "right"):
        assert got[side].dtype == ref[side].dtype == np.float32
        assert np.array_equal(got[side], ref[side], equal_nan=True), (tag, fr.label, side, "xyz")
        assert np.array_equal(got[side + "_rgb"], ref[side + "_rgb"]), (tag, fr.label, side, "rgb")
        if ref["plane_" + side] is not None:
            assert np.allclose(rec["plane_" + side], cc.plane_vec(ref["plane_" + side]), **PLANE_TOL), \
                (tag, fr.label, side, rec["plane_" + side], ref["plane_" + side])
    assert bool(rec["ok"]) == ref["ok"], (tag, fr.label, rec["ok"], ref["ok"])
    if ref["ok"]:
        assert abs(rec["dist"] - ref["dist"]) <= 1e-9 * ref["dist"], (tag, fr.label, rec["dist"], ref["dist"])
        assert np.allclose(rec["left_pt"], ref["left_pt"], rtol=1e-9, atol=1e-9), (tag, fr.label, rec["left_pt"], ref["left_pt"])


@pytest.mark.parametrize("name", FENCE)
def test_fence_chain_vs_oracle(eng, name):
    c = cc.fence_cases()[name]
    got = _run_fence(eng, c.frames, c.params, cc.fence_road_frames(len(c.frames)))
    for fr, g, ref in zip(c.frames, got, cc.fence_expected(name)):
        _check_fence_frame(name, fr, g, ref)


def test_fence_reversed_batch_is_the_same_frames(eng):
    """the main fence batch (and its road clouds) in reversed order: the forward batch's frames, permuted, byte for byte"""
    c = cc.fence_cases()["main"]
    roads = cc.fence_road_frames(len(c.frames))
    a = _run_fence(eng, c.frames, c.params, roads)
    r = _run_fence(eng, c.frames[::-1], c.params, roads[::-1])
    B = len(c.frames)
    for b, fr in enumerate(c.frames):
        ga, gr = a[b], r[B - 1 - b]
        assert ga["rec"].tobytes() == gr["rec"].tobytes(), (fr.label, ga["rec"], gr["rec"])
        for k in ("left", "left_rgb", "right", "right_rgb"):
            assert np.array_equal(ga[k], gr[k], equal_nan=True), (fr.label, k)
