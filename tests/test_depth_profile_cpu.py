"""CPU: the host statements of the depth profile (sd_road_width_profile_host, sd_f2f_profile_host; the arithmetic of csrc/rw_profile.hpp
that the kernels of rw_profile.hip share) against oracle.pcl on the crafted clouds of tests/depth_profile_cases.py, the seeded mistakes
those clouds must tell apart, the refusals, and the profile text file."""
import ctypes as C
import io

import numpy as np
import pytest

import __graft_entry__ as graft
import depth_profile_cases as dc
import pcl_chain_cases as cc
from oracle import pcl as oracle_pcl
from semantic_depth_amd import _lib as L
from semantic_depth_amd import outputs
from semantic_depth_amd.engine import F2F_DTYPE, F2FP_DTYPE, RW_DTYPE, RWP_DTYPE


@pytest.fixture(scope="module")
def lib():
    graft.build()
    return L.load()


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


# ------------------------------------------------------------------------------------------ road profile
@pytest.mark.parametrize("name", sorted(dc.batches()))
def test_host_profile_equals_the_oracle_per_frame_and_depth(lib, name):
    bt = dc.batches()[name]
    checked = found = 0
    for b, label in enumerate(bt.labels):
        rows = bt.rows(b)
        cloud64 = rows.astype(np.float64)
        for lname in bt.lists:
            depths = dc.depth_lists()[lname]
            got = dc.host_profile(rows, depths)
            for i, d in enumerate(depths):
                if i and depths[i] == depths[i - 1] and lname == "equal256":
                    assert got[i].tobytes() == got[0].tobytes(), (name, label, i)      # 256 equal depths: 256 equal records
                    continue
                want = dc.oracle_row(cloud64, float(d))
                assert dc.row_diff(got[i], want) is None, (name, label, lname, i, d, dc.row_diff(got[i], want), got[i], want)
                if not want["found"]:
                    assert got[i]["width"].tobytes() == np.float64(np.nan).tobytes()              # the kernel's quiet NaNs
                    for k in ("x_left", "x_right", "left_pt", "right_pt"):
                        assert np.all(np.atleast_1d(got[i][k]).view(np.uint32) == 0x7FC00000), (name, label, k)
                checked += 1
                found += int(want["found"])
    print(f"{name}: {checked} (frame, depth) pairs against the oracle, {found} with a road segment")
    assert found > 0


def test_the_clouds_hold_what_they_claim():
    """n = 0 / 1 / SLICE -/+ 1 / 3 SLICE + 1, a count past cap, a frame that misses every window, a one-row window whose two ends
    coincide, rows on the float32 values around every edge, ties across slices, a reversed twin, rows past SLICE * MAX_SLICES"""
    S = dc.SLICE
    sizes, edges, wrap = (dc.batches()[k] for k in ("sizes", "edges", "wrap"))
    assert [int(v) for v in sizes.n] == [0, 1, S - 1, S, S + 1, 3 * S + 1] and len(sizes.labels) == len(edges.labels) == 6
    assert edges.n[0] > edges.cap and len(edges.rows(0)) == edges.cap
    e = dict(zip(edges.labels, range(6)))
    for lname, depths in dc.depth_lists().items():
        assert all(r["found"] == 0 and r["n_window"] == 0 for r in dc.host_profile(edges.rows(e["all_miss"]), depths)), lname
    nine = dc.depth_lists()["nine"]
    assert len(nine) == 9 and len(set(nine)) == 8 and list(nine) != sorted(nine)
    single = [r for r in dc.host_profile(edges.rows(e["single"]), nine) if r["found"]]
    assert len(single) == 1 and single[0]["n_window"] == 1 and single[0]["width"] == 0.0 and np.array_equal(single[0]["left_pt"], single[0]["right_pt"])
    # a row of depth 3.02 lies in the windows of 3.0, 3.04 and 3.08
    tri = dc.host_profile(np.float32([[0.0, 0.0, -3.02]]), [3.0, 3.04, 3.08])
    assert [int(r["n_window"]) for r in tri] == [1, 1, 1]
    # every edge value and its neighbours are rows of the edge frame
    z = set(edges.rows(e["edge_rows"])[:, 2].tolist())
    for d in dc.all_depths():
        for edge in dc.window_of(d):
            c = np.float32(edge)
            assert {float(c), float(np.nextafter(c, np.float32(-np.inf))), float(np.nextafter(c, np.float32(np.inf)))} <= z
    ties = edges.rows(e["ties"])
    inside = np.flatnonzero((ties[:, 2].astype(np.float64) < dc.window_of(3.0)[1]) & (ties[:, 2].astype(np.float64) > dc.window_of(3.0)[0]))
    xs = ties[inside, 0]
    lo_rows, hi_rows = inside[xs == xs.min()], inside[xs == xs.max()]
    assert len(lo_rows) == 2 and lo_rows[0] // S != lo_rows[1] // S and len(hi_rows) == 2 and hi_rows[0] // S != hi_rows[1] // S
    assert np.array_equal(edges.rows(e["ties_reversed"]), ties[::-1])
    assert wrap.n[0] > S * dc.MAX_SLICES and dc.THREADS >= dc.MAX_DEPTHS and dc.TB % 64 == 0


def test_seeded_mistakes_each_change_a_compared_field():
    """the restated route equals the oracle as it stands, and each of the seven mistakes changes a compared field somewhere"""
    table = {}
    for name, bt in dc.batches().items():
        for b, label in enumerate(bt.labels):
            rows = bt.rows(b)
            cloud64 = rows.astype(np.float64)
            for lname in bt.lists:
                depths = dc.depth_lists()[lname]
                want = None
                if lname in ("one", "nine"):
                    want = [dc.oracle_row(cloud64, float(d)) for d in depths]
                    plain = dc.restated(rows, depths)
                    assert all(dc.row_diff(g, w) is None for g, w in zip(plain, want)), (name, label, lname)
                for m in dc.MISTAKES:
                    if m in table or want is None:
                        continue
                    bad = dc.restated(rows, depths, m)
                    hit = next(((i, dc.row_diff(g, w)) for i, (g, w) in enumerate(zip(bad, want)) if dc.row_diff(g, w)), None)
                    if hit:
                        table[m] = (name, label, lname, hit[0], hit[1])
    print("%-20s %-52s %s" % ("mistake", "what", "first (batch, frame, list, depth index, field) it changes"))
    for m, what in dc.MISTAKES.items():
        print("%-20s %-52s %s" % (m, what, table.get(m)))
    assert len(dc.MISTAKES) >= 6 and set(table) == set(dc.MISTAKES), sorted(set(dc.MISTAKES) - set(table))


def test_the_index_range_equals_the_brute_force_set():
    """rw_profile.hpp's range rule seen through n_window: sum over the depths of n_window == the number of (row, window) pairs counted
    one window at a time, on the edge frame where every row sits on or next to an edge"""
    bt = dc.batches()["edges"]
    rows = bt.rows(bt.labels.index("edge_rows"))
    z = rows[:, 2].astype(np.float64)
    for lname, depths in dc.depth_lists().items():
        got = dc.host_profile(rows, depths)
        for i, d in enumerate(depths):
            lo, hi = dc.window_of(d)
            assert int(got[i]["n_window"]) == int(((z < hi) & (z > lo)).sum()), (lname, i)


# ------------------------------------------------------------------------------------------ fence profile
def _fence_records():
    c = cc.fence_cases()["main"]
    planes = [r["plane"] for r in cc.road_oracle(cc.fence_road_frames(len(c.frames)), cc.FENCE_ROAD_PARAMS)]
    road = np.zeros(len(c.frames), RW_DTYPE)
    f2f = np.zeros(len(c.frames), F2F_DTYPE)
    exp = cc.fence_expected("main")
    for b, (e, rp) in enumerate(zip(exp, planes)):
        road[b]["plane"] = cc.plane_vec(rp)
        f2f[b]["counts"] = e["counts"]
        for side in ("left", "right"):
            f2f[b]["plane_" + side] = cc.plane_vec(e["plane_" + side]) if e["plane_" + side] is not None else np.nan
    return c, planes, exp, road, f2f


def test_host_f2f_profile_equals_the_oracle(lib):
    c, planes, exp, road, f2f = _fence_records()
    depths = dc.depth_lists()["nine"]
    n_ok = n_empty = 0
    for b, e in enumerate(exp):
        got = dc.host_f2f_profile(road[b], f2f[b], depths)
        assert (got["reserved"] == 0).all()
        if e["counts"][5] > 0 and e["counts"][6] > 0:
            for i, d in enumerate(depths):
                lp = oracle_pcl.planes_intersection_at_certain_depth(planes[b], e["plane_left"], float(d))
                rp = oracle_pcl.planes_intersection_at_certain_depth(planes[b], e["plane_right"], float(d))
                dist = float(oracle_pcl.compute_distance_in_3D(lp, rp))
                assert got[i]["ok"] == 1 and abs(got[i]["dist"] - dist) <= 1e-9 * dist, (c.frames[b].label, d, got[i]["dist"], dist)
                assert np.allclose(got[i]["left_pt"], lp[0], rtol=1e-8, atol=0) and np.allclose(got[i]["right_pt"], rp[0], rtol=1e-8, atol=0)
            n_ok += 1
        else:
            assert (got["ok"] == 0).all() and np.isnan(got["dist"]).all(), (c.frames[b].label, got)
            assert all(r["dist"].tobytes() == np.float64(np.nan).tobytes() for r in got)
            n_empty += 1
    assert n_ok >= 4 and n_empty >= 1, (n_ok, n_empty)
    # finite planes but an empty side: ok = 0, whatever the solve gives
    j = next(b for b, e in enumerate(exp) if e["counts"][5] > 0 and e["counts"][6] > 0)
    f = f2f[j].copy()
    f["counts"][6] = 0
    assert (dc.host_f2f_profile(road[j], f, depths)["ok"] == 0).all()


# ------------------------------------------------------------------------------------------ refusals
def test_host_calls_refuse_bad_arguments(lib):
    xyz = np.zeros((4, 3), np.float32)
    d = np.array([3.0, 4.0])
    out = np.zeros(2 * 48, np.uint8)

    def rw(x=xyz, n=4, dd=d, D=2, w=0.05, off=0.02, o=out):
        return lib.sd_road_width_profile_host(None if x is None else _ptr(x), n, None if dd is None else _ptr(dd), D, w, off,
                                              None if o is None else _ptr(o))
    assert rw() == L.SD_OK and rw(x=None, n=0) == L.SD_OK
    big = np.full(L.SD_PROFILE_MAX_DEPTHS + 1, 3.0)
    for bad in (dict(x=None), dict(dd=None), dict(o=None), dict(n=-1), dict(D=0), dict(dd=big, D=len(big)), dict(w=0.0), dict(w=-0.05),
                dict(w=np.nan), dict(w=np.inf), dict(off=np.nan), dict(off=-np.inf), dict(dd=np.array([3.0, np.nan])),
                dict(dd=np.array([np.inf, 3.0]))):
        assert rw(**bad) == L.SD_ERR_INVALID, bad
    road, f2f = np.zeros(1, RW_DTYPE), np.zeros(1, F2F_DTYPE)
    fo = np.zeros(2 * 64, np.uint8)

    def ff(r=road, f=f2f, dd=d, D=2, o=fo):
        return lib.sd_f2f_profile_host(None if r is None else _ptr(r), None if f is None else _ptr(f), None if dd is None else _ptr(dd), D,
                                       None if o is None else _ptr(o))
    assert ff() == L.SD_OK
    for bad in (dict(r=None), dict(f=None), dict(dd=None), dict(o=None), dict(D=0), dict(dd=big, D=len(big)), dict(dd=np.array([3.0, np.nan]))):
        assert ff(**bad) == L.SD_ERR_INVALID, bad
    ws = lib.sd_rw_profile_workspace
    assert ws(32, 524288, 64) > 0 and ws(1, 1, 1) > 0 and ws(65535, 1, 256) > 0
    for B, cap, D in ((0, 8, 1), (-1, 8, 1), (65536, 8, 1), (1, 0, 1), (1, -5, 1), (1, 8, 0), (1, 8, 257), (1, 8, -1)):
        assert ws(B, cap, D) == 0, (B, cap, D)
    # the workspace grows with B and D, and with cap only up to the slice cap
    assert ws(2, 8, 4) > ws(1, 8, 4) and ws(1, 8, 5) > ws(1, 8, 4)
    assert ws(1, dc.SLICE * dc.MAX_SLICES, 4) == ws(1, 10 * dc.SLICE * dc.MAX_SLICES, 4) > ws(1, dc.SLICE, 4)


# ------------------------------------------------------------------------------------------ records and the text file
def test_struct_sizes():
    assert C.sizeof(L.sd_rw_depth_result) == RWP_DTYPE.itemsize == 48
    assert C.sizeof(L.sd_f2f_depth_result) == F2FP_DTYPE.itemsize == 64
    for dt, st in ((RWP_DTYPE, L.sd_rw_depth_result), (F2FP_DTYPE, L.sd_f2f_depth_result)):
        for name in dt.names:
            assert dt.fields[name][1] == getattr(st, name).offset, name
    assert L.SD_PROFILE_MAX_DEPTHS == 256


def test_write_profile_is_savetxt(tmp_path):
    bt = dc.batches()["sizes"]
    depths = dc.depth_lists()["nine"]
    rows = dc.host_profile(bt.rows(5), depths)
    assert rows["found"].any()
    f2f = np.zeros(len(depths), F2FP_DTYPE)
    f2f["dist"] = np.linspace(7.123456, 9.0, len(depths))
    f2f["ok"] = 1
    f2f["ok"][2] = 0
    empty = dc.host_profile(np.zeros((0, 3), np.float32), depths)                        # every value missing
    for tag, rr, ff in (("rw", rows, None), ("both", rows, f2f), ("empty", empty, f2f)):
        path = outputs.write_profile(str(tmp_path / f"{tag}.txt"), depths, rr, ff)
        cols = [depths, rr["found"], np.where(rr["found"] != 0, rr["width"], np.nan), np.where(rr["found"] != 0, rr["x_left"], np.nan),
                np.where(rr["found"] != 0, rr["x_right"], np.nan), rr["n_window"]]
        fmt = ["%1.4f", "%d", "%1.4f", "%1.4f", "%1.4f", "%d"]
        head = "depth found width x_left x_right n_window"
        if ff is not None:
            cols.append(np.where(ff["ok"] != 0, ff["dist"], np.nan))
            fmt.append("%1.4f")
            head += " dist_f2f"
        buf = io.BytesIO()
        np.savetxt(buf, np.stack([np.asarray(c, np.float64) for c in cols], 1), fmt=fmt, header=head)
        assert open(path, "rb").read() == buf.getvalue(), tag
    text = open(str(tmp_path / "empty.txt")).read().splitlines()
    assert text[0] == "# depth found width x_left x_right n_window dist_f2f" and text[1].split()[1:6] == ["0", "nan", "nan", "nan", "0"]
    with pytest.raises(ValueError):
        outputs.profile_text(depths[:3], rows)
