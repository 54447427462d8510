"""Crafted clouds for the two batched chains the pipeline runs (sd_road_width, sd_fence_to_fence), a numpy model of which
branch of the kernels' median a column reaches, and the chains restated stage by stage on the oracle's functions so that a
seeded mistake can replace one step.

Nothing here is a reference for VALUES: those come from oracle.pcl / oracle.o3d / oracle.pipeline.  ``median_bracket`` models
only the DECISION of block_median_fast / med_sample + med_collect + med_pick (csrc/pcl.hip); its constants are parsed from the
kernels' constexpr lines, so a retune re-validates the cases (tests/test_pcl_chain_cases_cpu.py) instead of hollowing them.
"""
from __future__ import annotations

import functools
import os
import re
import warnings
from dataclasses import dataclass, field

import numpy as np

from oracle import o3d as oracle_o3d
from oracle import pcl as oracle_pcl
from oracle import pipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PCL_HIP = os.path.join(ROOT, "semantic_depth_amd", "csrc", "pcl.hip")


def kernel_constants(path: str = PCL_HIP) -> dict:
    """MED_S, MED_D, MED_CAP, CMP_G and TB as csrc/pcl.hip declares them."""
    src = open(path).read()
    out = {}
    for name in ("MED_S", "MED_D", "MED_CAP", "CMP_G", "TB"):
        m = re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, src)
        assert m, f"constexpr int {name} not found in {path}"
        out[name] = int(m.group(1))
    return out


K = kernel_constants()
MED_S, MED_D, MED_CAP, CMP_G, TB = (K[k] for k in ("MED_S", "MED_D", "MED_CAP", "CMP_G", "TB"))
SWITCH = 4 * MED_S                 # n below this takes the plain radix select
ROUTES = ("empty", "small", "nan", "hit", "miss", "overflow")


# ------------------------------------------------------------------------------------------ route model
def f2key(v):
    """the kernels' monotone float32 -> uint32 key"""
    u = np.ascontiguousarray(v, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def key2f(k):
    k = np.asarray(k, np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def median_bracket(column) -> dict:
    """the decision of block_median_fast / med_*, in the kernel's order of tests: n < 4*MED_S, NaN, systematic sample at
    (j*n)//MED_S, sample ranks ts -/+ MED_D clamped, cnt > MED_CAP, r1 < below or r2 >= below + cnt."""
    v = np.ascontiguousarray(column, np.float32)
    n = int(v.shape[0])
    if n == 0:
        return dict(route="empty", n=0)
    if n < SWITCH:
        return dict(route="small", n=n)
    if np.isnan(v).any():
        return dict(route="nan", n=n)
    keys = f2key(v)
    samp = np.sort(keys[(np.arange(MED_S, dtype=np.int64) * n) // MED_S])
    r1, r2 = (n - 1) // 2, n // 2
    ts = (r1 * MED_S) // n
    klo, khi = samp[max(ts - MED_D, 0)], samp[min(ts + MED_D, MED_S - 1)]
    inside = (keys >= klo) & (keys <= khi)
    below, cnt = int((keys < klo).sum()), int(inside.sum())
    if cnt > MED_CAP:
        route = "overflow"
    elif r1 < below or r2 >= below + cnt:
        route = "miss"
    else:
        route = "hit"
    return dict(route=route, n=n, klo=klo, khi=khi, below=below, cnt=cnt, r1=r1, r2=r2, inside=inside, keys=keys)


def median_route(column) -> str:
    return median_bracket(column)["route"]


# ------------------------------------------------------------------------------------------ the six seeded mistakes
MISTAKES = {
    "a_upper_middle": "even-n median takes the upper middle element",
    "b_miss_nearest": "a bracket miss returns the bracket's nearest element instead of falling back",
    "c_frame0_median": "the MAD predicate of frame b uses frame 0's median",
    "d_slice_last_row": "compaction drops the last row of each 256-row slice segment when the segment is full",
    "e_overflow_truncate": "overflow truncates the collected keys at MED_CAP and selects from them anyway",
    "f_last_tied": "the end-point pick takes the last tied row, not the first",
}


def _median(values, mistake=None):
    """np.median of a float32 column, or what one of the median mistakes would return instead"""
    v = np.ascontiguousarray(values, np.float32)
    n = v.shape[0]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        exact = np.median(v) if n else np.float32(np.nan)
    if mistake is None or n == 0 or np.isnan(v).any():
        return exact
    if mistake == "a_upper_middle":
        return np.sort(v)[n // 2] if n % 2 == 0 else exact
    if mistake in ("b_miss_nearest", "e_overflow_truncate"):
        b = median_bracket(v)
        if mistake == "b_miss_nearest" and b["route"] == "miss":
            return key2f(b["klo"] if b["r1"] < b["below"] else b["khi"])[()]
        if mistake == "e_overflow_truncate" and b["route"] == "overflow":
            buf = np.sort(b["keys"][b["inside"]][:MED_CAP])          # (the device order is arbitrary; row order is one of them)
            pick = lambda r: key2f(buf[min(max(r - b["below"], 0), MED_CAP - 1)])[()]
            return np.float32((pick(b["r1"]) + pick(b["r2"])) / np.float32(2.0))
    return exact


def _compact(keep, mistake=None):
    """the keep mask after the multi-block compaction (cmp_count + cmp_scatter walk each slice in 256-row segments)"""
    if mistake == "d_slice_last_row":
        keep = keep.copy()
        n = keep.shape[0]
        for i0 in range(0, n - 255, 256):          # slices are multiples of 256 rows, so segments start at multiples of 256
            if keep[i0:i0 + 256].all():
                keep[i0 + 255] = False
    return keep


# ------------------------------------------------------------------------------------------ the chains, stage by stage
def _mad_keep(v, thr, mistake, med_of_frame0=None):
    """oracle.pcl.mad_penalty(v) < thr with its three steps open: (keep, med, dev)"""
    med = _median(v, mistake)
    dev = abs(v - med)
    m = _median(dev, mistake)
    used = med if med_of_frame0 is None else med_of_frame0
    with np.errstate(divide="ignore", invalid="ignore"):
        keep = 0.6745 * abs(v - used) / m < thr
    return keep, med, dev


def _plane_keep(pts, axis, thr):
    u, v, dep = oracle_pcl._PLANE_COLS[axis]
    C = oracle_pcl.fit_plane(pts, axis)
    resid = C[0] * pts[:, u] + C[1] * pts[:, v] - pts[:, dep] + C[2]
    return abs(resid) < thr, oracle_pcl.plane_coefficients(C, axis)


ROAD_COUNTS = ("n_road", "n_zcut", "n_mad_y", "n_mad_x", "n_plane", "n_sor", "n_ror")


def road_chain(frames, p: pipeline.RoadWidthParams, cap=None, mistake=None):
    """oracle.pipeline.road_width_tail for a batch, one stage at a time (with ``mistake`` None it IS that function: the CPU test
    asserts it).  ``frames``: list of Frame.  Returns one dict per frame with the compared fields, the median routes and the
    column entering every MAD stage."""
    med_mist = mistake if mistake in ("a_upper_middle", "b_miss_nearest", "e_overflow_truncate") else None
    outs, med0 = [], {}
    for b, fr in enumerate(frames):
        n_in = fr.xyz.shape[0] if cap is None else min(fr.xyz.shape[0], cap)
        pts, col = fr.xyz[:n_in], fr.rgb[:n_in]
        o = dict(n_road=fr.n_passed, plane=None, routes={}, kept={})

        def step(keep, name, n_before):
            nonlocal pts, col
            keep = _compact(keep, mistake)
            pts, col = pts[keep], col[keep]
            o[name] = len(pts)
            o["kept"][name] = (len(pts), n_before)

        step(pts[:, 2] < -p.z_cut, "n_zcut", len(pts))
        for name, axis, thr in (("n_mad_y", 1, p.mad_y), ("n_mad_x", 0, p.mad_x)):
            v = pts[:, axis]
            keep, med, dev = _mad_keep(v, thr, med_mist, med0.get(name) if (mistake == "c_frame0_median" and b > 0) else None)
            if b == 0:
                med0[name] = med
            o["routes"][(name[2:], "col")] = median_route(v)
            o["routes"][(name[2:], "dev")] = median_route(dev)
            step(keep, name, len(pts))
        if len(pts) >= 1:
            keep, o["plane"] = _plane_keep(pts, 1, p.plane_thr)
            step(keep, "n_plane", len(pts))
        else:
            o["n_plane"] = 0
        if p.use_o3d:
            step(oracle_o3d.statistical_outlier_mask(pts, p.sor_k, p.sor_ratio)[0], "n_sor", len(pts))
            step(oracle_o3d.radius_outlier_mask(pts, p.ror_n, p.ror_r), "n_ror", len(pts))
        else:
            o["n_sor"] = o["n_ror"] = len(pts)
        pts = pts.astype(np.float64)
        o["points"], o["colors"] = pts, col
        z = pts[:, 2]
        depth = p.depth - p.depth_offset
        seg = pts[(z < -(depth - 0.05)) & (z > -(depth + 0.05))]
        o["found"] = len(seg) > 0
        o["n_window"] = len(seg)
        if o["found"]:
            xs = seg[:, 0]
            pick = -1 if mistake == "f_last_tied" else 0
            o["left_pt"], o["right_pt"] = seg[xs == xs.min()][pick], seg[xs == xs.max()][pick]
            o["ties"] = (int((xs == xs.min()).sum()), int((xs == xs.max()).sum()))
            o["x_left"], o["x_right"] = float(o["left_pt"][0]), float(o["right_pt"][0])
            o["width"] = float(abs(o["left_pt"][0] - o["right_pt"][0]))
        outs.append(o)
    return outs


def road_oracle(frames, p: pipeline.RoadWidthParams, cap=None):
    """the expected records: oracle.pipeline.road_width_tail itself on the first ``cap`` rows of every frame"""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return [pipeline.road_width_tail(fr.xyz[:cap], fr.rgb[:cap], p) for fr in frames]


FENCE_COUNTS = ("n_fence", "n_mad_y", "n_thr", "n_left", "n_right", "n_left_final", "n_right_final")


def fence_chain(frames, road_planes, p: pipeline.FenceParams, mistake=None):
    """oracle.pipeline.fence_tail one stage at a time, every stage an oracle.pcl function (or, under a median mistake, its
    restatement above), stopping a side where nothing is left instead of raising from an empty lstsq."""
    med_mist = mistake if mistake in ("a_upper_middle", "b_miss_nearest", "e_overflow_truncate") else None
    outs, med0 = [], {}
    for b, (fr, road_plane) in enumerate(zip(frames, road_planes)):
        o = dict(routes={}, kept={}, plane_left=None, plane_right=None, ok=False)

        def mad(pts, col, axis, thr, name):
            v = pts[:, axis]
            keep, med, dev = _mad_keep(v, thr, med_mist, med0.get(name) if (mistake == "c_frame0_median" and b > 0) else None)
            if b == 0:
                med0[name] = med
            o["routes"][(name, "col")] = median_route(v)
            o["routes"][(name, "dev")] = median_route(dev)
            o["kept"][name] = (int(keep.sum()), len(pts))
            if mistake is None:
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore", RuntimeWarning)
                    ref = oracle_pcl.remove_noise_by_mad(pts, col, axis, thr)
                assert np.array_equal(ref[0], pts[keep], equal_nan=True)
            return pts[keep], col[keep]

        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            pts, col = mad(fr.xyz, fr.rgb, 1, p.mad_y, "mad_y")
            n_mad_y = len(pts)
            o["thr_in_z"] = pts[:, 2].copy()
            pts, col = oracle_pcl.threshold_complete(pts, col, 2, p.z_max)
            o["kept"]["thr"] = (len(pts), n_mad_y)
            l, lc, r, rc = oracle_pcl.extract_pcls(pts, col)
        counts = [fr.n_passed, n_mad_y, len(pts), len(l), len(r)]
        for side, s_pts, s_col, thr in (("left", l, lc, p.mad_left), ("right", r, rc, p.mad_right)):
            s_pts, s_col = mad(s_pts, s_col, 0, thr, "mad_" + side)
            o["n_%s_mad" % side] = len(s_pts)
            o["rank_deficient_" + side] = 0 < len(s_pts) < 3
            if len(s_pts) > 0:
                n_before = len(s_pts)
                s_pts, s_col, o["plane_" + side] = oracle_pcl.remove_noise_by_fitting_plane(s_pts, s_col, axis=0, threshold=p.plane_thr)
                o["kept"]["plane_" + side] = (len(s_pts), n_before)
            o[side], o[side + "_rgb"] = s_pts, s_col
            counts.append(len(s_pts))
        o["counts"] = tuple(counts)
        if counts[5] > 0 and counts[6] > 0 and road_plane is not None:
            lp = oracle_pcl.planes_intersection_at_certain_depth(road_plane, o["plane_left"], p.depth)
            rp = oracle_pcl.planes_intersection_at_certain_depth(road_plane, o["plane_right"], p.depth)
            o.update(ok=True, left_pt=lp[0], right_pt=rp[0], dist=float(oracle_pcl.compute_distance_in_3D(lp, rp)))
        outs.append(o)
    return outs


# ------------------------------------------------------------------------------------------ cloud builders
@dataclass
class Frame:
    label: str
    xyz: np.ndarray                     # (n, 3) float32: the rows the tensor holds
    rgb: np.ndarray                     # (n, 3) uint8
    n_passed: int = -1                  # the device count handed to the call (> len(xyz) for a clamped fuse)
    degenerate: bool = False            # emptiness / rank deficiency is the point of this frame
    rank_deficient: bool = False        # its plane fit has < 3 points or collinear (u, v): outside the parity contract
    claims: dict = field(default_factory=dict)     # {(stage, "col" | "dev"): route} this frame is built to reach

    def __post_init__(self):
        self.xyz = np.ascontiguousarray(self.xyz, np.float32)
        self.rgb = np.ascontiguousarray(self.rgb, np.uint8)
        if self.n_passed < 0:
            self.n_passed = len(self.xyz)


def _colours(rng, n):
    return rng.integers(0, 256, (n, 3), dtype=np.uint8)


def _interleave(rng, kept, rejects):
    """rejects inserted at random positions; the kept rows stay in their order"""
    if len(rejects) == 0:
        return kept
    at = np.sort(rng.integers(0, len(kept) + 1, len(rejects)))
    return np.insert(kept, at, rejects, axis=0)


def road_rows(rng, n, density=300.0, slope=0.0, y_noise=0.02, y_out=0.01, x_out=0.01, z_near=-8.2, bounded_y=False):
    """n rows of a road patch that pass the z-cut: ``density`` points per square metre (so that the radius filter's 80
    neighbours within 0.5 m exist away from the rim), depth from z_near on, across the 9.98 m window whenever n allows it."""
    area = n / density
    if area >= 7.0 * 3.5:
        x_half, length = 3.5, area / 7.0
    else:
        x_half, length = max(area / 7.0, 0.05), 3.5
    x = rng.uniform(-x_half, x_half, n)
    z = rng.uniform(z_near - length, z_near, n)
    y = -1.5 + slope * (z + 10.0) + (rng.uniform(-1.5, 1.5, n) if bounded_y else rng.standard_normal(n)) * y_noise
    k = int(n * y_out)
    if k:
        i = rng.choice(n, k, replace=False)
        y[i] += rng.choice([-1.0, 1.0], k) * rng.uniform(0.5, 1.5, k)          # beyond the MAD cut of ~22 MAD = 0.3 m
    k = int(n * x_out)
    if k:
        i = rng.choice(n, k, replace=False)
        x[i] = rng.choice([-1.0, 1.0], k) * rng.uniform(1.7, 2.0, k) * x_half   # beyond 2.96 MAD = 1.48 x_half
    return np.stack([x, y, z], 1).astype(np.float32)


def zcut_rejects(rng, k):
    """rows the z-cut drops (z >= -7)"""
    return np.stack([rng.uniform(-4, 4, k), rng.uniform(-2, -1, k), rng.uniform(-6.9, -1.0, k)], 1).astype(np.float32)


def _frame(rng, label, kept, n_reject=0, **kw):
    xyz = _interleave(rng, kept, zcut_rejects(rng, n_reject))
    return Frame(label, xyz, _colours(rng, len(xyz)), **kw)


def _sample_rows(n):
    return (np.arange(MED_S, dtype=np.int64) * n) // MED_S


def _routes(y_col, y_dev, x_col, x_dev):
    return {("mad_y", "col"): y_col, ("mad_y", "dev"): y_dev, ("mad_x", "col"): x_col, ("mad_x", "dev"): x_dev}


def mixed_frames(seed=101):
    """sizes AFTER the z-cut: 0, 1, 4*MED_S - 1, 4*MED_S, 4*MED_S + 1 and 70 001, in shuffled batch positions.
    4*MED_S = 16384 is also where cmp_slice goes from 256 to 512 rows."""
    rng = np.random.default_rng(seed)
    f = {}
    f["zero"] = _frame(rng, "zcut0", np.zeros((0, 3), np.float32), 300, degenerate=True,
                       claims=_routes("empty", "empty", "empty", "empty"))
    f["one"] = _frame(rng, "zcut1", road_rows(rng, 1), 200, degenerate=True, claims=_routes("small", "small", "empty", "empty"))
    f["small"] = _frame(rng, "small16383", road_rows(rng, SWITCH - 1), 700, claims=_routes("small", "small", "small", "small"))
    # exactly 4*MED_S rows, bounded y noise so that the y stage keeps every row, and one row (NaN, y, -inf): it passes the
    # z-cut and the y stage and poisons the x column of a cloud that is still 4*MED_S long -> the NaN exit
    k = road_rows(rng, SWITCH, y_out=0.0, bounded_y=True)
    k[SWITCH // 3] = (np.nan, -1.5, -np.inf)
    f["hit_nan"] = _frame(rng, "hit16384_nanx", k, 900, claims=_routes("hit", "hit", "nan", "nan"))
    # every sampled row an outlier in y: the sample brackets the outliers, not the median
    k = road_rows(rng, SWITCH + 1, y_out=0.0)
    k[_sample_rows(SWITCH + 1), 1] = 2.0
    f["miss"] = _frame(rng, "miss16385", k, 500, claims=_routes("miss", "miss", "small", "small"))
    # 45 % of the y column equal to the median VALUE, at ranks 5.5 % .. 50.5 %: the bracket holds the tie block and the 3.9 % of
    # distinct values above it (> MED_CAP keys, not all equal); the deviations' median lies just above the zeros -> MAD > 0
    n = 70_001
    k = road_rows(rng, n, y_out=0.0, x_out=0.01)
    n_tie, n_lo = int(0.45 * n), int(0.055 * n)
    y = np.full(n, -1.5)
    y[n_tie:n_tie + n_lo] = -1.5 - (0.001 + 0.5 * rng.uniform(0, 1, n_lo) ** 3)
    y[n_tie + n_lo:] = -1.5 + (0.001 + 0.5 * rng.uniform(0, 1, n - n_tie - n_lo) ** 3)
    k[:, 1] = rng.permutation(y).astype(np.float32)
    f["overflow"] = _frame(rng, "overflow70001", k, 2000, claims=_routes("overflow", "hit", "hit", "hit"))
    order = ["miss", "zero", "overflow", "one", "hit_nan", "small"]
    return [f[k] for k in order]


@dataclass
class RoadCase:
    name: str
    frames: list
    params: pipeline.RoadWidthParams = field(default_factory=pipeline.RoadWidthParams)
    cap: int | None = None              # cap dimension of the tensors (None = the handle's)


def even_ties_frames(seed=202):
    rng = np.random.default_rng(seed)
    # even n; x: a tight cluster of n/2 rows in [-0.1, 0] and n/2 rows spread over [1, 4]: the two middle elements are ~1 m apart,
    # the exact median (their mean, 0.5) keeps x in about [-1.3, 2.3], the upper middle (1.0) keeps every row
    n = 20_000
    k = road_rows(rng, n, y_out=0.0, x_out=0.0, bounded_y=True)
    x = np.concatenate([rng.uniform(-0.1, 0.0, n // 2), rng.uniform(1.0, 4.0, n // 2)])
    k[:, 0] = rng.permutation(x).astype(np.float32)
    even = _frame(rng, "even_gap20000", k, 0, claims={("mad_y", "col"): "hit", ("mad_x", "col"): "hit"})
    small = _frame(rng, "small3000", road_rows(rng, 3000), 100, claims={("mad_y", "col"): "small"})
    k = road_rows(rng, 20_001, y_out=0.01)
    k[:, 1] = np.round(k[:, 1] * 100) / 100             # heavy ties: a handful of distinct y values, x on a 0.25 m lattice
    k[:, 0] = np.round(k[:, 0] * 4) / 4
    ties = _frame(rng, "ties20001", k, 300, claims={("mad_y", "col"): "hit"})
    return [even, small, ties]


def capacity_frames(seed=303, cap=24_576):
    """tensors with a cap dimension below the handle's; the second frame's count is the true count of a clamped fuse"""
    rng = np.random.default_rng(seed)
    a = _frame(rng, "plain20000", road_rows(rng, 20_000), 2000)
    b = _frame(rng, "clamped30000", road_rows(rng, 28_000), 2000)
    true_n = len(b.xyz)
    b = Frame(b.label, b.xyz[:cap], b.rgb[:cap], n_passed=true_n)
    return [a, b], cap


def end_point_frames(seed=404):
    rng = np.random.default_rng(seed)
    k = road_rows(rng, 17_000, x_out=0.0)
    k[:, 0] = np.clip(k[:, 0], -3.3, 3.3)               # ~3 % of the rows tied at each of x = -3.3 and x = +3.3, inside the window too
    tied = _frame(rng, "tied_ends17000", k, 400)
    k = road_rows(rng, 9000, z_near=-10.6)              # nothing nearer than 10.6 m: the depth window is empty
    nowin = _frame(rng, "empty_window9000", k, 200, degenerate=True)
    return [tied, nowin]


def small_pair_frames(seed=505):
    rng = np.random.default_rng(seed)
    a = _frame(rng, "small3001", road_rows(rng, 3001), 150)
    b = Frame("no_road", np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8), degenerate=True)
    return [a, b]


def sloped_frames(seed=606):
    """a road that climbs 0.3 m per metre: the y column's MAD is ~1 m, so rows lifted 8 m pass the y stage and only the plane
    stage (5 m) drops them -- the one stage the level clouds never make work"""
    rng = np.random.default_rng(seed)
    k = road_rows(rng, 18_000, slope=0.3, y_out=0.0)
    i = rng.choice(len(k), 150, replace=False)
    k[i, 1] += 8.0
    # seven rows of a full-rank patch: fewer than sor_k neighbours exist, and the radius filter then drops them all
    tiny = np.float32([[-0.9, -1.52, -9.1], [0.7, -1.49, -9.6], [0.1, -1.51, -10.2], [-0.4, -1.5, -10.9], [0.9, -1.48, -9.3],
                       [-0.2, -1.53, -9.9], [0.4, -1.5, -10.5]])
    return [_frame(rng, "slope18000", k, 500), _frame(rng, "tiny7", tiny, 3), _frame(rng, "small2500", road_rows(rng, 2500), 100)]


def rank_deficient_frames(seed=707):
    """two rows that survive both MAD stages (two values: equal deviations, penalty 0.6745), a cloud collinear in (x, z), and an
    ordinary frame whose results must not depend on its neighbours"""
    rng = np.random.default_rng(seed)
    two = Frame("two_rows", np.float32([[-1.0, -1.5, -9.0], [1.0, -1.4, -11.0]]), _colours(rng, 2), degenerate=True, rank_deficient=True)
    t = rng.uniform(-1, 1, 400)
    line = np.stack([2.0 * t, -1.5 + rng.standard_normal(400) * 0.02, -10.0 + 1.5 * t], 1).astype(np.float32)
    col = Frame("collinear400", line, _colours(rng, 400), degenerate=True, rank_deficient=True)
    normal = _frame(rng, "small4000", road_rows(rng, 4000), 100)
    return [two, normal, col]


ROAD_CASES = ("mixed", "mixed_reversed", "even_ties", "capacity", "end_points", "small_pair", "sloped", "rank_deficient")
FENCE_CASES = ("main", "main_reversed", "even", "keep_all", "keep_none")


@functools.lru_cache(maxsize=None)
def road_cases() -> dict:
    cf, cap = capacity_frames()
    mixed = mixed_frames()
    return {
        "mixed": RoadCase("mixed", mixed),
        "mixed_reversed": RoadCase("mixed_reversed", mixed[::-1]),
        "even_ties": RoadCase("even_ties", even_ties_frames()),
        "capacity": RoadCase("capacity", cf, cap=cap),
        "end_points": RoadCase("end_points", end_point_frames()),
        "small_pair": RoadCase("small_pair", small_pair_frames()),
        "sloped": RoadCase("sloped", sloped_frames()),
        "rank_deficient": RoadCase("rank_deficient", rank_deficient_frames()),
    }


@functools.lru_cache(maxsize=None)
def road_expected(name: str):
    """(oracle records, staged model) of one road case; computed once per process"""
    c = road_cases()[name]
    if name == "mixed_reversed":
        o, m = road_expected("mixed")
        return o[::-1], m[::-1]
    return road_oracle(c.frames, c.params, c.cap), road_chain(c.frames, c.params, c.cap)


# ------------------------------------------------------------------------------------------ fence clouds
def wall_rows(rng, n, x0, slope_y=0.0, noise=0.03, y_lo=-2.0, y_hi=0.5):
    """n rows of a near-vertical wall x = x0 + slope_y * y + 0.01 * z + noise that pass the y stage and |z| < 35"""
    y = rng.uniform(y_lo, y_hi, n)
    z = rng.uniform(-30.0, -5.0, n)
    x = x0 + slope_y * y + 0.01 * z + rng.standard_normal(n) * noise
    return np.stack([x, y, z], 1).astype(np.float32)


def fence_frame(rng, label, left, right, n_y_out=0, n_far=0, shuffle=True, **kw):
    """left and right wall rows in shuffled order (each side keeps its own row order), plus rows the y stage drops (8 m up) and rows
    beyond z_max"""
    side = np.concatenate([np.zeros(len(left), bool), np.ones(len(right), bool)])
    if shuffle:
        side = rng.permutation(side)
    xyz = np.empty((len(side), 3), np.float32)
    xyz[~side], xyz[side] = left, right
    extra = []
    if n_y_out:
        e = wall_rows(rng, n_y_out, 5.5)
        e[:, 1] = rng.uniform(7.0, 9.0, n_y_out)
        extra.append(e)
    if n_far:
        e = wall_rows(rng, n_far, -5.0)
        e[:, 2] = rng.uniform(-60.0, -36.0, n_far)
        extra.append(e)
    if extra:
        xyz = _interleave(rng, xyz, np.concatenate(extra))
    return Frame(label, xyz, _colours(rng, len(xyz)), **kw)


def _x_outliers(rng, left, k, dx):
    i = rng.choice(len(left), k, replace=False)
    left[i, 0] += dx
    return left


@dataclass
class FenceCase:
    name: str
    frames: list
    params: pipeline.FenceParams = field(default_factory=pipeline.FenceParams)


STRADDLE = tuple(range(TB * 4 - 6, TB * 4 + 7, 2)) + tuple(range(TB * 8 - 6, TB * 8 + 7, 2))


def pattern_frame(seed=818):
    """no row fails the y stage; the rows failing |z| < 35 are every other row across 4090 .. 4102 and 8186 .. 8198, the two
    boundaries of block_compact's TB*4-row iterations"""
    rng = np.random.default_rng(seed)
    fr = fence_frame(rng, "straddle9000", wall_rows(rng, 4600, -5.0, 0.3, 0.05), wall_rows(rng, 4400, 5.5))
    fr.xyz[list(STRADDLE), 2] = -40.0
    return fr


def fence_main_frames(seed=909):
    rng = np.random.default_rng(seed)
    fr = []
    # both sides >= 4*MED_S; the left wall leans (0.3 m per metre of y), so rows 1.2 m off it pass its MAD stage (cut ~1.4 m) and
    # fall to the plane stage (1 m)
    left = _x_outliers(rng, wall_rows(rng, 18_000, -5.0, 0.3, 0.05), 200, 1.2)
    # the right wall leans 2 m per metre of y (MAD ~1.25 m, cut 1.85 m): rows 1.3 m off it reach its plane stage too
    right = _x_outliers(rng, wall_rows(rng, 17_000, 7.0, 2.0), 300, 1.3)
    fr.append(fence_frame(rng, "hit", _x_outliers(rng, left, 150, -3.0), right, 300, 400,
                          claims={("mad_y", "col"): "hit", ("mad_left", "col"): "hit", ("mad_right", "col"): "hit"}))
    left = wall_rows(rng, 18_001, -5.0, 0.3, 0.05)
    left[_sample_rows(len(left)), 0] = -9.0
    fr.append(fence_frame(rng, "left_miss", left, wall_rows(rng, 16_500, 5.5), 0, 300, claims={("mad_left", "col"): "miss"}))
    fr.append(fence_frame(rng, "switch_l", wall_rows(rng, SWITCH, -5.0, 0.3, 0.05), wall_rows(rng, SWITCH - 1, 5.5), 200, 100,
                          claims={("mad_left", "col"): "hit", ("mad_right", "col"): "small"}))
    # 45 % of the y column one value, at ranks 5.5 % .. 50.5 % (as in the road chain's overflow frame)
    n = 42_000
    left, right = wall_rows(rng, n // 2, -5.0, 0.3, 0.05), wall_rows(rng, n // 2, 5.5)
    f = fence_frame(rng, "y_ties", left, right, claims={("mad_y", "col"): "overflow"})
    n_tie, n_lo = int(0.45 * n), int(0.055 * n)
    y = np.full(n, -0.75)
    y[n_tie:n_tie + n_lo] = -0.75 - (0.001 + 1.2 * rng.uniform(0, 1, n_lo) ** 3)
    y[n_tie + n_lo:] = -0.75 + (0.001 + 1.2 * rng.uniform(0, 1, n - n_tie - n_lo) ** 3)
    f.xyz[:, 1] = rng.permutation(y).astype(np.float32)
    fr.append(f)
    f = fence_frame(rng, "nan_row", wall_rows(rng, 9000, -5.0), wall_rows(rng, 9000, 5.5), degenerate=True, claims={("mad_y", "col"): "nan"})
    f.xyz[7777] = (np.nan, np.nan, -np.inf)
    fr.append(f)
    fr.append(Frame("no_fence", np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8), degenerate=True, claims={("mad_y", "col"): "empty"}))
    right = wall_rows(rng, 5000, 5.5)
    right[:, 0] = 5.5                                    # constant x: MAD = 0, the right side ends empty
    fr.append(fence_frame(rng, "right_const", wall_rows(rng, 6000, -5.0, 0.3, 0.05), right, 100, 100, degenerate=True))
    fr.append(pattern_frame())
    return fr


def fence_even_frames(seed=1010):
    """even n on the LDS path: the left side has 4*MED_S + 2 rows, half in a tight cluster at x = -5 and half spread over
    [-14, -6]; beside a switch frame mirrored (right side at 4*MED_S, left one row below)"""
    rng = np.random.default_rng(seed)
    n = SWITCH + 2
    left = wall_rows(rng, n, -5.0)
    x = np.concatenate([rng.uniform(-5.05, -5.0, n // 2), rng.uniform(-14.0, -6.0, n // 2)])
    left[:, 0] = rng.permutation(x).astype(np.float32)
    a = fence_frame(rng, "left_even_gap", left, wall_rows(rng, 17_000, 5.5), claims={("mad_left", "col"): "hit"})
    b = fence_frame(rng, "switch_r", wall_rows(rng, SWITCH - 1, -5.0, 0.3, 0.05), wall_rows(rng, SWITCH, 5.5), 100, 200,
                    claims={("mad_left", "col"): "small", ("mad_right", "col"): "hit"})
    return [a, b]


def fence_small_frames(seed=1111):
    rng = np.random.default_rng(seed)
    return [pattern_frame(), fence_frame(rng, "plain3000", wall_rows(rng, 1500, -5.0, 0.3, 0.05), wall_rows(rng, 1500, 5.5), 30, 30)]


@functools.lru_cache(maxsize=None)
def fence_cases() -> dict:
    main = fence_main_frames()
    small = fence_small_frames()
    return {
        "main": FenceCase("main", main),
        "main_reversed": FenceCase("main_reversed", main[::-1]),
        "even": FenceCase("even", fence_even_frames()),
        "keep_all": FenceCase("keep_all", small, pipeline.FenceParams(z_max=100.0)),
        "keep_none": FenceCase("keep_none", small, pipeline.FenceParams(z_max=1.0)),
    }


FENCE_ROAD_PARAMS = pipeline.RoadWidthParams(use_o3d=False)


@functools.lru_cache(maxsize=None)
def fence_road_frames(n_frames: int, seed=1212):
    """a plain planar road cloud per frame, each with its own tilt: only its plane enters the fence chain"""
    rng = np.random.default_rng(seed)
    return [_frame(rng, f"road{b}", road_rows(rng, 2500 + 37 * b, slope=0.01 * b), 50) for b in range(n_frames)]


@functools.lru_cache(maxsize=None)
def fence_expected(name: str):
    c = fence_cases()[name]
    if name == "main_reversed":
        return fence_expected("main")[::-1]
    roads = fence_road_frames(len(c.frames))
    planes = [r["plane"] for r in road_oracle(roads, FENCE_ROAD_PARAMS)]
    return fence_chain(c.frames, planes, c.params)


# ------------------------------------------------------------------------------------------ compared fields
def road_diff(a, b):
    """first compared field (the fields tests/test_gpu_pcl_chains.py compares) in which two road results differ, or None"""
    for k in ROAD_COUNTS:
        if a[k] != b[k]:
            return k
    if not np.array_equal(a["points"], b["points"], equal_nan=True):
        return "final_xyz"
    if not np.array_equal(a["colors"], b["colors"]):
        return "final_rgb"
    if a["found"] != b["found"]:
        return "found"
    if a["found"]:
        for k in ("x_left", "x_right", "width"):
            if a[k] != b[k]:
                return k
        for k in ("left_pt", "right_pt"):
            if not np.array_equal(a[k], b[k]):
                return k
    if (a["plane"] is None) != (b["plane"] is None):
        return "plane"
    if a["plane"] is not None and not np.allclose(plane_vec(a["plane"]), plane_vec(b["plane"]), rtol=1e-8, atol=1e-10, equal_nan=True):
        return "plane"
    return None


def fence_diff(a, b):
    if a["counts"] != b["counts"]:
        return "counts[%d]" % next(i for i in range(7) if a["counts"][i] != b["counts"][i])
    for side in ("left", "right"):
        if not np.array_equal(a[side], b[side], equal_nan=True):
            return side + "_xyz"
        if not np.array_equal(a[side + "_rgb"], b[side + "_rgb"]):
            return side + "_rgb"
        pa, pb = a["plane_" + side], b["plane_" + side]
        if (pa is None) != (pb is None) or (pa is not None and not np.allclose(plane_vec(pa), plane_vec(pb), rtol=1e-8, atol=1e-10)):
            return "plane_" + side
    if a["ok"] != b["ok"]:
        return "ok"
    if a["ok"] and not (np.isclose(a["dist"], b["dist"], rtol=1e-9, atol=0) and np.allclose(a["left_pt"], b["left_pt"], rtol=1e-9, atol=1e-9)):
        return "dist"
    return None


def plane_vec(c):
    return np.array([c[k] for k in ("Cx", "Cy", "Cz", "C")], np.float64)
