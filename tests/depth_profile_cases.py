"""Seeded clouds and depth lists for the depth profile (sd_road_width_profile / sd_f2f_profile), the host calls behind ctypes, and a numpy
restatement of the two-launch route (slices, partials, merge, permutation) in which a seeded mistake can replace one step.

Nothing here is a reference for VALUES: those come from oracle.pcl.  The slice length, the slice cap and the partial kernel's thread
count are parsed from csrc/rw_profile.hpp, TB from csrc/pcl.hip, so a retune re-validates the cases instead of hollowing them.
"""
from __future__ import annotations

import ctypes as C
import functools
import os
import re
from dataclasses import dataclass

import numpy as np

from oracle import pcl as oracle_pcl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "semantic_depth_amd", "csrc")


def _constant(path: str, name: str) -> int:
    m = re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, open(path).read())
    assert m, f"constexpr int {name} not found in {path}"
    return int(m.group(1))


SLICE = _constant(os.path.join(CSRC, "rw_profile.hpp"), "RWP_SLICE")
MAX_SLICES = _constant(os.path.join(CSRC, "rw_profile.hpp"), "RWP_MAX_SLICES")
THREADS = _constant(os.path.join(CSRC, "rw_profile.hpp"), "RWP_THREADS")
TB = _constant(os.path.join(CSRC, "pcl.hip"), "TB")          # end_points_kernel's workgroup, the single-cloud call compared on the GPU
WINDOW, OFFSET = 0.05, 0.02                                   # the oracle's literal window; the reference's depth - 0.02
CAP = 3 * SLICE + 1
MAX_DEPTHS = 256


# ------------------------------------------------------------------------------------------ depth lists
def _exact_edge_depths():
    """two-decimal depths at which forming e = d - OFFSET first matters: the other order of the two subtractions, -(d -/+ WINDOW) +
    OFFSET, rounds an edge to a different double, and a float32 z lies on one of the two, so that the strict comparison admits it
    under one order only.  Found by search, so the list follows the arithmetic and not a table."""
    out = []
    for c in range(200, 700):
        d = c / 100.0
        e = d - OFFSET
        good = (-(e + WINDOW), -(e - WINDOW))
        bad = (-(d + WINDOW) + OFFSET, -(d - WINDOW) + OFFSET)
        for z in (np.float64(np.float32(v)) for v in good + bad):
            if (good[0] < z < good[1]) != (bad[0] < z < bad[1]):
                out.append(d)
                break
    return out


EXACT = _exact_edge_depths()


@functools.lru_cache(maxsize=None)
def depth_lists() -> dict:
    on_edge = [d for d in EXACT if any(float(np.float32(v)) == v for v in window_of(d))]      # an edge that IS a float32: <= shows there
    assert EXACT and on_edge, (EXACT, on_edge)
    # unsorted; 2.5 twice; 3.0 / 3.04 / 3.08 overlap (a row at depth 3.02 lies in all three windows); two depths from EXACT
    nine = [5.0, 2.5, 3.04, on_edge[-1], 3.0, 2.5, 3.08, EXACT[0], 2.0]
    return {
        "one": np.array([3.0]),
        "nine": np.array(nine, np.float64),
        "equal256": np.full(MAX_DEPTHS, 3.0),
        "spread256": np.linspace(2.0, 6.98, MAX_DEPTHS),
    }


def all_depths():
    return np.unique(np.concatenate(list(depth_lists().values())))


def window_of(d, window=WINDOW, offset=OFFSET):
    e = np.float64(d) - np.float64(offset)
    return -(e + window), -(e - window)          # lo, hi


# ------------------------------------------------------------------------------------------ clouds
@dataclass
class Batch:
    name: str
    labels: list
    xyz: np.ndarray              # (B, cap, 3) float32, rows past a frame's count hold a sentinel inside a window
    n: np.ndarray                # (B,) int32 as handed to the call (may pass cap)
    lists: tuple = ("one", "nine", "equal256", "spread256")

    @property
    def cap(self):
        return self.xyz.shape[1]

    def rows(self, b):
        return self.xyz[b, :min(int(self.n[b]), self.cap)]


def _random_rows(rng, n, z_lo=-7.2, z_hi=-1.8):
    return np.stack([rng.normal(0.0, 2.5, n), rng.normal(-1.2, 0.05, n), rng.uniform(z_lo, z_hi, n)], 1).astype(np.float32)


def _pack(name, frames, n_passed=None, cap=CAP, **kw):
    """rows past a frame's count: x = -777 at z inside the window of depth 3.0 -- a read past n would win every left end"""
    xyz = np.empty((len(frames), cap, 3), np.float32)
    xyz[:] = (-777.0, 0.0, -2.98)
    for b, (_, rows) in enumerate(frames):
        assert len(rows) <= cap
        xyz[b, :len(rows)] = rows
    n = np.int32([len(r) for _, r in frames] if n_passed is None else n_passed)
    return Batch(name, [l for l, _ in frames], xyz, n, **kw)


def _edge_rows(rng):
    """for every depth of every list: the float32 nearest to lo and to hi, and its two float32 neighbours"""
    zs = []
    for d in all_depths():
        for edge in window_of(d):
            c = np.float32(edge)
            zs += [np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf))]
    zs = rng.permutation(np.array(zs, np.float32))
    rows = _random_rows(rng, len(zs))
    rows[:, 2] = zs
    return rows


def _tie_rows(rng):
    """3 SLICE + 1 rows; in the window of depth 3.0 the minimum x sits on rows of slice 0 and slice 1, the maximum on rows of slice 1
    and slice 2 (their y and z differ, so which tied row is taken shows in the end points)"""
    rows = _random_rows(rng, 3 * SLICE + 1)
    rows[:, 0] = np.clip(rows[:, 0], -9.0, 9.0)
    for r, x, z in ((100, -9.5, -2.981), (SLICE + 50, -9.5, -2.979), (SLICE + 700, 9.5, -2.983), (2 * SLICE + 9, 9.5, -2.977)):
        rows[r] = (x, -1.0 - 0.001 * (r % 7), z)
    return rows


@functools.lru_cache(maxsize=None)
def batches() -> dict:
    rng = np.random.default_rng(20240)
    sizes = [(f"n{n}", _random_rows(rng, n)) for n in (0, 1, SLICE - 1, SLICE, SLICE + 1, 3 * SLICE + 1)]
    sizes[1] = ("n1", np.float32([[0.25, -1.2, -2.99]]))                      # the one row is inside the window of depth 3.0
    ties = _tie_rows(rng)
    far = _random_rows(rng, 900, -9.5, -7.6)
    single = np.concatenate([far[:400], np.float32([[1.5, -1.1, -4.98]]), far[400:]])     # one row in the window of depth 5.0, nothing else within 2 m
    miss = np.concatenate([_random_rows(rng, 700, -1.7, -0.4), _random_rows(rng, 700, -9.5, -7.6)])
    edges = [("over_cap", _random_rows(rng, CAP)), ("all_miss", miss), ("edge_rows", _edge_rows(rng)), ("ties", ties), ("single", single),
             ("ties_reversed", ties[::-1].copy())]
    n_edges = [CAP + 1000] + [len(r) for _, r in edges[1:]]
    # past SLICE * MAX_SLICES rows a workgroup walks more than one slice; its extremes sit in the wrapped part
    big = SLICE * MAX_SLICES + 300
    wrap = _random_rows(rng, big)
    wrap[:, 0] = np.clip(wrap[:, 0], -9.0, 9.0)
    wrap[big - 7] = (-9.5, -1.0, -2.98)
    wrap[big - 200] = (9.5, -1.0, -2.98)
    return {
        "sizes": _pack("sizes", sizes),
        "edges": _pack("edges", edges, n_edges),
        "wrap": _pack("wrap", [("wrap", wrap), ("short", wrap[:SLICE + 3])], cap=big, lists=("nine",)),
    }


# ------------------------------------------------------------------------------------------ the host calls
FIELDS = ("found", "left_pt", "right_pt", "x_left", "x_right", "width", "n_window")


def host_profile(xyz, depths, window=WINDOW, offset=OFFSET, fill=0xA5):
    """sd_road_width_profile_host on one cloud -> structured array [D] (raises on a refusal)"""
    from semantic_depth_amd import _lib as L
    from semantic_depth_amd.engine import RWP_DTYPE
    lib = L.load()
    xyz = np.ascontiguousarray(xyz, np.float32)
    d = np.ascontiguousarray(depths, np.float64)
    out = np.full(len(d) * RWP_DTYPE.itemsize, fill, np.uint8)
    st = lib.sd_road_width_profile_host(xyz.ctypes.data_as(C.c_void_p), len(xyz), d.ctypes.data_as(C.c_void_p), len(d), window, offset,
                                        out.ctypes.data_as(C.c_void_p))
    assert st == 0, st
    return out.view(RWP_DTYPE)


def host_f2f_profile(road_rec, f2f_rec, depths):
    """sd_f2f_profile_host on one frame's two records (numpy structured scalars) -> structured array [D]"""
    from semantic_depth_amd import _lib as L
    from semantic_depth_amd.engine import F2FP_DTYPE
    lib = L.load()
    d = np.ascontiguousarray(depths, np.float64)
    r, f = np.ascontiguousarray(road_rec).copy(), np.ascontiguousarray(f2f_rec).copy()
    out = np.full(len(d) * F2FP_DTYPE.itemsize, 0xA5, np.uint8)
    st = lib.sd_f2f_profile_host(r.ctypes.data_as(C.c_void_p), f.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p), len(d),
                                 out.ctypes.data_as(C.c_void_p))
    assert st == 0, st
    return out.view(F2FP_DTYPE)


# ------------------------------------------------------------------------------------------ the oracle, per (frame, depth)
def oracle_row(cloud64, depth, count_from=None):
    """oracle.pcl.get_end_points_of_road on the float64 cloud at depth - OFFSET, as the compared fields; n_window a direct numpy count"""
    left, right = oracle_pcl.get_end_points_of_road(cloud64, depth - OFFSET)
    z = cloud64[:, 2]
    lo, hi = window_of(depth)
    n_window = int(((z < hi) & (z > lo)).sum())
    if left is None:
        return dict(found=0, n_window=n_window)
    l, r = left[0], right[0]
    return dict(found=1, left_pt=l, right_pt=r, x_left=l[0], x_right=r[0], width=abs(l[0] - r[0]), n_window=n_window)


def row_diff(got, want):
    """first compared field in which a record (structured scalar or dict) differs from an expected row, or None"""
    if int(got["found"]) != int(want["found"]):
        return "found"
    if int(got["n_window"]) != int(want["n_window"]):
        return "n_window"
    if want["found"]:
        for k in ("left_pt", "right_pt"):
            if not np.array_equal(np.asarray(got[k], np.float64), np.asarray(want[k], np.float64)):
                return k
        for k in ("x_left", "x_right", "width"):
            if float(got[k]) != float(want[k]):
                return k
    return None


# ------------------------------------------------------------------------------------------ the route restated, with seeded mistakes
MISTAKES = {
    "a_le_edge": "<= at a window edge",
    "b_offset_after": "depth_offset applied after the window, -(d -/+ window) + offset",
    "c_last_tied": "the last tied row instead of the first",
    "d_one_slice": "slice 0's result instead of the merge",
    "e_last_slice_count": "the count of the last slice only",
    "f_sorted_order": "results left in sorted order",
    "g_dup_unwritten": "a duplicate depth left unwritten",
}


def restated(xyz, depths, mistake=None, window=WINDOW, offset=OFFSET):
    """the device route in numpy: sort the depths, per slice the (first-min, first-max, count) of every window, merge over the slices,
    scatter to the caller's index.  Returns a list of D rows (dicts of the compared fields)."""
    xyz = np.ascontiguousarray(xyz, np.float32)
    depths = np.asarray(depths, np.float64)
    D, n = len(depths), len(xyz)
    order = np.argsort(depths, kind="stable")
    x, z = xyz[:, 0].astype(np.float64), xyz[:, 2].astype(np.float64)
    G = max(1, -(-n // SLICE))
    out = [None] * D
    seen = set()
    for w, i in enumerate(order):
        d = depths[i]
        if mistake == "b_offset_after":
            lo, hi = -(d + window) + offset, -(d - window) + offset
        else:
            lo, hi = window_of(d, window, offset)
        inside = ((z <= hi) & (z >= lo)) if mistake == "a_le_edge" else ((z < hi) & (z > lo))
        best_l = best_r = None
        count = 0
        for g in range(G):
            idx = np.flatnonzero(inside[g * SLICE:(g + 1) * SLICE]) + g * SLICE
            if mistake == "e_last_slice_count":
                count = len(idx)
            else:
                count += len(idx)
            if len(idx) == 0 or (mistake == "d_one_slice" and g > 0):
                continue
            xs = x[idx]
            pick = (lambda m: idx[np.flatnonzero(m)[-1]]) if mistake == "c_last_tied" else (lambda m: idx[np.flatnonzero(m)[0]])
            l, r = pick(xs == xs.min()), pick(xs == xs.max())
            later = mistake == "c_last_tied"
            if best_l is None or x[l] < x[best_l] or (later and x[l] == x[best_l]):
                best_l = l
            if best_r is None or x[r] > x[best_r] or (later and x[r] == x[best_r]):
                best_r = r
        if best_l is None:
            row = dict(found=0, n_window=count)
        else:
            l, r = xyz[best_l].astype(np.float64), xyz[best_r].astype(np.float64)
            row = dict(found=1, left_pt=l, right_pt=r, x_left=l[0], x_right=r[0], width=abs(l[0] - r[0]), n_window=count)
        dst = w if mistake == "f_sorted_order" else int(i)
        if mistake == "g_dup_unwritten" and d in seen:
            continue
        seen.add(d)
        out[dst] = row
    return [r if r is not None else dict(found=0, n_window=0) for r in out]
