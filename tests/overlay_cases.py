"""Shared by tests/test_overlay_cpu.py and tests/test_gpu_overlay_device.py: the crafted records, profiles and cameras of the measurement
lines' tests, built from seeds (no network is needed), and an INDEPENDENT statement of the rule of include/semdepth.h: the projection in plain
Python floats (Python does not contract), the slots in plain loops, the paint rule in numpy int64 with exact Python integers where a square
leaves that range.  Nothing here reads csrc/overlay_rule.hpp's results; the host functions are called only by host_segments / host_draw."""
import math

import numpy as np

from semantic_depth_amd import outputs
from semantic_depth_amd.engine import F2F_DTYPE, F2FP_DTYPE, RW_DTYPE, RWP_DTYPE, Camera

NET = (128, 256)                     # the network size the cameras belong to; the images are other sizes, so the scales are no integers
MAX_COORD = 32768


def camera(rng) -> Camera:
    """a camera near the sequence tool's, scaled to NET; none of the three values is a float32"""
    return Camera(cx=NET[1] / 2 + float(rng.uniform(-3, 3)) + 0.01, cy=NET[0] / 2 + float(rng.uniform(-2, 2)) + 0.003,
                  f=60.0 + float(rng.uniform(0, 20)) + 0.0001, b=0.22, disp_mult=3800.0)


def point_at(cam: Camera, size, fx: float, fy: float, zn: float, net=NET):
    """the 3D point (float64) that lands near output pixel (fx * w, fy * h) at depth zn"""
    h, w = size
    xn = (fx * w + 0.5) * net[1] / w - 0.5
    yn = (fy * h + 0.5) * net[0] / h - 0.5
    return np.array([(xn - cam.cx) * zn / cam.f, (cam.cy - yn) * zn / cam.f, -zn], np.float64)


# ---- the frames of the pool: (road line, fence line, expected flag), the lines as ((fx, fy), (fx, fy)) or None; `tweak` edits the 3D points
def _pool():
    nan = float("nan")
    return [
        dict(rw=((0.2, 0.6), (0.8, 0.6)), f2f=None, flag=0),                                      # horizontal
        dict(rw=None, f2f=None, flag=0),                                                          # not found, nothing drawn
        dict(rw=((0.5, 0.3), (0.5, 0.9)), f2f=((0.1, 0.75), (0.9, 0.75)), flag=0),                # vertical, crossed by the fence line
        dict(rw=((0.1, 0.3), (0.9, 0.9)), f2f=((0.1, 0.9), (0.9, 0.3)), flag=0),                  # two diagonals of two colours crossing
        dict(rw=((0.4, 0.5), (0.4, 0.5)), f2f=None, flag=0),                                      # zero length: a disc
        dict(rw=((-0.3, -0.2), (0.5, 0.5)), f2f=((0.5, 0.6), (1.4, 1.3)), flag=0),                # beyond the left / top and the right / bottom side
        dict(rw=((0.2, 0.5), (0.8, 0.5)), f2f=((0.2, 0.8), (0.8, 0.8)), flag=1, tweak=("rw", "right", 2, 1.0)),      # an end point with Z >= 0
        dict(rw=((0.2, 0.5), (0.8, 0.5)), f2f=((0.3, 0.7), (0.7, 0.7)), flag=1, tweak=("rw", "left", 0, nan)),       # a NaN coordinate
        dict(rw=((0.3, 0.55), (0.7, 0.55)), f2f=((0.2, 0.8), (0.8, 0.8)), flag=1, tweak=("f2f", "right", "past_cap")),  # a coordinate past the cap
        dict(rw=((0.3, 0.4), (0.7, 0.4)), f2f=((0.2, 0.8), (0.8, 0.8)), flag=0, tweak=("f2f", "right", "under_cap")),  # ... and one just under it
        dict(rw=((0.2, 0.6), (0.8, 0.6)), f2f=None, flag=1, tweak=("rw", "left", 2, 0.0)),        # Z == 0
    ]


def build(B: int, h: int, w: int, D: int = 0, fence: bool = True, seed: int = 0, thickness: int = 3, profile_thickness: int = 1,
          clip_top: int = 0, first: int = 0) -> dict:
    """a batch of B frames from the pool (frame b is pool entry (first + b) % len) at h x w with a D-depth profile:
    dict(B, h, w, D, cams, records RW_DTYPE [B], f2f F2F_DTYPE [B] | None, profile RWP_DTYPE [B,D] | None, f2f_profile F2FP_DTYPE [B,D] | None,
    lines, clip_top, flags [B] expected)"""
    rng = np.random.default_rng(seed)
    pool = _pool()
    size = (h, w)
    cams = [camera(rng) for _ in range(B)]
    recs = np.zeros((B,), RW_DTYPE)
    f2 = np.zeros((B,), F2F_DTYPE)
    prof = np.zeros((B, D), RWP_DTYPE) if D else None
    fprof = np.zeros((B, D), F2FP_DTYPE) if D and fence else None
    flags = np.zeros((B,), np.int32)
    for b in range(B):
        spec, cam = pool[(first + b) % len(pool)], cams[b]
        zn = 10.0 + float(rng.uniform(-1, 1))
        recs[b]["width"] = np.nan
        recs[b]["left_pt"] = recs[b]["right_pt"] = np.nan
        f2[b]["dist"] = np.nan
        f2[b]["left_pt"] = f2[b]["right_pt"] = np.nan
        if spec["rw"] is not None:
            recs[b]["found"] = 1
            recs[b]["left_pt"] = point_at(cam, size, *spec["rw"][0], zn).astype(np.float32)
            recs[b]["right_pt"] = point_at(cam, size, *spec["rw"][1], zn).astype(np.float32)
            recs[b]["width"] = 4.0
        if spec["f2f"] is not None:
            f2[b]["ok"] = 1
            f2[b]["left_pt"] = point_at(cam, size, *spec["f2f"][0], zn)
            f2[b]["right_pt"] = point_at(cam, size, *spec["f2f"][1], zn)
            f2[b]["dist"] = 9.0
        tw = spec.get("tweak")
        flag = spec["flag"]
        if tw is not None:
            rec = recs[b] if tw[0] == "rw" else f2[b]
            if tw[2] == "past_cap":                          # 40000 pixels to the right of the image
                rec[tw[1] + "_pt"] = point_at(cam, size, 40000.0 / w, 0.8, zn)
            elif tw[2] == "under_cap":
                rec[tw[1] + "_pt"] = point_at(cam, size, 32000.0 / w, 0.8, zn)
            else:
                rec[tw[1] + "_pt"][tw[2]] = tw[3]
            if tw[0] == "f2f" and not fence:
                flag = 0                                      # (the fence record is not passed: nothing is skipped)
        if D:
            depths = np.linspace(5.0, 40.0, D) if D > 1 else np.array([12.0])
            if b % 2 == 1:
                depths = depths[::-1]                         # depths given in descending order
            for i, d in enumerate(depths):
                t = (d - 5.0) / 35.0                          # the road narrows and rises with the depth
                jx, jy = float(rng.uniform(-0.01, 0.01)), float(rng.uniform(-0.01, 0.01))
                half = 0.45 * (1.0 - t) + 0.02
                y = 0.95 - 0.6 * t
                prof[b, i]["found"] = 1
                prof[b, i]["left_pt"] = point_at(cam, size, 0.5 - half + jx, y + jy, d).astype(np.float32)
                prof[b, i]["right_pt"] = point_at(cam, size, 0.5 + half + jx, y - jy, d).astype(np.float32)
                prof[b, i]["width"] = 2 * half
                prof[b, i]["n_window"] = 5
                if fprof is not None:
                    fprof[b, i]["ok"] = 1
                    fprof[b, i]["left_pt"] = point_at(cam, size, 0.5 - half - 0.04, y + 0.01, d)
                    fprof[b, i]["right_pt"] = point_at(cam, size, 0.5 + half + 0.04, y + 0.01, d)
            if D >= 3 and b % 2 == 0:                         # a hole in the middle breaks the edge polylines
                prof[b, D // 2]["found"] = 0
                prof[b, D // 2]["left_pt"] = prof[b, D // 2]["right_pt"] = np.nan
                if fprof is not None:
                    fprof[b, 1]["ok"] = 0
            if D >= 2 and b % 4 == 3:                         # an entry whose left end does not project: two segments are skipped
                prof[b, 0]["left_pt"][2] = 1.0
                flag |= 1
        flags[b] = flag
    return dict(B=B, h=h, w=w, D=D, cams=cams, records=recs, f2f=f2 if fence else None, profile=prof, f2f_profile=fprof,
                lines=outputs.OverlayLines(thickness=thickness, profile_thickness=profile_thickness), clip_top=clip_top, flags=flags)


# the case set of the CPU tests: every property the rule has, at sizes a Python loop walks in well under a second
CASES = {
    "mixed_one_tile": dict(B=11, h=16, w=64, D=0, seed=1),
    "mixed_partial_tiles": dict(B=11, h=37, w=130, D=0, seed=2, thickness=1),
    "no_fence_records": dict(B=11, h=37, w=130, D=0, fence=False, seed=3),
    "thick_and_clipped": dict(B=4, h=120, w=200, D=0, seed=4, thickness=32, profile_thickness=32, clip_top=60),      # clip_top cuts the thick line of frame 0
    "profile_one_depth": dict(B=5, h=60, w=200, D=1, seed=5, profile_thickness=2),
    "profile_seven": dict(B=5, h=120, w=300, D=7, seed=6, clip_top=30),
    "profile_seven_no_fence": dict(B=4, h=37, w=130, D=7, fence=False, seed=7, first=3),
    "profile_256": dict(B=4, h=120, w=300, D=256, seed=8, first=2),
    "profile_thick": dict(B=2, h=90, w=160, D=7, seed=9, thickness=5, profile_thickness=32, clip_top=45, first=2),
}


def case(name: str) -> dict:
    return build(**CASES[name])


def prefilled(seed, *shape):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


# ---- the host statement (the only place the library is called) ----
def host_segments(c: dict, b: int):
    return outputs.overlay_segments(c["records"][b], c["cams"][b], NET, (c["h"], c["w"]), c["lines"], f2f=None if c["f2f"] is None else c["f2f"][b],
                                    profile=None if c["profile"] is None else c["profile"][b],
                                    f2f_profile=None if c["f2f_profile"] is None else c["f2f_profile"][b], clip_top=c["clip_top"])


def host_draw(img, c: dict):
    """(images [B,h,w,3], flags [B]) of the host statement on a copy of ``img``"""
    out, flags = np.array(img, copy=True), np.zeros((c["B"],), np.int32)
    for b in range(c["B"]):
        segs, flags[b] = host_segments(c, b)
        out[b] = outputs.draw_lines(out[b], segs, c["clip_top"])
    return out, flags


# ---- the independent statement ----
def py_project(cam, pt, size, mistakes=()):
    """section 1 of the rule in Python floats: (qx, qy) in 1/256 pixel, or None when the point is dropped"""
    cx, cy, f = float(np.float32(cam.cx)), float(np.float32(cam.cy)), float(np.float32(cam.f))
    X, Y, Z = float(pt[0]), float(pt[1]), float(pt[2])
    zn = -Z
    if not zn > 0:
        return None
    s = f / zn
    xn = cx + X * s
    yn = cy + Y * s if "flip_y" in mistakes else cy - Y * s
    sx, sy = float(size[1]) / float(NET[1]), float(size[0]) / float(NET[0])
    if "no_centre" in mistakes:
        xo, yo = xn * sx, yn * sy
    else:
        xo, yo = (xn + 0.5) * sx - 0.5, (yn + 0.5) * sy - 0.5
    if not (abs(xo) <= MAX_COORD and abs(yo) <= MAX_COORD):
        return None
    return int(math.floor(xo * 256 + 0.5)), int(math.floor(yo * 256 + 0.5))


def py_segments(c: dict, b: int, mistakes=()):
    """(segments [(ax, ay, bx, by, bgr, thickness)] in slot order, flag) of frame b"""
    cam, size, ln, D = c["cams"][b], (c["h"], c["w"]), c["lines"], c["D"]
    segs, flag = [], 0

    def join(a, bb, colour, thickness):
        nonlocal flag
        if a == "absent" or bb == "absent":
            return
        if a is None or bb is None:
            flag |= 1
            return
        segs.append((a[0], a[1], bb[0], bb[1], tuple(colour), thickness))

    def pts(i):
        r = c["profile"][b, i]
        rl = rr = fl = fr = "absent"
        if r["found"]:
            rl, rr = py_project(cam, r["left_pt"], size, mistakes), py_project(cam, r["right_pt"], size, mistakes)
        if c["f2f_profile"] is not None and c["f2f_profile"][b, i]["ok"]:
            q = c["f2f_profile"][b, i]
            fl, fr = py_project(cam, q["left_pt"], size, mistakes), py_project(cam, q["right_pt"], size, mistakes)
        return rl, rr, fl, fr

    P = [pts(i) for i in range(D)]
    for i in range(D - 1):
        join(P[i][0], P[i + 1][0], ln.edge_bgr, ln.profile_thickness)
    for i in range(D - 1):
        join(P[i][1], P[i + 1][1], ln.edge_bgr, ln.profile_thickness)
    for i in range(D):
        join(P[i][0], P[i][1], ln.rw_bgr, ln.profile_thickness)
    for i in range(D):
        join(P[i][2], P[i][3], ln.f2f_bgr, ln.profile_thickness)
    r = c["records"][b]
    if r["found"]:
        join(py_project(cam, r["left_pt"], size, mistakes), py_project(cam, r["right_pt"], size, mistakes), ln.rw_bgr, ln.thickness)
    if c["f2f"] is not None and c["f2f"][b]["ok"]:
        q = c["f2f"][b]
        join(py_project(cam, q["left_pt"], size, mistakes), py_project(cam, q["right_pt"], size, mistakes), ln.f2f_bgr, ln.thickness)
    return segs, flag


def py_draw(img: np.ndarray, segs, clip_top: int, mistakes=()) -> np.ndarray:
    """the paint rule on a copy of u8 [h,w,3] ``img``: pixel (px, py), centre (256 px, 256 py), takes the colour of the LAST segment of the
    list whose distance to it is <= 128 thickness; rows above clip_top are never painted.  Only the pixels of a segment's bounding box
    widened by the radius are evaluated.  w.d, w x d, |w|^2 and |d|^2 stay below 2^50 in int64 (asserted); the two quantities beyond int64,
    (w x d)^2 and r^2 |d|^2, are compared as Python integers."""
    out = np.array(img, np.uint8, copy=True)
    h, w = out.shape[:2]
    top = clip_top + 1 if "clip_off_by_one" in mistakes else clip_top
    order = list(segs)[::-1] if "first_wins" in mistakes else list(segs)
    for ax, ay, bx, by, colour, thickness in order:
        r = 128 * thickness
        px0, px1 = max(0, -((r - min(ax, bx)) // 256)), min(w - 1, (max(ax, bx) + r) // 256)
        py0, py1 = max(top, -((r - min(ay, by)) // 256)), min(h - 1, (max(ay, by) + r) // 256)
        if px0 > px1 or py0 > py1:
            continue
        X = np.arange(px0, px1 + 1, dtype=np.int64)[None, :] * 256
        Y = np.arange(py0, py1 + 1, dtype=np.int64)[:, None] * 256
        dx, dy = bx - ax, by - ay
        wx, wy = X - ax, Y - ay
        dd = dx * dx + dy * dy
        t = wx * dx + wy * dy
        cross = wx * dy - wy * dx
        assert max(abs(dx), abs(dy)) <= 2 ** 24 and int(np.abs(wx).max()) < 2 ** 24 and int(np.abs(wy).max()) < 2 ** 24
        assert int(np.abs(cross).max()) < 2 ** 50 and int(np.abs(t).max()) < 2 ** 50 and dd < 2 ** 50
        near_a = (t <= 0) & (wx * wx + wy * wy <= r * r)
        near_b = (t >= dd) & ((wx - dx) ** 2 + (wy - dy) ** 2 <= r * r)
        between = (t > 0) & (t < dd)
        inside = np.zeros_like(between)
        if between.any():
            c2 = cross[between].astype(object) ** 2
            inside[between] = np.array([v <= r * r * dd for v in c2], bool)
        out[py0:py1 + 1, px0:px1 + 1][near_a | near_b | inside] = np.array(colour, np.uint8)
    return out


def py_frames(img, c: dict, mistakes=()):
    """(images, flags) of the independent statement for the whole batch"""
    out, flags = np.array(img, copy=True), np.zeros((c["B"],), np.int32)
    for b in range(c["B"]):
        segs, flags[b] = py_segments(c, b, mistakes)
        out[b] = py_draw(out[b], segs, c["clip_top"], mistakes)
    return out, flags
