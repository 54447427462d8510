"""Cases of the scene PLY tests (tests/test_scene_cpu.py, tests/test_gpu_scene.py): crafted frames for sd_scene_format /
sd_scene_format_host / outputs.scene_ply_bytes, the boxes of the lattice tests and a Python model of the lattice rule in which one
mistake at a time can be seeded.  Everything is seeded; nothing here needs a GPU."""
from fractions import Fraction

import numpy as np

from semantic_depth_amd.engine import BOX_DTYPE, F2F_DTYPE, RW_DTYPE

ROAD, ROAD_PLANE, RW_LINE, FENCE_L, FENCE_R, PLANE_L, PLANE_R, F2F_LINE = (1 << i for i in range(8))
ALL = 255
FILE_MASKS = {"scene": ALL, "road": ROAD, "fence": FENCE_L | FENCE_R}

ROAD_PLANE_COEF = (0.0125, -1.0, 0.021, -1.43)          # y = Cx x + Cz z + C
LEFT_PLANE_COEF = (-1.0, 0.031, -0.017, -3.2)           # x = Cy y + Cz z + C
RIGHT_PLANE_COEF = (-1.0, -0.027, 0.011, 3.4)


def box(lo_a, hi_a, lo_b, hi_b, n=1):
    b = np.zeros((), BOX_DTYPE)
    b["lo_a"], b["hi_a"], b["lo_b"], b["hi_b"], b["n"] = lo_a, hi_a, lo_b, hi_b, n
    return b


def frame(seed=0, n_road=300, n_left=200, n_right=180, found=True, ok=True):
    """one full frame: clouds about 1.0 x 1.5 m, so that every lattice is about 20 x 30 rows; the minimum z of the frame is a road point"""
    rng = np.random.default_rng(seed)

    def cloud(n, x0, y0):
        p = np.empty((n, 3), np.float32)
        p[:, 0] = x0 + rng.uniform(-0.5, 0.5, n)
        p[:, 1] = y0 + rng.uniform(-0.5, 0.5, n)
        p[:, 2] = rng.uniform(-9.0, -7.5, n)
        return p, rng.integers(0, 256, (n, 3), dtype=np.uint8)

    road_xyz, road_rgb = cloud(n_road, 0.0, -1.5)
    left_xyz, left_rgb = cloud(n_left, -3.0, -1.0)
    right_xyz, right_rgb = cloud(n_right, 3.0, -1.0)
    if n_road:
        road_xyz[n_road // 2, 2] = -9.5                 # the minimum z of the frame, alone
    rec = np.zeros((), RW_DTYPE)
    rec["found"], rec["n_road"], rec["n_ror"] = int(found), n_road, n_road
    rec["left_pt"], rec["right_pt"] = (-0.48, -1.52, -8.03), (0.47, -1.49, -7.97)
    rec["x_left"], rec["x_right"] = rec["left_pt"][0], rec["right_pt"][0]
    rec["width"] = abs(float(rec["x_left"]) - float(rec["x_right"])) if found else np.nan
    rec["plane"] = ROAD_PLANE_COEF
    f2 = np.zeros((), F2F_DTYPE)
    f2["ok"], f2["dist"] = int(ok), 6.1 if ok else np.nan
    f2["left_pt"], f2["right_pt"] = (-3.05, -1.61, -8.0), (3.02, -1.58, -8.0)
    f2["plane_left"], f2["plane_right"] = LEFT_PLANE_COEF, RIGHT_PLANE_COEF
    f2["counts"] = (n_left + n_right + 7, n_left + n_right + 5, n_left + n_right + 2, n_left + 1, n_right + 1, n_left, n_right)
    return dict(road_xyz=road_xyz, road_rgb=road_rgb, record=rec, f2f=f2,
                fence=dict(left_xyz=left_xyz, left_rgb=left_rgb, right_xyz=right_xyz, right_rgb=right_rgb),
                road_box=box(-0.5, 0.5, -9.0, -7.5, n_road + 9),
                fence_boxes=np.array([box(-1.5, -0.5, -9.0, -7.5, n_left + 3), box(-1.5, -0.48, -8.9, -7.5, n_right + 3)], BOX_DTYPE))


def without_left(f):
    """the left side ran empty: no left cloud, no left lattice (n == 0: the four floats are 0), not ok"""
    f = dict(f, f2f=f["f2f"].copy(), fence=dict(f["fence"]), fence_boxes=f["fence_boxes"].copy())
    f["fence"]["left_xyz"], f["fence"]["left_rgb"] = f["fence"]["left_xyz"][:0], f["fence"]["left_rgb"][:0]
    c = f["f2f"]["counts"].copy()
    c[3] = c[5] = 0
    f["f2f"]["counts"], f["f2f"]["ok"], f["f2f"]["dist"] = c, 0, np.nan
    f["f2f"]["plane_left"] = np.nan
    f["fence_boxes"][0] = box(0, 0, 0, 0, 0)
    return f


def with_min_in(f, where: str):
    """a copy of ``f`` whose global minimum z sits in segment ``where`` ("shared": in the road cloud and the left fence cloud alike)"""
    f = dict(f, road_xyz=f["road_xyz"].copy(), record=f["record"].copy(), f2f=f["f2f"].copy(),
             fence={k: v.copy() for k, v in f["fence"].items()}, road_box=f["road_box"].copy(), fence_boxes=f["fence_boxes"].copy())
    if where == "road":
        f["road_xyz"][3, 2] = -20.0
    elif where == "road_plane":                           # the whole first b row of the lattice is the minimum and goes
        f["road_box"]["lo_b"] = -30.0
        f["road_box"]["hi_b"] = -29.5
    elif where == "rw_line":                              # (line rows 0 and 1 are both the left end: two rows at the minimum)
        f["record"]["left_pt"][2] = -25.0
    elif where == "fence_l":
        f["fence"]["left_xyz"][5, 2] = -22.0
    elif where == "fence_r":
        f["fence"]["right_xyz"][7, 2] = -23.0
    elif where == "plane_l":
        f["fence_boxes"][0]["lo_b"], f["fence_boxes"][0]["hi_b"] = -31.0, -30.6
    elif where == "plane_r":
        f["fence_boxes"][1]["lo_b"], f["fence_boxes"][1]["hi_b"] = -32.0, -31.6
    elif where == "f2f_line":
        f["f2f"]["left_pt"][2] = -26.0
    elif where == "shared":
        f["road_xyz"][3, 2] = -20.0
        f["fence"]["left_xyz"][5, 2] = -20.0
    else:
        raise ValueError(where)
    return f


MIN_PLACES = ("road", "road_plane", "rw_line", "fence_l", "fence_r", "plane_l", "plane_r", "f2f_line", "shared")


def args(f, fence=True):
    """the keyword arguments of outputs.scene_ply_bytes / outputs.scene_format_host for frame ``f`` (``fence`` False: approach 'rw')"""
    kw = dict(road3D=f["road_xyz"], road_colors=f["road_rgb"], record=f["record"], road_box=f["road_box"])
    if fence:
        kw.update(fence=f["fence"], f2f=f["f2f"], fence_boxes=f["fence_boxes"])
    return kw


def gpu_frames(variant):
    """the three frames of the device formatter test (B = 3, cap = 1024, lattice_cap = 4096): a full one with a 512-row segment, one
    that is not found and has no left side, and one that is flagged under ``variant`` "flag1" / "flag3" (plain under any other)"""
    f0 = frame(21)
    f0["road_box"] = box(-0.4, 0.4, -9.0, -7.4, 300)                 # 16 x 32 = 512 rows: a segment that is a multiple of 256
    f1 = without_left(frame(22, found=False))
    f1["road_box"] = box(-0.2, -0.17, -9.0, -7.5, 4)                 # a 1 x n lattice (beside the empty left one)
    f2 = frame(23, n_road=513)                                       # (the longest file under every mask: a frame behind it fits where it did not)
    if variant == "flag1":
        f2["fence"]["left_xyz"][17, 0] = np.nan
    elif variant == "flag3":
        f2["fence_boxes"][1] = box(-1.5, -0.65, -19.55, -7.5, 50)    # 17 x 241 = 4097 rows
    return f0, f1, f2


# ------------------------------------------------------------------------------------------------ lattice boxes
def exact_multiple_boxes(count=2000, seed=11):
    """boxes whose a extent is a multiple of 0.05 (as float32 bounds), one or three samples along b: (lo_a, hi_a, lo_b, hi_b)"""
    rng = np.random.default_rng(seed)
    lo = rng.integers(-400, 400, count)
    k = rng.integers(1, 60, count)
    out = np.empty((count, 4), np.float32)
    out[:, 0], out[:, 1] = np.float32(lo * 0.05), np.float32((lo + k) * 0.05)
    out[:, 2], out[:, 3] = -8.0, -7.98
    out[1::2, 3] = -7.88                                # (every other box has three samples along b: the order of the axes shows)
    return out


def special_boxes():
    """negative bounds, an extent below 0.05 (one sample), a zero extent (no lattice), a two-axis lattice that is not square"""
    return np.array([(-3.7, -2.2, -9.3, -7.1), (1.0, 1.03, -8.0, -7.0), (2.0, 2.0, -8.0, -7.0), (-0.31, 0.44, -8.26, -7.93),
                     (-0.5, 0.5, -7.0, -7.0), (-12.5, -12.0, 0.125, 0.5)], np.float32)


def lattice_model(b4, plane, axis, mistake=None):
    """the rule of csrc/scene_format.hpp in Python floats -> f64 [rows,3]; ``mistake`` seeds one error: "count64" (the count from a
    float64 quotient), "b_fastest", "fused_lift" (one rounding for c_a * a + (c_b * b)), "delta_005" (0.05 as the step)"""
    lo_a, hi_a, lo_b, hi_b = (np.float32(v) for v in b4)

    def axis_samples(lo, hi):
        if mistake == "count64":
            n = max(0, int(np.ceil((float(hi) - float(lo)) / 0.05)))
        else:
            n = max(0, int(np.ceil(np.float32(np.float32(hi - lo) / np.float32(0.05)))))
        nxt = np.float32(lo + np.float32(0.05))
        d = 0.05 if mistake == "delta_005" else float(nxt) - float(lo)
        return [float(lo) if i == 0 else (float(lo) + i * d) for i in range(n)]

    A, Bv = axis_samples(lo_a, hi_a), axis_samples(lo_b, hi_b)
    ca, cb = (plane[0], plane[2]) if axis == 1 else (plane[1], plane[2])
    rows = []
    pairs = [(a, b) for a in A for b in Bv] if mistake == "b_fastest" else [(a, b) for b in Bv for a in A]
    for a, b in pairs:
        if mistake == "fused_lift":
            lift = float(Fraction(float(ca)) * Fraction(a) + Fraction(float(cb) * b)) + float(plane[3])
        else:
            lift = (float(ca) * a + float(cb) * b) + float(plane[3])
        rows.append((a, lift, b) if axis == 1 else (lift, a, b))
    return np.array(rows, np.float64).reshape(-1, 3)


MISTAKES = ("count64", "b_fastest", "fused_lift", "delta_005")
