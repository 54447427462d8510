"""Shared by tests/test_ply_device_cpu.py and tests/test_gpu_ply_device.py: the frames of the device PLY route (sd_ply_format_rw,
include/semdepth.h) -- a road cloud and an sd_rw_result each -- with the yardstick, outputs.rw_ply_bytes, and the host statement
sd_ply_format_rw_host as callables.  Every case is a dict(name, xyz f32 [n,3], rgb u8 [n,3], rec RW_DTYPE scalar)."""
import ctypes as C

import numpy as np

from semantic_depth_amd import _lib as L
from semantic_depth_amd import outputs
from semantic_depth_amd.engine import RW_DTYPE

ROW_CAP, HEADER_CAP, LINE_ROWS, BLOCK = 69, 209, 1001, 256
COLOURS = np.array([0, 9, 10, 99, 100, 255], np.uint8)
BIG = np.float32(2.0 ** 31 - 128)             # the largest f32 below 2^31


def lib():
    import __graft_entry__ as graft
    graft.build()
    return L.load()


def record(left=None, right=None):
    r = np.zeros((), RW_DTYPE)
    if left is None:                           # found = 0: the end points are not read, whatever they hold
        r["left_pt"] = r["right_pt"] = np.nan
        r["width"] = np.nan
        return r
    r["found"] = 1
    r["left_pt"], r["right_pt"] = np.asarray(left, np.float32), np.asarray(right, np.float32)
    r["x_left"], r["x_right"] = r["left_pt"][0], r["right_pt"][0]
    r["width"] = abs(float(r["x_left"]) - float(r["x_right"]))
    return r


def case(name, xyz, rgb=None, rec=None, seed=0):
    xyz = np.ascontiguousarray(np.asarray(xyz, np.float32).reshape(-1, 3))
    if rgb is None:
        rgb = np.random.default_rng(seed + len(xyz)).integers(0, 256, (len(xyz), 3))
    return dict(name=name, xyz=xyz, rgb=np.ascontiguousarray(np.asarray(rgb, np.uint8).reshape(-1, 3)), rec=record() if rec is None else rec)


def cloud(seed, n, z=None):
    rng = np.random.default_rng(seed)
    p = (rng.standard_normal((n, 3)) * [4.0, 0.5, 3.0] + [0.0, 1.5, 9.0]).astype(np.float32)
    if z is not None:
        p[:, 2] = z
    return p


LINE = record((-3.7123456, 1.2345678, 9.87654321), (4.1234567, -1.1111111, 10.123456))


def want(c):
    """the yardstick: outputs.rw_ply_bytes as SequenceOutputs' host route calls it"""
    r = c["rec"]
    left = right = None
    if r["found"]:
        left, right = r["left_pt"].astype(np.float64)[None, :], r["right_pt"].astype(np.float64)[None, :]
    return outputs.rw_ply_bytes(c["xyz"].astype(np.float64), c["rgb"], left, right)


def bound(n):
    return HEADER_CAP + (n + LINE_ROWS) * ROW_CAP


def host(c, cap=None):
    """sd_ply_format_rw_host(case) -> (status, bytes, flag); the buffer is filled with 0xA5 and must stay so behind the size"""
    n = len(c["xyz"])
    cap = bound(n) if cap is None else cap
    out = np.full(max(cap, 1) + 8, 0xA5, np.uint8)
    size, flag = C.c_size_t(123), C.c_int32(-7)
    rec = L.sd_rw_result.from_buffer_copy(c["rec"].tobytes())
    st = lib().sd_ply_format_rw_host(c["xyz"].ctypes.data_as(C.c_void_p), c["rgb"].ctypes.data_as(C.c_void_p), n, C.byref(rec),
                                     out.ctypes.data_as(C.c_void_p), cap, C.byref(size), C.byref(flag))
    if st == L.SD_OK:
        assert (out[size.value:] == 0xA5).all()
    return st, out[:size.value].tobytes() if st == L.SD_OK else None, flag.value


def first_difference(got, ref):
    if got == ref:
        return None
    m = min(len(got), len(ref))
    i = next((i for i in range(m) if got[i] != ref[i]), m)
    return f"first differing byte {i} (lengths {len(got)} / {len(ref)}): {got[max(i - 30, 0):i + 30]!r} / {ref[max(i - 30, 0):i + 30]!r}"


# ------------------------------------------------------------------------------------------------ (a) rounding
def rounding_values():
    f32 = np.float32
    v = [f32(j / 128) for j in range(1, 256, 2)] + [f32(-j / 128) for j in range(1, 64, 2)]              # exact ties at six decimals
    v += [f32(0.9999995), f32(9.9999999), f32(99999.9999996), f32(0.99999952), f32(-0.9999995)]
    v += [f32(0.0), f32(-0.0), f32(-1e-7), f32(5e-7), f32(-5e-7), f32(4.9999e-7), f32(1.5e-6), f32(2.5e-6)]
    v += [f32(1e-45), f32(-1e-45), f32(1e-40), f32(-1e-39), f32(1.1754942e-38), f32(1.17549435e-38)]       # f32 denormals and the first normal
    v += [BIG, -BIG, f32(2.0 ** 30), f32(-2.0 ** 30), f32(2.0 ** 24 + 1), f32(8388607.5), f32(-8388607.5), f32(4194303.75)]
    for k in range(-6, 10):
        p = f32(10.0 ** k)
        v += [p, np.nextafter(p, f32(np.inf)), np.nextafter(p, f32(-np.inf)), -p]
    bits = np.random.default_rng(20251017).integers(0, 2 ** 32, 6000, dtype=np.uint64).astype(np.uint32)
    r = bits.view(np.float32)
    with np.errstate(invalid="ignore"):        # (signalling NaN patterns are among the draws)
        r = r[np.isfinite(r) & (np.abs(r.astype(np.float64)) < 2.0 ** 31)][:2000]
    assert len(r) == 2000
    # random patterns are mostly tiny or huge: half of them are rescaled into the range where all the digits matter
    r = r.copy()
    e = np.random.default_rng(7).integers(-20, 31, 1000)
    r[:1000] = np.ldexp(np.frexp(r[:1000])[0], e).astype(np.float32)
    return np.concatenate([np.array(v, np.float32), r])


def rounding_cases():
    v = rounding_values()
    n = -(-len(v) // 3)
    pool = np.concatenate([v, v[:3 * n - len(v)]])
    out = []
    for k in range(3):                         # every value appears once as x, once as y and once as z
        xyz = np.roll(pool, k * n).reshape(3, n).T
        rgb = COLOURS[(np.arange(3 * n).reshape(n, 3) * 5 + k) % 6]
        out.append(case(f"rounding_{k}", xyz, rgb))
    return out


# ------------------------------------------------------------------------------------------------ (b) line points that are true doubles
def line_cases():
    return [case("line_long_fractions", cloud(1, 40), rec=LINE),
            case("line_mixed_signs", cloud(2, 17), rec=record((-0.0004999, -0.0100001, -0.3333333), (0.0005001, 0.0099999, 0.6666667))),
            case("line_wide", cloud(3, 5), rec=record((-123456.78, 98765.43, 1000.001), (654321.1, -0.015, 999.999))),
            case("line_at_the_bound", cloud(4, 9), rec=record((-BIG, -BIG, 1.0), (BIG, BIG, 3.0))),
            case("no_line_found_0", cloud(5, 33))]


# ------------------------------------------------------------------------------------------------ (c) the minimum-z filter
def filter_cases():
    shared = cloud(6, 50)
    shared[[3, 17, 18, 49], 2] = shared[:, 2].min()
    below = record((-1.0, 1.0, 1.0), (1.0, 1.0, 2.0))
    above = record((-1.0, 1.0, 6.0), (1.0, 1.0, 7.0))
    falling = record((-1.0, 1.0, 4.0), (1.0, 1.0, 2.5))                  # the minimum is the line's last point
    flat_line = record((-1.0, 1.0, 5.0), (1.0, 1.0, 5.0))                # every row at one z: nothing is kept
    return [case("shared_minimum", shared), case("shared_minimum_line", shared, rec=above),
            case("flat_cloud_line_below", cloud(7, 30, z=5.0), rec=below), case("flat_cloud_line_above", cloud(8, 30, z=5.0), rec=above),
            case("flat_cloud_no_line", cloud(9, 30, z=5.0)), case("all_rows_one_z", cloud(10, 12, z=5.0), rec=flat_line),
            case("minimum_on_a_line_point", cloud(11, 30, z=5.0), rec=falling), case("minus_zero_minimum", [[1, 1, 0.0], [2, 2, -0.0], [3, 3, 1.0]]),
            case("empty_no_line", np.zeros((0, 3))), case("empty_line", np.zeros((0, 3)), rec=LINE),
            case("one_point", cloud(12, 1)), case("one_point_line", cloud(13, 1), rec=LINE)]


# ------------------------------------------------------------------------------------------------ (d) block edges
def edge_cases():
    out = []
    for n in (255, 256, 257, 512):             # the cloud / line seam and, without a line, the last row on both sides of a 256-row block
        out.append(case(f"seam_{n}", cloud(20 + n, n), rec=LINE))
        out.append(case(f"last_{n}", cloud(30 + n, n)))
    for n in (22, 23, 24):                     # n + 1001 = 1023, 1024, 1025: the last line row on both sides of a block
        assert (n + LINE_ROWS) % BLOCK == (n - 23) % BLOCK
        out.append(case(f"line_end_{n}", cloud(40 + n, n), rec=LINE))
    return out


def good_cases():
    return rounding_cases() + line_cases() + filter_cases() + edge_cases()


# ------------------------------------------------------------------------------------------------ (e) frames the device does not format
def flagged_cases():
    nan = cloud(50, 60)
    nan[41, 1] = np.nan
    inf = cloud(51, 300)
    inf[299, 2] = -np.inf
    big = cloud(52, 20)
    big[0, 0] = 2.0 ** 31
    return [case("nan_in_cloud", nan, rec=LINE), case("inf_in_cloud", inf), case("two_to_the_31", big),
            case("nan_end_point", cloud(53, 10), rec=record((np.nan, 1.0, 2.0), (1.0, 1.0, 3.0))),
            case("inf_end_point", cloud(54, 10), rec=record((0.0, 1.0, 2.0), (1.0, np.inf, 3.0))),
            case("right_end_at_2_31", cloud(55, 10), rec=record((0.0, 1.0, 2.0), (2.0 ** 31, 1.0, 3.0)))]


def batches(cases, size=4):
    """the cases in groups of at most ``size`` frames, the largest cloud of a group first: its n is the group's cap"""
    order = sorted(cases, key=lambda c: -len(c["xyz"]))
    return [order[i:i + size] for i in range(0, len(order), size)]
