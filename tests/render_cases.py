"""Shared by tests/test_render_cpu.py and tests/test_gpu_render_device.py: the frames of the rendered clouds (sd_render_rw,
include/semdepth.h) -- a road cloud, an sd_rw_result and a camera each -- the host statement sd_render_rw_host as a callable, and an
INDEPENDENT statement of the rule in numpy: float64 arithmetic in the stated order, np.floor, the keys put together as uint64 and the
per-pixel minimum taken by sorting.  It shares no code with csrc/render_rule.hpp; the road-width line comes from
pcl.create_3Dline_from_3Dpoints, the yardstick of the PLY route.  Every case is a dict(name, xyz f32 [n,3], rgb u8 [n,3], rec RW_DTYPE scalar,
cam outputs.RenderCamera); everything is seeded."""
import ctypes as C

import numpy as np

from ply_device_cases import record
from semantic_depth_amd import _lib as L
from semantic_depth_amd import outputs, pcl

CAP = 1000                                     # the largest cloud of the shared cases
LINE = record((-3.7123456, 1.2345678, 19.87654321), (4.1234567, 1.1111111, 20.123456))
FLOOR = np.float32([0.0, 1.5, 1.0])            # a row below every other z: it is the frame's minimum and vanishes, so the others are drawn


def lib():
    import __graft_entry__ as graft
    graft.build()
    return L.load()


# ------------------------------------------------------------------------------------------------ cameras
def slanted_camera(width=96, height=64, **kw):
    """a camera off to the side of the road and above it (world y points down), looking at (0, 1.5, 12) with a roll: no entry of ext is 0"""
    pos, target = np.array([3.0, -6.0, -2.0]), np.array([0.0, 1.5, 12.0])
    z = (target - pos) / np.linalg.norm(target - pos)
    x = np.cross([0.1, 1.0, 0.05], z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    rot = np.stack([x, y, z])
    ext = np.concatenate([rot, (-rot @ pos)[:, None]], axis=1)
    return outputs.RenderCamera(ext=tuple(ext.reshape(-1)), fx=0.9 * width, fy=0.85 * width, cx=width / 2 - 0.3, cy=height / 2 + 0.2, width=width,
                                height=height, **kw)


def top(width=96, height=64, **kw):
    return outputs.top_camera(width, height, **kw)


def pixel_camera(width, height, point_size, z_near=0.5, background=(9, 200, 77)):
    """world (x, y, 2) lands on u = x, v = y exactly: ext = identity, fx = fy = 2, cx = cy = 0"""
    return outputs.RenderCamera(ext=(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0), fx=2.0, fy=2.0, cx=0.0, cy=0.0, width=width, height=height, z_near=z_near,
                                point_size=point_size, background=background)


# ------------------------------------------------------------------------------------------------ the two statements
def host(c, n=None):
    """sd_render_rw_host(case) -> (status, image u8 [h,w,3] or None, flag); the buffer is filled with 0xA5 and must stay so behind the image"""
    cam = c["cam"]
    n = len(c["xyz"]) if n is None else n
    size = cam.height * cam.width * 3
    out = np.full(size + 16, 0xA5, np.uint8)
    flag = C.c_int32(-7)
    rec = L.sd_rw_result.from_buffer_copy(c["rec"].tobytes())
    st = lib().sd_render_rw_host(c["xyz"].ctypes.data_as(C.c_void_p), c["rgb"].ctypes.data_as(C.c_void_p), n, C.byref(rec), C.byref(cam.struct()),
                                 out.ctypes.data_as(C.c_void_p), C.byref(flag))
    if st != L.SD_OK:
        assert (out == 0xA5).all()
        return st, None, flag.value
    assert (out[size:] == 0xA5).all()
    return st, out[:size].reshape(cam.height, cam.width, 3).copy(), flag.value


def reference(c):
    """the rule of include/semdepth.h in numpy -> u8 [height,width,3] BGR"""
    cam, rec = c["cam"], c["rec"]
    n = len(c["xyz"])
    pts, col = c["xyz"].astype(np.float64).reshape(-1, 3), c["rgb"].astype(np.uint8).reshape(-1, 3)
    if rec["found"]:
        line, line_col = pcl.create_3Dline_from_3Dpoints(rec["left_pt"].astype(np.float64)[None, :], rec["right_pt"].astype(np.float64)[None, :], [250, 0, 0])
        assert line.shape == (1001, 3)
        pts, col = np.append(pts, line, axis=0), np.append(col, np.asarray(line_col, np.uint8), axis=0)
    img = np.empty((cam.height, cam.width, 3), np.uint8)
    img[:] = np.asarray(cam.background, np.uint8)
    fin = np.isfinite(pts).all(axis=1)
    if not fin.any():
        return img
    keep = fin & (pts[:, 2] > pts[fin, 2].min())
    e = np.asarray(cam.ext, np.float64).reshape(3, 4)
    s = int(cam.point_size)
    with np.errstate(all="ignore"):
        x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
        X = ((e[0, 0] * x + e[0, 1] * y) + e[0, 2] * z) + e[0, 3]
        Y = ((e[1, 0] * x + e[1, 1] * y) + e[1, 2] * z) + e[1, 3]
        Z = ((e[2, 0] * x + e[2, 1] * y) + e[2, 2] * z) + e[2, 3]
        keep &= Z >= cam.z_near
        u = np.float64(cam.fx) * (X / Z) + np.float64(cam.cx)
        v = np.float64(cam.fy) * (Y / Z) + np.float64(cam.cy)
        keep &= (-s <= u) & (u < cam.width + s) & (-s <= v) & (v < cam.height + s)
        zbits = Z.astype(np.float32).view(np.uint32)
    rows = np.nonzero(keep)[0]
    if not len(rows):
        return img
    px, py = np.floor(u[rows]).astype(np.int64), np.floor(v[rows]).astype(np.int64)
    keys = (zbits[rows].astype(np.uint64) << np.uint64(32)) | rows.astype(np.uint64)
    offs = np.arange(-((s - 1) // 2), s // 2 + 1)
    xs = (px[:, None, None] + offs[None, None, :]) + 0 * offs[None, :, None]
    ys = (py[:, None, None] + offs[None, :, None]) + 0 * offs[None, None, :]
    kk = np.broadcast_to(keys[:, None, None], xs.shape)
    inside = (xs >= 0) & (xs < cam.width) & (ys >= 0) & (ys < cam.height)
    pix, kk = (ys * cam.width + xs)[inside], kk[inside]
    order = np.lexsort((kk, pix))                                       # by pixel, then by key: the first of a pixel is its minimum
    pix, kk = pix[order], kk[order]
    first = np.ones(len(pix), bool)
    first[1:] = pix[1:] != pix[:-1]
    win = (kk[first] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    img.reshape(-1, 3)[pix[first]] = col[win][:, ::-1]
    assert (col[n:] == [250, 0, 0]).all()
    return img


# ------------------------------------------------------------------------------------------------ cases
def case(name, xyz, cam, rgb=None, rec=None, seed=0):
    xyz = np.ascontiguousarray(np.asarray(xyz, np.float32).reshape(-1, 3))
    if rgb is None:
        rgb = np.random.default_rng(seed + len(xyz)).integers(0, 250, (len(xyz), 3))      # (250 0 0 is the line's alone)
    return dict(name=name, xyz=xyz, rgb=np.ascontiguousarray(np.asarray(rgb, np.uint8).reshape(-1, 3)), rec=record() if rec is None else rec, cam=cam)


def cloud(seed, n):
    """a road-like cloud in front of both cameras: x in -6..6, y near 1.5, z in 5..35"""
    rng = np.random.default_rng(seed)
    return (rng.random((n, 3)) * [12.0, 0.4, 30.0] + [-6.0, 1.3, 5.0]).astype(np.float32)


def size_cases():
    out = []
    for cname, cam in (("slanted", slanted_camera()), ("top", top())):
        for n in (0, 1, 300, CAP):
            out.append(case(f"{cname}_{n}", cloud(100 + n, n), cam))
            out.append(case(f"{cname}_{n}_line", cloud(200 + n, n), cam, rec=LINE))
    return out


def point_size_cases():
    return [case(f"point_size_{s}_{cname}", cloud(7, 300), make(point_size=s), rec=LINE)
            for s in (1, 4, 5, 16) for cname, make in (("slanted", slanted_camera), ("top", top))]


def depth_cases():
    cam = top(64, 48, point_size=4)
    a, b = [0.0, 1.5, 20.0], [0.0, 0.5, 20.0]                            # one pixel; b is a metre nearer to the camera above
    red, green = [200, 10, 10], [10, 200, 10]
    out = [case("tie_lower_index_wins", [FLOOR, a, a], cam, rgb=[[0, 0, 0], red, green]),
           case("tie_lower_index_wins_swapped", [FLOOR, a, a], cam, rgb=[[0, 0, 0], green, red]),
           case("near_then_far", [FLOOR, b, a], cam, rgb=[[0, 0, 0], red, green]),
           case("far_then_near", [FLOOR, a, b], cam, rgb=[[0, 0, 0], red, green])]
    behind = cloud(8, 40)
    behind[::2, 1] = -50.0                                               # above the camera, which looks down: Z < 0
    out.append(case("rows_behind_the_camera", behind, cam))
    near = outputs.top_camera(64, 48, z_near=0.5, point_size=3)          # the camera is at y = -40, Z = y + 40
    at, below = np.float32(-39.5), np.nextafter(np.float32(-39.5), np.float32(-np.inf))
    out.append(case("z_at_the_near_plane", [FLOOR, [0.0, at, 20.0]], near))
    out.append(case("z_below_the_near_plane", [FLOOR, [0.0, below, 20.0]], near))
    out.append(case("z_at_and_below_the_near_plane", [FLOOR, [-0.01, below, 20.0], [0.01, at, 20.02]], near))
    return out


def border_cases():
    out = []
    w, h = 23, 17
    for s in (1, 4, 5, 16):
        cam = pixel_camera(w, h, s)
        lo, hi = (s - 1) // 2, s // 2
        # u just inside the image's reach on either side, the last value whose square still shows, the bounds of the rule and beyond
        us = [-float(s), -float(s) - 0.25, -hi - 0.5, -hi + 0.5, 0.0, w - 1.0, w - 1 + lo + 0.5, w + lo + 0.5, w + s - 0.25, float(w + s)]
        vs = [-float(s), -float(s) - 0.25, -hi - 0.5, -hi + 0.5, 0.0, h - 1.0, h - 1 + lo + 0.5, h + lo + 0.5, h + s - 0.25, float(h + s)]
        mid_u, mid_v = w // 2 + 0.5, h // 2 + 0.5
        for k, u in enumerate(us):
            out.append(case(f"border_x_{s}_{k}", [FLOOR, [u, mid_v, 2.0]], cam, rgb=[[0, 0, 0], [10 + k, 20, 30]]))
        for k, v in enumerate(vs):
            out.append(case(f"border_y_{s}_{k}", [FLOOR, [mid_u, v, 2.0]], cam, rgb=[[0, 0, 0], [10, 20 + k, 30]]))
        corners = [(-hi + 0.5, -hi + 0.5), (w - 1 + lo + 0.5, -hi + 0.5), (-hi + 0.5, h - 1 + lo + 0.5), (w - 1 + lo + 0.5, h - 1 + lo + 0.5)]
        out.append(case(f"corners_{s}", [FLOOR] + [[u, v, 2.0] for u, v in corners], cam, rgb=[[0, 0, 0], [1, 2, 3], [4, 5, 6], [7, 8, 9], [10, 11, 12]]))
    return out


def special_cases():
    cam = top()
    odd = cloud(9, 300)
    odd[5, 0] = np.nan
    odd[6, 1] = np.inf
    odd[7, 2] = -np.inf                                                  # not the minimum: the row is not finite
    odd[8] = [1e30, 1.5, 20.0]
    odd[9] = [0.0, 1e30, 20.0]
    odd[10] = [0.0, 1.5, 1e30]
    odd[11] = [np.nan, np.nan, np.nan]
    shared = cloud(10, 300)
    shared[[3, 17, 18, 299], 2] = shared[:, 2].min()
    flat = cloud(11, 50)
    flat[:, 2] = 20.0                                                    # every row at the minimum: nothing is drawn
    return [case("non_finite_rows", odd, cam, rec=LINE), case("non_finite_rows_slanted", odd, slanted_camera()),
            case("nan_end_point", cloud(12, 100), cam, rec=record((np.nan, 1.0, 19.0), (4.0, 1.0, 21.0))),
            case("shared_minimum", shared, cam), case("shared_minimum_line", shared, cam, rec=LINE), case("all_rows_one_z", flat, cam),
            case("one_z_line_above", flat, cam, rec=LINE)]


def line_cases():
    """a dense road plane at y = 1.5; the line lies over it (y = 1.0: nearer to the camera above, it hides the cloud) or under it (y = 2.0: the
    cloud hides it where it has points)"""
    cam = outputs.top_camera(128, 128)
    gx, gz = np.meshgrid(np.arange(-4.0, 4.01, 0.25), np.arange(16.0, 24.01, 0.25))
    plane = np.stack([gx.ravel(), np.full(gx.size, 1.5), gz.ravel()], axis=1)
    over = record((-5.0, 1.0, 19.6), (5.0, 1.0, 20.4))
    under = record((-5.0, 2.0, 19.6), (5.0, 2.0, 20.4))
    return [case("line_in_front_of_the_cloud", plane, cam, rec=over), case("line_behind_the_cloud", plane, cam, rec=under),
            case("no_line_found_0", plane, cam)]


def all_cases():
    return size_cases() + point_size_cases() + depth_cases() + border_cases() + special_cases() + line_cases()


def line_pixels(img):
    return int((img == [0, 0, 250]).all(-1).sum())
