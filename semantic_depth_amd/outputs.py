"""On-disk outputs of the tool and the focal-length sweep driver (§8f-4) — host-side formatting only.

    write_times / write_distances   <- semantic_depth.py:445-458  (``<name>_times.txt`` / ``<name>_distances.txt``)
    overlay_items / draw_overlay    <- semantic_depth.py:339-406  (banner + the text the reference draws; seq:301-327)
    render_rw / RenderCamera        <- utils/render_ply.py (every _rw.ply behind a saved Open3D pinhole camera) as z-buffered square points
                                       with a rule of the project's own (opt-in, render=camera; not Open3D's OpenGL pixels)
    draw_text                       <- the cv2.putText calls of :352-401 / seq:313-327 on the project's own stroke font (opt-in, text="draw")
    overlay_segments / draw_lines   <- the print_line_on_image calls the reference left commented out (seq:330-333): the measured lines, with a
                                       rule of the project's own (opt-in, lines=OverlayLines(); not cv2.line's pixels)
    save_frame_outputs              <- semantic_depth.py:339-441  (``_only_segmentation.png``, the annotated ``.png``, ``_ROAD`` / ``_FENCE`` /
                                       combined / ``_ALL`` PLY files, incl. the three visualisation planes of the combined cloud)
    road_plane_grid / fence_plane_grids <- the ``plane3D`` arrays of :215-219, :294-309 rebuilt through the reference's own pcl call sequence
    focal_sweep                     <- semantic_depth.py:854-944  (``results/<f>/data.txt``, ``best_focal_lengths.txt``)
    focal_sweep_batched             the same files behind one network pass per frame (Engine.camera_sweep)
    write_png                       <- cv2.imwrite(...png) at :406 (zlib-deflated 8-bit RGB; pixel-identical, not byte-identical)
    disparity_image / write_disp_image <- semantic_depth.py:681-683 (``<name>_disp.png``: scipy.misc.imresize + plt.imsave, pixel for pixel)
    SequenceOutputs                 <- the files of the sequence tool, semantic_depth_cityscapes_sequence.py:303-361 (``result_sequence_imgs/<name>.png``,
                                       ``result_sequence_ply/<name>_rw.ply``), written from the batched driver (distributed.run_sequence_files)

The text files are byte-identical to what the reference's own statements write (tests/test_outputs.py holds fixtures produced
by executing those statements, extracted from the reference by ``tests/golden/make_golden.py``).  The PIXELS of
``cv2.putText`` (Hershey fonts, part of OpenCV) are NOT reproduced: ``draw_overlay`` paints the banner rectangle and returns
the text items (string, origin, scale, colour, thickness) the reference passes to putText; they are also written next to the
image as ``<name>_overlay.json``.  By default that is all.  With ``text="draw"`` (save_frame_outputs, SequenceOutputs,
make_engine_step) the items are also rasterised into the image, with a stroke font and an exact-integer raster rule of the
project's own (include/semdepth.h, csrc/text_draw.hpp): ``draw_text`` on the host (sd_text_draw_host), Engine.draw_result_text on
the GPU for the sequence tool.  The strings, origins, scales, colours and thicknesses are the reference's; the glyph shapes are not.
"""
from __future__ import annotations

import contextlib
import dataclasses
import json
import os
import struct
import zlib

import numpy as np

from . import pcl
from .point_cloud_2_ply import PointCloud2Ply

TIME_KEYS = ("read", "semantic", "disparity", "to3D", "road", "rw", "fences", "f2f", "global")


def write_times(output_name: str, t: dict) -> str:
    """semantic_depth.py:445-454.  ``t``: seconds under the keys of TIME_KEYS."""
    path = "{}_times.txt".format(output_name)
    with open(path, "w") as f:
        f.write("Time read:       {}\n".format(t["read"]))
        f.write("Time semantic:   {}\n".format(t["semantic"]))
        f.write("Time disparity:  {}\n".format(t["disparity"]))
        f.write("Time to3D:       {}\n".format(t["to3D"]))
        f.write("Time road:       {}\n".format(t["road"]))
        f.write("Time rw:      {}\n".format(t["rw"]))
        f.write("Time fences:     {}\n".format(t["fences"]))
        f.write("Time f2f:   {}\n".format(t["f2f"]))
        f.write("Time global:     {}\n".format(t["global"]))
    return path


def write_distances(output_name: str, dist_rw, dist_f2f) -> str:
    """semantic_depth.py:456-458"""
    path = "{}_distances.txt".format(output_name)
    with open(path, "w") as f:
        f.write("rw distance:    {}\n".format(dist_rw))
        f.write("f2f distance: {}\n".format(dist_f2f))
    return path


PROFILE_COLUMNS = ("depth", "found", "width", "x_left", "x_right", "n_window")


def profile_text(depths, rows, dist_f2f=None) -> str:
    """the text of a depth-profile file: ``# depth found width x_left x_right n_window`` (``dist_f2f`` behind it when given), then one row
    per depth in the caller's order; numbers as numpy.savetxt(fmt='%1.4f') formats the calibration tables, found / n_window as integers,
    a missing value as ``nan``.  ``rows[i]`` is indexable by those names (a record of Engine.profile_records or a dict)."""
    if len(rows) != len(depths) or (dist_f2f is not None and len(dist_f2f) != len(depths)):
        raise ValueError("a depth profile has one row per depth")
    lines = ["# " + " ".join(PROFILE_COLUMNS + (("dist_f2f",) if dist_f2f is not None else ()))]
    for i, d in enumerate(depths):
        r = rows[i]
        found = int(r["found"])
        vals = [float(r[k]) if found else float("nan") for k in ("width", "x_left", "x_right")]
        line = "%1.4f %d %1.4f %1.4f %1.4f %d" % (float(d), found, vals[0], vals[1], vals[2], int(r["n_window"]))
        if dist_f2f is not None:
            v = dist_f2f[i]
            line += " %1.4f" % (float("nan") if v is None else float(v))
        lines.append(line)
    return "\n".join(lines) + "\n"


def write_profile(path: str, depths, rw_rows, f2f_rows=None) -> str:
    """one depth-profile text file (profile_text): ``rw_rows`` the D records of one frame (Engine.profile_records(...)[b]), ``f2f_rows``
    (optional) its D fence records (Engine.f2f_profile_records(...)[b]): dist_f2f is their dist, ``nan`` where ok == 0."""
    dist = None if f2f_rows is None else [float(r["dist"]) if int(r["ok"]) else None for r in f2f_rows]
    with open(path, "w") as f:
        f.write(profile_text(depths, rw_rows, dist))
    return path


# ------------------------------------------------------------------------------------------------ overlay
def overlay_items(w: int, h: int, depth: float, is_city: bool, left_pt_rw, right_pt_rw, dist_rw, approach: str = "rw",
                  left_pt_f2f=None, right_pt_f2f=None, dist_f2f=None):
    """the cv2.rectangle / cv2.putText calls of semantic_depth.py:346-401 as data: (banner, [items]).
    banner = ((x0, y0), (x1, y1), bgr); item = dict(text, org, fontFace, fontScale, color, thickness)."""
    if is_city:
        thickness, fontScale, left, right, middle = 2, 2, 0.01, 0.68, 0.33
    else:
        thickness, fontScale, left, right, middle = 5, 4, 0.01, 0.67, 0.33
    h_zero, h_first, h_second = 0.05 * h, 0.12 * h, 0.18 * h
    banner = ((0, 0), (w, int(0.2 * h)), (156, 157, 159))

    def item(text, x, y):
        return dict(text=text, org=(int(x * w), int(y)), fontFace=16, fontScale=fontScale, color=(255, 255, 255), thickness=thickness)

    items = [item("At {:.2f}m depth:".format(depth), middle, h_zero)]
    if approach == "both":
        items.append(item("{:.2f}m to l fence".format(-left_pt_f2f[0][0]), left, h_first))
        items.append(item("{:.2f}m to r fence".format(right_pt_f2f[0][0]), right, h_first))
        items.append(item("Fence2Fence: {:.2f}m".format(dist_f2f), middle, h_first))
    items.append(item("{:.2f}m to road's l".format(-left_pt_rw[0][0]), left, h_second))
    items.append(item("{:.2f}m to road's r".format(right_pt_rw[0][0]), right, h_second))
    items.append(item("Road's width: {:.2f}m".format(dist_rw), middle, h_second))
    return banner, items


def overlay_items_sequence(w: int, h: int, depth: float, line_found: bool, left_pt_rw=None, right_pt_rw=None, dist_rw=None):
    """the sequence tool's variant, semantic_depth_cityscapes_sequence.py:301-327 (fontScale 2 / 2.2, 25 % banner, or the
    green 'Cannot compute' line and no banner)."""
    thickness, fontScale = 2, 2

    def item(text, x, y, scale, color=(255, 255, 255)):
        return dict(text=text, org=(int(x * w), int(y * h)), fontFace=16, fontScale=scale, color=color, thickness=thickness)

    if not line_found:
        return None, [item("Cannot compute width of road at {:.2f} m depth:".format(depth), 0.28, 0.035, fontScale + 0.2, (0, 255, 0))]
    banner = ((0, 0), (w, int(0.25 * h)), (156, 157, 159))
    return banner, [item("At {:.2f} m depth:".format(depth), 0.36, 0.05, fontScale + 0.2),
                    item("{:.2f}m to road's left end".format(-left_pt_rw[0][0]), 0.05, 0.13, fontScale),
                    item("{:.2f}m to road's right end".format(right_pt_rw[0][0]), 0.5, 0.13, fontScale),
                    item("Road's width: {:.2f} m".format(dist_rw), 0.35, 0.22, fontScale)]


def draw_overlay(segmented_frame: np.ndarray, banner, items):
    """cv2.rectangle(img, pt1, pt2, color, -1) of :346 (both corners inclusive, clipped to the image); text is returned, not
    rasterised (module docstring)."""
    img = np.array(segmented_frame, copy=True)
    if banner is not None:
        (x0, y0), (x1, y1), col = banner
        img[max(y0, 0):min(y1, img.shape[0] - 1) + 1, max(x0, 0):min(x1, img.shape[1] - 1) + 1] = np.asarray(col, img.dtype)
    return img, items


def _check_text(text: str) -> str:
    if text not in ("json", "draw"):
        raise ValueError(f"text must be 'json' or 'draw', got {text!r}")
    return text


def text_items(items):
    """overlay_items' dicts as a ctypes array of _lib.sd_text_item: the string's bytes (latin-1, at most 64), org, lround(fontScale * 256),
    the colour's three values in the order given (the image's channel order), thickness"""
    from . import _lib as L
    arr = (L.sd_text_item * max(len(items), 1))()
    for a, it in zip(arr, items):
        raw = it["text"].encode("latin-1", "replace")
        if len(raw) > L.SD_TEXT_MAX_BYTES:
            raise ValueError(f"draw_text: {it['text']!r} is longer than {L.SD_TEXT_MAX_BYTES} bytes")
        a.text[:len(raw)] = raw
        a.len = len(raw)
        a.org_x, a.org_y = int(it["org"][0]), int(it["org"][1])
        a.scale_q8 = int(np.floor(float(it["fontScale"]) * 256 + 0.5))
        a.thickness = int(it["thickness"])
        a.bgr[:] = [int(c) for c in it["color"]]
    return arr


def draw_text(img: np.ndarray, items) -> np.ndarray:
    """the cv2.putText calls the items stand for, rasterised into a copy of u8 [h,w,3] ``img`` in list order on the project's own stroke font
    (sd_text_draw_host: the rule of include/semdepth.h, the pixels Engine.draw_result_text paints on the GPU -- not OpenCV's)."""
    import ctypes as C

    from . import _lib as L
    out = np.array(img, dtype=np.uint8, order="C", copy=True)
    if out.ndim != 3 or out.shape[2] != 3:
        raise ValueError(f"draw_text: the image must be u8 [h,w,3], got {out.shape}")
    st = L.load().sd_text_draw_host(out.ctypes.data_as(C.c_void_p), out.shape[0], out.shape[1], text_items(items), len(items))
    if st != L.SD_OK:
        raise ValueError(f"draw_text: an item or the image is outside the caps of include/semdepth.h (status {st})")
    return out


# ------------------------------------------------------------------------------------------------ measurement lines
SEG_DTYPE = np.dtype([("ax", "<i4"), ("ay", "<i4"), ("bx", "<i4"), ("by", "<i4"), ("bgr", "u1", 3), ("thickness", "u1")])      # sd_overlay_segment


@dataclasses.dataclass(frozen=True)
class OverlayLines:
    """the style of the measurement lines drawn into the result images (sd_overlay_style, include/semdepth.h; opt-in, lines=): ``rw_bgr``
    colours the road-width line and the road rungs of a depth profile, ``f2f_bgr`` the fence-to-fence line and the fence rungs, ``edge_bgr``
    the road's left and right edge along the profile, in the image's channel order; ``thickness`` (1..32 pixels) is that of the two measured
    lines, ``profile_thickness`` that of everything from the profile.  The two line colours are the reference's (seq:331-332); the edge
    colour and the thicknesses are the project's choice."""
    rw_bgr: tuple = (0, 0, 255)
    f2f_bgr: tuple = (0, 255, 0)
    edge_bgr: tuple = (0, 255, 255)
    thickness: int = 3
    profile_thickness: int = 1

    def __post_init__(self):
        for k in ("rw_bgr", "f2f_bgr", "edge_bgr"):
            c = tuple(int(v) for v in getattr(self, k))
            if len(c) != 3 or not all(0 <= v <= 255 for v in c):
                raise ValueError(f"OverlayLines: {k} holds three values 0..255, got {getattr(self, k)!r}")
            object.__setattr__(self, k, c)
        for k in ("thickness", "profile_thickness"):
            t = int(getattr(self, k))
            if not 1 <= t <= 32:
                raise ValueError(f"OverlayLines: {k} must be 1..32, got {getattr(self, k)!r}")
            object.__setattr__(self, k, t)

    def struct(self, clip_top: int = 0):
        """the style as a _lib.sd_overlay_style; rows above ``clip_top`` are never painted"""
        from . import _lib as L
        s = L.sd_overlay_style()
        s.rw_bgr[:], s.f2f_bgr[:], s.edge_bgr[:] = self.rw_bgr, self.f2f_bgr, self.edge_bgr
        s.thickness, s.profile_thickness, s.clip_top = self.thickness, self.profile_thickness, int(clip_top)
        return s

    def as_dict(self) -> dict:
        return {k: list(v) if isinstance(v, tuple) else v for k, v in dataclasses.asdict(self).items()}


def _check_lines(lines):
    if lines is not None and not isinstance(lines, OverlayLines):
        raise ValueError(f"lines must be None or an outputs.OverlayLines, got {lines!r}")
    return lines


def overlay_segments(record, camera, net_size: tuple, size: tuple, lines: OverlayLines | None = None, f2f=None, profile=None, f2f_profile=None,
                     clip_top: int = 0):
    """the measurement lines of one frame as data (sd_overlay_segments_host: the rule of include/semdepth.h, the segments
    Engine.draw_result_lines draws on the GPU): ``record`` a record of engine.RW_DTYPE, ``camera`` the frame's Camera (cx, cy, f) at the
    network size ``net_size`` = (h, w), ``size`` = (h, w) of the image drawn into, ``f2f`` a record of engine.F2F_DTYPE or None,
    ``profile`` / ``f2f_profile`` the D records of engine.RWP_DTYPE / F2FP_DTYPE of a depth profile or None.  Returns (``segs``, ``flag``):
    the valid segments in paint order as an array of SEG_DTYPE, end points in 1/256 pixel, and the frame's flag (bit 0: a segment was
    skipped because an end point does not project)."""
    import ctypes as C

    from . import _lib as L
    from .engine import F2F_DTYPE, F2FP_DTYPE, RW_DTYPE, RWP_DTYPE
    lines = _check_lines(lines) or OverlayLines()

    def raw(a, dt, n):
        if a is None:
            return None
        b = np.asarray(a)
        b = np.ascontiguousarray(b.reshape(-1).view(np.uint8) if b.dtype == dt else b, dtype=np.uint8).reshape(-1)
        if b.size != n * dt.itemsize:
            raise ValueError(f"overlay_segments: expected {n} record(s) of {dt.itemsize} bytes, got {b.size} bytes")
        return b

    D = 0 if profile is None else int(np.asarray(profile).shape[0])
    if f2f_profile is not None and profile is None:
        raise ValueError("overlay_segments: f2f_profile needs profile")
    rec, fr, pr, fpr = raw(record, RW_DTYPE, 1), raw(f2f, F2F_DTYPE, 1), raw(profile, RWP_DTYPE, D), raw(f2f_profile, F2FP_DTYPE, D)
    ptr = lambda a: None if a is None or a.size == 0 else a.ctypes.data_as(C.c_void_p)      # noqa: E731
    cam = L.sd_camera(float(camera.cx), float(camera.cy), float(camera.f), float(getattr(camera, "b", 0.0)), float(getattr(camera, "disp_mult", 0.0)))
    segs = np.zeros((4 * D + 2,), SEG_DTYPE)
    n, flag = C.c_int(), C.c_int32()
    st = L.load().sd_overlay_segments_host(C.byref(L.sd_rw_result.from_buffer_copy(rec.tobytes())), ptr(fr), ptr(pr), ptr(fpr), D, C.byref(cam),
                                           int(net_size[0]), int(net_size[1]), int(size[0]), int(size[1]), C.byref(lines.struct(clip_top)),
                                           segs.ctypes.data_as(C.POINTER(L.sd_overlay_segment)), C.byref(n), C.byref(flag))
    if st != L.SD_OK:
        raise ValueError(f"overlay_segments: refused (status {st}): extents 1..16384, at most 256 depths, clip_top 0..h, a finite camera")
    return segs[:n.value].copy(), int(flag.value)


def segments_json(segs) -> list:
    """overlay_segments' array as the list an ``_overlay.json`` carries under "lines": [ax, ay, bx, by] in 1/256 pixel, colour, thickness"""
    return [dict(a=[int(s["ax"]), int(s["ay"])], b=[int(s["bx"]), int(s["by"])], color=[int(c) for c in s["bgr"]], thickness=int(s["thickness"]))
            for s in segs]


def draw_lines(img: np.ndarray, segs, clip_top: int = 0) -> np.ndarray:
    """overlay_segments' segments rasterised into a copy of u8 [h,w,3] ``img`` in list order, rows above ``clip_top`` untouched
    (sd_overlay_draw_host: the rule of include/semdepth.h, the pixels Engine.draw_result_lines paints on the GPU -- not cv2.line's)."""
    import ctypes as C

    from . import _lib as L
    out = np.array(img, dtype=np.uint8, order="C", copy=True)
    if out.ndim != 3 or out.shape[2] != 3:
        raise ValueError(f"draw_lines: the image must be u8 [h,w,3], got {out.shape}")
    s = np.ascontiguousarray(np.asarray(segs, dtype=SEG_DTYPE).reshape(-1))
    st = L.load().sd_overlay_draw_host(out.ctypes.data_as(C.c_void_p), out.shape[0], out.shape[1],
                                       s.ctypes.data_as(C.POINTER(L.sd_overlay_segment)) if len(s) else None, len(s), int(clip_top))
    if st != L.SD_OK:
        raise ValueError(f"draw_lines: a segment, the image or clip_top is outside the caps of include/semdepth.h (status {st})")
    return out


# ------------------------------------------------------------------------------------------------ rendered clouds
@dataclasses.dataclass(frozen=True)
class RenderCamera:
    """the pinhole camera of the rendered clouds (sd_render_camera, include/semdepth.h): ``ext`` = world -> camera, row-major 3 x 4 (twelve
    numbers; Open3D's convention: x right, y down, z forward), the intrinsics, the near plane, the image size, the side of a point's square in
    pixels and the background in the image's channel order.  point_size 5 and a white background are Open3D's defaults."""
    ext: tuple
    fx: float
    fy: float
    cx: float
    cy: float
    width: int
    height: int
    z_near: float = 0.1
    point_size: int = 5
    background: tuple = (255, 255, 255)

    def __post_init__(self):
        object.__setattr__(self, "ext", tuple(float(v) for v in np.asarray(self.ext, np.float64).reshape(-1)))
        object.__setattr__(self, "background", tuple(int(v) for v in self.background))
        if len(self.ext) != 12 or len(self.background) != 3:
            raise ValueError("RenderCamera: ext holds twelve numbers (3 x 4, row-major), background three")

    def struct(self):
        """the camera as a _lib.sd_render_camera"""
        from . import _lib as L
        c = L.sd_render_camera()
        c.ext[:] = self.ext
        c.fx, c.fy, c.cx, c.cy, c.z_near = float(self.fx), float(self.fy), float(self.cx), float(self.cy), float(self.z_near)
        c.width, c.height, c.point_size = int(self.width), int(self.height), int(self.point_size)
        c.background[:] = self.background
        return c

    @classmethod
    def from_open3d_json(cls, path: str, z_near: float = 0.1, point_size: int = 5, background=(255, 255, 255)) -> "RenderCamera":
        """Open3D's PinholeCameraParameters file (write_pinhole_camera_parameters; the reference's ``top.json``): ``extrinsic`` = 16 numbers,
        the 4 x 4 world -> camera matrix COLUMN by column, ``intrinsic.intrinsic_matrix`` = 9 numbers, column by column, and
        ``intrinsic.width`` / ``height``.  The file has no near plane, point size or background: they are arguments."""
        with open(path) as f:
            d = json.load(f)
        e = np.asarray(d["extrinsic"], np.float64).reshape(4, 4).T
        k = np.asarray(d["intrinsic"]["intrinsic_matrix"], np.float64).reshape(3, 3).T
        return cls(ext=tuple(e[:3].reshape(-1)), fx=float(k[0, 0]), fy=float(k[1, 1]), cx=float(k[0, 2]), cy=float(k[1, 2]),
                   width=int(d["intrinsic"]["width"]), height=int(d["intrinsic"]["height"]), z_near=z_near, point_size=point_size,
                   background=tuple(background))

    def to_open3d_json(self, path: str) -> str:
        """the same file; read_pinhole_camera_parameters of Open3D takes it"""
        e = np.concatenate([np.asarray(self.ext, np.float64).reshape(3, 4), [[0.0, 0.0, 0.0, 1.0]]])
        k = np.array([[self.fx, 0.0, self.cx], [0.0, self.fy, self.cy], [0.0, 0.0, 1.0]])
        with open(path, "w") as f:
            json.dump({"class_name": "PinholeCameraParameters", "extrinsic": [float(v) for v in e.T.reshape(-1)],
                       "intrinsic": {"height": int(self.height), "intrinsic_matrix": [float(v) for v in k.T.reshape(-1)], "width": int(self.width)},
                       "version_major": 1, "version_minor": 0}, f, indent=1)
        return path


def top_camera(width: int = 512, height: int = 512, centre=(0.0, 0.0, 20.0), altitude: float = 40.0, fov_deg: float = 60.0, z_near: float = 0.1,
               point_size: int = 5, background=(255, 255, 255)) -> RenderCamera:
    """a top view of the road (the reference ships no ``top.json``): the camera sits at ``centre`` - altitude * (world y) -- world y points
    down, so that is above the road -- and looks along +y; image x is world x and image up is world +z, so far is at the top.
    fx = fy = (width / 2) / tan(fov / 2), cx = width / 2 - 0.5, cy = height / 2 - 0.5: ``centre`` lands on the central pixel."""
    c = np.asarray(centre, np.float64)
    rot = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])       # rows: the camera's x (world x), y (down = world -z), z (world +y)
    pos = c - float(altitude) * np.array([0.0, 1.0, 0.0])
    ext = np.concatenate([rot, (-rot @ pos)[:, None]], axis=1)
    f = (width / 2.0) / np.tan(np.deg2rad(fov_deg) / 2.0)
    return RenderCamera(ext=tuple(ext.reshape(-1)), fx=float(f), fy=float(f), cx=width / 2.0 - 0.5, cy=height / 2.0 - 0.5, width=int(width),
                        height=int(height), z_near=z_near, point_size=point_size, background=tuple(background))


def _check_render(render):
    if render is not None and not isinstance(render, RenderCamera):
        raise ValueError(f"render must be None or an outputs.RenderCamera, got {render!r}")
    return render


def render_rw(xyz, rgb, left_pt=None, right_pt=None, camera: RenderCamera | None = None, return_flag: bool = False):
    """the rendered view of one frame's ``_rw.ply`` on the host (sd_render_rw_host: the rule of include/semdepth.h, the pixels
    Engine.render_rw draws on the GPU -- not Open3D's): ``xyz`` [n,3] and ``rgb`` [n,3] of the final road cloud (taken as f32 / u8),
    ``left_pt`` / ``right_pt`` the end points of the road-width line or None when none was found -> u8 [height,width,3] BGR."""
    import ctypes as C

    from . import _lib as L
    from .engine import RW_DTYPE
    if camera is None:
        camera = top_camera()
    _check_render(camera)
    p = np.ascontiguousarray(np.asarray(xyz, np.float32).reshape(-1, 3))
    c = np.ascontiguousarray(np.asarray(rgb, np.uint8).reshape(-1, 3))
    if len(p) != len(c):
        raise ValueError(f"render_rw: {len(p)} points and {len(c)} colours")
    rec = np.zeros((), RW_DTYPE)
    if left_pt is not None and right_pt is not None:
        rec["found"] = 1
        rec["left_pt"], rec["right_pt"] = np.asarray(left_pt, np.float32).reshape(3), np.asarray(right_pt, np.float32).reshape(3)
    out = np.empty((camera.height, camera.width, 3), np.uint8)
    flag = C.c_int32()
    st = L.load().sd_render_rw_host(p.ctypes.data_as(C.c_void_p), c.ctypes.data_as(C.c_void_p), len(p), C.byref(L.sd_rw_result.from_buffer_copy(rec.tobytes())),
                                    C.byref(camera.struct()), out.ctypes.data_as(C.c_void_p), C.byref(flag))
    if st != L.SD_OK:
        raise ValueError(f"render_rw: the camera is outside the caps of include/semdepth.h (status {st})")
    return (out, flag.value) if return_flag else out


# ------------------------------------------------------------------------------------------------ disparity images
DISP_MAPS = ("gray", "plasma")              # SD_CMAP_GRAY, SD_CMAP_PLASMA: the reference's choice and its commented-out one (monodepth's own)


def _check_disp(disp):
    if disp is not None and disp not in DISP_MAPS:
        raise ValueError(f"disp must be None, 'gray' or 'plasma', got {disp!r}")
    return disp


def disp_colormap(cmap: str = "gray") -> np.ndarray:
    """the 256 entries of a colour map as u8 [256,3] RGB (sd_disp_colormap: matplotlib's table, kept as data)"""
    import ctypes as C

    from . import _lib as L
    if cmap not in DISP_MAPS:
        raise ValueError(f"cmap must be 'gray' or 'plasma', got {cmap!r}")
    out = np.empty((256, 3), np.uint8)
    st = L.load().sd_disp_colormap(DISP_MAPS.index(cmap), out.ctypes.data_as(C.c_void_p))
    assert st == L.SD_OK, st
    return out


def disparity_image(disp, out_h: int, out_w: int, cmap: str = "gray", mults=None):
    """DepthFrame.disp_to_image (semantic_depth.py:681-683: scipy.misc.imresize(disp, [h, w]) then plt.imsave(cmap=)) for
    f32 [B,h,w] (or [h,w]) ``disp`` on the host (sd_disp_image_host: the rule of include/semdepth.h, the bytes Engine.disparity_image
    makes on the GPU): per frame the map times ``mults[b]`` (None: 1) is byte-scaled over its finite range, resampled with Pillow's bilinear
    filter to out_h x out_w, normalised over the range of the resized bytes and looked up in matplotlib's ``cmap`` table.  Returns
    (``images`` u8 [B,out_h,out_w,3] BGR, ``flags`` i32 [B]; flags[b] = 1: frame b holds a non-finite value, which became byte 0)."""
    import ctypes as C

    from . import _lib as L
    if cmap not in DISP_MAPS:
        raise ValueError(f"cmap must be 'gray' or 'plasma', got {cmap!r}")
    d = np.ascontiguousarray(disp, dtype=np.float32)
    if d.ndim == 2:
        d = d[None]
    if d.ndim != 3:
        raise ValueError(f"disparity_image: the maps must be f32 [B,h,w] or [h,w], got {d.shape}")
    B, h, w = d.shape
    m = None
    if mults is not None:
        m = np.ascontiguousarray(mults, dtype=np.float32).reshape(-1)
        if m.shape != (B,):
            raise ValueError(f"disparity_image: {m.size} multipliers for {B} frames")
    out = np.empty((B, int(out_h), int(out_w), 3), np.uint8)
    flags = np.empty((B,), np.int32)
    st = L.load().sd_disp_image_host(d.ctypes.data_as(C.c_void_p), None if m is None else m.ctypes.data_as(C.c_void_p), B, h, w, int(out_h), int(out_w),
                                     DISP_MAPS.index(cmap), out.ctypes.data_as(C.c_void_p), flags.ctypes.data_as(C.c_void_p))
    if st != L.SD_OK:
        raise ValueError(f"disparity_image: {h}x{w} -> {out_h}x{out_w} is outside what the resample accepts (extents 1..16384, a downscale "
                         f"factor of at most 32; status {st})")
    return out, flags


def write_disp_image(output_name: str, disp, h: int, w: int, cmap: str = "gray", mult: float = 1.0) -> str:
    """``<output_name>_disp.png`` of semantic_depth.py:681-683 for one f32 [H,W] map: disparity_image at h x w through write_png (8-bit
    RGB; imsave's pixels, not its RGBA file bytes)"""
    d = np.asarray(disp, dtype=np.float32).squeeze()
    img, _ = disparity_image(d, h, w, cmap, [mult])
    return write_png("{}_disp.png".format(output_name), img[0])


def write_png(path: str, img_bgr: np.ndarray, level: int = 3) -> str:
    """8-bit PNG of a BGR (cv2 convention) or single-channel image; filter type 0 rows, one IDAT."""
    a = np.ascontiguousarray(img_bgr, dtype=np.uint8)
    if a.ndim == 3:
        a = a[..., ::-1]                       # cv2 stores BGR, PNG is RGB
        ctype, ch = 2, 3
    else:
        ctype, ch = 0, 1
    h, w = a.shape[:2]
    raw = np.zeros((h, 1 + w * ch), np.uint8)
    raw[:, 1:] = a.reshape(h, w * ch)

    def chunk(tag: bytes, data: bytes) -> bytes:
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n")
        f.write(chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, ctype, 0, 0, 0)))
        f.write(chunk(b"IDAT", zlib.compress(raw.tobytes(), level)))
        f.write(chunk(b"IEND", b""))
    return path


# ------------------------------------------------------------------------------------------------ per-frame outputs
def road_plane_grid(road3D, road_colors, z_cut: float = 7.0, mad_y: float = 15.0, mad_x: float = 2.0, plane_thr: float = 5.0):
    """``road_plane3D, road_colors_plane`` of semantic_depth.py:215-219: the 5 cm visualisation lattice over the bounding box of the
    cloud that ENTERS the plane fit (after the z-cut and the two MAD filters, :206-212), lifted onto the fitted plane.  The batched
    road chain keeps only the filtered cloud, so the save path replays the reference's own call sequence through the pcl module
    (the same kernels, one cloud at a time) on the gathered road cloud.  (None, None) when a filter empties the cloud."""
    p3, c = np.asarray(road3D), np.asarray(road_colors)
    if not len(p3):
        return None, None
    p3, c = pcl.remove_from_to(p3, c, 2, 0.0, z_cut)
    for axis, thr in ((1, mad_y), (0, mad_x)):
        if not len(p3):
            return None, None
        p3, c = pcl.remove_noise_by_mad(p3, c, axis, thr)
    if not len(p3):
        return None, None
    _, _, plane3D, colors_plane, _ = pcl.remove_noise_by_fitting_plane(p3, c, axis=1, threshold=plane_thr, plane_color=[200, 200, 200])
    return plane3D, colors_plane


def fence_plane_grids(fence3D, fence_colors, mad_y: float = 5.0, z_max: float = 35.0, mad_left: float = 5.0, mad_right: float = 1.0,
                      plane_thr: float = 1.0):
    """``fence_left_plane3D, fence_left_colors_plane, fence_right_plane3D, fence_right_colors_plane`` of semantic_depth.py:279-309,
    replayed through the pcl module like road_plane_grid.  A side that runs empty gives (None, None) for that side."""
    out = [None, None, None, None]
    p3, c = np.asarray(fence3D), np.asarray(fence_colors)
    if not len(p3):
        return tuple(out)
    p3, c = pcl.remove_noise_by_mad(p3, c, 1, mad_y)
    if not len(p3):
        return tuple(out)
    p3, c = pcl.threshold_complete(p3, c, 2, z_max)
    if not len(p3):
        return tuple(out)
    l3, lc, r3, rc = pcl.extract_pcls(p3, c)
    for i, (q3, qc, thr) in enumerate(((l3, lc, mad_left), (r3, rc, mad_right))):
        if not len(q3):
            continue
        q3, qc = pcl.remove_noise_by_mad(q3, qc, 0, thr)
        if not len(q3):
            continue
        _, _, out[2 * i], out[2 * i + 1], _ = pcl.remove_noise_by_fitting_plane(q3, qc, axis=0, threshold=plane_thr, plane_color=[40, 70, 40])
    return tuple(out)


def resize_to_original(segmented_frame: np.ndarray, original_width: int, original_height: int) -> np.ndarray:
    """``cv2.resize(segmented_frame, (original_width, original_height), interpolation=cv2.INTER_CUBIC)`` of semantic_depth.py:341-342,
    on the GPU (sd_resize_cubic_u8, the kernel of the input stage)."""
    import torch
    e = pcl._eng()
    fr = torch.from_numpy(np.ascontiguousarray(segmented_frame, dtype=np.uint8))[None].to(e.device)
    return e.resize_cubic(fr, original_height, original_width)[0].cpu().numpy()


def save_frame_outputs(output_name: str, res: dict, depth: float, approach: str = "rw", segmented_frame: np.ndarray | None = None,
                       is_city: bool = False, times: dict | None = None, road_plane3D=None, road_colors_plane=None,
                       points3D_all=None, colors_all=None, original_size: tuple | None = None, params=None, fence_params=None,
                       text: str = "json", render: RenderCamera | None = None, profile=None, lines: OverlayLines | None = None, camera=None):
    """what FrameProcessor.process_frame writes when --save_data is set (semantic_depth.py:339-458), from the dict
    ``api.FrameProcessor.process_frame(..., want_clouds=True)`` returns.  Returns the list of files written.
    ``original_size`` = (original_height, original_width): the overlay is cubic-resized back to it before anything is drawn (:341);
    ``params`` / ``fence_params`` (engine.RoadWidthParams / FenceParams): the chain literals the visualisation planes are rebuilt with.
    ``text``: "json" (default) leaves the banner of the annotated image empty; "draw" rasterises the items into it (draw_text).  The
    ``_overlay.json`` is written either way.
    ``render``: None (default) or a RenderCamera: also ``<output_name>_render.png``, the final road cloud and the road-width line of the
    record behind that camera (render_rw, the host statement of the sequence tool's rendered clouds).
    ``profile``: None (default) or the depth profile of the frame (``res["profile"]`` of FrameProcessor(depths=); True takes it from
    ``res``): also ``<output_name>_profile.txt`` (profile_text).
    ``lines``: None (default) or an OverlayLines: the measured road-width line, with approach 'both' the fence-to-fence line and, when ``res``
    carries a depth profile's records, the road's edges and the rungs along it are drawn into the annotated image on the host
    (overlay_segments + draw_lines) behind the cubic resize and before the text, below the banner (clip_top = int(0.2 h)); the
    ``_overlay.json`` gains "lines".  It needs ``camera`` (the frame's engine.Camera at the size of ``segmented_frame`` as given) and
    ``segmented_frame``: ValueError otherwise, before anything is written."""
    _check_text(text)
    _check_render(render)
    if _check_lines(lines) is not None and (camera is None or segmented_frame is None):
        raise ValueError("save_frame_outputs: lines= needs camera= and segmented_frame=")
    files = []
    rec = res["record"]
    if not rec["found"]:
        # semantic_depth.py indexes left_pt_rw[0] unconditionally (:259) and dies on (None, None); the sequence tool guards it
        # (seq:232-234).  Here: the same TypeError the reference raises, before anything is written.
        raise TypeError("'NoneType' object is not subscriptable (no road point in the depth window: left_pt_rw is None)")
    left_rw, right_rw = rec["left_pt"].astype(np.float64)[None, :], rec["right_pt"].astype(np.float64)[None, :]
    dist_rw = res["dist_rw"]
    line_rw, colors_line_rw = pcl.create_3Dline_from_3Dpoints(left_rw.copy(), right_rw.copy(), [250, 0, 0])
    line_rw[:, 2] += 0.2                                   # :265 "for better visualization, shift it a bit"
    f2 = res.get("f2f_record")
    both = approach == "both" and f2 is not None
    if both:
        left_f2f, right_f2f = f2["left_pt"][None, :].copy(), f2["right_pt"][None, :].copy()
        line_f2f, colors_line_f2f = pcl.create_3Dline_from_3Dpoints(left_f2f.copy(), right_f2f.copy(), [0, 255, 0])
    if segmented_frame is not None:
        net_size = tuple(segmented_frame.shape[:2])
        if original_size is not None and tuple(segmented_frame.shape[:2]) != tuple(original_size):
            segmented_frame = resize_to_original(segmented_frame, int(original_size[1]), int(original_size[0]))     # :341-342
        files.append(write_png("{}_only_segmentation.png".format(output_name), segmented_frame))                  # :345
        h, w = segmented_frame.shape[:2]
        banner, items = overlay_items(w, h, depth, is_city, left_rw, right_rw, dist_rw, "both" if both else "rw",
                                      left_f2f if both else None, right_f2f if both else None, res.get("dist_f2f"))
        img, items = draw_overlay(segmented_frame, banner, items)
        doc = dict(banner=banner, items=items)
        if lines is not None:
            clip = int(0.2 * h)
            segs, _ = overlay_segments(rec, camera, net_size, (h, w), lines, f2f=f2 if both else None, profile=res.get("profile_records"),
                                       f2f_profile=res.get("f2f_profile_records") if both and res.get("profile_records") is not None else None,
                                       clip_top=clip)
            img = draw_lines(img, segs, clip)
            doc["lines"] = segments_json(segs)
        if text == "draw":
            img = draw_text(img, items)
        files.append(write_png("{}.png".format(output_name), img))
        with open("{}_overlay.json".format(output_name), "w") as f:
            json.dump(doc, f)
        files.append("{}_overlay.json".format(output_name))
    if render is not None:
        files.append(write_png("{}_render.png".format(output_name), render_rw(res["road3D_final"], res["road_colors_final"], rec["left_pt"], rec["right_pt"], render)))
    road3D, road_colors = res["road3D_final"].astype(np.float64), res["road_colors_final"]
    pc = PointCloud2Ply(road3D, road_colors, "{}_ROAD".format(output_name))                 # :408-410
    pc.prepare_and_save_point_cloud()
    files.append("{}_ROAD.ply".format(output_name))
    if both and "fence3D_left" in res:                                                      # :412-415
        pc = PointCloud2Ply(res["fence3D_left"], res["fence_left_colors"], "{}_FENCE".format(output_name))
        pc.add_extra_point_cloud(res["fence3D_right"], res["fence_right_colors"])
        pc.prepare_and_save_point_cloud()
        files.append("{}_FENCE.ply".format(output_name))
    pc = PointCloud2Ply(road3D, road_colors, output_name)                                   # :421-434
    if road_plane3D is None and "road3D" in res:                                            # the visualisation plane of :215-219
        kw = {k: getattr(params, k) for k in ("z_cut", "mad_y", "mad_x", "plane_thr")} if params is not None else {}
        road_plane3D, road_colors_plane = road_plane_grid(res["road3D"], res["road_colors"], **kw)
    if road_plane3D is not None:
        pc.add_extra_point_cloud(road_plane3D, road_colors_plane)
    pc.add_extra_point_cloud(line_rw, colors_line_rw)
    if both and "fence3D_left" in res:
        pc.add_extra_point_cloud(res["fence3D_left"], res["fence_left_colors"])
        pc.add_extra_point_cloud(res["fence3D_right"], res["fence_right_colors"])
        if "fence3D" in res:                                                                # :428-431
            kw = ({k: getattr(fence_params, k) for k in ("mad_y", "z_max", "mad_left", "mad_right", "plane_thr")} if fence_params is not None else {})
            lp, lcp, rp, rcp = fence_plane_grids(res["fence3D"], res["fence_colors"], **kw)
            if lp is not None:
                pc.add_extra_point_cloud(lp, lcp)
            if rp is not None:
                pc.add_extra_point_cloud(rp, rcp)
        pc.add_extra_point_cloud(line_f2f, colors_line_f2f)
    pc.prepare_and_save_point_cloud()
    files.append("{}.ply".format(output_name))
    if points3D_all is not None:                                                            # :437-441
        pc = PointCloud2Ply(np.asarray(points3D_all).reshape(-1, 3), np.asarray(colors_all).reshape(-1, 3), "{}_ALL".format(output_name))
        pc.add_extra_point_cloud(line_rw, colors_line_rw)
        if both:
            pc.add_extra_point_cloud(line_f2f, colors_line_f2f)
        pc.prepare_and_save_point_cloud()
        files.append("{}_ALL.ply".format(output_name))
    if times is not None:
        files.append(write_times(output_name, times))
    files.append(write_distances(output_name, dist_rw, res.get("dist_f2f")))
    if profile is not None and profile is not False:
        rows = res["profile"] if profile is True else profile
        dist = [r["dist_f2f"] for r in rows] if rows and "dist_f2f" in rows[0] else None
        with open("{}_profile.txt".format(output_name), "w") as f:
            f.write(profile_text([r["depth"] for r in rows], rows, dist))
        files.append("{}_profile.txt".format(output_name))
    return files


# ------------------------------------------------------------------------------------------------ per-frame metrics log
def append_metrics_jsonl(path: str, name: str, res: dict, times: dict | None = None, extra: dict | None = None) -> str:
    """one JSON line per processed frame (SURVEY §5 "Metrics / logging": the reference only prints): frame name, both distances, the
    kept-point count after every stage of the road chain, the plane, the end points, the stage times when given.  ``res`` is the dict
    api.FrameProcessor.process_frame returns."""
    rec = res["record"]
    line = {"frame": name, "dist_rw": res.get("dist_rw"), "dist_f2f": res.get("dist_f2f"), "found": bool(rec["found"]),
            "points": {k: int(rec[k]) for k in ("n_road", "n_zcut", "n_mad_y", "n_mad_x", "n_plane", "n_sor", "n_ror")},
            "road_plane": [float(v) for v in rec["plane"]],
            "left_pt": [float(v) for v in rec["left_pt"]] if rec["found"] else None,
            "right_pt": [float(v) for v in rec["right_pt"]] if rec["found"] else None}
    if res.get("f2f_record") is not None:
        f2 = res["f2f_record"]
        line["fence"] = {"ok": bool(f2["ok"]), "counts": [int(c) for c in f2["counts"]], "plane_left": [float(v) for v in f2["plane_left"]],
                         "plane_right": [float(v) for v in f2["plane_right"]]}
    if times is not None:
        line["times_s"] = {k: float(times[k]) for k in TIME_KEYS if k in times}
    if extra:
        line.update(extra)
    with open(path, "a") as f:
        f.write(json.dumps(line) + "\n")
    return path


# ------------------------------------------------------------------------------------------------ focal-length sweep
def write_sweep_data(f_directory: str, all_data, n_frames: int):
    """semantic_depth.py:907-936: rows (real, rw, f2f, |real-rw|, |real-f2f|) + a last row holding the two MAEs in columns
    3 and 4, ``fmt='%1.4f'``.  Returns (mae_rw, mae_f2f)."""
    all_data_array = np.asarray(all_data)
    mae_rw = np.sum(all_data_array[:, 3]) / n_frames
    mae_f2f = np.sum(all_data_array[:, 4]) / n_frames
    mae_for_file = np.zeros((1, 5))
    mae_for_file[:, 3] = mae_rw
    mae_for_file[:, 4] = mae_f2f
    np.savetxt("{}/data.txt".format(f_directory), np.concatenate((all_data_array, mae_for_file)), fmt="%1.4f")
    return mae_rw, mae_f2f


def focal_sweep(process, input_frames: dict, frame_depther, focal_lengths=(380, 580), results_directory: str = "results"):
    """the ``args.f is None`` branch of main(), semantic_depth.py:854-944.
    ``process(name) -> (dist_rw, dist_f2f)`` runs the pipeline on one frame (FrameProcessor.process_frame);
    ``input_frames``: name -> ground-truth width at the measuring depth (:837); ``frame_depther.f`` is reassigned per trial
    (:859).  Writes ``<results>/<f>/data.txt`` and ``<results>/best_focal_lengths.txt``; returns the summary dict."""
    best = dict(rw=(-1, None), f2f=(-1, None), overall=(-1, None))
    per_f = {}
    for f in focal_lengths:
        frame_depther.f = f
        f_directory = os.path.join(results_directory, str(f))
        os.makedirs(f_directory, exist_ok=True)
        all_data = []
        for name, real_distance in sorted(input_frames.items()):
            dist_rw, dist_f2f = process(name)
            all_data.append([real_distance, dist_rw, dist_f2f, abs(real_distance - dist_rw), abs(real_distance - dist_f2f)])
        mae_rw, mae_f2f = write_sweep_data(f_directory, all_data, len(input_frames))
        mae_overall = mae_rw + mae_f2f
        per_f[f] = dict(mae_rw=float(mae_rw), mae_f2f=float(mae_f2f), rows=all_data)
        for key, mae in (("rw", mae_rw), ("f2f", mae_f2f), ("overall", mae_overall)):
            if best[key][0] == -1 or mae < best[key][0]:
                best[key] = (mae, f)
    with open("{}/best_focal_lengths.txt".format(results_directory), "w") as fh:
        fh.write("Best f road's width: {}\n".format(best["rw"][1]))
        fh.write("Best f fence2fence:  {}\n".format(best["f2f"][1]))
        fh.write("Best f overall:      {}\n".format(best["overall"][1]))
    return dict(best_f_rw=best["rw"][1], best_f_f2f=best["f2f"][1], best_f_overall=best["overall"][1], per_f=per_f)


def sweep_cameras(frame_depther, focal_lengths, multipliers) -> list:
    """cams[t][b] = ``frame_depther.camera(multipliers[b])`` with f = focal_lengths[t]; ``frame_depther.f`` is left alone"""
    return [[dataclasses.replace(frame_depther.camera(m), f=f) for m in multipliers] for f in focal_lengths]


def sweep_distances_batched(frames: dict, input_frames: dict, frame_segmenter, frame_depther, focal_lengths, depth: float = 10.0,
                            approach: str = "both", disp_multiplier=None, params=None, fence_params=None) -> dict:
    """(focal length, frame name) -> (dist_rw, dist_f2f) as FrameProcessor.process_frame reports them (None where found == 0 / ok == 0),
    with ONE pass of each network per frame: each batch of frames (at most the engine's max_batch; 1 is legal and simply gets no trial
    batching) goes through Engine.camera_sweep, the trial focal lengths as a batch axis of the tail.  ``frames``: name -> u8 BGR frame
    of any size (cubic-resized to the network shape like process_frame does); a frame's disparity multiplier is its original width,
    or ``disp_multiplier``."""
    import torch

    from .engine import Engine, FenceParams, RoadWidthParams
    focal_lengths = list(focal_lengths)
    e = frame_depther.engine
    if getattr(frame_segmenter, "_engine", e) is None and (e.H, e.W) == tuple(frame_segmenter.input_shape):
        frame_segmenter._engine = e                           # built independently of the DepthFrame: join its Engine (as FrameProcessor)
    if frame_segmenter.engine is not e:
        raise ValueError("the batched sweep needs the segmenter and the depther on one Engine")
    params = params or RoadWidthParams(depth=depth)
    fence_params = fence_params or FenceParams(depth=depth)
    names = sorted(input_frames)
    dists = {}
    for b0 in range(0, len(names), e.max_batch):
        batch = names[b0:b0 + e.max_batch]
        fr, mults = [], []
        for name in batch:
            frame = np.ascontiguousarray(frames[name], dtype=np.uint8)
            mults.append(disp_multiplier if disp_multiplier is not None else frame.shape[1])
            t = torch.from_numpy(frame)[None].to(e.device)
            fr.append(t if tuple(t.shape[1:3]) == (e.H, e.W) else e.resize_cubic(t))
        out = e.camera_sweep(torch.cat(fr).contiguous(), sweep_cameras(frame_depther, focal_lengths, mults), params, approach=approach,
                             fence_params=fence_params)
        recs = Engine.records(out["records"])                 # the one read-back of the batch: every trial's record
        f2fs = Engine.f2f_records(out["f2f"]) if out.get("f2f") is not None else None
        e.check_range()
        for t, f in enumerate(focal_lengths):
            for b, name in enumerate(batch):
                rec = recs[t * len(batch) + b]
                f2 = f2fs[t * len(batch) + b] if f2fs is not None else None
                dists[(f, name)] = (float(rec["width"]) if rec["found"] else None, float(f2["dist"]) if (f2 is not None and f2["ok"]) else None)
    return dists


def focal_sweep_batched(frames: dict, input_frames: dict, frame_segmenter, frame_depther, focal_lengths=(380, 580),
                        results_directory: str = "results", depth: float = 10.0, approach: str = "both", disp_multiplier=None, params=None,
                        fence_params=None):
    """focal_sweep over FrameProcessor.process_frame behind one network pass per frame (sweep_distances_batched): the same
    ``<results>/<f>/data.txt``, ``best_focal_lengths.txt`` and returned dict -- focal_sweep itself writes them, fed from the table --
    without touching ``frame_depther.f``.  A (focal length, frame) without a distance (the reference and focal_sweep die there on
    ``abs(real - None)``) raises ValueError before any file is written."""
    focal_lengths = list(focal_lengths)
    dists = sweep_distances_batched(frames, input_frames, frame_segmenter, frame_depther, focal_lengths, depth, approach, disp_multiplier,
                                    params, fence_params)
    for f in focal_lengths:
        for name in sorted(input_frames):
            for what, v in zip(("road width", "fence-to-fence distance"), dists[(f, name)]):
                if v is None:
                    raise ValueError(f"focal_sweep_batched: no {what} for focal length {f}, frame {name!r}")

    class Trial:                                              # stands in for the operator whose f focal_sweep reassigns per trial
        f = None

    trial = Trial()
    return focal_sweep(lambda name: dists[(trial.f, name)], input_frames, trial, focal_lengths, results_directory)


# ------------------------------------------------------------------------------------------------ the sequence tool's files
SEQ_IMG_DIR, SEQ_PLY_DIR = "result_sequence_imgs", "result_sequence_ply"          # semantic_depth_cityscapes_sequence.py:671-680
SEQ_PROFILE_DIR = "result_sequence_profile"                                       # the per-frame depth profiles (SequenceOutputs(profile=))
SEQ_RENDER_DIR = "rendered_sequence"                                              # utils/render_ply.py's output folder
SEQ_DISP_DIR = "result_sequence_disp"                                             # the per-frame disparity images (SequenceOutputs(disp=))


# ------------------------------------------------------------------------------------------------ result video
@dataclasses.dataclass(frozen=True)
class Video:
    """the result video of the sequence tool (opt-in, SequenceOutputs(video=)): the composed result images as a Motion-JPEG AVI at ``fps``
    frames per second, every frame a baseline JPEG file at the IJG ``quality`` 1..100 (the format of include/semdepth.h).  ``route``:
    "device" (Engine.encode_jpeg makes the files on the GPU, only their bytes travel) or "host" (the raw images travel and
    sd_jpeg_encode_bgr_host makes the same bytes on the writer threads)."""
    fps: float = 30.0
    quality: int = 90
    route: str = "device"

    def __post_init__(self):
        object.__setattr__(self, "fps", float(self.fps))
        object.__setattr__(self, "quality", int(self.quality))
        if not (self.fps > 0 and np.isfinite(self.fps)):
            raise ValueError(f"Video: fps must be a positive number, got {self.fps!r}")
        if not 1 <= self.quality <= 100:
            raise ValueError(f"Video: quality must be 1..100, got {self.quality!r}")
        if self.route not in ("device", "host"):
            raise ValueError(f"Video: route must be 'device' or 'host', got {self.route!r}")


def _check_video(video):
    if video is not None and not isinstance(video, Video):
        raise ValueError(f"video must be None or an outputs.Video, got {video!r}")
    return video


def encode_jpeg_host(img_bgr: np.ndarray, quality: int = 90) -> bytes:
    """one u8 [h,w,3] BGR image -> the bytes of its baseline JPEG file (sd_jpeg_encode_bgr_host: the CPU statement of Engine.encode_jpeg,
    the same bytes)"""
    import ctypes as C

    from . import _lib as L
    a = np.ascontiguousarray(img_bgr, dtype=np.uint8)
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"image must be u8 [h,w,3], got {a.shape}")
    h, w = a.shape[:2]
    lib = L.load()
    bound, size = C.c_size_t(), C.c_size_t()
    if lib.sd_jpeg_encode_workspace(1, h, w, None, C.byref(bound)) != L.SD_OK:
        raise ValueError(f"encode_jpeg_host: extents must be 1..16384, got {h} x {w}")
    out = np.empty(bound.value, np.uint8)
    st = lib.sd_jpeg_encode_bgr_host(a.ctypes.data_as(C.c_void_p), h, w, int(quality), out.ctypes.data_as(C.c_void_p), out.size, C.byref(size))
    if st != L.SD_OK:
        raise ValueError(f"encode_jpeg_host: refused (status {st}; quality must be 1..100)")
    return out[:size.value].tobytes()


AVI_RIFF_LIMIT = 2 ** 31 - 2 ** 24          # a part is closed before its RIFF chunk would pass this


class MjpegAviWriter:
    """a Motion-JPEG AVI written frame by frame: RIFF 'AVI ' = LIST hdrl (avih; LIST strl (strh 'vids' / 'MJPG', strf = a 40-byte
    BITMAPINFOHEADER)), LIST movi (one '00dc' chunk per frame, padded to even length) and idx1 (one key-frame entry per chunk, offsets
    relative to the 'movi' fourcc).  ``append(jpeg_bytes)`` adds a frame (a complete JPEG file of width x height), ``close()`` writes the
    index and patches the counts and sizes of the headers.  Before the RIFF chunk would pass 2^31 - 2^24 bytes the file is closed and the
    frames continue in ``<stem>_part<k>.avi`` (k = 1, 2, ...); ``paths`` lists the files written, in order.  fps becomes the rational
    dwRate / dwScale with a denominator of at most 1001 (29.97 -> 30000 / 1001)."""
    HEADER_BYTES = 224                      # everything in front of the first '00dc' chunk; the 'movi' fourcc is at 220

    def __init__(self, path: str, width: int, height: int, fps: float = 30.0, _max_riff_bytes: int = AVI_RIFF_LIMIT):
        from fractions import Fraction
        if not (1 <= int(width) <= 65535 and 1 <= int(height) <= 65535):
            raise ValueError("MjpegAviWriter: width and height must be 1..65535")
        if not (float(fps) > 0 and np.isfinite(float(fps))):
            raise ValueError("MjpegAviWriter: fps must be a positive number")
        fr = Fraction(float(fps)).limit_denominator(1001)
        if fr <= 0:
            raise ValueError("MjpegAviWriter: fps too small")
        self.rate, self.scale = fr.numerator, fr.denominator
        self.width, self.height, self.fps = int(width), int(height), float(fps)
        self.stem, self.ext = os.path.splitext(path)
        self.limit = int(_max_riff_bytes)
        self.paths, self.frames = [], 0
        self._f = None
        self._open(path)

    def _header(self, nframes: int, movi_bytes: int, riff_bytes: int, max_chunk: int) -> bytes:
        usec = int(round(1e6 * self.scale / self.rate))
        bps = int(min(2 ** 32 - 1, max_chunk * self.rate // self.scale + 1)) if nframes else 0
        avih = struct.pack("<14I", usec, bps, 0, 0x10, nframes, 0, 1, max_chunk, self.width, self.height, 0, 0, 0, 0)
        strh = struct.pack("<4s4sIHHIIIIIIII4h", b"vids", b"MJPG", 0, 0, 0, 0, self.scale, self.rate, 0, nframes, max_chunk, 0xFFFFFFFF, 0,
                           0, 0, self.width, self.height)
        strf = struct.pack("<IiiHH4sIiiII", 40, self.width, self.height, 1, 24, b"MJPG", self.width * self.height * 3, 0, 0, 0, 0)
        strl = b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh + b"strf" + struct.pack("<I", len(strf)) + strf
        hdrl = b"hdrl" + b"avih" + struct.pack("<I", len(avih)) + avih + b"LIST" + struct.pack("<I", len(strl)) + strl
        out = (b"RIFF" + struct.pack("<I", riff_bytes) + b"AVI " + b"LIST" + struct.pack("<I", len(hdrl)) + hdrl +
               b"LIST" + struct.pack("<I", movi_bytes) + b"movi")
        assert len(out) == self.HEADER_BYTES, len(out)
        return out

    def _open(self, path: str):
        self._f = open(path, "wb")
        self.paths.append(path)
        self._index, self._movi, self._max_chunk = [], 4, 0            # _movi: bytes of the LIST movi payload so far ('movi' itself: 4)
        self._f.write(self._header(0, 4, 0, 0))

    def _riff_bytes(self, movi: int, entries: int) -> int:
        return self.HEADER_BYTES - 8 - 4 + movi + 8 + 16 * entries

    def _close_part(self):
        f, self._f = self._f, None
        idx = b"".join(struct.pack("<4sIII", b"00dc", 0x10, off, size) for off, size in self._index)
        f.write(b"idx1" + struct.pack("<I", len(idx)) + idx)
        f.seek(0)
        f.write(self._header(len(self._index), self._movi, self._riff_bytes(self._movi, len(self._index)), self._max_chunk))
        f.close()

    def append(self, jpeg: bytes):
        if self._f is None:
            raise RuntimeError("MjpegAviWriter.append after close")
        data = bytes(jpeg) if not isinstance(jpeg, (bytes, bytearray, memoryview)) else jpeg
        n = len(data)
        padded = n + (n & 1)
        if self._index and self._riff_bytes(self._movi + 8 + padded, len(self._index) + 1) > self.limit:
            self._close_part()
            self._open("{}_part{}{}".format(self.stem, len(self.paths), self.ext))
        self._index.append((self._movi, n))
        self._f.write(b"00dc" + struct.pack("<I", n))
        self._f.write(data)
        if n & 1:
            self._f.write(b"\0")
        self._movi += 8 + padded
        self._max_chunk = max(self._max_chunk, n)
        self.frames += 1

    def close(self) -> list:
        if self._f is not None:
            self._close_part()
        return list(self.paths)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def join_mjpeg_avi(paths, out: str, _max_riff_bytes: int = AVI_RIFF_LIMIT) -> list:
    """the frames of the Motion-JPEG AVIs ``paths`` (the parts of a rolled-over file, the shards of the ranks), in that order, re-muxed into
    ``out`` (and ``<stem>_part<k>.avi`` when it rolls over itself): the chunks are copied, nothing is decoded.  Size and frame rate are the
    first file's; a file of another size is refused.  Returns the files written."""
    from .frame_io import avi_frames, avi_info
    paths = list(paths)
    if not paths:
        raise ValueError("join_mjpeg_avi: no input")
    first = avi_info(paths[0])
    with MjpegAviWriter(out, first["width"], first["height"], first["rate"] / first["scale"], _max_riff_bytes=_max_riff_bytes) as wr:
        for p in paths:
            info = avi_info(p)
            if (info["width"], info["height"]) != (first["width"], first["height"]):
                raise ValueError(f"join_mjpeg_avi: {p} is {info['width']} x {info['height']}, the first file {first['width']} x {first['height']}")
            for frame in avi_frames(p):
                wr.append(frame)
    return wr.paths


def sequence_names(paths) -> list:
    """``output_name`` of every frame in the order the sequence tool visits them (seq:689-699): basename without extension of
    ``sorted(paths)``"""
    return [os.path.splitext(os.path.basename(p))[0] for p in sorted(paths)]


def write_png_batch(paths, frames_bgr, level: int = 1, threads: int = 0) -> list:
    """cv2.imwrite(paths[i], frames_bgr[i]) for u8 [n,h,w,3] BGR frames: 8-bit RGB PNGs at zlib ``level``, encoded and written by ONE native
    call on ``threads`` C++ threads (sd_png_encode_bgr_files; 0 = one per CPU), no interpreter lock held.  Pixel-exact (sd_png_decode_bgr /
    any PNG reader gives the frames back), not byte-identical to OpenCV's files.  Returns the paths."""
    import ctypes as C

    from . import _lib as L
    a = np.ascontiguousarray(frames_bgr, dtype=np.uint8)
    if a.ndim != 4 or a.shape[3] != 3 or a.shape[0] != len(paths):
        raise ValueError(f"frames must be u8 [n,h,w,3] with n = len(paths), got {a.shape} for {len(paths)} paths")
    n, h, w = a.shape[:3]
    if n == 0:
        return []
    arr = (C.c_char_p * n)(*[os.fsencode(p) for p in paths])
    status = (C.c_int * n)()
    st = L.load().sd_png_encode_bgr_files(arr, n, h, w, a.ctypes.data_as(C.c_void_p), h * w * 3, int(level), int(threads), status)
    if st != L.SD_OK:
        bad = [(paths[i], status[i]) for i in range(n) if status[i] != L.SD_OK]
        raise OSError(f"write_png_batch: {len(bad) or n} image(s) could not be written (status {st}): {bad[:3]}")
    return list(paths)


def write_png_streams(paths, streams, sizes, h: int, w: int, threads: int = 0) -> list:
    """the files of the device route: ``streams`` u8 [n,stride] and ``sizes`` [n] (host arrays: Engine.encode_png's tensors, copied) are
    finished zlib streams of h x w RGB frames; ONE native call (sd_png_write_streams_files, ``threads`` C++ threads, 0 = one per CPU) wraps
    each in signature, IHDR, IDAT chunks and IEND and writes it to paths[i].  Returns the paths."""
    import ctypes as C

    from . import _lib as L
    a = np.ascontiguousarray(streams, dtype=np.uint8)
    sz = np.ascontiguousarray(sizes).astype(np.uint64)
    if a.ndim != 2 or a.shape[0] != len(paths) or sz.shape != (len(paths),):
        raise ValueError(f"streams must be u8 [n,stride] and sizes [n] with n = len(paths), got {a.shape}, {sz.shape} for {len(paths)} paths")
    n = len(paths)
    if n == 0:
        return []
    arr = (C.c_char_p * n)(*[os.fsencode(p) for p in paths])
    status = (C.c_int * n)()
    st = L.load().sd_png_write_streams_files(arr, n, int(h), int(w), a.ctypes.data_as(C.c_void_p), a.shape[1], sz.ctypes.data_as(C.c_void_p),
                                             int(threads), status)
    if st != L.SD_OK:
        bad = [(paths[i], status[i]) for i in range(n) if status[i] != L.SD_OK]
        raise OSError(f"write_png_streams: {len(bad) or n} image(s) could not be written (status {st}): {bad[:3]}")
    return list(paths)


def rw_ply_bytes(road3D, road_colors, left_pt_rw=None, right_pt_rw=None) -> bytes:
    """the bytes of ``<name>_rw.ply`` (seq:357-361): PointCloud2Ply(road3D, road_colors, ...) plus, when the line was found (both end
    points given, [1,3] each), create_3Dline_from_3Dpoints(left, right, [250,0,0]), after prepare_and_save_point_cloud's minimum-z filter.
    An empty road cloud (the reference's np.min raises there) gives a file with no vertex."""
    from .point_cloud_2_ply import format_rows
    pts, col = np.asarray(road3D).reshape(-1, 3), np.asarray(road_colors).reshape(-1, 3)
    if left_pt_rw is not None and right_pt_rw is not None:
        line, colors_line = pcl.create_3Dline_from_3Dpoints(np.array(left_pt_rw, np.float64), np.array(right_pt_rw, np.float64), [250, 0, 0])
        pts, col = np.append(pts, line, axis=0), np.append(col, colors_line, axis=0)
    if len(pts):
        keep = pts[:, 2] > pts[:, 2].min()
        pts, col = pts[keep], col[keep]
    return PointCloud2Ply.ply_header.format(vertex_count=len(pts)).encode() + format_rows(pts, col, threads=1)


# ------------------------------------------------------------------------------------------------ scene PLYs
# the files of Scene(files=): key -> (suffix of <name> in result_sequence_ply, the segments of sd_scene_format's mask)
SCENE_FILES = {"scene": ("_scene.ply", 255), "road": ("_ROAD.ply", 1), "fence": ("_FENCE.ply", 8 | 16)}


@dataclasses.dataclass(frozen=True)
class Scene:
    """the 3D products of semantic_depth.py:404-431 for every frame of the sequence tool (opt-in, SequenceOutputs(scene=)), in
    ``result_sequence_ply``: ``<name>_scene.ply`` (road cloud, road plane lattice, road-width line, both fence clouds, both fence plane
    lattices, fence-to-fence line -- the fence part only with approach 'both'), ``<name>_ROAD.ply`` (the road cloud) and, with approach
    'both', ``<name>_FENCE.ply`` (both fence clouds); ``files`` chooses among "scene", "road", "fence".  The format is
    include/semdepth.h's (sd_scene_format): the road-width line is the sequence tool's, without the single-frame tool's z += 0.2.
    ``route``: "device" (Engine.format_scene_ply makes the text on the GPU, only its bytes travel; a lattice of more than ``lattice_cap``
    rows or a file beyond its share of ``capacity_per_frame`` bytes per frame of the batch sends that frame to the host formatter) or
    "host" (the raw clouds, boxes and records travel and sd_scene_format_host makes the same bytes on the writer threads)."""
    route: str = "device"
    files: tuple = ("scene", "road", "fence")
    lattice_cap: int = 1 << 18
    capacity_per_frame: int = 24 << 20

    def __post_init__(self):
        object.__setattr__(self, "files", tuple(self.files))
        object.__setattr__(self, "lattice_cap", int(self.lattice_cap))
        object.__setattr__(self, "capacity_per_frame", int(self.capacity_per_frame))
        if self.route not in ("device", "host"):
            raise ValueError(f"Scene: route must be 'device' or 'host', got {self.route!r}")
        if not self.files or len(set(self.files)) != len(self.files) or any(f not in SCENE_FILES for f in self.files):
            raise ValueError(f"Scene: files must be distinct names among {tuple(SCENE_FILES)}, got {self.files!r}")
        if not 0 <= self.lattice_cap < 1 << 29 or self.capacity_per_frame < 0:
            raise ValueError("Scene: lattice_cap must be 0 .. 2^29 - 1 and capacity_per_frame >= 0")


def _check_scene(scene):
    if scene is not None and not isinstance(scene, Scene):
        raise ValueError(f"scene must be None or an outputs.Scene, got {scene!r}")
    return scene


def _scene_lattice(box, plane, axis: int, color):
    """pcl.plane_grid over a cloud that has the box's bounds; (None, None) when the box is empty (n == 0), the lattice has no point or
    np.arange refuses the bounds (a NaN)"""
    if box is None or int(box["n"]) == 0:
        return None, None
    ia, ib = [(1, 2), (0, 2), (0, 1)][axis]
    corners = np.zeros((2, 3), np.float32)
    corners[:, ia], corners[:, ib] = (box["lo_a"], box["hi_a"]), (box["lo_b"], box["hi_b"])
    try:
        pts, col = pcl.plane_grid(corners, dict(Cx=plane[0], Cy=plane[1], Cz=plane[2], C=plane[3]), axis, list(color))
    except ValueError:
        return None, None
    return (pts, col) if len(pts) else (None, None)


def scene_ply_bytes(road3D, road_colors, record, fence: dict | None = None, f2f=None, road_box=None, fence_boxes=None, mask: int = 255) -> bytes:
    """the bytes of a scene file in plain numpy -- what sd_scene_format / sd_scene_format_host write, and what a frame they flag 1 is
    written through: the segments ``mask`` selects (SCENE_FILES) in the order of semantic_depth.py:418-431, appended with np.append,
    behind prepare_and_save_point_cloud's minimum-z filter, rows from sd_ply_format_rows.
    ``road3D`` / ``road_colors``: the final road cloud; ``record``: its RW_DTYPE record; ``fence``: dict(left_xyz, left_rgb, right_xyz,
    right_rgb) of the denoised fence clouds (already cut to their sizes) and ``f2f`` their F2F_DTYPE record, or None; ``road_box`` /
    ``fence_boxes`` ([2]): the BOX_DTYPE boxes the lattices (pcl.plane_grid) are laid over, or None."""
    from .point_cloud_2_ply import format_rows
    parts = []
    if mask & 1:
        parts.append((np.asarray(road3D, np.float64).reshape(-1, 3), np.asarray(road_colors).reshape(-1, 3)))
    if mask & 2:
        parts.append(_scene_lattice(road_box, record["plane"], 1, (200, 200, 200)))
    if mask & 4 and record["found"]:
        parts.append(pcl.create_3Dline_from_3Dpoints(record["left_pt"].astype(np.float64)[None, :], record["right_pt"].astype(np.float64)[None, :],
                                                     [250, 0, 0]))
    if f2f is not None:
        for bit, side in ((8, "left"), (16, "right")):
            if mask & bit and fence is not None:
                parts.append((np.asarray(fence[side + "_xyz"], np.float64).reshape(-1, 3), np.asarray(fence[side + "_rgb"]).reshape(-1, 3)))
        for bit, k, side in ((32, 0, "plane_left"), (64, 1, "plane_right")):
            if mask & bit and fence_boxes is not None:
                parts.append(_scene_lattice(fence_boxes[k], f2f[side], 0, (40, 70, 40)))
        if mask & 128 and f2f["ok"]:
            parts.append(pcl.create_3Dline_from_3Dpoints(np.array(f2f["left_pt"], np.float64)[None, :], np.array(f2f["right_pt"], np.float64)[None, :],
                                                         [0, 255, 0]))
    pts, col = np.zeros((0, 3), np.float64), np.zeros((0, 3), np.float64)
    for p, c in parts:
        if p is not None:
            pts, col = np.append(pts, p, axis=0), np.append(col, c, axis=0)
    if len(pts):
        keep = pts[:, 2] > pts[:, 2].min()
        pts, col = pts[keep], col[keep]
    return PointCloud2Ply.ply_header.format(vertex_count=len(pts)).encode() + format_rows(pts, col, threads=1)


def scene_format_host(road3D, road_colors, record, fence: dict | None = None, f2f=None, road_box=None, fence_boxes=None, mask: int = 255,
                      lattice_cap: int = 0):
    """sd_scene_format_host on one frame (the arguments of scene_ply_bytes; float32 clouds, u8 colours) -> (bytes, flag): the file and 0,
    or b"" and flag 1 (a coordinate the integer coder does not take: write the frame through scene_ply_bytes) or 3 (a lattice above
    ``lattice_cap``; 0: no cap)."""
    import ctypes as C

    from . import _lib as L
    from .engine import BOX_DTYPE, F2F_DTYPE, RW_DTYPE
    lib = L.load()
    keep = []                                               # (the arrays the pointers below point into)

    def arr(a, dt, shape=None):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=dt)
        keep.append(a if shape is None else a.reshape(shape))
        return keep[-1].ctypes.data_as(C.c_void_p)

    xyz = np.ascontiguousarray(road3D, np.float32).reshape(-1, 3)
    n = len(xyz)
    rec = np.ascontiguousarray(np.asarray(record, RW_DTYPE).reshape(1))
    f2 = None if f2f is None else np.ascontiguousarray(np.asarray(f2f, F2F_DTYPE).reshape(1))
    ptr = [arr(xyz, np.float32), arr(np.asarray(road_colors).reshape(-1, 3), np.uint8)]
    rows = n + 2 * L.SD_PLY_LINE_ROWS
    for side, j in (("left", 5), ("right", 6)):
        given = fence is not None and f2 is not None
        if given and len(np.asarray(fence[side + "_xyz"]).reshape(-1, 3)) < int(f2["counts"][0][j]):
            raise ValueError(f"scene_format_host: the {side} fence cloud is shorter than its record says")
        ptr += [arr(fence[side + "_xyz"], np.float32), arr(fence[side + "_rgb"], np.uint8)] if given else [None, None]
        rows += int(f2["counts"][0][j]) if given else 0
    rb = None if road_box is None else np.ascontiguousarray(np.asarray(road_box, BOX_DTYPE).reshape(1))
    fb = None if fence_boxes is None else np.ascontiguousarray(np.asarray(fence_boxes, BOX_DTYPE).reshape(2))
    na, nb = C.c_uint32(), C.c_uint32()
    for box, plane, axis in ([(rb, rec["plane"][0], 1)] if rb is not None else []) + \
                            ([(fb[k:k + 1], f2[side][0], 0) for k, side in enumerate(("plane_left", "plane_right"))] if fb is not None and f2 is not None else []):
        if int(box["n"][0]) and lib.sd_scene_lattice_host(box.ctypes.data_as(C.c_void_p), np.ascontiguousarray(plane, np.float64).ctypes.data_as(C.c_void_p),
                                                          axis, C.byref(na), C.byref(nb), None, 0) == L.SD_OK:
            rows += na.value * nb.value                     # (a box the rule refuses: the call below flags the frame)
    out = np.empty(L.SD_PLY_HEADER_CAP + max(rows, 0) * L.SD_PLY_ROW_CAP, np.uint8)
    size, flag = C.c_size_t(), C.c_int32()
    st = lib.sd_scene_format_host(ptr[0], ptr[1], n, ptr[2], ptr[3], ptr[4], ptr[5], rec.ctypes.data_as(C.c_void_p),
                                  None if f2 is None else f2.ctypes.data_as(C.c_void_p), None if rb is None else rb.ctypes.data_as(C.c_void_p),
                                  None if fb is None else fb.ctypes.data_as(C.c_void_p), int(mask), int(lattice_cap), out.ctypes.data_as(C.c_void_p),
                                  out.size, C.byref(size), C.byref(flag))
    if st != L.SD_OK or flag.value == 2:
        raise RuntimeError(f"sd_scene_format_host failed (status {st}, flag {flag.value})")
    return out[:size.value].tobytes(), int(flag.value)


@dataclasses.dataclass(frozen=True)
class _PngFamily:
    """one family of per-frame PNG files of SequenceOutputs; all of them go through the PNG route chosen (``png``, described there)"""
    key: str                                # what a batch's payload of the family is filed under
    subdir: str                             # the files are <directory>/<subdir>/<name><suffix>
    suffix: str
    size: str                               # (h, w) of the images: "frame" (the original frames') or "camera" (the RenderCamera's)
    manifest_key: str | None                # the manifest lists the files under it (None: only under 'files')
    early_dir: bool                         # the directory is made by the constructor (else by every batch that writes into it)


_PNG_FAMILIES = (_PngFamily("images", SEQ_IMG_DIR, ".png", "frame", None, True),
                 _PngFamily("render", SEQ_RENDER_DIR, "_render.png", "camera", "render", False),
                 _PngFamily("disp", SEQ_DISP_DIR, "_disp.png", "frame", "disp", False))


@dataclasses.dataclass
class _Batch:
    """one batch as submit() accepted it: device or host tensors, the payloads of the routes that are off already None"""
    slot: int                               # which of the two in-flight slots (stager, pinned buffers) it travels through
    k: int                                  # batch index: its turn in the video
    lo: int
    size: tuple
    ev: object                              # an event of the producing stream, None for a host batch
    records: object
    png: dict                               # family key -> the raw images u8 [n,h,w,3] or (streams, sizes), for the families that are on
    images: object = None                   # the raw result images with video=: its frames (route "host") / the source of a flagged one
    final: object = None
    ply_text: object = None
    video_streams: object = None
    profile: object = None
    f2f_profile: object = None
    disp_flags: object = None
    lines_flags: object = None
    f2f: object = None
    cams: object = None                     # the frames' cameras and the network size (host values): the writer restates the lines from them
    net_size: object = None
    scene: object = None                    # with scene=: dict(fence_final, f2f, boxes, text) as submit() describes it


@dataclasses.dataclass
class _HostBatch:
    """numpy views of a _Batch on the host (pinned staging or the host tensors themselves), valid until its slot's next batch"""
    records: np.ndarray
    png: dict = dataclasses.field(default_factory=dict)            # family key -> (raw images [n,h,w,3], None) or ([n,stride] zlib
    #                                                                streams of which [i, :sizes[i]] was copied, sizes)
    clouds: list | None = None              # per frame (xyz, rgb), None for a frame whose text the device formatted
    ply_text: np.ndarray | None = None      # frame i's file is ply_text[ply_offsets[i]:ply_offsets[i + 1]] where ply_flags[i] == 0
    ply_offsets: np.ndarray | None = None
    ply_flags: np.ndarray | None = None
    video: np.ndarray | None = None         # [n,stride] JPEG files, video[i, :video_sizes[i]] copied where video_flags[i] == 0
    video_sizes: np.ndarray | None = None
    video_flags: np.ndarray | None = None
    video_raw: dict = dataclasses.field(default_factory=dict)      # frame -> raw image of a flagged video frame
    profile: np.ndarray | None = None       # [n,D,48] depth-profile records
    f2f_profile: np.ndarray | None = None   # [n,D,64]
    disp_flags: np.ndarray | None = None    # [n] non-zero: the frame's map held a non-finite value
    lines_flags: np.ndarray | None = None   # [n] bit 0: a measurement line of the frame was skipped
    f2f: np.ndarray | None = None           # [n,152] fence records, for the lines of approach 'both'
    scene: dict | None = None               # with scene=: f2f [n,152] / None, road_box [n,24], fence_box [n,2,24] / None, fence: per frame the
    #                                         four raw fence arrays or None, text: {file: (text, offsets, flags)} on the device route


class _Stager:
    """the device-to-host transfer of one in-flight slot of SequenceOutputs: pinned buffers that only grow, a side stream, and the wait for
    the batch's event.  Inside ``with stager.behind(ev):`` every method returns a numpy view: of a pinned copy enqueued on the side stream
    (valid after the next ``sync()``) for a device tensor, of the input itself, without a copy, for a host tensor, a numpy array or a host
    batch (``ev`` None)."""

    def __init__(self):
        self._buffers, self._stream, self._ev = {}, None, None

    def event(self, t):
        """an event on the current stream of ``t``'s device for behind() to wait for; None when ``t`` is on the host"""
        import torch
        if not t.is_cuda:
            return None
        if self._stream is None:
            self._stream = torch.cuda.Stream(t.device)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(t.device))
        return ev

    @contextlib.contextmanager
    def behind(self, ev):
        import torch
        self._ev = ev
        if ev is None:
            yield
            return
        with torch.cuda.stream(self._stream):
            self._stream.wait_event(ev)
            yield

    def sync(self):
        if self._ev is not None:
            self._stream.synchronize()

    def _pinned(self, key: str, shape, dtype):
        import torch
        buf = self._buffers.get(key)
        numel = int(np.prod(shape))
        if buf is None or buf.numel() < numel or buf.dtype != dtype:
            buf = self._buffers[key] = torch.empty(max(numel, 1), dtype=dtype, pin_memory=True)
        return buf[:numel].view(*shape)

    def _on_host(self, t):
        import torch
        if self._ev is not None and isinstance(t, torch.Tensor) and t.is_cuda:
            return None
        return np.asarray(t.cpu() if isinstance(t, torch.Tensor) else t)

    def fixed(self, key: str, t):
        """a tensor whose shape is known (None stays None)"""
        if t is None:
            return None
        a = self._on_host(t)
        if a is None:
            buf = self._pinned(key, tuple(t.shape), t.dtype)
            buf.copy_(t, non_blocking=True)
            a = buf.numpy()
        return a

    def rows(self, key: str, src, sizes):
        """``src`` [n,stride] of which only src[i, :sizes[i]] is meaningful (``sizes``: on the host) -> an [n,stride] view; only those bytes
        are copied, a row of size 0 not at all"""
        a = self._on_host(src)
        if a is None:
            buf = self._pinned(key, tuple(src.shape), src.dtype)
            for i, size in enumerate(sizes):
                if size:
                    buf[i, :int(size)].copy_(src[i, :int(size)], non_blocking=True)
            a = buf.numpy()
        return a

    def ragged(self, key: str, src, counts):
        """``src`` [n,cap,...] -> the list of src[i, :counts[i]] (``counts``: on the host); device rows are packed back to back into one
        pinned buffer of sum(counts) rows, a row of count 0 is not copied"""
        a = self._on_host(src)
        if a is not None:
            return [a[i, :c] for i, c in enumerate(counts)]
        off = np.concatenate([[0], np.cumsum(counts)])
        buf = self._pinned(key, (int(off[-1]),) + tuple(src.shape[2:]), src.dtype)
        for i, c in enumerate(counts):
            if c:
                buf[off[i]:off[i + 1]].copy_(src[i, :c], non_blocking=True)
        a = buf.numpy()
        return [a[off[i]:off[i + 1]] for i in range(len(counts))]


class SequenceOutputs:
    """what the sequence tool writes for every frame (seq:303-361), fed batch by batch by the step of ``make_engine_step(..., outputs=)``:

        <directory>/result_sequence_imgs/<name>.png           the overlay at the original frame size, 25 % banner when the line was found
                                                              (``images``; Engine.compose_result_frames on the GPU)
        <directory>/result_sequence_imgs/<name>_overlay.json  the banner and the cv2.putText items of overlay_items_sequence (``items``)
        <directory>/result_sequence_ply/<name>_rw.ply         the denoised road cloud + the red road-width line (``ply``; rw_ply_bytes)
        <directory>/result_sequence_ply/<name>_scene.ply      only with scene=: the frame's 3D scene; beside it <name>_ROAD.ply and, with approach
                                                              'both', <name>_FENCE.ply (``scene``; scene_ply_bytes)
        <directory>/rendered_sequence/<name>_render.png       only with render=: the top view of the _rw.ply's rows (``render``)
        <directory>/result_imgs.avi                           only with video=: the result images as a Motion-JPEG AVI (``video``;
                                                              result_imgs_rank<r>.avi when world > 1, _part<k> when a file rolls over)
        <directory>/result_sequence_profile/<name>.txt        only with profile=: the frame's depth profile (``profile``; profile_text)
        <directory>/result_sequence_disp/<name>_disp.png      only with disp=: the frame's disparity image (``disp``; disparity_image)
        <directory>/manifest_rank<r>.json                     written last by close(): the files of this rank and 'ok' / 'range_error' / 'error'

    ``names``: output names of the WHOLE sorted frame list (sequence_names), indexed by global frame index.  submit() takes the device
    tensors of one batch, copies them into pinned staging on a side stream behind an event of the current stream, and writes them on
    worker threads -- at most two batches in flight -- with the per-pixel and per-point work in native code (no interpreter lock).  The
    transfer has two phases (_fetch): first everything whose shape is known -- the records, whole images, and every count, size, offset
    and flag -- then exactly the bytes those call for.
    ``threads``: native encoder threads per batch and PLY writer threads (0: frame_io.default_decode_workers()).
    The choices that follow can also be made after construction and before the first batch, by configure() (all at once; what
    make_engine_step and run_sequence_files do with their keywords of the same names) or by set_png / set_ply / set_text / set_render /
    set_video / set_disp / set_lines / set_profile.  All but png="host", ply="host", text="json" and Video(route="host") need the step of
    make_engine_step, which does the GPU half (its docstring: what it launches for each, in which order); submit()'s docstring names the
    keyword each payload arrives under.  Every choice that defaults to None then writes, copies and launches nothing more, changes no byte
    of any file and leaves the manifest what it was.
    ``png``: the route of every family of per-frame PNG files (_PNG_FAMILIES: the result images, the renders, the disparity images).
    "host" (default): the raw images are copied to the host and deflated there (sd_png_encode_bgr_files at ``level``); "device": each
    frame's finished zlib stream comes from the GPU (Engine.encode_png): the sizes are copied first, then each stream's exact byte
    count, and the host only writes the PNG chunks (sd_png_write_streams_files).  Same names, manifest and pixels.
    ``ply``: False (no PLY files), True / "host" (default: the raw clouds are copied to the host and formatted there, rw_ply_bytes) or "device":
    the finished text of every file comes from the GPU (Engine.format_rw_ply); the offsets and flags are copied first, then
    text[:offsets[n]] in one copy, and the host only writes each slice.  A frame the device did not format (a non-zero flag: a non-finite
    coordinate or |v| >= 2^31) has its raw cloud copied and goes through rw_ply_bytes; the manifest names those frames under 'ply_fallback'.
    Same names and the same bytes.  (Whether PLYs are written at all stays what the constructor was given, ``self.ply``; the route is
    ``self.ply_route``.)
    ``text``: "json" (default: the banner of the images stays empty, the text is in the ``_overlay.json`` files) or "draw": it is also
    rasterised into the composed images on the GPU (Engine.draw_result_text) before they reach either PNG route or the video.
    ``render``: None or a RenderCamera: every frame's final road cloud and road-width line are drawn behind that camera on the GPU
    (Engine.render_rw); the manifest names the ``<name>_render.png`` files under 'render'.
    ``video``: None or a Video: the composed result images -- the very images of the PNGs, lines and banner text included -- also become
    the frames of ``result_imgs.avi``, in global frame order although two batches are in flight (the appends are serialised by batch
    index); the manifest names the files under 'video'.  route "device": the finished JPEG files come from the GPU (Engine.encode_jpeg);
    sizes and flags are copied first, then each file's exact bytes; a flagged frame (its file passed the stream stride) is encoded on the
    host from a raw copy of that frame and named under 'video_fallback'.  route "host": the raw images travel whole and
    sd_jpeg_encode_bgr_host makes the same bytes on the writer threads; it needs png="host".  Works with images=False too (submit still
    gets the images then).
    ``profile``: None or the list of depths of a depth profile (Engine.process_batch(depths=)): the [n,D,48] / [n,D,64] record tensors
    travel with the batch's other small records in the first phase.  The manifest names the depths under 'profile_depths' and the files
    under 'profile'.
    ``disp``: None, "gray" or "plasma": every frame's post-processed disparity map becomes the image of DepthFrame.disp_to_image
    (semantic_depth.py:681-683) at the original frame size on the GPU (Engine.disparity_image).  The manifest names the files under
    'disp' and the frames whose map held a non-finite value (it became byte 0) under 'disp_nonfinite'.  Works with images=False too.
    ``lines``: None or an OverlayLines: the measured road-width line -- with approach 'both' the fence-to-fence line, with profile= the
    road's two edges and a rung per depth -- is drawn into the composed images on the GPU (Engine.draw_result_lines, below the banner
    rows: clip_top = int(0.25 h)), so the PNGs of both routes and the video show them.  The writer restates the segments
    (overlay_segments) from the frames' cameras and records: each ``_overlay.json`` gains "lines", the manifest 'lines' (the style) and
    'lines_flagged' (the frames of which a segment was skipped because an end point does not project).
    ``scene``: None or a Scene: every frame's 3D products (semantic_depth.py:404-431) as ``<name>_scene.ply``, ``<name>_ROAD.ply`` and, with
    approach 'both', ``<name>_FENCE.ply`` in ``result_sequence_ply`` (Scene's docstring).  The step keeps the final road and fence clouds
    and the boxes of the three plane fits (process_batch(want_final=True, want_boxes=True)).  route "device": the finished text of every
    file comes from the GPU (Engine.format_scene_ply); offsets and flags are copied first, then each file's text[:offsets[n]] in one
    copy; a flagged frame has its raw clouds copied and goes through sd_scene_format_host (flags 2 and 3: the capacity, a lattice above
    lattice_cap) or scene_ply_bytes (flag 1: a coordinate the integer coder does not take).  route "host": the raw clouds, boxes and
    records travel and sd_scene_format_host makes the same bytes on the writer threads.  The manifest names the files under 'scene' and
    the frames of which the device left a file to the host under 'scene_fallback'."""

    png, ply_route, text, render, video, disp, lines, scene, _k = "host", "host", "json", None, None, None, None, None, 0    # (what configure() starts from)

    def __init__(self, directory: str, names, depth: float = 10.0, images: bool = True, ply: bool | str = True, items: bool = True, level: int = 1,
                 threads: int = 0, road_color=(128, 64, 128), fence_color=(190, 153, 153), alpha: int = 64, png: str = "host", text: str = "json",
                 render: RenderCamera | None = None, video: Video | None = None, profile=None, disp: str | None = None,
                 lines: OverlayLines | None = None, scene: Scene | None = None):
        import threading
        from concurrent.futures import ThreadPoolExecutor

        from .frame_io import default_decode_workers
        if not 0 <= level <= 9:
            raise ValueError("PNG compression level must be 0..9")
        if png is None or ply is None or text is None:                # (None leaves a choice as it is only in configure)
            raise ValueError(f"png, ply and text must be given, got {png!r}, {ply!r}, {text!r}")
        self.configure(png, "host" if isinstance(ply, bool) else ply, text, render, video, disp, lines, scene)
        self.directory, self.names, self.depth = directory, list(names), float(depth)
        self.images, self.ply, self.items, self.level = bool(images), bool(ply), bool(items), int(level)
        self.road_color, self.fence_color, self.alpha = tuple(road_color), tuple(fence_color), int(alpha)
        self.threads = threads if threads > 0 else default_decode_workers()
        self.img_dir, self.ply_dir = os.path.join(directory, SEQ_IMG_DIR), os.path.join(directory, SEQ_PLY_DIR)
        self.profile_dir = os.path.join(directory, SEQ_PROFILE_DIR)
        self.profile = None
        self.set_profile(profile)
        for d in [self._dir(f) for f in self._families if f.early_dir] + [self.img_dir] * self.items + [self.ply_dir] * self.ply:
            os.makedirs(d, exist_ok=True)
        self.rank, self.world, self.shard = 0, 1, (0, len(self.names))
        self._batches = ThreadPoolExecutor(max_workers=2)           # one per batch in flight
        self._writers = ThreadPoolExecutor(max_workers=self.threads)  # PLY / JSON files of a batch
        self._jobs, self._files = [], []
        self._stagers = [_Stager(), _Stager()]                       # one per in-flight slot
        self.manifest = None
        # manifest key -> global indices of the frames that took the other path: recomputed on bf16x3 (on_range='recompute'), sent through
        # rw_ply_bytes by ply="device", encoded on the host by video route "device", a non-finite value in the disparity map, a segment
        # skipped by lines=
        self._frames = {key: [] for key in ("recomputed", "ply_fallback", "video_fallback", "disp_nonfinite", "lines_flagged", "scene_fallback")}
        self._scene_files = []                                       # the scene=  files written (they share result_sequence_ply with the _rw.ply)
        self._video_writer, self._video_next, self._video_turn = None, 0, threading.Condition()

    # ---------------------------------------------------------------- driver interface
    def configure(self, png: str | None = None, ply: str | None = None, text: str | None = None, render=None, video=None, disp: str | None = None,
                  lines=None, scene=None):
        """choose the routes described in the class docstring, before the first batch: ``png`` and ``ply`` "host" or "device", ``text`` "json"
        or "draw", ``render`` a RenderCamera, ``video`` a Video, ``disp`` "gray" or "plasma", ``lines`` an OverlayLines, ``scene`` a Scene; None
        leaves a choice as it is.  Nothing changes when the resulting combination is refused."""
        new = dict(png=png, ply_route=ply, text=text, render=render, video=video, disp=disp, lines=lines, scene=scene)
        new = {name: getattr(self, name) if v is None else v for name, v in new.items()}
        if new["png"] not in ("host", "device"):
            raise ValueError(f"png must be 'host' or 'device', got {new['png']!r}")
        if new["ply_route"] not in ("host", "device") or isinstance(new["ply_route"], bool):
            raise ValueError(f"ply must be 'host' or 'device', got {new['ply_route']!r}")
        for check, name in ((_check_text, "text"), (_check_render, "render"), (_check_video, "video"), (_check_disp, "disp"), (_check_lines, "lines"),
                            (_check_scene, "scene")):
            check(new[name])
        if self._k:
            raise RuntimeError("SequenceOutputs.configure after the first batch")
        if new["png"] == "device" and new["video"] is not None and new["video"].route == "host":
            raise ValueError("Video(route='host') needs png='host': with png='device' no raw image reaches the host")
        vars(self).update(new)

    def set_lines(self, lines):
        """the OverlayLines the measurement lines are drawn with (before the first batch)"""
        self.configure(lines=lines)

    def set_png(self, png: str):
        """where the result images are compressed: "host" or "device" (before the first batch)"""
        self.configure(png=png)

    def set_ply(self, ply: str):
        """where the road PLYs are formatted: "host" or "device" (before the first batch)"""
        self.configure(ply=ply)

    def set_text(self, text: str):
        """whether the banner text is drawn into the result images: "json" or "draw" (before the first batch)"""
        self.configure(text=text)

    def set_render(self, render):
        """the RenderCamera the road clouds are rendered from (before the first batch)"""
        self.configure(render=render)

    def set_video(self, video):
        """the Video the result images also become (before the first batch)"""
        self.configure(video=video)

    def set_scene(self, scene):
        """the Scene whose PLY files are written for every frame (before the first batch)"""
        self.configure(scene=scene)

    def set_disp(self, disp: str):
        """the colour map of the per-frame disparity images: "gray" or "plasma" (before the first batch)"""
        self.configure(disp=disp)

    def set_profile(self, depths):
        """the depths of the per-frame depth profile, or None for no profile (before the first batch)"""
        if self._k:
            raise RuntimeError("SequenceOutputs.set_profile after the first batch")
        if depths is not None:
            depths = [float(d) for d in np.asarray(depths, dtype=np.float64).reshape(-1)]
            if not depths or not all(np.isfinite(depths)):
                raise ValueError("profile must be a non-empty list of finite depths")
        self.profile = depths

    def begin(self, rank: int, world: int, lo: int, hi: int):
        """the shard [lo, hi) this rank writes (run_sequence_files calls it before the first batch)"""
        self.rank, self.world, self.shard = int(rank), int(world), (int(lo), int(hi))

    # ---------------------------------------------------------------- the routes, each condition stated once
    @property
    def device_png(self) -> bool:
        """the PNG families arrive as zlib streams (png="device")"""
        return self.png == "device"

    @property
    def device_ply(self) -> bool:
        """PLYs are written and arrive as text (ply="device")"""
        return self.ply and self.ply_route == "device"

    @property
    def device_video(self) -> bool:
        """a video is written and its frames arrive as JPEG files (route "device")"""
        return self.video is not None and self.video.route == "device"

    @property
    def wants_final(self) -> bool:
        """the step has to keep the final road clouds: for the PLYs, the renders or the scene files"""
        return self.ply or self.render is not None or self.scene is not None

    @property
    def device_scene(self) -> bool:
        """scene files are written and arrive as text (route "device")"""
        return self.scene is not None and self.scene.route == "device"

    @property
    def wants_composed(self) -> bool:
        """the step has to compose the result images: for their PNGs or the video"""
        return self.images or self.video is not None

    @property
    def _images_travel(self) -> bool:
        """whether the raw result images cross to the host whole: for the host PNG route or the host video route"""
        return not self.device_png and (self.images or self.video is not None and not self.device_video)

    @property
    def _families(self) -> tuple:
        """the PNG families that are on"""
        on = dict(images=self.images, render=self.render is not None, disp=self.disp is not None)
        return tuple(f for f in _PNG_FAMILIES if on[f.key])

    def _dir(self, family: _PngFamily) -> str:
        return os.path.join(self.directory, family.subdir)

    def submit(self, lo: int, records, size: tuple, images=None, final=None, png_streams=None, ply_text=None, renders=None, render_streams=None,
               video_streams=None, profile=None, f2f_profile=None, disp_images=None, disp_streams=None, disp_flags=None, lines_flags=None,
               f2f=None, cams=None, net_size=None, scene=None):
        """one batch: ``records`` u8 [n,104] (sd_rw_result) and ``size`` = (h, w) of the original frames, then what the choices of the class
        docstring call for (anything else is ignored).  Device or host tensors; the device ones must stay unmodified until the batch is
        written (they are new tensors of every step).
        The PNG families, each as raw images u8 [n,h,w,3] with png="host" or as (streams u8 [n,stride], sizes i64 [n]) of Engine.encode_png
        with png="device":
            result images (``images``)      ``images`` (Engine.compose_result_frames)   | ``png_streams``
            renders (render=)               ``renders`` (Engine.render_rw)              | ``render_streams``
            disparity images (disp=)        ``disp_images`` (Engine.disparity_image)    | ``disp_streams``
        ``images`` is also needed raw, on either PNG route and with images=False, by video=: as the frames on its "host" route, beside
        ``video_streams`` = (streams u8 [n,stride], sizes i64 [n], flags i32 [n]) of Engine.encode_jpeg on its "device" route, where a flagged
        frame is encoded from it.
        ``final`` = dict(xyz f32 [n,cap,3], rgb u8 [n,cap,3], n i32 [n]) (process_batch(want_final=True)'s road_final) with ``ply``, and
        beside it on the ply="device" route (the flagged frames are written from it) ``ply_text`` = (text u8 [capacity], offsets i64 [n+1],
        flags i32 [n]) of Engine.format_rw_ply.
        ``profile`` = u8 [n,D,48] of Engine.road_width_profile (process_batch(depths=)'s ``profile``) with profile=, ``f2f_profile`` = u8
        [n,D,64] beside it (optional: the dist_f2f column).
        ``disp_flags`` = the i32 [n] flags of Engine.disparity_image with disp= (optional: the manifest's 'disp_nonfinite').
        With lines=: ``cams`` = the n frames' Camera and ``net_size`` = (h, w) of the network they belong to (host values), ``f2f`` = u8
        [n,152] fence records (optional: the fence lines) and ``lines_flags`` = i32 [n] of Engine.draw_result_lines (optional: without them
        the writer's own restatement flags the frames).
        With scene=: ``final`` as above and ``scene`` = dict(fence_final = process_batch(want_final=True)'s fence_final or None (approach
        'rw'), f2f = u8 [n,152] or None, boxes = process_batch(want_boxes=True)'s plane_boxes, text = None on the "host" route, on the
        "device" route {file: (text, offsets, flags) of Engine.format_scene_ply with that file's mask} for the files of Scene.files)."""
        if self.manifest is not None:
            raise RuntimeError("SequenceOutputs.submit after close")
        n = int(records.shape[0])
        # family key -> its payload: of its two keywords (raw images, zlib streams) the one the PNG route calls for
        payload = dict(images=(images, png_streams), render=(renders, render_streams), disp=(disp_images, disp_streams))
        payload = {key: pair[self.device_png] for key, pair in payload.items()}
        if lo < 0 or lo + n > len(self.names):
            raise ValueError(f"frames {lo}..{lo + n - 1} are beyond the {len(self.names)} names")
        lacking = (
            (self.images and payload["images"] is None or (self.ply or self.scene is not None) and final is None,
             "this batch lacks the images (png='device': the streams) / final road clouds the outputs ask for"),
            (self.device_ply and ply_text is None, "ply='device' needs the text of Engine.format_rw_ply (submit(ply_text=))"),
            (self.render is not None and payload["render"] is None,
             "render= needs the images of Engine.render_rw (submit(renders=); png='device': render_streams=)"),
            (self.device_video and video_streams is None, "video route 'device' needs the files of Engine.encode_jpeg (submit(video_streams=))"),
            (self.video is not None and not self.device_video and images is None, "video route 'host' needs the raw images (submit(images=))"),
            (self.profile is not None and (profile is None or tuple(profile.shape[:2]) != (n, len(self.profile))),
             "profile= needs the [n, D, 48] records of Engine.road_width_profile (submit(profile=))"),
            (_check_disp(self.disp) is not None and payload["disp"] is None,
             "disp= needs the images of Engine.disparity_image (submit(disp_images=); png='device': disp_streams=)"),
            (self.lines is not None and (cams is None or net_size is None or len(cams) != n),
             "lines= needs the frames' cameras and the network size (submit(cams=, net_size=))"),
            (self.scene is not None and (scene is None or scene.get("boxes") is None or self.device_scene and not scene.get("text")),
             "scene= needs the boxes of process_batch(want_boxes=True) and, on the device route, the text of Engine.format_scene_ply "
             "(submit(scene=))"))
        for lacks, what in lacking:
            if lacks:
                raise ValueError("SequenceOutputs: " + what)
        while len(self._jobs) >= 2:                                    # at most two batches in flight
            self._files.extend(self._jobs.pop(0).result())
        slot = self._k & 1
        batch = _Batch(slot, self._k, lo, tuple(size), self._stagers[slot].event(records), records,
                       png={f.key: payload[f.key] for f in self._families},
                       images=images if self.video is not None else None,
                       final=final,
                       ply_text=ply_text if self.device_ply else None,
                       video_streams=video_streams if self.device_video else None,
                       profile=profile if self.profile is not None else None,
                       f2f_profile=f2f_profile if self.profile is not None else None,
                       disp_flags=disp_flags if self.disp is not None else None,
                       scene=scene if self.scene is not None else None)
        if self.lines is not None:
            batch.lines_flags, batch.f2f, batch.cams, batch.net_size = lines_flags, f2f, list(cams), tuple(net_size)
        self._k += 1
        self._jobs.append(self._batches.submit(self._write_batch, batch))

    def mark_recomputed(self, frames):
        """global frame indices whose outputs came from the bf16x3 recompute (make_engine_step(on_range='recompute')): the manifest lists
        their names under 'recomputed'"""
        self._frames["recomputed"].extend(int(i) for i in frames)

    def _flag(self, key: str, lo: int, flags):
        """the frames lo + i whose flags[i] is non-zero join the manifest's list ``key`` (None: the batch carries no such flags)"""
        if flags is not None:
            self._frames[key].extend(lo + int(i) for i in np.flatnonzero(flags))

    def close(self, status: str = "ok") -> str:
        """wait for every batch, then write this rank's manifest LAST: the files written and ``status`` ('ok'; 'range_error' / 'error':
        the run failed and the files listed are not valid outputs).  Returns the manifest path."""
        if self.manifest is not None:
            return self.manifest
        err = None
        for f in self._jobs:
            try:
                self._files.extend(f.result())
            except Exception as e:                                    # (a failed write is reported after the manifest says so)
                err = err or e
        self._jobs = []
        self._batches.shutdown()
        self._writers.shutdown()
        video_files = []
        if self._video_writer is not None:
            video_files = self._video_writer.close()
            self._files.extend(video_files)
        if err is not None and status == "ok":
            status = "error"
        self.manifest = os.path.join(self.directory, "manifest_rank{}.json".format(self.rank))
        files = sorted(os.path.relpath(p, self.directory) for p in self._files)

        def below(subdir):
            return [f for f in files if f.startswith(subdir + os.sep)]

        value = {key: [self.names[i] for i in sorted(set(frames))] for key, frames in self._frames.items()}
        value.update({f.manifest_key: below(f.subdir) for f in self._families if f.manifest_key})
        value.update(video=[os.path.relpath(p, self.directory) for p in video_files], profile_depths=self.profile, profile=below(SEQ_PROFILE_DIR),
                     lines=None if self.lines is None else self.lines.as_dict(),
                     scene=sorted(os.path.relpath(p, self.directory) for p in self._scene_files))
        manifest = dict(rank=self.rank, world=self.world, frames=list(self.shard), status=status, valid=status == "ok", files=files,
                        recomputed=value["recomputed"])
        # (the choice, the keys it adds when it is on), in the manifest's order
        for choice, keys in ((self.device_ply or None, ("ply_fallback",)), (self.render, ("render",)), (self.video, ("video", "video_fallback")),
                             (self.profile, ("profile_depths", "profile")), (self.disp, ("disp", "disp_nonfinite")),
                             (self.lines, ("lines", "lines_flagged")), (self.scene, ("scene", "scene_fallback"))):
            if choice is not None:
                manifest.update((key, value[key]) for key in keys)
        with open(self.manifest, "w") as f:
            json.dump(manifest, f, indent=1)
        if err is not None:
            raise err
        return self.manifest

    # ---------------------------------------------------------------- worker side
    def _fetch(self, b: _Batch) -> _HostBatch:
        """the batch on the host, through its slot's stager, in the two phases of the class docstring: two synchronisations per batch,
        however many families are on"""
        st = self._stagers[b.slot]
        with st.behind(b.ev):
            host = _HostBatch(st.fixed("rec", b.records), profile=st.fixed("profile", b.profile), f2f_profile=st.fixed("f2f_profile", b.f2f_profile),
                              disp_flags=st.fixed("disp_flags", b.disp_flags), lines_flags=st.fixed("lines_flags", b.lines_flags),
                              f2f=st.fixed("f2f", b.f2f))
            for key, p in b.png.items():
                host.png[key] = (None, st.fixed(key + "_sizes", p[1])) if self.device_png else (st.fixed(key, p), None)
            if self._images_travel and "images" not in b.png:         # images=False: the host video route still needs them whole
                host.png["images"] = (st.fixed("images", b.images), None)
            counts = None if b.final is None else st.fixed("n", b.final["n"])
            if b.ply_text is not None:
                host.ply_offsets, host.ply_flags = st.fixed("ply_offsets", b.ply_text[1]), st.fixed("ply_flags", b.ply_text[2])
            if b.video_streams is not None:
                host.video_sizes, host.video_flags = st.fixed("video_sizes", b.video_streams[1]), st.fixed("video_flags", b.video_streams[2])
            if b.scene is not None:                                    # the fence records, the boxes and, on the device route, offsets and flags
                boxes = b.scene["boxes"]
                host.scene = dict(f2f=st.fixed("scene_f2f", b.scene.get("f2f")), road_box=st.fixed("scene_rbox", boxes["road"]),
                                  fence_box=st.fixed("scene_fbox", boxes.get("fence")), fence=None,
                                  text={key: (None, st.fixed("scene_off_" + key, t[1]), st.fixed("scene_flag_" + key, t[2]))
                                        for key, t in (b.scene.get("text") or {}).items()})
            st.sync()
            if self.device_png:
                for key, p in b.png.items():
                    sizes = host.png[key][1]
                    host.png[key] = (st.rows(key + "_png", p[0], sizes), sizes)
            if b.ply_text is not None:
                host.ply_text = st.fixed("ply_text", b.ply_text[0][:int(host.ply_offsets[-1])])
            scene_raw = None
            if b.scene is not None:
                # a frame's raw clouds travel on the host route, and on the device route when one of its files is flagged
                scene_raw = np.ones(len(counts), bool)
                if host.scene["text"]:
                    scene_raw = np.zeros(len(counts), bool)
                    for key, (_, offsets, flags) in host.scene["text"].items():
                        host.scene["text"][key] = (st.fixed("scene_text_" + key, b.scene["text"][key][0][:int(offsets[-1])]), offsets, flags)
                        scene_raw |= flags != 0
                ff = b.scene.get("fence_final")
                if ff is not None and host.scene["f2f"] is not None:
                    from .engine import F2F_DTYPE
                    fc = np.ascontiguousarray(host.scene["f2f"]).view(F2F_DTYPE).reshape(-1)["counts"]
                    side = {k: st.ragged("scene_" + k, ff[k], np.where(scene_raw, np.clip(fc[:, j], 0, ff[k].shape[1]), 0).astype(np.int64))
                            for k, j in (("left_xyz", 5), ("left_rgb", 5), ("right_xyz", 6), ("right_rgb", 6))}
                    host.scene["fence"] = [{k: v[i] for k, v in side.items()} if scene_raw[i] else None for i in range(len(counts))]
            if b.final is not None:
                # which frames' raw road clouds travel: with PLYs on, all of them on the host route and the flagged ones on the device
                # route (as before scene= existed); with PLYs off nothing read them, and now only scene= can ask for them (ply=False
                # with final= given used to copy clouds that no writer looked at).  write_ply decides by the flags, not by this.
                raw = np.zeros(len(counts), bool)
                if self.ply:
                    raw = np.ones(len(counts), bool) if b.ply_text is None else host.ply_flags != 0
                if scene_raw is not None:
                    raw = raw | scene_raw
                cn = np.where(raw, counts, 0).astype(np.int64)
                xyz, rgb = st.ragged("xyz", b.final["xyz"], cn), st.ragged("rgb", b.final["rgb"], cn)
                host.clouds = [(xyz[i], rgb[i]) if raw[i] else None for i in range(len(cn))]
            if b.video_streams is not None:
                host.video = st.rows("video", b.video_streams[0], np.where(host.video_flags != 0, 0, host.video_sizes))
                # a flagged frame is encoded from its raw image: a row of the whole images where they travel, else a copy of that frame alone
                whole = host.png["images"][0] if self._images_travel else None
                for i in np.flatnonzero(host.video_flags):
                    if b.images is None:
                        raise ValueError("SequenceOutputs: a flagged video frame needs the raw images (submit(images=))")
                    host.video_raw[int(i)] = whole[i] if whole is not None else st.fixed(f"video_raw{i}", b.images[i])
            st.sync()
        return host

    def _video_frames(self, b: _Batch, host: _HostBatch) -> list:
        """the JPEG files of the batch's frames, in order: route "host": the raw images through sd_jpeg_encode_bgr_host on the writer
        threads; route "device": the files as they came, a flagged frame encoded here from its raw image"""
        q = self.video.quality
        if host.video is None:
            return list(self._writers.map(lambda a: encode_jpeg_host(a, q), list(host.png["images"][0])))
        self._flag("video_fallback", b.lo, host.video_flags)
        return [encode_jpeg_host(host.video_raw[i], q) if i in host.video_raw else host.video[i, :int(size)].tobytes()
                for i, size in enumerate(host.video_sizes)]

    def _write_batch(self, b: _Batch) -> list:
        from .engine import RW_DTYPE
        frames = None
        try:
            host = self._fetch(b)
            recs = np.ascontiguousarray(host.records).view(RW_DTYPE).reshape(-1)
            n = len(recs)
            names = self.names[b.lo:b.lo + n]
            h, w = b.size
            files, futs = [], []

            def ends(r):
                if not r["found"]:
                    return None, None
                return r["left_pt"].astype(np.float64)[None, :], r["right_pt"].astype(np.float64)[None, :]

            def write_ply(i):
                path = os.path.join(self.ply_dir, "{}_rw.ply".format(names[i]))
                if host.ply_text is not None and host.ply_flags[i] == 0:     # the device route: the slice is the file
                    with open(path, "wb") as f:
                        f.write(host.ply_text[int(host.ply_offsets[i]):int(host.ply_offsets[i + 1])].data)
                    return path
                left, right = ends(recs[i])
                xyz, rgb = host.clouds[i]
                with open(path, "wb") as f:
                    f.write(rw_ply_bytes(xyz.astype(np.float64), rgb, left, right))
                return path

            def write_scene(i, key):
                """one scene= file of frame i: the device's slice, or sd_scene_format_host from the raw copy (the host route, flags 2 and
                3), or scene_ply_bytes (flag 1)"""
                from .engine import BOX_DTYPE, F2F_DTYPE
                sc = host.scene
                suffix, mask = SCENE_FILES[key]
                path = os.path.join(self.ply_dir, names[i] + suffix)
                text = sc["text"].get(key)
                if text is not None and text[2][i] == 0:
                    data = text[0][int(text[1][i]):int(text[1][i + 1])].data
                else:
                    xyz, rgb = host.clouds[i]
                    kw = dict(road3D=xyz, road_colors=rgb, record=recs[i], mask=mask,
                              road_box=np.ascontiguousarray(sc["road_box"][i]).view(BOX_DTYPE).reshape(())
                              )
                    if sc["f2f"] is not None:
                        kw["f2f"] = np.ascontiguousarray(sc["f2f"][i]).view(F2F_DTYPE).reshape(())
                        kw["fence"] = None if sc["fence"] is None else sc["fence"][i]
                        if sc["fence_box"] is not None:
                            kw["fence_boxes"] = np.ascontiguousarray(sc["fence_box"][i]).view(BOX_DTYPE).reshape(2)
                    data, flag = scene_format_host(**kw)
                    if flag:
                        data = scene_ply_bytes(**kw)
                with open(path, "wb") as f:
                    f.write(data)
                return path

            def write_items(i):
                r = recs[i]
                left, right = ends(r)
                banner, items = overlay_items_sequence(w, h, self.depth, bool(r["found"]), left, right, float(r["width"]) if r["found"] else None)
                path = os.path.join(self.img_dir, "{}_overlay.json".format(names[i]))
                doc = dict(banner=banner, items=items)
                if self.lines is not None:                             # the segments the step drew, restated on the host
                    segs, flag = overlay_segments(r, b.cams[i], b.net_size, (h, w), self.lines, f2f=None if host.f2f is None else host.f2f[i],
                                                  profile=None if host.profile is None else host.profile[i],
                                                  f2f_profile=None if host.f2f_profile is None else host.f2f_profile[i], clip_top=int(0.25 * h))
                    doc["lines"] = segments_json(segs)
                    if flag and host.lines_flags is None:
                        self._frames["lines_flagged"].append(b.lo + i)
                with open(path, "w") as f:
                    json.dump(doc, f)
                return path

            def write_profile_file(i):
                from .engine import F2FP_DTYPE, RWP_DTYPE
                rows = np.ascontiguousarray(host.profile[i]).view(RWP_DTYPE).reshape(-1)
                f2 = None if host.f2f_profile is None else np.ascontiguousarray(host.f2f_profile[i]).view(F2FP_DTYPE).reshape(-1)
                return write_profile(os.path.join(self.profile_dir, "{}.txt".format(names[i])), self.profile, rows, f2)

            def write_family(family):
                """the batch's files of one PNG family, through whichever route its payload came by"""
                data, sizes = host.png[family.key]
                fh, fw = (self.render.height, self.render.width) if family.size == "camera" else (h, w)
                if not family.early_dir:
                    os.makedirs(self._dir(family), exist_ok=True)
                paths = [os.path.join(self._dir(family), nm + family.suffix) for nm in names]
                if sizes is not None:
                    return write_png_streams(paths, data, sizes, fh, fw, self.threads)
                assert data.shape == (n, fh, fw, 3), (data.shape, (n, fh, fw))
                return write_png_batch(paths, data, self.level, self.threads)

            if host.profile is not None:
                os.makedirs(self.profile_dir, exist_ok=True)
                futs.extend(self._writers.submit(write_profile_file, i) for i in range(n))
            for key, flags in (("lines_flagged", host.lines_flags), ("ply_fallback", host.ply_flags), ("disp_nonfinite", host.disp_flags)):
                self._flag(key, b.lo, flags)
            scene_futs = []
            if host.scene is not None:
                os.makedirs(self.ply_dir, exist_ok=True)
                # (the _FENCE file only with the fence chain: approach 'both')
                keys = [k for k in self.scene.files if k != "fence" or host.scene["f2f"] is not None]
                scene_futs = [self._writers.submit(write_scene, i, key) for i in range(n) for key in keys]
                for key, (_, _, flags) in host.scene["text"].items():
                    self._flag("scene_fallback", b.lo, flags)
            for i in range(n):
                if self.ply:
                    futs.append(self._writers.submit(write_ply, i))
                if self.items:
                    futs.append(self._writers.submit(write_items, i))
            for family in self._families:
                files.extend(write_family(family))
            if self.video is not None:
                frames = self._video_frames(b, host)
            files.extend(f.result() for f in futs)
            scene_files = [f.result() for f in scene_futs]
            self._scene_files.extend(scene_files)
            files.extend(scene_files)
            return files
        finally:
            if self.video is not None:
                # this batch's turn in the video (batches finish in any order; the frames go in in batch order): taken and passed on exactly
                # once, whatever raised above -- ``frames`` is then None, nothing is appended, and the batches behind do not wait for ever
                with self._video_turn:
                    self._video_turn.wait_for(lambda: self._video_next == b.k)
                    try:
                        if frames is not None:
                            if self._video_writer is None:
                                name = "result_imgs.avi" if self.world == 1 else "result_imgs_rank{}.avi".format(self.rank)
                                self._video_writer = MjpegAviWriter(os.path.join(self.directory, name), b.size[1], b.size[0], self.video.fps)
                            for fr in frames:
                                self._video_writer.append(fr)
                    finally:
                        self._video_next += 1
                        self._video_turn.notify_all()
