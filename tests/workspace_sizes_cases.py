"""Every public workspace size query and the handle arena's total, as (function, arguments) -> what the library answers.

tests/golden/workspace_sizes.json holds the answers of the commit named in its header; tests/test_workspace_layouts_cpu.py asks the
library of the tree the same questions.  The arguments travel in the JSON, so the golden file alone says what was asked: grid() below
only made the list once.  Extents and counts are chosen so that products are no multiples of 16 or 256 (alignment padding is
exercised), and every query's refusals are in the list (they must still refuse)."""
import ctypes as C
import itertools
import json
import os

import conv_forms_cases as F
from semantic_depth_amd import _lib as L

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "workspace_sizes.json")

BS = (1, 3, 32)
EXTENTS = (1, 17, 250, 1025)
CAPS = (1, 257, 65536)
DS = (1, 256)


def _jpeg_desc(h, w, ncomp, hmax, vmax):
    d = L.sd_jpeg_frame_desc()
    d.height, d.width, d.ncomp, d.hmax, d.vmax, d.orientation, d.adobe_transform = h, w, ncomp, hmax, vmax, 1, -1
    off = 0
    for i in range(ncomp):
        ch, cv = (hmax, vmax) if i == 0 else (1, 1)
        d.blocks_w[i] = (w + 8 * hmax - 1) // (8 * hmax) * ch
        d.blocks_h[i] = (h + 8 * vmax - 1) // (8 * vmax) * cv
        d.coef_offset[i] = off
        off += d.blocks_w[i] * d.blocks_h[i] * 64
    return d


def _render_camera(width, height):
    cam = L.sd_render_camera()
    for i in (0, 5, 10):
        cam.ext[i] = 1.0
    cam.fx = cam.fy = 100.0
    cam.cx, cam.cy, cam.z_near = width / 2, height / 2, 0.1
    cam.width, cam.height, cam.point_size = width, height, 1
    return cam


def call(lib, fn, args):
    """[status or None, outputs...] of one query"""
    f = getattr(lib, fn)
    if fn in ("sd_text_workspace_bytes", "sd_overlay_workspace_bytes", "sd_fuse_sweep_workspace", "sd_rw_profile_workspace"):
        return [None, int(f(*args))]                               # (these return the size; 0 is their refusal)
    a, b = C.c_size_t(0), C.c_size_t(0)
    if fn == "sd_jpeg_reconstruct_workspace":                      # args: the frames as [height, width, ncomp, hmax, vmax]
        descs = (L.sd_jpeg_frame_desc * max(len(args), 1))(*[_jpeg_desc(*fr) for fr in args])
        return [int(f(descs, len(args), C.byref(a))), a.value]
    if fn == "sd_render_workspace":                                # args: B, cap, width, height
        cam = _render_camera(args[2], args[3])
        return [int(f(args[0], args[1], C.byref(cam), C.byref(a))), a.value]
    if fn in ("sd_png_encode_workspace", "sd_jpeg_encode_workspace", "sd_ply_format_workspace", "sd_scene_workspace"):
        return [int(f(*args, C.byref(a), C.byref(b))), a.value, b.value]      # (the second: the stream stride / stream bound / text bound)
    return [int(f(*args, C.byref(a))), a.value]


def handle_total(lib, cfg):
    """sd_query_memory's workspace bytes of a conv_forms_cases configuration (enc, prec, H, W, B, small-batch level, switches)"""
    with F.handle(lib, tuple(cfg)) as h:
        return F.workspace(lib, h)


def grid():
    """the (function, arguments) list the golden file was recorded over"""
    q = []
    add = lambda fn, *args: q.append([fn, list(args)])
    for B in BS + (0, 65535, 65536):
        add("sd_png_reconstruct_workspace", B)
        add("sd_text_workspace_bytes", B)
        for stride in (0, 1, 17, 1025):
            add("sd_jpeg_entropy_workspace", B, stride)
            for pieces in (0, 1, 255, 256, 257, 65537):
                add("sd_jpeg_sync_workspace", B, stride, pieces)
        for D in DS + (0, 7, 257, -1):
            add("sd_overlay_workspace_bytes", B, D)
            for cap in CAPS + (0, 2047, 2049):
                add("sd_rw_profile_workspace", B, cap, D)
        for cap in CAPS + (0, -1):
            add("sd_ply_format_workspace", B, cap)
            for w, h in ((1, 1), (17, 250), (1025, 17), (16384, 1), (16385, 1), (0, 5)):
                add("sd_render_workspace", B, cap, w, h)
        for cr, cf, lat, mask in itertools.product((0, 1, 257, 65536), (0, 257), (0, 1000, 0xFFFFFFFF), (255, 1, 8, 2, 128, 0, 256)):
            add("sd_scene_workspace", B, cr, cf, lat, mask)
        add("sd_scene_workspace", B, -1, 0, 0, 255)
        for h, w in itertools.product(EXTENTS + (16384, 16385, 0), EXTENTS):
            add("sd_png_encode_workspace", B, h, w)
            add("sd_jpeg_encode_workspace", B, h, w)
        for T, h, w in itertools.product((1, 3, 21, 0), (1, 17, 250), (17, 1025)):
            add("sd_fuse_sweep_workspace", B, T, h, w)
        add("sd_fuse_sweep_workspace", B, 65536 // max(B, 1) + 1, 17, 17)
        for sh, sw, dh, dw in ((1, 1, 1, 1), (17, 250, 17, 250), (250, 1025, 17, 250), (17, 17, 250, 1025), (1025, 250, 250, 17), (1025, 1025, 32, 33),
                               (1025, 1025, 33, 32), (16384, 17, 512, 17), (16385, 17, 17, 17), (17, 0, 17, 17)):
            for ch in (1, 3, 2):
                add("sd_resize_pil_workspace", B, sh, sw, dh, dw, ch)
            add("sd_disp_image_workspace", B, sh, sw, dh, dw)
    frames = [[1, 1, 1, 1, 1], [17, 250, 3, 1, 1], [250, 1025, 3, 2, 1], [1025, 17, 3, 2, 2], [250, 250, 1, 1, 1]]
    for n in (1, 3, 32):
        add("sd_jpeg_reconstruct_workspace", *[frames[i % len(frames)] for i in range(n)])
    add("sd_jpeg_reconstruct_workspace", [17, 250, 3, 2, 2], [17, 250, 2, 1, 1])      # (a descriptor that is not self-consistent)
    add("sd_jpeg_reconstruct_workspace")                                                # (B = 0)
    # the handle's arena: these totals also pin the Open3D, compaction and both fuse scratches, which have no query of their own
    handles = []
    for (H, W), B in itertools.product(((128, 256), (256, 640)), BS):
        for level in (0, 1, 2):
            handles.append(["resnet50", "f16x2", H, W, B, level, ""])
        handles.append(["resnet50", "bf16x3", H, W, B, 0, ""])
        handles.append(["vgg", "f32", H, W, B, 0, ""])
    return q, handles


def record(lib, commit):
    """the golden document of `lib`"""
    q, handles = grid()
    return {"header": f"answers of the library built from commit {commit}; regenerate only from that commit (tests/workspace_sizes_cases.py record())",
            "queries": [[fn, args, call(lib, fn, args)] for fn, args in q],
            "handles": [[cfg, handle_total(lib, cfg)] for cfg in handles]}


def golden():
    with open(GOLDEN) as f:
        return json.load(f)
