"""Shared by tests/test_text_cpu.py, tests/test_gpu_text_device.py and tests/test_outputs_text.py: the records and item lists of the text
route's tests, and an INDEPENDENT statement of the raster rule of include/semdepth.h in exact integers.  It reads the font only through
sd_text_glyph; everything else -- the positions, the rule -- is restated here in numpy int64, whose range is checked per item (below)."""
import ctypes as C

import numpy as np

from semantic_depth_amd import _lib as L
from semantic_depth_amd import outputs
from semantic_depth_amd.engine import RW_DTYPE

REQUIRED = " 0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz.,:;'-+/()%="


def glyph(code: int):
    """(segments int [n,4] as {x0, y0, x1, y1} in units, advance) of byte ``code``"""
    segs = (C.c_int8 * (4 * L.SD_TEXT_MAX_SEGS))()
    n, adv = C.c_int(), C.c_int()
    assert L.load().sd_text_glyph(code, segs, C.byref(n), C.byref(adv)) == L.SD_OK
    return np.array(segs[:4 * n.value], np.int64).reshape(-1, 4), adv.value


def item(text, org, scale=2, color=(255, 255, 255), thickness=2):
    return dict(text=text, org=tuple(org), fontFace=16, fontScale=scale, color=tuple(color), thickness=thickness)


def reference_draw(img: np.ndarray, items) -> np.ndarray:
    """the rule on a copy of u8 [h,w,3] ``img``, items in list order: in 1/256 pixel, vertex (ux, uy) of the glyph at pen position p is
    (org_x * 256 + (p + ux) * s, org_y * 256 - uy * s) with s = lround(fontScale * 256); pixel (px, py), centre (256 px, 256 py), is painted
    iff its squared distance to some segment is <= (128 thickness)^2.  Only the pixels of a segment's bounding box widened by the radius
    are evaluated (a point outside it is farther than the radius from every point inside the unwidened box).  int64 suffices there for
    s <= 1024 and thickness <= 8: |d| <= 28 * 1024 < 2^15 and |w| < 2^15 + 2^11 per axis keep every sum of two products far below 2^62,
    and the two quantities that are squared or multiplied again, |w x d| and r^2 |d|^2, are asserted below 2^31 and 2^62 on their values."""
    out = np.array(img, np.uint8, copy=True)
    h, w = out.shape[:2]
    for it in items:
        s = int(np.floor(float(it["fontScale"]) * 256 + 0.5))
        r = int(it["thickness"]) * 128
        assert 1 <= s <= 1024 and 1 <= r <= 1024
        ox, oy = int(it["org"][0]) * 256, int(it["org"][1]) * 256
        col = np.array(it["color"], np.uint8)
        pen = 0
        for code in it["text"].encode("latin-1"):
            segs, adv = glyph(code)
            for x0, y0, x1, y1 in segs.tolist():
                ax, ay, bx, by = ox + (pen + x0) * s, oy - y0 * s, ox + (pen + x1) * s, oy - y1 * s
                px0, px1 = max(0, -((r - min(ax, bx)) // 256)), min(w - 1, (max(ax, bx) + r) // 256)
                py0, py1 = max(0, -((r - min(ay, by)) // 256)), min(h - 1, (max(ay, by) + r) // 256)
                if px0 > px1 or py0 > py1:
                    continue
                X = np.arange(px0, px1 + 1, dtype=np.int64)[None, :] * 256
                Y = np.arange(py0, py1 + 1, dtype=np.int64)[:, None] * 256
                dx, dy = bx - ax, by - ay
                wx, wy = X - ax, Y - ay
                dd = dx * dx + dy * dy
                t = wx * dx + wy * dy
                cross = wx * dy - wy * dx
                assert int(np.abs(cross).max()) < 2 ** 31 and r * r * dd < 2 ** 62
                near_a = (t <= 0) & (wx * wx + wy * wy <= r * r)
                near_b = (t >= dd) & ((wx - dx) ** 2 + (wy - dy) ** 2 <= r * r)
                inside = (t > 0) & (t < dd) & (cross * cross <= r * r * dd)
                out[py0:py1 + 1, px0:px1 + 1][near_a | near_b | inside] = col
            pen += adv
    return out


# ---- records ----
def record(found=1, left=-3.4150002, right=0.125, width=4.41000023):
    rec = np.zeros((), RW_DTYPE)
    rec["found"] = found
    rec["left_pt"] = (np.float32(left), 1.6, 10.0)
    rec["right_pt"] = (np.float32(right), 1.6, 10.0)
    rec["width"] = width
    return rec


def records():
    """found / not found, the rounding values of the issue as float32 end points (widened to double by the layout) and double widths"""
    r = [record(), record(found=0, width=np.nan), record(left=-0.375, right=2.675, width=9.995), record(left=0.001, right=123456.789, width=1 / 3),
         record(left=0.0, right=-0.0, width=2.0000000000000004), record(left=9.995, right=0.375, width=0.125)]
    return np.array(r, RW_DTYPE)


def special_records():
    """NaN / inf / 3e9: drawn as nan / inf / inf (and -inf for the negated left end)"""
    return np.array([record(left=np.nan, right=np.inf, width=3e9), record(left=np.inf, right=-3e9, width=np.nan),
                     record(left=3e9, right=np.nan, width=-np.inf)], RW_DTYPE)


def python_items(rec, h, w, depth=10.0):
    """the yardstick of the strings: outputs.overlay_items_sequence, Python's own formatter"""
    if not rec["found"]:
        return outputs.overlay_items_sequence(w, h, depth, False)[1]
    return outputs.overlay_items_sequence(w, h, depth, True, rec["left_pt"].astype(np.float64)[None, :], rec["right_pt"].astype(np.float64)[None, :],
                                          float(rec["width"]))[1]


def host_items(rec, h, w, depth=10.0):
    """sd_text_items_rw_host: (ctypes array, n)"""
    arr = (L.sd_text_item * L.SD_TEXT_MAX_ITEMS)()
    n = C.c_int()
    r = L.sd_rw_result.from_buffer_copy(np.asarray(rec).tobytes())
    st = L.load().sd_text_items_rw_host(C.byref(r), "{:.2f}".format(depth).encode(), h, w, arr, C.byref(n))
    assert st == L.SD_OK, st
    return arr, n.value


def item_dicts(arr, n):
    return [item(bytes(arr[i].text[:arr[i].len]).decode("latin-1"), (arr[i].org_x, arr[i].org_y), arr[i].scale_q8 / 256.0, tuple(arr[i].bgr),
                 arr[i].thickness) for i in range(n)]


def host_draw(img, arr, n):
    """sd_text_draw_host on a copy"""
    out = np.array(img, np.uint8, order="C", copy=True)
    assert L.load().sd_text_draw_host(out.ctypes.data_as(C.c_void_p), out.shape[0], out.shape[1], arr, n) == L.SD_OK
    return out


def prefilled(seed, *shape):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


# ---- the two rendered samples kept under tests/golden/ (a reader judges legibility by eye; a test pins every pixel) ----
SAMPLES = (("text_sample_found.png", True), ("text_sample_not_found.png", False))


def sample_image(found: bool) -> np.ndarray:
    """a plain 1024 x 2048 scene (bands from sky to ground, a road trapezoid in the overlay's colour) with the sequence layout drawn on it"""
    h, w = 1024, 2048
    yy, xx = np.arange(h)[:, None], np.arange(w)[None, :]
    base = np.zeros((h, w, 3), np.uint8)
    base[..., 0] = 90 + (yy // 64) * 4
    base[..., 1] = 80 + (yy // 64) * 3
    base[..., 2] = 70 + (yy // 64) * 2
    base[(yy > 560) & (np.abs(xx - 1024) < (yy - 560) * 1.6 + 60)] = (128, 80, 128)
    banner, items = outputs.overlay_items_sequence(w, h, 10.0, found, [[-3.4150002, 1.6, 10.0]], [[0.995, 1.6, 10.0]], 4.41000023)
    img, items = outputs.draw_overlay(base, banner, items)
    return outputs.draw_text(img, items)
