"""Crafted PNG files for the split PNG input route (sd_png_inflate_rows + png_in_gpu.hip), shared by tests/test_png_in_cpu.py,
tests/test_gpu_png_in_device.py and scripts/fuzz_png_rows.cpp (through dump()).  The encoder here is independent of the library: it
FILTERS raw rows with numpy (PNG spec §9, types 0-4) and lets zlib compress them; the yardstick of every comparison is the existing host
decoder sd_png_decode_bgr / frame_io.decode_png, never the new code against itself.  schedule_decode() restates the kernel's schedule
(bands, skew, ring, carry; the constants are read from csrc/png_unfilter.hpp) in Python, with switches for five seeded mistakes."""
import ctypes as C
import functools
import os
import re
import struct
import zlib

import numpy as np

from semantic_depth_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}


@functools.lru_cache(None)
def consts() -> dict:
    """the schedule constants csrc/png_unfilter.hpp exports (kBandRows, kWaves, kPassRows, kPhase, kLag, kRing, kMaxExtent)"""
    txt = open(os.path.join(ROOT, "semantic_depth_amd", "csrc", "png_unfilter.hpp")).read()
    return {k: int(v) for k, v in re.findall(r"constexpr int (k[A-Za-z]+) = (\d+);", txt)}


# ---- the independent encoder ------------------------------------------------------------------------------------------------------
def _chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def filter_rows(img, ftypes) -> np.ndarray:
    """img u8 [h,w,ch], ftypes [h] -> the filtered rows u8 [h, 1 + w*ch] (forward filters on the RAW neighbours, vectorised per frame)"""
    h, w, ch = img.shape
    cur = img.reshape(h, w * ch).astype(np.int32)
    a = np.zeros_like(cur)
    a[:, ch:] = cur[:, :-ch]
    b = np.zeros_like(cur)
    b[1:] = cur[:-1]
    c = np.zeros_like(cur)
    c[1:, ch:] = cur[:-1, :-ch]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    preds = [np.zeros_like(cur), a, b, (a + b) >> 1, paeth]
    ft = np.asarray(ftypes, np.int32)
    out = np.empty((h, 1 + w * ch), np.uint8)
    out[:, 0] = ft
    for t in range(5):
        m = ft == t
        if m.any():
            out[m, 1:] = ((cur[m] - preds[t][m]) & 255).astype(np.uint8)
    return out


def png_from_rows(rows, h, w, ctype, palette=None, split_idat=False, depth=8, interlace=0, level=1) -> bytes:
    z = zlib.compress(np.ascontiguousarray(rows).tobytes(), level)
    out = b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, interlace))
    if palette is not None:
        out += _chunk(b"PLTE", np.asarray(palette, np.uint8).tobytes())
    if split_idat:
        k = max(1, len(z) // 3)
        out += b"".join(_chunk(b"IDAT", z[i:i + k]) for i in range(0, len(z), k))
    else:
        out += _chunk(b"IDAT", z)
    return out + _chunk(b"IEND", b"")


def make_png(img, ctype, ftypes, palette=None, **kw) -> bytes:
    h, w, ch = img.shape
    assert ch == CHANNELS[ctype]
    return png_from_rows(filter_rows(img, ftypes), h, w, ctype, palette=palette, **kw)


def _image(rng, h, w, ctype, lo=0, hi=256, npal=256):
    if ctype == 3:
        return rng.integers(0, npal, (h, w, 1), dtype=np.uint8)
    return rng.integers(lo, hi, (h, w, CHANNELS[ctype]), dtype=np.uint8)


def _palette(rng, n=256):
    return rng.integers(0, 256, (n, 3), dtype=np.uint8)


SMALL_SIZES = [(1, 1), (1, 7), (7, 1), (63, 5), (64, 5), (65, 5), (129, 3), (130, 257)]
TIE_VALUES = np.array([60, 80, 100, 110, 120, 140], np.uint8)


@functools.lru_cache(None)
def cases():
    """[(name, file bytes)]: every file is accepted by sd_png_decode_bgr"""
    k = consts()
    rng = np.random.default_rng(20261020)
    out = []
    # every size x every colour type, a seeded per-row mix of the five filters
    for (h, w) in SMALL_SIZES:
        for ct in (0, 2, 3, 4, 6):
            pal = _palette(rng, 200) if ct == 3 else None
            img = _image(rng, h, w, ct, npal=200)
            out.append((f"mix_{h}x{w}_ct{ct}", make_png(img, ct, rng.integers(0, 5, h), palette=pal, split_idat=(h + ct) % 2 == 1)))
    # every filter type uniformly, every colour type (two bands and a bit) and two RGB frames of more than one ring
    for ft in range(5):
        for ct in (0, 2, 3, 4, 6):
            pal = _palette(rng) if ct == 3 else None
            out.append((f"uniform_ft{ft}_65x5_ct{ct}", make_png(_image(rng, 65, 5, ct), ct, [ft] * 65, palette=pal)))
        out.append((f"uniform_ft{ft}_130x257_ct2", make_png(_image(rng, 130, 257, 2), 2, [ft] * 130)))
    # one full pass of the shipped workgroup -1 / +0 / +1 row at width 9
    P = k["kPassRows"]
    for h in (P - 1, P, P + 1):
        out.append((f"pass_{h}x9_ct2", make_png(_image(rng, h, 9, 2), 2, rng.integers(0, 5, h))))
    out.append((f"pass_{P + 1}x9_ct4", make_png(_image(rng, P + 1, 9, 4), 4, rng.integers(0, 5, P + 1))))
    # every filter type on row 0, on row 64 and on the first row of the second pass
    for ft in range(5):
        fts = rng.integers(0, 5, P + 1)
        fts[[0, k["kBandRows"], P]] = ft
        out.append((f"edges_ft{ft}_{P + 1}x9_ct6", make_png(_image(rng, P + 1, 9, 6), 6, fts)))
    # Paeth rows rich in ties (few distinct values), Average rows with a + b >= 256 (bright pixels), sums that wrap
    for ct in (0, 2, 4):
        img = TIE_VALUES[rng.integers(0, len(TIE_VALUES), (65, 33, CHANNELS[ct]))]
        out.append((f"paeth_ties_65x33_ct{ct}", make_png(img, ct, [4] * 65)))
    out.append(("average_bright_65x33_ct2", make_png(_image(rng, 65, 33, 2, 200, 256), 2, [3] * 65)))
    out.append(("average_bright_70x9_ct4", make_png(_image(rng, 70, 9, 4, 128, 256), 4, [3] * 70)))
    # the carry row at the extent cap
    yy, xx = np.mgrid[0:66, 0:k["kMaxExtent"]]
    wide = np.stack([(xx * 7 + yy) & 255, (xx // 3 + yy * 5) & 255, (xx ^ yy) & 255, (xx + 3 * yy) & 255], -1).astype(np.uint8)
    wide ^= rng.integers(0, 4, wide.shape, dtype=np.uint8)
    out.append((f"wide_66x{k['kMaxExtent']}_ct6", make_png(wide, 6, rng.integers(0, 5, 66))))
    # Pillow-written files: adaptive filtering (RGB), a palette image
    try:
        import io

        from PIL import Image
        yy, xx = np.mgrid[0:130, 0:257]
        smooth = np.stack([(yy + xx) // 2 % 256, (yy * 2 + xx // 3) % 256, (xx * 3 // 2) % 256], -1).astype(np.uint8)
        smooth ^= rng.integers(0, 3, smooth.shape, dtype=np.uint8)
        for name, im in (("pillow_adaptive_130x257_rgb", Image.fromarray(smooth)), ("pillow_130x257_rgba", Image.fromarray(np.dstack([smooth, smooth[..., :1]]))),
                         ("pillow_130x257_palette", Image.fromarray(smooth).quantize(37)), ("pillow_130x257_la", Image.fromarray(smooth).convert("LA"))):
            b = io.BytesIO()
            im.save(b, "PNG")
            out.append((name, b.getvalue()))
    except ImportError:
        pass
    return out


@functools.lru_cache(None)
def overflow_case():
    """(file, y, x): a 70 x 9 palette frame of 5 entries whose pixel (y, x) holds index 5.  sd_png_decode_bgr refuses it;
    sd_png_inflate_rows accepts it (the one exception) and the kernel flags it."""
    rng = np.random.default_rng(77)
    img = rng.integers(0, 5, (70, 9, 1), dtype=np.uint8)
    img[66, 4, 0] = 5
    return make_png(img, 3, rng.integers(0, 5, 70), palette=_palette(rng, 5)), 66, 4


@functools.lru_cache(None)
def damaged():
    """[(name, file bytes)]: files both entry points must refuse with the same status"""
    rng = np.random.default_rng(5)
    out = []
    good = make_png(_image(rng, 70, 9, 2), 2, rng.integers(0, 5, 70))
    for cut in (0, 7, 20, 33, 40, len(good) // 2, len(good) - 13, len(good) - 20):
        out.append((f"truncated_{cut}", good[:cut]))
    img = _image(rng, 70, 9, 2)
    for y in (0, 35, 69):
        rows = filter_rows(img, rng.integers(0, 5, 70))
        rows[y, 0] = 5
        out.append((f"filter5_row{y}", png_from_rows(rows, 70, 9, 2)))
    out.append(("missing_plte", make_png(_image(rng, 70, 9, 3), 3, [0] * 70)))
    out.append(("depth16", png_from_rows(filter_rows(_image(rng, 8, 18, 0), [0] * 8), 8, 9, 0, depth=16)))
    out.append(("depth16_rgb", png_from_rows(filter_rows(_image(rng, 8, 54, 0), [0] * 8), 8, 9, 2, depth=16)))
    out.append(("interlaced", make_png(_image(rng, 8, 9, 2), 2, [0] * 8, interlace=1)))
    out.append(("short_stream", png_from_rows(filter_rows(_image(rng, 69, 9, 2), [1] * 69), 70, 9, 2)))
    out.append(("colour_type_5", png_from_rows(filter_rows(_image(rng, 8, 9, 2), [0] * 8), 8, 9, 5)))
    out.append(("not_a_png", b"\xff\xd8\xff\xe0" + bytes(64)))
    return out


# ---- the library's entry points ---------------------------------------------------------------------------------------------------
def host_decode(buf):
    """sd_png_decode_bgr -> (status, u8 [h,w,3] | None)"""
    lib = L.load()
    hh, ww = C.c_int(), C.c_int()
    st = lib.sd_png_decode_bgr(buf, len(buf), None, 0, C.byref(hh), C.byref(ww))
    if st != L.SD_OK:
        return st, None
    out = np.zeros((hh.value, ww.value, 3), np.uint8)
    st = lib.sd_png_decode_bgr(buf, len(buf), out.ctypes.data_as(C.c_void_p), out.size, None, None)
    return st, (out if st == L.SD_OK else None)


def inflate_rows(buf, capacity=None, fill=0):
    """sd_png_inflate_rows -> (status, rows u8 [capacity], descriptor).  capacity None: what the descriptor query asks for"""
    lib = L.load()
    d = L.sd_png_frame_desc()
    st = lib.sd_png_inflate_rows(buf, len(buf), None, 0, C.byref(d))
    if st != L.SD_OK:
        return st, None, d
    cap = d.rows_bytes() if capacity is None else capacity
    rows = np.full((max(cap, 1),), fill, np.uint8)
    st = lib.sd_png_inflate_rows(buf, len(buf), rows.ctypes.data_as(C.c_void_p), cap, C.byref(d))
    return st, rows, d


def unfilter_host(rows, d):
    """sd_png_unfilter_bgr (+ the palette loop of png_decode) on inflated rows -> (u8 [h,w,3], index beyond the palette seen)"""
    lib = L.load()
    out = np.zeros((d.height, d.width, 3), np.uint8)
    st = lib.sd_png_unfilter_bgr(rows.ctypes.data_as(C.c_void_p), d.height, d.width, d.channels, out.ctypes.data_as(C.c_void_p))
    assert st == L.SD_OK
    if d.color_type != 3:
        return out, False
    pal = np.ctypeslib.as_array(d.palette).reshape(256, 3)
    idx = out[..., 0].astype(np.int64)
    over = bool((idx >= d.palette_entries).any())
    idx = np.where(idx >= d.palette_entries, 0, idx)
    return pal[idx][..., ::-1].copy(), over


# ---- the kernel's schedule, restated ------------------------------------------------------------------------------------------------
MISTAKES = ("drop_band_carry", "paeth_tie_order", "average_8bit", "gray_alpha_bpp1", "first_pixel_like_others")


def _predict(ft, a, b, c, mistake):
    """vectors of one channel: filter types ft, neighbours a, b, c (int64)"""
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    if mistake == "paeth_tie_order":
        paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb < pc, b, c))
    else:
        paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    avg = (((a + b) & 255) >> 1) if mistake == "average_8bit" else ((a + b) >> 1)
    return np.select([ft == 0, ft == 1, ft == 2, ft == 3], [np.zeros_like(a), a, b, avg], paeth)


def _lds_read(src, x, wv, y0, phase):
    slot = x if src["mask"] is None else x & src["mask"]
    assert src["x"][slot] == x and src["rows"][slot] == y0 - 1, ("the slot holds another pixel", wv, x, int(src["x"][slot]), int(src["rows"][slot]))
    assert src["ph"][slot] < phase or src["wv"][slot] == wv, ("read in the phase of the write", wv, x)
    return src["v"][slot].copy()


def schedule_decode(rows, h, w, ch, waves, mistake=None):
    """the reconstructed samples u8 [h,w,ch] by the kernel's schedule: lane l of wave v owns row pass0 + 64 v + l and does pixel t - l at its
    step t; wave v runs kLag * kPhase steps behind wave v - 1; the last row of a band goes through a ring of kRing pixels (the row buffer
    for the last wave of a pass); a barrier every kPhase steps.  Every ring / row-buffer read asserts that the slot holds the pixel it
    expects and was written in an EARLIER phase or earlier by the same wave: a schedule that reads too early fails here, without a GPU."""
    k = consts()
    BR, PH, LAG, RING = k["kBandRows"], k["kPhase"], k["kLag"], k["kRing"]
    R = np.asarray(rows[:h * (1 + w * ch)], np.uint8).reshape(h, 1 + w * ch)
    FT = R[:, 0].astype(np.int64)
    S = R[:, 1:].reshape(h, w, ch).astype(np.int64)
    out = np.zeros((h, w, ch), np.int64)
    lanes = np.arange(BR)
    # LDS: value, pixel index held, (phase, wave) of the write
    carry = dict(v=np.zeros((w, ch), np.int64), x=np.full(w, -1), ph=np.full(w, -1), wv=np.full(w, -1), rows=np.full(w, -1), mask=None)
    ring = [dict(v=np.zeros((RING, ch), np.int64), x=np.full(RING, -1), ph=np.full(RING, -1), wv=np.full(RING, -1), rows=np.full(RING, -1), mask=RING - 1)
            for _ in range(waves)]
    prev = np.zeros((waves, BR, ch), np.int64)          # never re-zeroed: pixel 0 sees zeros through the x > 0 rule alone
    bprev = np.zeros((waves, BR, ch), np.int64)
    above = np.zeros((waves, ch), np.int64)
    phase = 0
    for pass0 in range(0, h, BR * waves):
        bands = min(waves, -(-(h - pass0) // BR))
        steps = (bands - 1) * LAG * PH + w + BR - 1
        for g0 in range(0, steps, PH):
            phase += 1
            for wv in range(bands):
                t0 = g0 - wv * LAG * PH
                if not (0 <= t0 < w + BR - 1):
                    continue
                src = carry if wv == 0 else ring[wv - 1]
                dst = carry if wv == waves - 1 else ring[wv]
                y0 = pass0 + wv * BR
                y = y0 + lanes
                row_ok = y < h
                ysafe = np.minimum(y, h - 1)
                ft = FT[ysafe]
                has_above = y0 > 0 and mistake != "drop_band_carry"
                for t in range(t0, t0 + PH):
                    x = t - lanes
                    act = row_ok & (x >= 0) & (x < w)
                    if not act.any():
                        continue
                    up = np.zeros((BR, ch), np.int64)
                    up[1:] = prev[wv, :-1]
                    if has_above and t < w:
                        if t == t0 == 0:
                            above[wv] = _lds_read(src, 0, wv, y0, phase)
                        up[0] = above[wv]
                        if t + 1 < w:                    # one step ahead of its use, as the kernel reads it
                            above[wv] = _lds_read(src, t + 1, wv, y0, phase)
                    b = np.where((y > 0)[:, None], up, 0)
                    first = (x > 0)[:, None] if mistake != "first_pixel_like_others" else np.ones((BR, 1), bool)
                    a = np.where(first, prev[wv], 0)
                    c = np.where(first, bprev[wv], 0)
                    xs = np.clip(x, 0, w - 1)
                    s = S[ysafe, xs]
                    o = np.zeros((BR, ch), np.int64)
                    if mistake == "gray_alpha_bpp1" and ch == 2:
                        # the left neighbour taken one BYTE back: channel 0 sees the previous pixel's alpha, channel 1 this pixel's gray
                        o[:, 0] = (s[:, 0] + _predict(ft, a[:, 1], b[:, 0], c[:, 1], mistake)) & 255
                        o[:, 1] = (s[:, 1] + _predict(ft, o[:, 0], b[:, 1], b[:, 0], mistake)) & 255
                    else:
                        for q in range(ch):
                            o[:, q] = (s[:, q] + _predict(ft, a[:, q], b[:, q], c[:, q], mistake)) & 255
                    prev[wv] = np.where(act[:, None], o, prev[wv])
                    bprev[wv] = np.where(act[:, None], b, bprev[wv])
                    out[ysafe[act], xs[act]] = o[act]
                    if act[BR - 1]:
                        xl = int(x[BR - 1])
                        slot = xl if dst["mask"] is None else xl & dst["mask"]
                        dst["v"][slot], dst["x"][slot], dst["ph"][slot], dst["wv"][slot], dst["rows"][slot] = o[BR - 1], xl, phase, wv, y0 + BR - 1
    return out.astype(np.uint8)


def samples_to_bgr(samples, d):
    """the channel map and the guarded palette lookup of the kernel -> (u8 [h,w,3], flagged)"""
    ct = d.color_type
    if ct in (2, 6):
        return samples[..., 2::-1].copy(), False
    if ct == 3:
        pal = np.ctypeslib.as_array(d.palette).reshape(256, 3)
        idx = samples[..., 0].astype(np.int64)
        over = idx >= d.palette_entries
        return pal[np.where(over, 0, idx)][..., ::-1].copy(), bool(over.any())
    return np.repeat(samples[..., :1], 3, axis=2), False


def paeth_tie_census(img):
    """counts of Paeth ties among the (a, b, c) neighbourhoods of a raw image with DISTINCT a, b, c: {"pa==pb", "pb==pc", "pa==pc"} and, with
    a == b == c (the only way all three distances are equal: |b-c| = |a-c| = |a+b-2c| forces a = b = c), "all"."""
    h, w, ch = img.shape
    cur = img.reshape(h, w * ch).astype(np.int64)
    a, b, c = cur[1:, :-ch], cur[:-1, ch:], cur[:-1, :-ch]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    distinct = (a != b) & (b != c) & (a != c)
    return {"pa==pb": int((distinct & (pa == pb)).sum()), "pb==pc": int((distinct & (pb == pc)).sum()),
            "pa==pc": int((distinct & (pa == pc)).sum()), "all": int(((pa == pb) & (pb == pc)).sum())}


def dump(directory):
    """write every case, the overflow case and the damaged files into `directory` (the seed corpus of scripts/fuzz_png_rows.cpp)"""
    os.makedirs(directory, exist_ok=True)
    for name, buf in cases() + [("overflow", overflow_case()[0])] + damaged():
        if len(buf) < (256 << 10):
            open(os.path.join(directory, name + ".png"), "wb").write(buf)
