"""CPU: the host statement of the text route (sd_text_items_rw_host, sd_text_draw_host, sd_text_glyph; csrc/text_draw.hpp) against Python's
own formatter (outputs.overlay_items_sequence) and an independent statement of the raster rule (tests/text_cases.py), byte for byte."""
import ctypes as C
import os

import numpy as np
import pytest

import __graft_entry__ as graft
import text_cases as T
from semantic_depth_amd import _lib as L
from semantic_depth_amd import outputs


@pytest.fixture(scope="module", autouse=True)
def lib():
    graft.build()
    return L.load()


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(96, 256), (333, 1001), (1024, 2048)]


@pytest.mark.parametrize("h,w", SIZES)
def test_items_equal_overlay_items_sequence(h, w):
    for rec in T.records():
        arr, n = T.host_items(rec, h, w)
        want = T.python_items(rec, h, w)
        assert n == len(want) == (4 if rec["found"] else 1)
        for a, it in zip(arr, want):
            assert bytes(a.text[:a.len]).decode() == it["text"]
            assert not any(a.text[a.len:]) and a.reserved == 0
            assert (a.org_x, a.org_y) == it["org"]
            assert a.scale_q8 == int(np.floor(it["fontScale"] * 256 + 0.5)) and a.thickness == it["thickness"]
            assert tuple(a.bgr) == it["color"]
        assert len({tuple(a.bgr) for a in arr[:n]}) == 1            # one colour per frame: the device runs a frame's items as parallel grid slices


def test_the_rounding_cases_print_what_the_issue_names():
    texts = [bytes(a.text[:a.len]).decode() for rec in T.records() for a in T.host_items(rec, 96, 256)[0][:4 if rec["found"] else 1]]
    joined = "|".join(texts)
    for s in ("3.42m to road's left end", "0.12m to", "0.38m to", "-0.00m to road's left end", "123456.79m to road's right end", "-0.00m to road's right end",
              "Cannot compute width of road at 10.00 m depth:", "At 10.00 m depth:", "Road's width: 0.33 m", "Road's width: 2.00 m"):
        assert s in joined, (s, texts)
    # 2.675 and 9.995 as float32 widened to double, and 9.995 as a double: whatever Python prints
    for v in (float(np.float32(2.675)), float(np.float32(9.995)), 9.995):
        assert "{:.2f}".format(v) in joined


def test_non_finite_and_out_of_range_numbers():
    recs = T.special_records()
    texts = [[bytes(a.text[:a.len]).decode() for a in T.host_items(rec, 200, 640)[0]] for rec in recs]
    assert texts[0][1:] == ["nanm to road's left end", "infm to road's right end", "Road's width: inf m"]
    assert texts[1][1:] == ["-infm to road's left end", "-infm to road's right end", "Road's width: nan m"]
    assert texts[2][1:] == ["-infm to road's left end", "nanm to road's right end", "Road's width: -inf m"]
    # the non-finite ones are Python's strings too; only |v| >= 2^31 deviates (Python prints the digits)
    assert "{:.2f}".format(float("nan")) == "nan" and "{:.2f}".format(-float("inf")) == "-inf"


def test_argument_checks(lib):
    rec = L.sd_rw_result()
    arr, n = (L.sd_text_item * 4)(), C.c_int()
    assert lib.sd_text_items_rw_host(C.byref(rec), b"1" * 24, 96, 256, arr, C.byref(n)) == L.SD_ERR_INVALID
    assert lib.sd_text_items_rw_host(C.byref(rec), b"1" * 23, 96, 256, arr, C.byref(n)) == L.SD_OK and arr[0].len == 64
    assert lib.sd_text_items_rw_host(C.byref(rec), b"10.00", 0, 256, arr, C.byref(n)) == L.SD_ERR_INVALID
    assert lib.sd_text_items_rw_host(C.byref(rec), b"10.00", 96, 16385, arr, C.byref(n)) == L.SD_ERR_INVALID
    img = np.full((8, 8, 3), 7, np.uint8)
    for kw in (dict(scale=0), dict(scale=16.01), dict(thickness=0), dict(thickness=33), dict(org=(32769, 0)), dict(org=(0, -32769))):
        items = outputs.text_items([T.item("A", kw.pop("org", (1, 6)), **kw)])
        assert lib.sd_text_draw_host(img.ctypes.data_as(C.c_void_p), 8, 8, items, 1) == L.SD_ERR_INVALID
    assert lib.sd_text_draw_host(img.ctypes.data_as(C.c_void_p), 8, 16385, items, 0) == L.SD_ERR_INVALID
    assert (img == 7).all()
    assert lib.sd_text_workspace_bytes(0) == 0 and lib.sd_text_workspace_bytes(2) == 2 * lib.sd_text_workspace_bytes(1) > 0


# ------------------------------------------------------------------------------------------------ the font
def test_the_header_table_is_the_output_of_its_construction():
    """scripts/make_text_font.py builds every glyph from strokes and sampled ellipse arcs; text_draw.hpp carries exactly what it prints"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_text_font", os.path.join(ROOT, "scripts", "make_text_font.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.header_table() == mod.table()


def test_font_invariants(lib):
    seen = {}
    for ch in T.REQUIRED:
        segs, adv = T.glyph(ord(ch))
        assert len(segs) <= L.SD_TEXT_MAX_SEGS and 1 <= adv <= 24, ch
        assert (len(segs) > 0) == (ch != " "), ch
        if len(segs):
            assert segs[:, [0, 2]].min() >= 0 and segs[:, [0, 2]].max() <= adv and segs[:, [1, 3]].min() >= -7 and segs[:, [1, 3]].max() <= 21, ch
        key = tuple(map(tuple, segs.tolist()))
        assert key not in seen, (ch, seen.get(key))
        seen[key] = ch
        # the same strokes in another order or direction are the same drawing
        canon = tuple(sorted(min((a, b, c, d), (c, d, a, b)) for a, b, c, d in segs.tolist()))
        assert ("canon", canon) not in seen, (ch, seen.get(("canon", canon)))
        seen[("canon", canon)] = ch
    # proportions: capitals and digits reach the cap height and stand on the baseline; x-height letters reach 14; descenders reach -7
    for ch in "ABCDEFGHIJKLMNOPRSTUVWXYZ0123456789":
        segs, _ = T.glyph(ord(ch))
        assert segs[:, [1, 3]].max() == 21 and segs[:, [1, 3]].min() == 0, ch
    for ch in "acemnorsuvwxz":
        segs, _ = T.glyph(ord(ch))
        assert segs[:, [1, 3]].max() == 14 and segs[:, [1, 3]].min() == 0, ch
    for ch in "gjpqy":
        assert T.glyph(ord(ch))[0][:, [1, 3]].min() == -7, ch
    box, badv = T.glyph(0)
    assert len(box) == 4 and tuple(map(tuple, box.tolist())) not in seen
    for code in (1, ord("#"), ord("@"), ord("~"), 127, 128, 200, 255):
        segs, adv = T.glyph(code)
        assert np.array_equal(segs, box) and adv == badv, code
    n, adv = C.c_int(), C.c_int()
    segs = (C.c_int8 * 128)()
    assert lib.sd_text_glyph(256, segs, C.byref(n), C.byref(adv)) == L.SD_ERR_INVALID
    assert lib.sd_text_glyph(-1, segs, C.byref(n), C.byref(adv)) == L.SD_ERR_INVALID


# ------------------------------------------------------------------------------------------------ the rasteriser
def _check(img, items):
    got = outputs.draw_text(img, items)
    want = T.reference_draw(img, items)
    assert np.array_equal(got, want), int((got != want).any(-1).sum())
    return got


@pytest.mark.parametrize("scale", [0.5, 1, 2.2])
@pytest.mark.parametrize("thickness", [1, 2, 3])
def test_draw_host_equals_the_independent_statement(scale, thickness):
    img = T.prefilled(int(scale * 10) + thickness, 64, 192, 3)
    got = _check(img, [T.item("Road's 4.41m (g,j;Q)", (3, 40), scale, (1, 254, 3), thickness)])
    assert (got != img).any()


def test_clipped_items():
    img = T.prefilled(5, 64, 192, 3)
    for org in ((-30, 40), (20, 8), (150, 40), (20, 75), (-400, 40), (20, 300)):
        _check(img, [T.item("Wg/y%8", org, 2, (9, 8, 7), 2)])


def test_overlapping_items_are_drawn_in_list_order():
    img = T.prefilled(6, 64, 192, 3)
    a, b = T.item("OOOOO", (5, 45), 2, (255, 0, 0), 3), T.item("XXXXX", (9, 45), 2, (0, 0, 255), 3)
    ab, ba = _check(img, [a, b]), _check(img, [b, a])
    assert not np.array_equal(ab, ba)


def test_empty_and_full_strings():
    img = T.prefilled(7, 64, 192, 3)
    assert np.array_equal(_check(img, [T.item("", (5, 40))]), img)
    assert np.array_equal(_check(img, []), img)
    full = "".join(T.REQUIRED[(7 * i) % len(T.REQUIRED)] for i in range(64))
    big = T.prefilled(8, 40, 700, 3)
    _check(big, [T.item(full, (2, 28), 0.5, (200, 100, 50), 1)])
    with pytest.raises(ValueError):
        outputs.draw_text(big, [T.item(full + "x", (2, 28))])


def test_every_glyph_and_the_box():
    img = T.prefilled(9, 60, 900, 3)
    _check(img, [T.item(T.REQUIRED[:38], (2, 24), 1, (255, 255, 255), 1), T.item(T.REQUIRED[38:] + "#\x7f\xff", (2, 52), 1, (0, 255, 255), 2)])


def test_sequence_layout_clipped_at_the_top_and_right():
    h, w = 200, 640
    img = T.prefilled(10, h, w, 3)
    for rec in T.records()[:3]:
        arr, n = T.host_items(rec, h, w)
        got = T.host_draw(img, arr, n)
        want = T.reference_draw(img, T.python_items(rec, h, w))
        assert np.array_equal(got, want), int((got != want).any(-1).sum())
        if rec["found"]:            # the top row is painted, and on a wider canvas the same items go on beyond column w
            wide = np.zeros((h, w + 800, 3), np.uint8)
            assert (got[0] != img[0]).any() and T.reference_draw(wide, T.python_items(rec, h, w))[:, w:].any()
