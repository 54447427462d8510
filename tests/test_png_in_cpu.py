"""CPU: the host half of the split PNG input route (sd_png_inflate_rows, sd_inflate_files_png) against the existing decoder
sd_png_decode_bgr, and the schedule of png_in_gpu.hip restated in Python (tests/png_in_cases.py) against the same bytes.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as graft
import png_in_cases as P
from semantic_depth_amd import _lib as L


@pytest.fixture(scope="module", autouse=True)
def built():
    graft.build()


@pytest.fixture(scope="module")
def decoded():
    """{name: (rows, descriptor, reference BGR)} -- computed once, read-only"""
    out = {}
    for name, buf in P.cases():
        st, ref = P.host_decode(buf)
        assert st == L.SD_OK, name
        st, rows, d = P.inflate_rows(buf)
        assert st == L.SD_OK, name
        ref.setflags(write=False)
        rows.setflags(write=False)
        out[name] = (rows, d, ref)
    return out


def test_case_list_covers_what_it_names():
    k = P.consts()
    assert k["kPassRows"] == k["kBandRows"] * k["kWaves"] == 1024 and k["kMaxExtent"] == 16384
    names = [n for n, _ in P.cases()]
    assert len(set(names)) == len(names) and any(n.startswith("pillow_adaptive") for n in names)
    rng = np.random.default_rng(20261020)
    img = P.TIE_VALUES[rng.integers(0, len(P.TIE_VALUES), (65, 33, 1))]
    census = P.paeth_tie_census(img)
    assert all(v > 0 for v in census.values()), census


def test_inflate_then_unfilter_gives_the_bytes_of_the_decoder(decoded):
    seen = set()
    for name, (rows, d, ref) in decoded.items():
        h, w = ref.shape[:2]
        assert (d.height, d.width, d.reserved) == (h, w, 0) and d.channels == P.CHANNELS[d.color_type], name
        assert d.rows_bytes() == rows.size == h * (1 + w * d.channels), name
        assert (d.palette_entries > 0) == (d.color_type == 3), name
        pal = np.ctypeslib.as_array(d.palette).reshape(256, 3)
        assert not pal[d.palette_entries:].any(), name
        got, over = P.unfilter_host(rows, d)
        assert not over and np.array_equal(got, ref), name
        seen.add(d.color_type)
    assert seen == {0, 2, 3, 4, 6}
    assert C.sizeof(L.sd_png_frame_desc) == 24 + 768


def test_palette_index_beyond_the_palette_is_the_one_exception():
    buf, y, x = P.overflow_case()
    assert P.host_decode(buf)[0] == L.SD_ERR_INVALID
    st, rows, d = P.inflate_rows(buf)
    assert st == L.SD_OK and d.palette_entries == 5
    _, over = P.unfilter_host(rows, d)
    assert over


def test_damaged_files_are_refused_alike():
    lib = L.load()
    for name, buf in P.damaged():
        st_dec, _ = P.host_decode(buf)
        if st_dec == L.SD_OK:                            # the size query passed: the full decode decides
            st_dec = P.host_decode(buf)[0]
        d = L.sd_png_frame_desc()
        st_q = lib.sd_png_inflate_rows(buf, len(buf), None, 0, C.byref(d))
        hh, ww = C.c_int(), C.c_int()
        assert st_q == lib.sd_png_decode_bgr(buf, len(buf), None, 0, C.byref(hh), C.byref(ww)), name
        if st_q == L.SD_OK:
            rows = np.zeros(d.rows_bytes(), np.uint8)
            out = np.zeros(d.height * d.width * 3, np.uint8)
            st_full = lib.sd_png_inflate_rows(buf, len(buf), rows.ctypes.data_as(C.c_void_p), rows.size, C.byref(d))
            st_ref = lib.sd_png_decode_bgr(buf, len(buf), out.ctypes.data_as(C.c_void_p), out.size, None, None)
            assert st_full == st_ref == L.SD_ERR_INVALID, (name, st_full, st_ref)
        else:
            assert st_q == L.SD_ERR_INVALID, name


def test_short_capacity_writes_nothing_and_null_rows_fill_the_descriptor():
    name, buf = P.cases()[7 * 5 + 1]                      # 130 x 257 RGB
    st, rows, d = P.inflate_rows(buf)
    assert st == L.SD_OK
    st, short, _ = P.inflate_rows(buf, capacity=d.rows_bytes() - 1, fill=0xA5)
    assert st == L.SD_ERR_INVALID and (short == 0xA5).all()
    st, exact, _ = P.inflate_rows(buf, capacity=d.rows_bytes(), fill=0xA5)
    assert st == L.SD_OK and np.array_equal(exact, rows)


def test_batch_form_statuses(tmp_path):
    """sd_inflate_files_png beside sd_decode_files_bgr: wrong size and refused PNGs are SD_ERR_INVALID on both, a file that is not a PNG is
    SD_ERR_FORMAT (nothing written), a missing file SD_ERR_NOTFOUND"""
    lib = L.load()
    by = dict(P.cases())
    files = [("a.png", by["mix_65x5_ct2"]), ("b.png", by["mix_65x5_ct3"]), ("c.png", by["mix_64x5_ct2"]), ("d.jpg", b"\xff\xd8\xff\xe0" + bytes(32)),
             ("e.png", dict(P.damaged())["filter5_row35"]), ("f.png", by["mix_65x5_ct6"])]
    paths = []
    for n, b in files:
        (tmp_path / n).write_bytes(b)
        paths.append(str(tmp_path / n))
    paths.append(str(tmp_path / "missing.png"))
    n = len(paths)
    arr = (C.c_char_p * n)(*[p.encode() for p in paths])
    stride = -(-(65 * (1 + 5 * 4)) // 16) * 16
    rows = np.full((n, stride), 0xA5, np.uint8)
    descs = (L.sd_png_frame_desc * n)()
    status = (C.c_int * n)()
    st = lib.sd_inflate_files_png(arr, n, 65, 5, rows.ctypes.data_as(C.c_void_p), stride, descs, 3, status)
    assert st == L.SD_ERR_INVALID
    assert list(status) == [L.SD_OK, L.SD_OK, L.SD_ERR_INVALID, L.SD_ERR_FORMAT, L.SD_ERR_INVALID, L.SD_OK, L.SD_ERR_NOTFOUND]
    assert (rows[2] == 0xA5).all() and (rows[3] == 0xA5).all() and (rows[6] == 0xA5).all()
    bgr = np.zeros((n, 65 * 5 * 3), np.uint8)
    status2 = (C.c_int * n)()
    lib.sd_decode_files_bgr(arr, n, 65, 5, bgr.ctypes.data_as(C.c_void_p), 65 * 5 * 3, 3, status2)
    for i in (0, 1, 2, 4, 5, 6):
        assert status[i] == status2[i], i
    for i in (0, 1, 5):
        got, _ = P.unfilter_host(rows[i, :descs[i].rows_bytes()].copy(), descs[i])
        assert np.array_equal(got.ravel(), bgr[i])
    # only SD_OK and SD_ERR_FORMAT statuses: SD_OK
    ok = [0, 1, 3, 5]
    arr2 = (C.c_char_p * 4)(*[paths[i].encode() for i in ok])
    assert lib.sd_inflate_files_png(arr2, 4, 65, 5, rows.ctypes.data_as(C.c_void_p), stride, descs, 2, status) == L.SD_OK
    # a stride that cannot hold a frame is refused for that frame before anything is written
    rows[:] = 0xA5
    assert lib.sd_inflate_files_png(arr2, 4, 65, 5, rows.ctypes.data_as(C.c_void_p), 65 * (1 + 5 * 3), descs, 2, status) == L.SD_ERR_INVALID
    assert list(status)[:4] == [L.SD_OK, L.SD_OK, L.SD_ERR_FORMAT, L.SD_ERR_INVALID]


@pytest.mark.parametrize("waves", [1, P.consts()["kWaves"]])
def test_the_kernels_schedule_restated_reproduces_the_host_bytes(decoded, waves):
    for name, (rows, d, ref) in decoded.items():
        samples = P.schedule_decode(rows, d.height, d.width, d.channels, waves)
        got, over = P.samples_to_bgr(samples, d)
        assert not over and np.array_equal(got, ref), (name, waves)


@pytest.mark.parametrize("mistake", P.MISTAKES)
def test_seeded_mistakes_change_compared_bytes(decoded, mistake):
    """each mistake, planted in the restated schedule, changes at least one byte of a case the clean schedule reproduces"""
    k = P.consts()
    pick = {"drop_band_carry": ("mix_65x5_ct2", "uniform_ft2_65x5_ct0"), "paeth_tie_order": ("paeth_ties_65x33_ct0", "paeth_ties_65x33_ct2"),
            "average_8bit": ("average_bright_65x33_ct2",), "gray_alpha_bpp1": ("mix_63x5_ct4", "average_bright_70x9_ct4"),
            "first_pixel_like_others": (f"pass_{k['kPassRows'] + 1}x9_ct2", "uniform_ft4_65x5_ct2")}[mistake]
    changed = 0
    for name in pick:
        rows, d, ref = decoded[name]
        for waves in (1, k["kWaves"]):
            try:
                samples = P.schedule_decode(rows, d.height, d.width, d.channels, waves, mistake=mistake)
            except AssertionError:
                continue
            changed += int((P.samples_to_bgr(samples, d)[0] != ref).sum())
    assert changed > 0, mistake
