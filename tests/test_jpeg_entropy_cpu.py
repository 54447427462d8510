"""CPU: the JPEG entropy route as its host statement -- the plan (sd_jpeg_entropy_plan: a header parse and a byte scan for the restart
markers) followed by sd_jpeg_entropy_decode_host, a plain loop over the intervals calling the function the kernel calls
(semantic_depth_amd/csrc/jpeg_entropy.hpp) -- against the existing host decoder sd_jpeg_decode_coefficients, element for element."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as graft
import jpeg_cases as J
import jpeg_entropy_cases as E
from semantic_depth_amd import _lib as L


@pytest.fixture(scope="module", autouse=True)
def _built():
    graft.build()


def _run_eligible(files):
    for name, buf in files:
        plan = E.Plan(buf)
        assert plan.eligible, (name, plan.status)
        st, coef, status = E.Batch([plan]).host()
        assert st == L.SD_OK, name
        E.check_frame(name, plan, coef[0], status[0])
    plans = [E.Plan(buf) for _, buf in files]                  # and all of them in one call: mixed sizes, samplings and tables
    st, coef, status = E.Batch(plans).host()
    assert st == L.SD_OK
    for i, (name, _) in enumerate(files):
        E.check_frame(name, plans[i], coef[i], status[i])


def test_eligible_files_of_the_projects_encoder():
    files = E.own_files()
    assert [E.Plan(b).frame.n_intervals for _, b in files] == [1, 2, 3, 3, 11]
    _run_eligible(files)


def test_eligible_files_of_pillow():
    PILImage = pytest.importorskip("PIL.Image")
    files = E.pil_files(PILImage)
    assert len(files) == 9
    n = {name: E.Plan(b).frame.n_intervals for name, b in files}
    assert n["pil_136x136_blocks1_444"] == 289 and n["pil_50x70_blocks3_ss2"] == 7          # (20 MCUs of 16 x 16 in intervals of 3: a short last one)
    _run_eligible(files)


def _assert_ineligible(name, buf):
    plan = E.Plan(buf)
    assert plan.status == L.SD_OK and plan.frame.eligible == 0, (name, plan.status, plan.frame.eligible)
    st, coef, status = E.Batch([plan]).host()
    assert st == L.SD_OK and status[0] == 0 and (coef == E.FILL16).all(), name


def test_ineligible_files_are_reported_and_left_alone():
    for name, buf in J.accepted_crafted_jpegs().items():
        _assert_ineligible(name, buf)
    _assert_ineligible("scan_script", J.scan_script_file()[1])
    name, good = E.own_files()[4]
    assert E.Plan(good).eligible
    _assert_ineligible("last byte cut", good[:-1])
    at = good.index(b"\xff\xd3", E.scan_start(good))
    _assert_ineligible("RST renumbered", good[:at + 1] + b"\xd4" + good[at + 2:])
    _assert_ineligible("fill bytes before a marker", good[:at] + b"\xff\xff" + good[at:])
    # a file that ends in an SOS segment of length 2: the segment's payload begins at the end of the buffer (exact-size copy: nothing behind it)
    sos_at = E.scan_start(good) - 14
    assert good[sos_at:sos_at + 2] == b"\xff\xda"
    _assert_ineligible("empty SOS at the end of the file", good[:sos_at] + b"\xff\xda\x00\x02")
    fr = L.sd_jpeg_entropy_frame()
    fr.eligible = 7
    tables, iv = (L.sd_jpeg_huff_table * 8)(), (L.sd_jpeg_interval * 4)()
    assert L.load().sd_jpeg_entropy_plan(b"BM" + bytes(8), 10, C.byref(L.sd_jpeg_frame_desc()), C.byref(fr), tables, iv, 4) == L.SD_ERR_FORMAT and fr.eligible == 0
    fr.eligible = 7
    assert L.load().sd_jpeg_entropy_plan(good, len(good), None, C.byref(fr), tables, iv, 4) == L.SD_ERR_INVALID and fr.eligible == 0
    for buf in (b"\x89PNG\r\n\x1a\n" + bytes(64), b"BM" + bytes(64), b"\xff"):
        assert E.Plan(buf).status == L.SD_ERR_FORMAT
    # not enough room for the ranges: SD_ERR_INVALID, not eligible, and the count the file needs
    small = E.Plan(good, cap=10)
    assert small.status == L.SD_ERR_INVALID and small.frame.eligible == 0 and small.frame.n_intervals == 11


def test_ineligible_files_of_the_pillow_matrix():
    PILImage = pytest.importorskip("PIL.Image")
    n = 0
    for name, buf in J.pil_matrix(PILImage):
        if name.startswith("restart"):
            assert E.Plan(buf).eligible, name
            continue
        _assert_ineligible(name, buf)                          # progressive files and files without DRI
        n += 1
    assert n > 250


def damaged_outcomes(PILImage):
    """[(file, plan, host status, host coefficients or None)] of the damaged scans the plan still calls eligible"""
    out = []
    for f in E.damaged_scans(PILImage):
        plan = E.Plan(f)
        if not plan.eligible:
            continue
        st, ref, _ = J.coef_decode(f)
        out.append((f, plan, st, ref))
    return out


def test_damaged_scans_agree_with_the_host_decoder():
    """150 mutations per seed; for every file the plan still calls eligible the CPU statement agrees with the host decoder: equal
    coefficients and status 0 where it accepts, a non-zero status where it refuses.  With this generator's draw order the host decoder
    alone accepts 342 of the 450 files and refuses 63 among those the plan calls eligible; the floors are 85 % of those counts (290, 53)
    and keep the test from passing by skipping."""
    PILImage = pytest.importorskip("PIL.Image")
    accepted = refused = 0
    for f, plan, st_host, ref in damaged_outcomes(PILImage):
        st, coef, status = E.Batch([plan]).host()
        assert st == L.SD_OK
        if st_host == L.SD_OK:
            E.check_frame("accepted", plan, coef[0], status[0])
            accepted += 1
        else:
            assert status[0] != 0
            refused += 1
    print("eligible-and-accepted", accepted, "eligible-and-refused", refused)
    assert accepted >= 290 and refused >= 53, (accepted, refused)


def test_argument_checks():
    """an interval range that ends outside its frame's byte stride, a coefficient stride one block short and a record whose MCU counts
    disagree with its descriptor are SD_ERR_INVALID, and the output keeps its fill"""
    files = E.own_files()
    batch = E.Batch([E.Plan(b) for _, b in files])
    big = max(p.desc.coef_elems() for p in batch.plans)
    descs, frames, intervals = batch.copies()
    intervals[4 * batch.interval_stride + 10].end = batch.byte_stride + 1
    bad_frames = batch.copies()[1]
    bad_frames[1].mcus_x += 1
    bad_tables = batch.copies()[1]
    bad_tables[2].comp_ac[0] = 4
    for over in (dict(intervals=intervals), dict(coef_stride_bytes=(big - 64) * 2), dict(frames=bad_frames), dict(frames=bad_tables),
                 dict(interval_stride=batch.interval_stride - 1)):
        st, coef, status = batch.host(**over)
        assert st == L.SD_ERR_INVALID, over.keys()
        assert (coef == E.FILL16).all() and (status == -1).all(), over.keys()
    st, coef, status = batch.host()
    assert st == L.SD_OK and (status == 0).all()
