"""CPU: the JPEG sync route as its host statement -- the plan (sd_jpeg_sync_plan: a header parse and a byte walk that writes the clean
stream) followed by sd_jpeg_sync_decode_host, the passes of semantic_depth_amd/csrc/jpeg_sync.hpp with the kernels' lanes run in a loop --
against the existing host decoder sd_jpeg_decode_coefficients, element for element, at piece lengths 32 and 128."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as graft
import jpeg_cases as J
import jpeg_entropy_cases as E
import jpeg_sync_cases as S
from semantic_depth_amd import _lib as L


@pytest.fixture(scope="module", autouse=True)
def _built():
    graft.build()


@pytest.mark.parametrize("piece", S.PIECES)
def test_intact_files_equal_the_host_decoder_and_none_is_flagged(piece):
    """files with DRI (the entropy route's), the same recipes without DRI, a gray frame, five workgroups of noise, a scan shorter than a
    piece, a last token completed by zero bits: one by one and all in one call"""
    PILImage = pytest.importorskip("PIL.Image")
    files = S.intact_files(PILImage)
    assert len(files) == 5 + 9 + 11 + 1
    plans = [S.Plan(buf, piece) for _, buf in files]
    for (name, _), plan in zip(files, plans):
        assert plan.eligible, (name, plan.status)
        st, coef, status = S.Batch([plan]).host()
        assert st == L.SD_OK, name
        S.check_frame(name, plan, coef[0], status[0])
    by_name = {name: p.frame for (name, _), p in zip(files, plans)}
    assert by_name["pil_136x136_blocks1_444"].n_intervals == 289 and by_name["plain_136x136_444"].n_intervals == 1
    assert by_name["plain_136x136_444"].restart_interval == 17 * 17
    if piece == 32:
        assert by_name["plain_q100_noise_422_96x160"].n_pieces > 4 * S.GROUP
    else:
        assert by_name["plain_16x16_q30"].n_pieces == 1
    st, coef, status = S.Batch(plans).host()                   # mixed sizes, samplings, tables and interval counts in one call
    assert st == L.SD_OK
    for i, (name, _) in enumerate(files):
        S.check_frame(name, plans[i], coef[i], status[i])


def test_the_clean_stream_is_the_scan_without_stuffing_and_markers():
    name, buf = E.own_files()[3]                               # dozens of stuffed bytes, three intervals
    plan = S.Plan(buf, 64)
    scan = buf[plan.frame.scan_begin:plan.frame.scan_end]
    want = scan.replace(b"\xff\x00", b"\xff")
    for k in range(8):
        want = want.replace(bytes([0xFF, 0xD0 + k]), b"")
    assert plan.eligible and plan.clean == want and plan.frame.clean_bytes == len(want) < len(scan)
    ivs = [plan.intervals[i] for i in range(plan.frame.n_intervals)]
    assert ivs[0].begin == 0 and ivs[-1].end == len(want) and all(a.end == b.begin for a, b in zip(ivs, ivs[1:]))
    pieces = [max(1, -(-(v.end - v.begin) // 64)) for v in ivs]
    assert [v.first_piece for v in ivs] == [sum(pieces[:i]) for i in range(len(ivs))] and plan.frame.n_pieces == sum(pieces)


def _assert_ineligible(name, buf):
    plan = S.Plan(buf, 32)
    assert plan.status == L.SD_OK and plan.frame.eligible == 0, (name, plan.status, plan.frame.eligible)
    st, coef, status = S.Batch([plan]).host()
    assert st == L.SD_OK and status[0] == 0 and (coef == S.FILL16).all(), name


def test_ineligible_files_are_reported_and_left_alone():
    PILImage = pytest.importorskip("PIL.Image")
    _assert_ineligible("scan_script", J.scan_script_file()[1])           # multi-scan
    n = 0
    for name, buf in J.pil_matrix(PILImage):
        if name.endswith("_prog"):
            _assert_ineligible(name, buf)
            n += 1
        else:
            assert S.Plan(buf, 32).eligible, name                        # baseline and optimised files without DRI are this route's
    assert n > 80
    name, good = E.own_files()[4]
    _assert_ineligible("last byte cut", good[:-1])
    at = good.index(b"\xff\xd3", E.scan_start(good))
    _assert_ineligible("RST renumbered", good[:at + 1] + b"\xd4" + good[at + 2:])
    plain = S.dri_less_files(PILImage)[0][1]
    mid = (E.scan_start(plain) + len(plain)) // 2
    _assert_ineligible("a restart marker in a scan without DRI", plain[:mid] + b"\xff\xd0" + plain[mid:])
    fr = L.sd_jpeg_sync_frame()
    tables, iv = (L.sd_jpeg_huff_table * 8)(), (L.sd_jpeg_sync_interval * 4)()
    for bad_piece in (0, 16, 48, 2048):
        fr.eligible = 7
        assert L.load().sd_jpeg_sync_plan(good, len(good), bad_piece, C.byref(L.sd_jpeg_frame_desc()), C.byref(fr), tables, iv, 4, None, 0) == L.SD_ERR_INVALID
        assert fr.eligible == 0
    assert S.Plan(b"\x89PNG\r\n\x1a\n" + bytes(64), 32).status == L.SD_ERR_FORMAT
    small = S.Plan(good, 32, cap=10)                           # not enough room for the ranges: the count the file needs
    assert small.status == L.SD_ERR_INVALID and small.frame.eligible == 0 and small.frame.n_intervals == 11


@pytest.mark.parametrize("piece", S.PIECES)
def test_damaged_scans_agree_with_the_host_decoder(piece):
    """900 mutated scans (450 with DRI, 450 without).  A file the host decoder refuses is flagged; a file with status 0 equals the host
    decoder's result; and not every host-accepted file may be flagged.  The counts of host-accepted files flagged 5 or 6 are printed
    (DESIGN.md records them).  With this generator's draw order the host decoder alone accepts 693 of the eligible files and refuses
    147; the floors are 85 % of those counts (589, 125) and keep the test from passing by skipping."""
    PILImage = pytest.importorskip("PIL.Image")
    accepted_ok = refused = 0
    flagged = {}
    for f in S.damaged_scans(PILImage):
        plan = S.Plan(f, piece)
        if not plan.eligible:
            continue
        st_host, ref, _ = J.coef_decode(f)
        st, coef, status = S.Batch([plan]).host()
        assert st == L.SD_OK
        if st_host != L.SD_OK:
            assert status[0] != 0
            refused += 1
        elif status[0] == 0:
            S.check_frame("accepted", plan, coef[0], status[0])
            accepted_ok += 1
        else:
            flagged[int(status[0])] = flagged.get(int(status[0]), 0) + 1
    print("piece", piece, "host-accepted and status 0:", accepted_ok, "host-accepted but flagged {code: files}:", flagged, "host-refused:", refused)
    assert set(flagged) <= {L.SD_JPEG_SYNC_NOT_SYNCHRONISED, L.SD_JPEG_SYNC_BITS_RAN_OUT}, flagged
    assert accepted_ok > 0
    assert accepted_ok + sum(flagged.values()) >= 589 and refused >= 125, (accepted_ok, flagged, refused)


def test_a_stream_that_never_synchronises_is_flagged_not_decoded_wrongly():
    """every token one byte, a DC-like byte at every multiple of 64: a late starter stays 62 zigzag positions off for ever.  At 32-byte
    pieces the stream is longer than three workgroups: the second workgroup is put right from the first one's end, the third is
    started from the second's SPECULATIVE end and stays wrong -- the verification sees it.  At 128-byte pieces the stream is one
    workgroup, whose rounds carry the true state to the end."""
    buf = S.never_synchronising()
    st, ref, desc = J.coef_decode(buf)
    assert st == L.SD_OK and int(np.abs(ref).sum()) == 399 * 63
    plan = S.Plan(buf, 32)
    assert plan.eligible and plan.frame.n_pieces == 799 > 3 * S.GROUP
    st, coef, status = S.Batch([plan]).host()
    assert st == L.SD_OK and status[0] == L.SD_JPEG_SYNC_NOT_SYNCHRONISED
    plan = S.Plan(buf, 128)
    assert plan.frame.n_pieces == 200
    st, coef, status = S.Batch([plan]).host()
    assert st == L.SD_OK
    S.check_frame("one workgroup", plan, coef[0], status[0])


def _small_files(PILImage):
    files = dict(S.intact_files(PILImage))
    names = ["own_176x16_q80", "pil_50x70_blocks3_ss2", "pil_gray_33x41_rows1", "plain_50x70_ss0", "plain_50x70_ss1", "plain_50x70_ss2",
             "plain_50x70_ss2_opt", "plain_q100_noise_422_40x56", "crafted_last_token_past_the_end"]
    return [(n, files[n]) for n in names]


def test_the_restatement_is_the_statement_and_every_seeded_mistake_is_caught():
    """the Python restatement (jpeg_sync_cases.Model) gives the statement's status words and coefficients on nine small files at
    32-byte pieces; with each of the three mistakes it no longer gives the host decoder's result on at least one of them"""
    PILImage = pytest.importorskip("PIL.Image")
    files = _small_files(PILImage)
    plans = [S.Plan(buf, 32) for _, buf in files]
    for (name, buf), plan in zip(files, plans):
        st, coef, status = S.Batch([plan]).host()
        got_status, got = S.Model(plan).decode()
        assert got_status == status[0] == 0, name
        assert np.array_equal(got, coef[0, :len(got)]), name
    for mistake in S.MISTAKES:
        caught = []
        for (name, buf), plan in zip(files, plans):
            ref = J.coef_decode(buf)[1]
            got_status, got = S.Model(plan, mistake).decode()
            if got_status != 0 or not np.array_equal(got, ref[:len(got)]):
                caught.append((name, got_status))
        print(mistake, "caught on", caught)
        assert caught, mistake


def test_argument_checks():
    """damaged ranges, piece indices, strides, piece lengths, records and tables are SD_ERR_INVALID, and the output keeps its fill"""
    PILImage = pytest.importorskip("PIL.Image")
    files = E.own_files() + S.dri_less_files(PILImage)[:3]
    batch = S.Batch([S.Plan(b, 64) for _, b in files])
    big = max(p.desc.coef_elems() for p in batch.plans)
    overs = []
    iv = batch.copies()[2]
    iv[4 * batch.interval_stride + 10].end = batch.frames[4].clean_bytes + 1
    overs.append(dict(intervals=iv))
    iv = batch.copies()[2]
    iv[4 * batch.interval_stride + 3].first_piece += 1
    overs.append(dict(intervals=iv))
    iv = batch.copies()[2]
    iv[4 * batch.interval_stride + 2].begin, iv[4 * batch.interval_stride + 2].end = 9, 8
    overs.append(dict(intervals=iv))
    for field, delta in (("mcus_x", 1), ("n_pieces", 1), ("clean_bytes", 1 << 20), ("restart_interval", -1), ("subseq_bytes", 64)):
        fr = batch.copies()[1]
        setattr(fr[5], field, getattr(fr[5], field) + delta)
        overs.append(dict(frames=fr))
    fr = batch.copies()[1]
    fr[2].comp_ac[0] = 4
    overs.append(dict(frames=fr))
    tb = batch.copies()[3]
    tb[3 * 8 + 4 + batch.frames[3].comp_ac[0]].look[5] = 12 << 8         # a look-ahead entry that claims a 12-bit code
    overs.append(dict(tables=tb))
    tb = batch.copies()[3]
    tb[3 * 8 + batch.frames[3].comp_dc[0]].valptr[11], tb[3 * 8 + batch.frames[3].comp_dc[0]].maxcode[11] = 250, 40
    tb[3 * 8 + batch.frames[3].comp_dc[0]].mincode[11] = 0
    overs.append(dict(tables=tb))
    overs += [dict(coef_stride_bytes=(big - 64) * 2), dict(interval_stride=batch.interval_stride - 1), dict(byte_stride=batch.byte_stride - 16),
              dict(subseq_bytes=128), dict(subseq_bytes=48), dict(byte_stride=1 << 28)]
    for over in overs:
        st, coef, status = batch.host(**over)
        assert st == L.SD_ERR_INVALID, over.keys()
        assert (coef == S.FILL16).all() and (status == -1).all(), over.keys()
    st, coef, status = batch.host()
    assert st == L.SD_OK and (status == 0).all()
