"""CPU: the split JPEG route's host side.  sd_jpeg_decode_coefficients (Huffman decoding to quantised coefficients) followed by
sd_jpeg_reconstruct_bgr_host (the back half, the CPU statement of the device kernels) must write the bytes of the one-call decoder
sd_jpeg_decode_bgr, accept and refuse exactly the files it does, and honour its capacity checks.  The file sets are tests/jpeg_cases.py."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import __graft_entry__ as graft
import jpeg_cases as J
from semantic_depth_amd import _lib as L
from semantic_depth_amd import frame_io, outputs


@pytest.fixture(scope="module", autouse=True)
def built():
    graft.build()


def _check_split_equals_one_call(name, buf, want=None):
    st_q, st, ref = J.host_decode(buf)
    assert st_q == L.SD_OK and st == L.SD_OK, name
    if want is not None:
        assert ref.shape == want.shape and np.array_equal(ref, want), name
    st, coef, d = J.coef_decode(buf)
    assert st == L.SD_OK, name
    assert d.oriented_size() == ref.shape[:2], name
    st, got = J.host_reconstruct(coef, d)
    assert st == L.SD_OK and np.array_equal(got, ref), name
    return d


def test_struct_layout_matches_the_header():
    """include/semdepth.h: eight int32, two int32[3], int64[3] at an 8-byte boundary, uint16[3][64]"""
    assert C.sizeof(L.sd_jpeg_frame_desc) == 8 * 4 + 2 * 12 + 3 * 8 + 3 * 64 * 2 == 464
    assert L.sd_jpeg_frame_desc.coef_offset.offset == 56 and L.sd_jpeg_frame_desc.qt.offset == 80
    assert L.SD_ERR_FORMAT == -5 and L.load().sd_status_string(L.SD_ERR_FORMAT) == b"not a JPEG file"


def test_split_route_on_the_committed_golden_vectors():
    files = J.golden_files()
    assert len(files) >= 6
    seen = set()
    for name, buf, want in files:
        d = _check_split_equals_one_call(name, buf, want)
        seen.add((d.ncomp, d.hmax, d.vmax))
        for o in range(2, 9):                              # the same frames under every EXIF orientation (no Pillow needed)
            assert _check_split_equals_one_call(f"{name} orientation {o}", J.with_orientation(buf, o)).orientation == o
    assert {(3, 1, 1), (3, 2, 1), (3, 2, 2), (1, 1, 1)} <= seen         # 4:4:4, 4:2:2, 4:2:0, gray


def test_split_route_on_the_references_scan_script():
    ref, buf = J.scan_script_file()
    _check_split_equals_one_call("scan_script", buf)
    st, coef, d = J.coef_decode(buf)
    st, got = J.host_reconstruct(coef, d)
    assert hashlib.sha256(got.tobytes()).hexdigest() == ref["bgr_sha256"]


def test_split_route_on_the_pillow_matrix():
    PILImage = pytest.importorskip("PIL.Image")
    files = J.pil_matrix(PILImage) + J.pil_orientations(PILImage) + J.pil_orientations(PILImage, 23, 37, 2) + J.pil_orientations(PILImage, 9, 1, 1)
    assert len(files) > 250
    seen = set()
    for name, buf in files:
        d = _check_split_equals_one_call(name, buf)
        cw = (d.width + d.hmax - 1) // d.hmax
        seen.add((d.ncomp, d.hmax, d.vmax, d.orientation, cw == 1))
    assert {o for (_, _, _, o, _) in seen} == set(range(1, 9))
    assert (3, 2, 1, 1, True) in seen and (3, 2, 2, 1, True) in seen     # the cw == 1 branches of both fancy filters


def test_header_only_size_is_what_the_full_call_fills_and_capacity_is_checked_first():
    GUARD = 64
    for name, buf, _ in J.golden_files():
        st, d0 = J.coef_header(buf)
        assert st == L.SD_OK
        n = d0.coef_elems()
        assert n == d0.coef_offset[d0.ncomp - 1] + 64 * d0.blocks_w[d0.ncomp - 1] * d0.blocks_h[d0.ncomp - 1]
        # exactly n elements are written: the buffer is pre-filled with a value no coefficient of these files takes, the guard stays
        raw = np.full(n + GUARD, 0x5A5A, np.int16)
        d = L.sd_jpeg_frame_desc()
        st = L.load().sd_jpeg_decode_coefficients(buf, len(buf), raw.ctypes.data_as(C.c_void_p), n * 2, C.byref(d))
        assert st == L.SD_OK and (raw[n:] == 0x5A5A).all() and not (raw[:n] == 0x5A5A).any(), name
        assert bytes(d)[:80] == bytes(d0)[:80], name                        # the geometry of the header-only call
        # one byte short: refused, nothing written
        raw = np.full(n + GUARD, 0x5A5A, np.int16)
        st = L.load().sd_jpeg_decode_coefficients(buf, len(buf), raw.ctypes.data_as(C.c_void_p), n * 2 - 1, C.byref(d))
        assert st == L.SD_ERR_INVALID and (raw == 0x5A5A).all(), name
        # the reconstruction checks its output capacity and its descriptor
        st, coef, d = J.coef_decode(buf)
        h, w = d.oriented_size()
        out = np.full(h * w * 3 + GUARD, 0xA5, np.uint8)
        lib = L.load()
        assert lib.sd_jpeg_reconstruct_bgr_host(coef.ctypes.data_as(C.c_void_p), C.byref(d), out.ctypes.data_as(C.c_void_p), h * w * 3 - 1) == L.SD_ERR_INVALID
        assert (out == 0xA5).all()
        bad = L.sd_jpeg_frame_desc.from_buffer_copy(bytes(d))
        bad.blocks_w[0] += 1
        assert lib.sd_jpeg_reconstruct_bgr_host(coef.ctypes.data_as(C.c_void_p), C.byref(bad), out.ctypes.data_as(C.c_void_p), h * w * 3) == L.SD_ERR_INVALID
        assert (out == 0xA5).all()


def _same_verdict(buf, name):
    """both routes on one (possibly hostile) file: the same verdict from the header calls and from the decodes; equal pixels when accepted"""
    GUARD = 64
    lib = L.load()
    h, w = C.c_int(0), C.c_int(0)
    st_q = lib.sd_jpeg_decode_bgr(buf, len(buf), None, 0, C.byref(h), C.byref(w))
    st_cq, d0 = J.coef_header(buf)
    assert (st_q == L.SD_OK) == (st_cq == L.SD_OK) and st_q == st_cq, name
    if st_q != L.SD_OK:
        # (the full calls refuse too, whatever the capacity)
        out = np.full(4096 + GUARD, 0xA5, np.uint8)
        assert lib.sd_jpeg_decode_bgr(buf, len(buf), out.ctypes.data_as(C.c_void_p), 4096, None, None) != L.SD_OK
        d = L.sd_jpeg_frame_desc()
        assert lib.sd_jpeg_decode_coefficients(buf, len(buf), out.ctypes.data_as(C.c_void_p), 4096, C.byref(d)) != L.SD_OK
        assert (out[4096:] == 0xA5).all(), name
        return False
    assert d0.oriented_size() == (h.value, w.value), name
    need = h.value * w.value * 3
    need_c = d0.coef_elems() * 2
    if need > (1 << 22):                                   # a mutated header announces gigapixels: both refuse on capacity, nothing written
        out = np.full((1 << 16) + GUARD, 0xA5, np.uint8)
        assert lib.sd_jpeg_decode_bgr(buf, len(buf), out.ctypes.data_as(C.c_void_p), 1 << 16, None, None) != L.SD_OK
        d = L.sd_jpeg_frame_desc()
        assert lib.sd_jpeg_decode_coefficients(buf, len(buf), out.ctypes.data_as(C.c_void_p), 1 << 16, C.byref(d)) != L.SD_OK
        assert (out == 0xA5).all(), name
        return False
    out = np.full(need + GUARD, 0xA5, np.uint8)
    st = lib.sd_jpeg_decode_bgr(buf, len(buf), out.ctypes.data_as(C.c_void_p), need, None, None)
    raw = np.full(need_c + GUARD, 0xA5, np.uint8)
    d = L.sd_jpeg_frame_desc()
    st_c = lib.sd_jpeg_decode_coefficients(buf, len(buf), raw.ctypes.data_as(C.c_void_p), need_c, C.byref(d))
    assert (out[need:] == 0xA5).all() and (raw[need_c:] == 0xA5).all(), name
    assert st == st_c, (name, st, st_c)
    if st != L.SD_OK:
        return False
    got = np.empty(need, np.uint8)
    assert lib.sd_jpeg_reconstruct_bgr_host(raw.ctypes.data_as(C.c_void_p), C.byref(d), got.ctypes.data_as(C.c_void_p), need) == L.SD_OK
    assert np.array_equal(got, out[:need]), name
    return True


def test_crafted_hostile_files_get_the_same_verdict_from_both_routes():
    verdicts = {name: _same_verdict(f, name) for name, f in J.crafted_jpegs().items()}
    for name in J.ACCEPTED_CRAFTED:                         # (accepted by both, with equal pixels: _same_verdict compared them)
        assert verdicts.pop(name) is True, name
    assert not any(verdicts.values()), verdicts


def test_unscanned_components_of_a_sequential_file_keep_the_one_call_decoders_samples():
    """a sequential file need not scan every component; the one-call decoder leaves such a plane at sample 0, and the split route must
    hand on coefficients that transform to exactly that.  8 x 8, only Cb scanned (all-zero coefficients -> 128): Y = 0, Cb = 128, Cr = 0, so
    B = 0 + 0, G = 0 + ((32768 + 46802 * 128) >> 16) = 91, R = clamp(0 - 179) = 0 from both routes, not the gray (128, 128, 128) of three
    transformed zero blocks."""
    files = J.accepted_crafted_jpegs()
    buf = files["three_components_one_scanned"]
    _, st, ref = J.host_decode(buf)
    assert st == L.SD_OK and (ref == np.array([0, 91, 0], np.uint8)).all()
    for name, f in files.items():
        _check_split_equals_one_call(name, f)


def test_mutated_files_get_the_same_verdict_from_both_routes():
    PILImage = pytest.importorskip("PIL.Image")
    files = J.mutated_jpegs(PILImage)
    ok = sum(_same_verdict(f, f"mutation {i}") for i, f in enumerate(files))
    assert ok > 30 and len(files) - ok > 30, (ok, len(files))


def test_batch_reader_reports_per_file(tmp_path):
    """sd_decode_files_jpeg_coef: a missing file, a frame of another size and a PNG are reported per file; the frames around them are
    decoded; a stride that cannot hold a frame refuses that frame"""
    golden = {name: (buf, want) for name, buf, want in J.golden_files()}
    names = ["synthetic_2", "synthetic_2_rot180"]          # one size after the orientation
    other = "synthetic_3"
    golden["synthetic_2_rot180"] = (J.with_orientation(golden["synthetic_2"][0], 3), golden["synthetic_2"][1][::-1, ::-1])
    h, w = golden[names[0]][1].shape[:2]
    paths = {}
    for n in names + [other]:
        paths[n] = str(tmp_path / (n + ".jpg"))
        open(paths[n], "wb").write(golden[n][0])
    png = outputs.write_png(str(tmp_path / "frame.png"), np.zeros((h, w, 3), np.uint8))
    lst = [paths[names[0]], str(tmp_path / "missing.jpg"), png, paths[other], paths[names[1]]]
    stride = frame_io.FrameFeeder.coef_stride_bytes(h, w)
    coef = np.zeros((5, stride // 2), np.int16)
    descs = (L.sd_jpeg_frame_desc * 5)()
    status = (C.c_int * 5)()
    arr = (C.c_char_p * 5)(*[p.encode() for p in lst])
    lib = L.load()
    st = lib.sd_decode_files_jpeg_coef(arr, 5, h, w, coef.ctypes.data_as(C.c_void_p), stride, descs, 3, status)
    assert st == L.SD_ERR_INVALID and list(status) == [0, L.SD_ERR_NOTFOUND, L.SD_ERR_FORMAT, L.SD_ERR_INVALID, 0]
    for i, n in ((0, names[0]), (4, names[1])):
        s2, got = J.host_reconstruct(coef[i], descs[i])
        assert s2 == L.SD_OK and np.array_equal(got, golden[n][1]), n
    # only good JPEGs and a PNG: SD_OK, the PNG is left to the BGR reader
    arr3 = (C.c_char_p * 3)(*[p.encode() for p in (lst[0], png, lst[4])])
    assert lib.sd_decode_files_jpeg_coef(arr3, 3, h, w, coef.ctypes.data_as(C.c_void_p), stride, descs, 2, status) == L.SD_OK
    assert list(status)[:3] == [0, L.SD_ERR_FORMAT, 0]
    # a stride below the frame's coefficients
    small = (descs[0].coef_elems() * 2 - 16) // 16 * 16
    assert lib.sd_decode_files_jpeg_coef(arr3, 1, h, w, coef.ctypes.data_as(C.c_void_p), small, descs, 1, status) == L.SD_ERR_INVALID
    assert status[0] == L.SD_ERR_INVALID


def test_feeder_arguments():
    with pytest.raises(ValueError, match="device='cpu'"):
        frame_io.FrameFeeder([], batch=2, device="cpu", jpeg="device")
    with pytest.raises(ValueError, match="needs engine="):
        frame_io.FrameFeeder([], batch=2, device="cuda", jpeg="device")
    with pytest.raises(ValueError, match="jpeg must be"):
        frame_io.FrameFeeder([], batch=2, device="cpu", jpeg="gpu")
    # the worst-case stride covers every sampling the reader takes, in both orientations
    for name, buf, want in J.golden_files():
        st, d = J.coef_header(buf)
        h, w = d.oriented_size()
        assert d.coef_elems() * 2 <= frame_io.FrameFeeder.coef_stride_bytes(h, w) == frame_io.FrameFeeder.coef_stride_bytes(w, h)
