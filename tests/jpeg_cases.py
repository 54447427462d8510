"""The JPEG files the split-route tests run on (tests/test_jpeg_coefficients.py on the CPU, tests/test_gpu_jpeg_device.py on the GPU),
and the three calls they compare: the one-call host decoder (the yardstick, pinned to libjpeg-turbo by the committed goldens), the
coefficient decoder, and the host reconstruction.  The Pillow-written sets follow the recipes of tests/test_frame_io.py (size x
subsampling x quality x entropy mode, restart intervals, EXIF orientations, mutated and hand-crafted hostile files) and add widths 1 and 2
(the cw == 1 branches of the fancy upsamplers), gray frames and an Adobe RGB file."""
import base64
import ctypes as C
import io
import json
import os

import numpy as np

from semantic_depth_amd import _lib as L

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden_files():
    """[(name, file bytes, expected BGR pixels)]: the committed vectors (no Pillow needed)"""
    out = []
    for f in json.load(open(os.path.join(GOLDEN, "jpeg_golden.json")))["files"]:
        out.append((f["name"], base64.b64decode(f["jpeg_base64"]), np.asarray(f["bgr"], np.uint8).reshape(f["height"], f["width"], 3)))
    return out


def scan_script_file():
    ref = json.load(open(os.path.join(GOLDEN, "jpeg_scan_script.json")))
    return ref, open(os.path.join(GOLDEN, ref["file"]), "rb").read()


def with_orientation(buf, o):
    """the file with an APP1 Exif segment behind SOI whose IFD0 holds Orientation = o (big-endian TIFF, one SHORT entry)"""
    tiff = b"MM\x00\x2a\x00\x00\x00\x08" + b"\x00\x01" + b"\x01\x12\x00\x03\x00\x00\x00\x01" + bytes([0, o, 0, 0]) + b"\x00\x00\x00\x00"
    assert buf[:2] == b"\xff\xd8"
    return buf[:2] + _seg(0xE1, b"Exif\x00\x00" + tiff) + buf[2:]


def _img(rng, h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    a = np.stack([(yy * 3 + xx * 2) % 256, (xx * 5 + yy) % 256, (yy * yy // 7 + xx) % 256], -1).astype(np.uint8)
    return a ^ rng.integers(0, 32, a.shape, dtype=np.uint8)


MATRIX_SIZES = [(16, 16), (17, 23), (64, 48), (8, 9), (57, 130), (5, 1), (9, 2), (1, 7), (33, 2), (2, 1)]


def pil_matrix(PILImage):
    """[(name, bytes)]: size x subsampling x quality x entropy mode, gray frames, restart intervals, an Adobe RGB file"""
    rng = np.random.default_rng(5)
    out = []
    for (h, w) in MATRIX_SIZES:
        for ss in (0, 1, 2):
            for q in (35, 90, 100):
                for tag, kw in (("base", {}), ("opt", {"optimize": True}), ("prog", {"progressive": True})):
                    b = io.BytesIO()
                    try:
                        PILImage.fromarray(_img(rng, h, w)).save(b, "JPEG", quality=q, subsampling=ss, **kw)
                    except OSError:
                        continue            # (Pillow's encoder refuses some tiny optimised files on an in-memory stream)
                    out.append((f"{h}x{w}_ss{ss}_q{q}_{tag}", b.getvalue()))
        for tag, kw in (("base", {}), ("prog", {"progressive": True})):
            b = io.BytesIO()
            PILImage.fromarray(_img(rng, h, w)).convert("L").save(b, "JPEG", quality=80, **kw)
            out.append((f"{h}x{w}_gray_{tag}", b.getvalue()))
    for ss in (0, 2):
        b = io.BytesIO()
        PILImage.fromarray(_img(rng, 50, 70)).save(b, "JPEG", quality=80, subsampling=ss, restart_marker_blocks=3)
        assert b"\xff\xdd" in b.getvalue()
        out.append((f"restart_ss{ss}", b.getvalue()))
    b = io.BytesIO()
    try:                                    # the three components ARE R, G, B (Adobe marker, transform 0)
        PILImage.fromarray(_img(rng, 21, 35)).save(b, "JPEG", quality=90, subsampling=0, keep_rgb=True)
        out.append(("adobe_rgb", b.getvalue()))
    except (OSError, TypeError, ValueError):
        pass
    return out


def pil_orientations(PILImage, h=24, w=40, subsampling=0):
    """[(name, bytes)]: one frame under the EXIF orientations 1..8"""
    rng = np.random.default_rng(6)
    base = PILImage.fromarray(_img(rng, h, w))
    out = []
    for o in range(1, 9):
        ex = PILImage.Exif()
        ex[0x0112] = o
        b = io.BytesIO()
        base.save(b, "JPEG", quality=90, subsampling=subsampling, exif=ex)
        out.append((f"orientation{o}_ss{subsampling}", b.getvalue()))
    return out


def _seg(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def crafted_jpegs():
    """the hand-built hostile files of tests/test_frame_io.py::_crafted_jpegs, by the same recipe"""
    out = {}
    bits = [200] + [0] * 15
    out["dht_oversubscribed"] = b"\xff\xd8" + _seg(0xC4, [0x00] + bits + list(range(200)))
    bits = [0, 0, 0, 0, 0, 0, 0, 0, 255] + [0] * 7
    out["dht_len9_ok_header_only"] = b"\xff\xd8" + _seg(0xC4, [0x00] + bits + list(range(255)))
    bits = [1, 0, 0, 0, 0, 0, 0, 0, 255] + [0] * 7
    out["dht_len1_plus_len9"] = b"\xff\xd8" + _seg(0xC4, [0x00] + bits + list(range(256)))
    dqt = _seg(0xDB, [0x00] + [1] * 64)
    dht_dc = _seg(0xC4, [0x00] + [1] + [0] * 15 + [0])
    dht_ac = _seg(0xC4, [0x10] + [1] + [0] * 15 + [0])

    def sof(m, h, w):
        return _seg(m, [8] + list(h.to_bytes(2, "big")) + list(w.to_bytes(2, "big")) + [1, 1, 0x11, 0])
    sos = _seg(0xDA, [1, 1, 0x00, 0, 63, 0]) + b"\x00" * 4
    out["two_sof_reshaped"] = b"\xff\xd8" + dqt + dht_dc + dht_ac + sof(0xC0, 8, 8) + sos + sof(0xC0, 1, 64) + sos + b"\xff\xd9"
    sos_p = _seg(0xDA, [1, 1, 0x00, 0, 0, 0]) + b"\x00" * 4
    out["sof0_then_sof2"] = b"\xff\xd8" + dqt + dht_dc + dht_ac + sof(0xC0, 8, 8) + sos + sof(0xC2, 8, 8) + sos_p + b"\xff\xd9"
    out["progressive_without_dqt"] = b"\xff\xd8" + dht_dc + dht_ac + sof(0xC2, 8, 8) + sos_p + b"\xff\xd9"
    out["control_ok"] = b"\xff\xd8" + dqt + dht_dc + dht_ac + sof(0xC0, 8, 8) + sos + b"\xff\xd9"
    out.update(accepted_crafted_jpegs())
    return out


ACCEPTED_CRAFTED = ("control_ok", "three_components_one_scanned", "three_components_two_scanned_420")


def accepted_crafted_jpegs():
    """hand-built files BOTH routes accept, where their pixels must agree: sequential three-component files whose scans do not cover every
    component (a non-interleaved file cut between two scans).  The one-call decoder never transforms a block of an unscanned component,
    so its plane keeps the sample value 0 (not the 128 of a transformed all-zero block)."""
    out = {}
    dqt = _seg(0xDB, [0x00] + [1] * 64)
    dht_dc = _seg(0xC4, [0x00] + [1] + [0] * 15 + [0])
    dht_ac = _seg(0xC4, [0x10] + [1] + [0] * 15 + [0])

    def sof3(h, w, y_sampling):
        return _seg(0xC0, [8] + list(h.to_bytes(2, "big")) + list(w.to_bytes(2, "big")) + [3, 1, y_sampling, 0, 2, 0x11, 0, 3, 0x11, 0])

    def sos1(cid):
        return _seg(0xDA, [1, cid, 0x00, 0, 63, 0]) + b"\x00" * 16
    head = b"\xff\xd8" + dqt + dht_dc + dht_ac
    out["three_components_one_scanned"] = head + sof3(8, 8, 0x11) + sos1(2) + b"\xff\xd9"
    out["three_components_two_scanned_420"] = head + sof3(19, 21, 0x22) + sos1(1) + sos1(3) + b"\xff\xd9"
    return out


def mutated_jpegs(PILImage):
    """the mutation loop of tests/test_frame_io.py::test_readers_survive_mutated_files on its three JPEG seeds, by the same recipe"""
    rng = np.random.default_rng(11)
    yy, xx = np.mgrid[0:45, 0:61]
    a = (np.stack([(yy * 3 + xx) % 256, (xx * 5) % 256, (yy * xx) % 256], -1).astype(np.uint8)) ^ rng.integers(0, 32, (45, 61, 3), dtype=np.uint8)
    seeds = []
    for kw in ({"subsampling": 2}, {"subsampling": 0, "progressive": True}, {"subsampling": 1, "restart_marker_blocks": 2}):
        b = io.BytesIO()
        PILImage.fromarray(a).save(b, "JPEG", quality=80, **kw)
        seeds.append(b.getvalue())
    out = []
    for seed in seeds:
        for it in range(150):
            f = bytearray(seed)
            kind = it % 5
            if kind == 0:
                del f[int(rng.integers(0, len(f))):]
            elif kind == 1:
                for _ in range(int(rng.integers(1, 8))):
                    f[int(rng.integers(0, len(f)))] = int(rng.integers(0, 256))
            elif kind == 2:
                for _ in range(int(rng.integers(1, 48))):
                    f[int(rng.integers(0, len(f)))] ^= 1 << int(rng.integers(0, 8))
            elif kind == 3:
                p = int(rng.integers(0, len(f)))
                f[p:p + int(rng.integers(1, 48))] = b"\xff" * 8
            else:
                for _ in range(int(rng.integers(1, 6))):
                    f[int(rng.integers(0, min(len(f), 640)))] = int(rng.integers(0, 256))
            out.append(bytes(f))
    return out


# ---------------------------------------------------------------------------------------------------------------- the three calls
def host_decode(buf, cap_limit=None):
    """sd_jpeg_decode_bgr: (status of the size query, status of the decode, u8 [h,w,3] or None)"""
    lib = L.load()
    h, w = C.c_int(0), C.c_int(0)
    st_q = lib.sd_jpeg_decode_bgr(buf, len(buf), None, 0, C.byref(h), C.byref(w))
    if st_q != L.SD_OK:
        return st_q, None, None
    need = h.value * w.value * 3
    if cap_limit is not None and need > cap_limit:
        return st_q, None, None
    out = np.empty((h.value, w.value, 3), np.uint8)
    st = lib.sd_jpeg_decode_bgr(buf, len(buf), out.ctypes.data_as(C.c_void_p), out.nbytes, None, None)
    return st_q, st, out if st == L.SD_OK else None


def coef_header(buf):
    """the header-only call: (status, descriptor)"""
    d = L.sd_jpeg_frame_desc()
    return L.load().sd_jpeg_decode_coefficients(buf, len(buf), None, 0, C.byref(d)), d


def coef_decode(buf, elems=None):
    """the full call into a buffer of ``elems`` int16 (default: what the header-only call announces): (status, int16 array, descriptor)"""
    st, d = coef_header(buf)
    if st != L.SD_OK:
        return st, None, None
    n = d.coef_elems() if elems is None else elems
    coef = np.zeros(max(n, 1), np.int16)
    d2 = L.sd_jpeg_frame_desc()
    st = L.load().sd_jpeg_decode_coefficients(buf, len(buf), coef.ctypes.data_as(C.c_void_p), n * 2, C.byref(d2))
    return st, coef, d2


def host_reconstruct(coef, desc):
    h, w = desc.oriented_size()
    out = np.empty((h, w, 3), np.uint8)
    st = L.load().sd_jpeg_reconstruct_bgr_host(coef.ctypes.data_as(C.c_void_p), C.byref(desc), out.ctypes.data_as(C.c_void_p), out.nbytes)
    return st, out
