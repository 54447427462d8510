"""CPU: the JPEG encoder of the result video as its host statement, sd_jpeg_encode_bgr_host (the function whose bytes the kernels of
jpeg_enc_gpu.hip must reproduce; tests/test_gpu_jpeg_enc_device.py).  Its files are held to the project's own coefficient reader
(sd_jpeg_decode_coefficients, itself held to libjpeg-turbo in tests/test_frame_io.py), to a float64 DCT of an independent numpy statement
of the planes, to PIL as a foreign decoder and table source, and to the marker grammar of T.81."""
import ctypes as C
import io

import numpy as np
import pytest

from semantic_depth_amd import _lib as L
from semantic_depth_amd import frame_io

import jpeg_enc_cases as JC

CASES = JC.CASE_NAMES


def _entropy(data):
    segs, start = JC.segments(data)
    assert data[-2:] == b"\xff\xd9"
    return segs, data[start:-2]


@pytest.mark.parametrize("name", CASES)
def test_descriptor_and_dct_accuracy(name):
    """the decoded coefficients q of every block satisfy |q Q - c| <= Q / 2 + 1 against the float64 orthonormal DCT c of the planes"""
    from scipy.fft import dctn
    img, quality = JC.cases()[name]
    h, w = img.shape[:2]
    mh, mw = -(-h // 16), -(-w // 16)
    d, comps = JC.decoded_coefficients(JC.host_stream(name))
    assert (d.ncomp, d.hmax, d.vmax, d.height, d.width) == (3, 2, 2, h, w)
    assert list(d.blocks_w) == [2 * mw, mw, mw] and list(d.blocks_h) == [2 * mh, mh, mh]
    worst = -1e9
    for c, plane in enumerate(JC.planes(img)):
        bh, bw = plane.shape[0] // 8, plane.shape[1] // 8
        blocks = (plane.astype(np.float64) - 128.0).reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3)
        ref = dctn(blocks, axes=(2, 3), norm="ortho").reshape(bh, bw, 64)
        Q = np.array(d.qt[c][:], np.float64)
        err = np.abs(comps[c].astype(np.float64) * Q - ref) - Q / 2
        worst = max(worst, float(err.max()))
    print(f"{name}: max |qQ - c| - Q/2 = {worst:.4f}")
    assert worst <= 1.0, worst


@pytest.mark.parametrize("name", CASES)
def test_pil_reads_the_same_pixels(name):
    PILImage = pytest.importorskip("PIL.Image")
    img, _ = JC.cases()[name]
    data = JC.host_stream(name)
    im = PILImage.open(io.BytesIO(data))
    im.load()
    assert im.size == (img.shape[1], img.shape[0]) and im.mode == "RGB" and im.format == "JPEG"
    assert np.array_equal(np.asarray(im), frame_io.decode_jpeg(data)[..., ::-1])


@pytest.mark.parametrize("quality", [1, 10, 49, 50, 51, 75, 90, 100])
def test_tables_equal_pil(quality):
    PILImage = pytest.importorskip("PIL.Image")
    img = JC.mixed_frame(3, 24, 24)
    ours_q, ours_h = JC.tables(JC.encode_host(img, quality))
    buf = io.BytesIO()
    PILImage.fromarray(img[..., ::-1]).save(buf, "JPEG", quality=quality, subsampling=2, optimize=False)
    pil_q, pil_h = JC.tables(buf.getvalue())
    assert ours_q == pil_q and sorted(ours_q) == [0, 1]
    assert ours_h == pil_h and sorted(ours_h) == [0x00, 0x01, 0x10, 0x11]
    # Image.quantization gives the tables in natural order: bring ours there
    quant = PILImage.open(io.BytesIO(buf.getvalue())).quantization
    for t in (0, 1):
        nat = [0] * 64
        for k, n in enumerate(JC.ZIGZAG):
            nat[n] = ours_q[t][k]
        assert list(quant[t]) == nat


def _psnr(a, b):
    return 10.0 * np.log10(255.0 ** 2 / np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))


@pytest.mark.parametrize("name", ["smooth_q50", "smooth_q90"])
def test_fidelity_beside_pil(name):
    """PSNR of our decoded file against the source is within 0.5 dB of PIL's own file of the same quality and subsampling.
    Measured gaps (ours - PIL): see profiles/mjpeg_device_rate.json."""
    PILImage = pytest.importorskip("PIL.Image")
    img, quality = JC.cases()[name]
    buf = io.BytesIO()
    PILImage.fromarray(img[..., ::-1]).save(buf, "JPEG", quality=quality, subsampling=2)
    ours = _psnr(frame_io.decode_jpeg(JC.host_stream(name)), img)
    pil = _psnr(frame_io.decode_jpeg(buf.getvalue()), img)
    print(f"{name}: ours {ours:.3f} dB, PIL {pil:.3f} dB")
    assert ours >= pil - 0.5, (ours, pil)


@pytest.mark.parametrize("name", CASES)
def test_structure(name):
    img, _ = JC.cases()[name]
    h, w = img.shape[:2]
    mh, mw = -(-h // 16), -(-w // 16)
    data = JC.host_stream(name)
    segs, ecs = _entropy(data)
    assert [m for m, _ in segs] == [0xD8, 0xE0, 0xDB, 0xC0, 0xC4, 0xDD, 0xDA]
    assert len(data) - len(ecs) - 2 == JC.HEADER_LEN
    assert segs[1][1] == b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00"
    assert segs[3][1] == bytes([8, h >> 8, h & 255, w >> 8, w & 255, 3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])
    assert int.from_bytes(segs[5][1], "big") == mw
    assert segs[6][1] == bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])
    rst, i = [], 0
    while i < len(ecs):
        if ecs[i] == 0xFF:
            assert i + 1 < len(ecs) and (ecs[i + 1] == 0 or 0xD0 <= ecs[i + 1] <= 0xD7), (i, ecs[i + 1] if i + 1 < len(ecs) else None)
            if ecs[i + 1]:
                rst.append(ecs[i + 1] - 0xD0)
            i += 2
        else:
            i += 1
    assert rst == [r % 8 for r in range(mh - 1)]
    assert len(data) <= JC.bound(h, w)


def test_content_cases_exercise_what_they_are_for():
    # constant: no AC coefficient, one DC value per component, so every difference behind an interval's first is zero
    _, comps = JC.decoded_coefficients(JC.host_stream("constant"))
    for c in comps:
        assert not c[..., 1:].any() and (c[..., 0] == c[0, 0, 0]).all()
    # noise at quality 100: stuffed FF bytes
    _, ecs = _entropy(JC.host_stream("noise_q100"))
    assert ecs.count(b"\xff\x00") >= 1
    # the checkerboard: a run of 16 or more zeros before a non-zero coefficient (ZRL) and a non-zero coefficient 63 (no EOB)
    _, comps = JC.decoded_coefficients(JC.host_stream("checker_q100"))
    zz = comps[0][0, 0][JC.ZIGZAG]
    nz = np.flatnonzero(zz[1:]) + 1
    assert zz[63] != 0 and len(nz) and max(np.diff(np.concatenate([[0], nz])) - 1) >= 16, zz
    # black and white blocks: DC differences of category 11
    _, comps = JC.decoded_coefficients(JC.host_stream("bw_blocks_q100"))
    dc = comps[0][..., 0].astype(np.int64)
    assert np.abs(np.diff(dc, axis=1)).max() >= 1024
    # the RST counter wraps
    assert JC.host_stream("geom_150x40").count(b"\xff\xd0") >= 2


def test_capacity():
    for name in ("geom_17x33", "noise_q100", "constant"):
        img, q = JC.cases()[name]
        data = JC.host_stream(name)
        st, size, out = JC.encode_host_raw(img, q, cap=len(data))
        assert st == L.SD_OK and size == len(data) and out.tobytes() == data
        st, size, out = JC.encode_host_raw(img, q, cap=len(data) - 1)
        assert st == L.SD_ERR_INVALID and size == 12345 and (out == 0xA5).all()


def test_argument_errors():
    lib = JC.lib()
    img = JC.mixed_frame(1, 16, 16)
    for h, w, q in ((0, 16, 90), (16, 0, 90), (16385, 16, 90), (16, 16385, 90), (16, 16, 0), (16, 16, 101), (-1, 16, 90)):
        out = np.full(JC.bound(16, 16), 0xA5, np.uint8)
        size = C.c_size_t(777)
        st = lib.sd_jpeg_encode_bgr_host(img.ctypes.data_as(C.c_void_p), h, w, q, out.ctypes.data_as(C.c_void_p), out.size, C.byref(size))
        assert st == L.SD_ERR_INVALID and size.value == 777 and (out == 0xA5).all(), (h, w, q)
    out = np.full(JC.bound(16, 16), 0xA5, np.uint8)
    size = C.c_size_t(777)
    assert lib.sd_jpeg_encode_bgr_host(None, 16, 16, 90, out.ctypes.data_as(C.c_void_p), out.size, C.byref(size)) == L.SD_ERR_INVALID
    assert lib.sd_jpeg_encode_bgr_host(img.ctypes.data_as(C.c_void_p), 16, 16, 90, None, out.size, C.byref(size)) == L.SD_ERR_INVALID
    assert lib.sd_jpeg_encode_bgr_host(img.ctypes.data_as(C.c_void_p), 16, 16, 90, out.ctypes.data_as(C.c_void_p), out.size, None) == L.SD_ERR_INVALID
    assert size.value == 777 and (out == 0xA5).all()


def test_workspace_and_bound():
    lib = JC.lib()
    ws, bd = C.c_size_t(7), C.c_size_t(7)
    for B, h, w in ((0, 8, 8), (-1, 8, 8), (1, 0, 8), (1, 8, 0), (1, 16385, 8), (1, 8, 16385)):
        assert lib.sd_jpeg_encode_workspace(B, h, w, C.byref(ws), C.byref(bd)) == L.SD_ERR_INVALID and ws.value == 7 and bd.value == 7
    for B, h, w in ((1, 1, 1), (3, 50, 70), (32, 1024, 2048), (1, 16384, 16384)):
        assert lib.sd_jpeg_encode_workspace(B, h, w, C.byref(ws), C.byref(bd)) == L.SD_OK
        assert bd.value == JC.bound(h, w) and ws.value >= 12 * B * (-(-h // 16)) and ws.value % 16 == 0
