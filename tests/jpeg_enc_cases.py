"""Shared by tests/test_jpeg_enc_cpu.py and tests/test_gpu_jpeg_enc_device.py: the frames of the JPEG encoder behind the result video
(sd_jpeg_encode_bgr / sd_jpeg_encode_bgr_host, include/semdepth.h), the host statement as a callable, a marker walk of a file and an
independent numpy statement of the padded planes."""
import ctypes as C
import functools
import struct

import numpy as np

from semantic_depth_amd import _lib as L

from png_device_cases import smooth_frame

HEADER_LEN = 613

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


def lib():
    import __graft_entry__ as graft
    graft.build()
    return L.load()


def bound(h, w):
    """the bound of include/semdepth.h, restated"""
    return HEADER_LEN + (-(-h // 16)) * (2 * 208 * 6 * (-(-w // 16)) + 2)


def encode_host_raw(img, quality, cap=None, fill=0xA5):
    """sd_jpeg_encode_bgr_host(img) -> (status, size, the whole output buffer of ``cap`` bytes, filled with ``fill`` before the call)"""
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape[:2]
    cap = bound(h, w) if cap is None else cap
    out = np.full(max(cap, 1), fill, np.uint8)
    size = C.c_size_t(12345)
    st = lib().sd_jpeg_encode_bgr_host(img.ctypes.data_as(C.c_void_p), h, w, quality, out.ctypes.data_as(C.c_void_p), cap, C.byref(size))
    return st, size.value, out


def encode_host(img, quality):
    """sd_jpeg_encode_bgr_host(img) as bytes; the buffer behind the size must be untouched"""
    st, size, out = encode_host_raw(img, quality)
    assert st == L.SD_OK, st
    assert size <= out.size and (out[size:] == 0xA5).all()
    return out[:size].tobytes()


def mixed_frame(seed, h, w):
    """a smooth frame with a flat banner and a patch of noise: blocks of every kind at any size"""
    x = smooth_frame(seed, h, w, sigma=3.0)
    rng = np.random.default_rng(seed + 100)
    x[h // 2:, w // 2:] = rng.integers(0, 256, x[h // 2:, w // 2:].shape, dtype=np.uint8)
    return np.ascontiguousarray(x)


GEOMETRIES = [(1, 1), (8, 8), (16, 16), (17, 33), (50, 70), (150, 40), (16, 272), (272, 16)]


def _checkerboard(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    v = (128 + np.where((yy + xx) & 1, 1, -1)).astype(np.uint8)
    return np.ascontiguousarray(np.repeat(v[..., None], 3, axis=2))


def _bw_blocks(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    v = np.where(((yy >> 3) + (xx >> 3)) & 1, 255, 0).astype(np.uint8)
    return np.ascontiguousarray(np.repeat(v[..., None], 3, axis=2))


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (u8 [h,w,3] BGR frame, quality)"""
    out = {}
    for h, w in GEOMETRIES:
        out[f"geom_{h}x{w}"] = (mixed_frame(h * 1000 + w, h, w), 75)
    out["constant"] = (np.full((50, 70, 3), (31, 200, 90), np.uint8), 90)
    out["noise_q100"] = (np.random.default_rng(5).integers(0, 256, (50, 70, 3), dtype=np.uint8), 100)
    out["checker_q100"] = (_checkerboard(40, 48), 100)
    out["bw_blocks_q100"] = (_bw_blocks(32, 64), 100)
    out["smooth_q50"] = (np.ascontiguousarray(smooth_frame(11, 64, 96)), 50)
    out["smooth_q90"] = (np.ascontiguousarray(smooth_frame(11, 64, 96)), 90)
    out["smooth_q1"] = (np.ascontiguousarray(smooth_frame(12, 48, 80)), 1)
    out["smooth_q100"] = (np.ascontiguousarray(smooth_frame(12, 48, 80)), 100)
    return out


CASE_NAMES = [f"geom_{h}x{w}" for h, w in GEOMETRIES] + ["constant", "noise_q100", "checker_q100", "bw_blocks_q100", "smooth_q50", "smooth_q90",
                                                         "smooth_q1", "smooth_q100"]


@functools.lru_cache(maxsize=None)
def host_stream(name):
    """the host statement's file of a case, computed once"""
    img, q = cases()[name]
    return encode_host(img, q)


def segments(data):
    """[(marker, payload)] of the file up to and including SOS, and the offset of the first entropy-coded byte"""
    assert data[:2] == b"\xff\xd8"
    out, i = [(0xD8, b"")], 2
    while True:
        assert data[i] == 0xFF, i
        m = data[i + 1]
        n = struct.unpack(">H", data[i + 2:i + 4])[0]
        out.append((m, data[i + 4:i + 2 + n]))
        i += 2 + n
        if m == 0xDA:
            return out, i


def tables(data):
    """({table id: 64 zigzag-order entries} from DQT, {(class << 4 | id): payload bytes (BITS + HUFFVAL)} from DHT)"""
    dqt, dht = {}, {}
    for m, p in segments(data)[0]:
        if m == 0xDB:
            while p:
                assert p[0] >> 4 == 0
                dqt[p[0] & 15] = list(p[1:65])
                p = p[65:]
        elif m == 0xC4:
            while p:
                n = sum(p[1:17])
                dht[p[0]] = bytes(p[1:17 + n])
                p = p[17 + n:]
    return dqt, dht


def planes(img):
    """the padded planes as include/semdepth.h states them, in numpy: (Y [16mh,16mw], Cb [8mh,8mw], Cr [8mh,8mw]) int64"""
    h, w = img.shape[:2]
    ph, pw = -(-h // 16) * 16, -(-w // 16) * 16
    x = np.pad(img.astype(np.int64), ((0, ph - h), (0, pw - w), (0, 0)), mode="edge")
    B, G, R = x[..., 0], x[..., 1], x[..., 2]
    Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16
    Cb = (-11059 * R - 21709 * G + 32768 * B + 8421375) >> 16
    Cr = (32768 * R - 27439 * G - 5329 * B + 8421375) >> 16

    def box(p):
        return (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 2) >> 2

    return Y, box(Cb), box(Cr)


def decoded_coefficients(data):
    """sd_jpeg_decode_coefficients(data) -> (descriptor, [per component: int16 [blocks_h, blocks_w, 64] in natural order])"""
    from jpeg_cases import coef_decode
    st, coef, d = coef_decode(data)
    assert st == L.SD_OK, st
    comps = []
    for c in range(d.ncomp):
        n = d.blocks_w[c] * d.blocks_h[c] * 64
        comps.append(coef[d.coef_offset[c]:d.coef_offset[c] + n].reshape(d.blocks_h[c], d.blocks_w[c], 64))
    return d, comps
