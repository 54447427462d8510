"""CPU: the device route of the result images as its host statement, sd_png_encode_zlib_host (the function whose bytes the kernels of
png_gpu.hip must reproduce, tests/test_gpu_png_device.py), against zlib's inflater and a numpy statement of the Paeth rows; and the
writer that wraps finished streams in PNG chunks, sd_png_write_streams_files.  The stream format is the comment in include/semdepth.h."""
import ctypes as C
import struct
import zlib

import numpy as np
import pytest

import png_device_cases as P
from semantic_depth_amd import _lib as L
from semantic_depth_amd import frame_io, outputs

CHUNK = P.CHUNK


def _frame(rng, h, w):
    """content with flat regions, repeats and noise"""
    img = (rng.integers(0, 256, (h, w, 3)) // 32 * 32).astype(np.uint8)
    img[: max(h // 4, 1)] = (159, 157, 156)
    if w > 8:
        img[:, w // 2:] = rng.integers(0, 256, (h, w - w // 2, 3), dtype=np.uint8)
    return img


@pytest.mark.parametrize("h,w", [(1, 1), (1, 7), (37, 53), (96, 700)])
def test_round_trip_through_zlib(h, w):
    img = _frame(np.random.default_rng(h * 1000 + w), h, w)
    P.check_stream(P.encode_host(img), img)


@pytest.mark.parametrize("n", [CHUNK - 1, CHUNK, CHUNK + 1])
def test_round_trip_at_the_chunk_size(n):
    h, w = P.shape_for(n)
    assert h * (1 + 3 * w) == n
    img = _frame(np.random.default_rng(n), h, w)
    P.check_stream(P.encode_host(img), img)


@pytest.mark.parametrize("h,w", [(37, 53), (96, 700)])
def test_noise_takes_the_stored_fallback(h, w):
    img = np.random.default_rng(5).integers(0, 256, (h, w, 3), dtype=np.uint8)
    s = P.encode_host(img)
    P.check_stream(s, img)
    raw = h * (1 + 3 * w)
    nchunks = -(-raw // CHUNK)
    assert len(s) <= raw + 16 * nchunks + 18
    pos = 2                                          # every chunk: 00 LEN NLEN bytes 00 00 00 FF FF
    for c in range(nchunks):
        n = min(CHUNK, raw - c * CHUNK)
        assert s[pos:pos + 5] == bytes([0]) + struct.pack("<HH", n, n ^ 0xFFFF)
        assert s[pos + 5 + n:pos + 10 + n] == b"\x00\x00\x00\xff\xff"
        pos += n + 10
    assert pos == len(s) - 9


@pytest.fixture(scope="module")
def forced():
    return {name: P.forced(h, w, flat) for name, (h, w, flat) in P.forced_cases().items()}


@pytest.mark.parametrize("name", sorted(P.forced_cases()))
def test_forced_residual_streams_decode_to_their_bytes(forced, name):
    img, flat = forced[name]
    s = P.encode_host(img)
    assert zlib.decompress(s) == flat.tobytes()
    P.check_stream(s, img)


def test_constant_stream_is_one_literal_and_matches(forced):
    img, flat = forced["constant_3_chunks"]
    s = P.encode_host(img)
    n = len(flat)
    toks = P.decode_tokens(s, 2)                     # the first chunk: 32768 equal bytes = a literal, 127 matches of 258, one byte left
    full, rest = divmod(CHUNK - 1, 258)
    assert rest < 3
    assert toks == [("lit", 4)] + [("match", 258, 1)] * full + [("lit", 4)] * rest
    assert len(s) < 3 * 200 + 18 and n > 2 * CHUNK


def test_exact_run_lengths_become_the_documented_tokens(forced):
    img, flat = forced["exact_runs"]
    toks = P.decode_tokens(P.encode_host(img), 2)
    out, want = [], []
    i = 0
    while i < len(toks):                             # group the tokens of every run of the byte 4 behind the filter byte
        if toks[i] == ("lit", 4) and i > 0:
            j, run = i + 1, []
            while j < len(toks) and (toks[j][0] == "match" or toks[j] == ("lit", 4)):
                run.append(toks[j][1] if toks[j][0] == "match" else "lit")
                j += 1
            out.append(run)
            i = j
        else:
            i += 1
    for n in P.RUNS:
        if n < 4:
            want.append(["lit"] * (n - 1))
        else:
            rest, run = n - 1, []
            while rest > 258:
                run.append(258)
                rest -= 258
            run += [rest] if rest >= 3 else ["lit"] * rest
            want.append(run)
    assert out == want
    assert want[3] == [258] and want[4] == [258, "lit"] and want[5] == [258, "lit", "lit"] and want[6] == [258, 3] and want[8] == [258, 258]


def test_geometric_histogram_is_limited_to_15_bits_with_a_complete_code(forced):
    img, flat = forced["geometric"]
    counts = np.bincount(flat, minlength=256)
    assert sorted(counts[counts > 0]) == [1, 1] + [2 ** k for k in range(1, 15)]
    s = P.encode_host(img)
    ll, dl = P.parse_dynamic_header(s, 2)
    used = [v for v in ll if v]
    assert len(used) == 17                           # 16 byte values and the end-of-block symbol
    assert max(used) <= 15
    assert sum(2 ** (15 - v) for v in used) == 2 ** 15            # Kraft sum exactly 1
    assert max(used) == 15                           # (the unconstrained tree would be 16 deep: the limit is active)
    assert dl == [1, 1]
    assert zlib.decompress(s) == flat.tobytes()


def test_chunks_without_a_match_still_carry_the_complete_distance_tree(forced):
    img, _ = forced["no_run"]
    s = P.encode_host(img)
    ll, dl = P.parse_dynamic_header(s, 2)
    assert dl == [1, 1] and all(t[0] == "lit" for t in P.decode_tokens(s, 2))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_smooth_frames_are_no_larger_than_the_host_writer(seed):
    img = P.smooth_frame(seed)
    h, w = img.shape[:2]
    rows0 = np.zeros((h, 1 + 3 * w), np.uint8)
    rows0[:, 1:] = img[..., ::-1].reshape(h, 3 * w)
    base = len(zlib.compress(rows0.tobytes(), 1))
    s = P.encode_host(img)
    print(f"seed {seed}: device format {len(s)} B, host writer (filter 0, level 1) {base} B, ratio {len(s) / base:.3f}")
    P.check_stream(s, img)
    assert len(s) <= base


def _png_chunks(data):
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, out = 8, []
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + body) & 0xFFFFFFFF
        out.append((tag, body))
        pos += 12 + n
    return out


def test_write_streams_files(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(3)
    h, w = 600, 700                                  # the noise frame's stream is above 1 MiB: more than one IDAT
    imgs = [_frame(rng, h, w), rng.integers(0, 256, (h, w, 3), dtype=np.uint8), np.zeros((h, w, 3), np.uint8)]
    streams = [P.encode_host(i) for i in imgs]
    stride = P.bound(h, w)
    buf = np.full((3, stride), 0xA5, np.uint8)
    for i, s in enumerate(streams):
        buf[i, :len(s)] = np.frombuffer(s, np.uint8)
    paths = [str(tmp_path / f"f{i}.png") for i in range(3)]
    assert outputs.write_png_streams(paths, buf, [len(s) for s in streams], h, w, threads=2) == paths
    for p, img, s in zip(paths, imgs, streams):
        data = open(p, "rb").read()
        assert np.array_equal(frame_io.imread(p), img)
        got = np.empty((h, w, 3), np.uint8)
        hh, ww = C.c_int(), C.c_int()
        assert P.lib().sd_png_decode_bgr(data, len(data), got.ctypes.data_as(C.c_void_p), got.size, C.byref(hh), C.byref(ww)) == L.SD_OK
        assert (hh.value, ww.value) == (h, w) and np.array_equal(got, img)
        assert np.array_equal(np.asarray(Image.open(p).convert("RGB"))[..., ::-1], img)
        chunks = _png_chunks(data)
        assert [t for t, _ in chunks][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
        assert chunks[0][1] == struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)
        idat = [b for t, b in chunks if t == b"IDAT"]
        assert b"".join(idat) == s and len(idat) == -(-len(s) // (1 << 20))
    assert len(streams[1]) > 1 << 20


def test_write_streams_files_reports_an_unwritable_path(tmp_path):
    img = _frame(np.random.default_rng(4), 8, 9)
    s = P.encode_host(img)
    buf = np.zeros((2, P.bound(8, 9)), np.uint8)
    buf[:, :len(s)] = np.frombuffer(s, np.uint8)
    paths = [str(tmp_path / "ok.png"), str(tmp_path / "no_such_dir" / "x.png")]
    arr = (C.c_char_p * 2)(*[p.encode() for p in paths])
    status = (C.c_int * 2)()
    sizes = np.array([len(s), len(s)], np.uint64)
    st = P.lib().sd_png_write_streams_files(arr, 2, 8, 9, buf.ctypes.data_as(C.c_void_p), buf.shape[1], sizes.ctypes.data_as(C.c_void_p), 2, status)
    assert st != L.SD_OK and list(status) == [L.SD_OK, L.SD_ERR_NOTFOUND]
    assert np.array_equal(frame_io.imread(paths[0]), img)
    with pytest.raises(OSError):
        outputs.write_png_streams(paths, buf, sizes, 8, 9)
    sizes[0] = buf.shape[1] + 1                      # a size beyond the stride is refused before anything is written
    assert P.lib().sd_png_write_streams_files(arr, 2, 8, 9, buf.ctypes.data_as(C.c_void_p), buf.shape[1], sizes.ctypes.data_as(C.c_void_p), 2,
                                              status) == L.SD_ERR_INVALID


def test_encoder_refuses_bad_extents_and_small_buffers():
    lib = P.lib()
    ws, stride, size = C.c_size_t(), C.c_size_t(), C.c_size_t()
    for B, h, w in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (1, 16385, 8), (1, 8, 16385)):
        assert lib.sd_png_encode_workspace(B, h, w, C.byref(ws), C.byref(stride)) == L.SD_ERR_INVALID
    assert lib.sd_png_encode_workspace(1, 16384, 16384, C.byref(ws), C.byref(stride)) == L.SD_OK
    assert stride.value == P.bound(16384, 16384) and ws.value > 16384 * (1 + 3 * 16384)
    img = np.zeros((8, 8, 3), np.uint8)
    out = np.zeros(8, np.uint8)
    assert lib.sd_png_encode_zlib_host(img.ctypes.data_as(C.c_void_p), 8, 8, out.ctypes.data_as(C.c_void_p), out.size, C.byref(size)) == L.SD_ERR_INVALID
    assert lib.sd_png_encode_zlib_host(img.ctypes.data_as(C.c_void_p), 0, 8, out.ctypes.data_as(C.c_void_p), out.size, C.byref(size)) == L.SD_ERR_INVALID


def test_sequence_outputs_png_choice_is_checked(tmp_path):
    import torch
    with pytest.raises(ValueError):
        outputs.SequenceOutputs(str(tmp_path), ["a"], png="gpu")
    o = outputs.SequenceOutputs(str(tmp_path), ["a"], ply=False, png="device")
    assert o.png == "device"
    with pytest.raises(ValueError):                  # the device route needs the streams, not the images
        o.submit(0, torch.zeros((1, 104), dtype=torch.uint8), (4, 4), images=np.zeros((1, 4, 4, 3), np.uint8))
    o.close()


def test_sequence_outputs_device_route_from_host_arrays(tmp_path):
    """the writer side alone (no GPU): host arrays in place of Engine.encode_png's tensors give the files of the host route"""
    rng = np.random.default_rng(8)
    h, w, n = 24, 40, 3
    imgs = np.stack([_frame(rng, h, w) for _ in range(n)])
    stride = P.bound(h, w)
    buf, sizes = np.full((n, stride), 0xA5, np.uint8), np.zeros(n, np.int64)
    for i in range(n):
        s = P.encode_host(imgs[i])
        buf[i, :len(s)], sizes[i] = np.frombuffer(s, np.uint8), len(s)
    names = [f"f{i}" for i in range(n)]
    import torch
    rec = torch.zeros((n, 104), dtype=torch.uint8)
    files = {}
    for route in ("host", "device"):
        o = outputs.SequenceOutputs(str(tmp_path / route), names, ply=False, png=route, threads=2)
        if route == "host":
            o.submit(0, rec, (h, w), images=imgs)
        else:
            o.submit(0, rec, (h, w), png_streams=(buf, sizes))
        o.close()
        import json
        files[route] = json.load(open(o.manifest))["files"]
        for nm, img in zip(names, imgs):
            assert np.array_equal(frame_io.imread(str(tmp_path / route / outputs.SEQ_IMG_DIR / (nm + ".png"))), img)
    assert files["host"] == files["device"] and len(files["host"]) == 2 * n
