"""GPU: the device half of the split PNG input route (png_in_gpu.hip through sd_png_reconstruct_bgr, Engine.png_reconstruct and
FrameFeeder(png="device")) against the existing host decoder (frame_io.decode_png = sd_png_decode_bgr), byte for byte.  Both
instantiations of the kernel run: the shipped 16-wave workgroup and the one-wave form (SEMDEPTH_DISABLE=png_waves, latched when the
engine is created).  The file sets are tests/png_in_cases.py."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as graft
import png_in_cases as P
from semantic_depth_amd import _lib as L
from semantic_depth_amd import frame_io, outputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engines():
    """{"waves16": engine, "wave1": engine}"""
    import os
    graft.build()
    from semantic_depth_amd.engine import Engine
    out = {"waves16": Engine(128, 256, 2, "resnet50")}
    old = os.environ.get("SEMDEPTH_DISABLE")
    os.environ["SEMDEPTH_DISABLE"] = "png_waves"
    try:
        out["wave1"] = Engine(128, 256, 2, "resnet50")
    finally:
        if old is None:
            del os.environ["SEMDEPTH_DISABLE"]
        else:
            os.environ["SEMDEPTH_DISABLE"] = old
    yield out
    for e in out.values():
        e.close()


@pytest.fixture(scope="module")
def eng(engines):
    return engines["waves16"]


@pytest.fixture(scope="module")
def refs():
    """{name: (file, reference BGR by frame_io.decode_png)} -- computed once, read-only"""
    out = {}
    for name, buf in P.cases():
        ref = frame_io.decode_png(buf)
        ref.setflags(write=False)
        out[name] = (buf, ref)
    return out


def _call(eng, bufs, pad_in=0, pad_out=0, ws_fill=0x00, expect=L.SD_OK):
    """files of ONE size through the C call with padded strides and prefilled buffers -> (frames u8 [B,h,w,3], status int32 [B]); the
    padding of the output (0xA5) and of the rows (0xFF) must come back unchanged"""
    import torch
    inf = [P.inflate_rows(b) for b in bufs]
    assert all(st == L.SD_OK for st, _, _ in inf)
    B = len(bufs)
    h, w = inf[0][2].height, inf[0][2].width
    fstride = max(-(-d.rows_bytes() // 16) * 16 for _, _, d in inf) + pad_in
    ostride = h * w * 3 + pad_out
    rows = np.full((B, fstride), 0xFF, np.uint8)
    descs = (L.sd_png_frame_desc * B)()
    for i, (_, r, d) in enumerate(inf):
        rows[i, :d.rows_bytes()] = r[:d.rows_bytes()]
        descs[i] = d
    rdev = torch.from_numpy(rows).cuda()
    out = torch.full((B, ostride), 0xA5, dtype=torch.uint8, device="cuda")
    status = torch.full((B,), 0x7F7F7F7F, dtype=torch.int32, device="cuda")
    need = C.c_size_t()
    assert eng.lib.sd_png_reconstruct_workspace(B, C.byref(need)) == L.SD_OK and need.value >= B * C.sizeof(L.sd_png_frame_desc)
    ws = torch.full((need.value,), ws_fill, dtype=torch.uint8, device="cuda")
    st = eng.lib.sd_png_reconstruct_bgr(eng.h, C.c_void_p(rdev.data_ptr()), fstride, descs, B, h, w, C.c_void_p(out.data_ptr()), ostride,
                                        C.c_void_p(status.data_ptr()), C.c_void_p(ws.data_ptr()), need.value, eng._stream())
    assert st == expect
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert (o[:, h * w * 3:] == 0xA5).all(), "bytes beyond a frame were written"
    assert np.array_equal(rdev.cpu().numpy(), rows), "the rows were written"
    return o[:, :h * w * 3].reshape(B, h, w, 3), status.cpu().numpy()


@pytest.mark.parametrize("form", ["waves16", "wave1"])
def test_every_case_equals_the_host_decoder(engines, refs, form):
    import torch
    e = engines[form]
    for name, (buf, ref) in refs.items():
        st, rows, d = P.inflate_rows(buf)
        stride = -(-d.rows_bytes() // 16) * 16
        r = np.zeros((1, stride), np.uint8)
        r[0, :d.rows_bytes()] = rows
        descs = (L.sd_png_frame_desc * 1)(d)
        out, status = e.png_reconstruct(torch.from_numpy(r).cuda(), descs)
        got = out.cpu().numpy()[0]
        assert got.shape == ref.shape and np.array_equal(got, ref), (name, form, int((got != ref).sum()))
        assert int(status[0]) == 0, name


@pytest.mark.parametrize("form", ["waves16", "wave1"])
@pytest.mark.parametrize("B", [1, 3, 33])
def test_mixed_colour_types_in_one_call_with_padded_strides(engines, refs, form, B):
    """frames of different colour types batched, both strides padded, output / padding / workspace prefilled; the workspace prefilled with
    0x00 and with 0xFF gives the same bytes"""
    e = engines[form]
    names = [f"mix_130x257_ct{ct}" for ct in (2, 3, 0, 6, 4)] + [f"uniform_ft{ft}_130x257_ct2" for ft in range(5)] + \
            ["pillow_adaptive_130x257_rgb", "pillow_130x257_palette", "pillow_130x257_la", "pillow_130x257_rgba"]
    names = [n for n in names if n in refs]
    pick = [names[i % len(names)] for i in range(B)]
    want = np.stack([refs[n][1] for n in pick])
    for ws_fill in (0x00, 0xFF):
        got, status = _call(e, [refs[n][0] for n in pick], pad_in=48, pad_out=7, ws_fill=ws_fill)
        assert np.array_equal(got, want), (form, B, ws_fill, [pick[i] for i in range(B) if not np.array_equal(got[i], want[i])])
        assert not status.any()


def test_the_same_call_after_a_different_batch_gives_the_same_bytes(eng, refs):
    a = [refs[f"mix_65x5_ct{ct}"][0] for ct in (2, 3, 4)]
    first, _ = _call(eng, a)
    _call(eng, [refs["wide_66x16384_ct6"][0]])
    _call(eng, [refs[f"uniform_ft{ft}_130x257_ct2"][0] for ft in (4, 3)], ws_fill=0xFF)
    again, _ = _call(eng, a)
    assert np.array_equal(first, again) and np.array_equal(first, np.stack([refs[f"mix_65x5_ct{ct}"][1] for ct in (2, 3, 4)]))


def test_arguments_are_checked_before_anything_is_launched(eng, refs):
    import torch
    buf = refs["mix_65x5_ct2"][0]
    _, rows, d = P.inflate_rows(buf)
    dev = torch.zeros((4096,), dtype=torch.uint8, device="cuda")
    outd = torch.zeros((4096,), dtype=torch.uint8, device="cuda")
    status = torch.zeros((1,), dtype=torch.int32, device="cuda")
    need = C.c_size_t()
    eng.lib.sd_png_reconstruct_workspace(1, C.byref(need))
    ws = torch.zeros((need.value,), dtype=torch.uint8, device="cuda")

    def call(desc, h, w, fstride=1376, ostride=65 * 5 * 3, wsb=None, rows_ptr=None):
        descs = (L.sd_png_frame_desc * 1)(desc)
        return eng.lib.sd_png_reconstruct_bgr(eng.h, C.c_void_p(rows_ptr or dev.data_ptr()), fstride, descs, 1, h, w, C.c_void_p(outd.data_ptr()),
                                              ostride, C.c_void_p(status.data_ptr()), C.c_void_p(ws.data_ptr()), need.value if wsb is None else wsb,
                                              eng._stream())
    assert call(d, 65, 5) == L.SD_OK
    big = L.sd_png_frame_desc.from_buffer_copy(d)
    big.height = 16385
    assert call(big, 16385, 5) == L.SD_ERR_INVALID and b"16384" in eng.lib.sd_last_error(eng.h)
    big.height, big.width = 65, 16385
    assert call(big, 65, 16385) == L.SD_ERR_INVALID
    assert call(d, 64, 5) == L.SD_ERR_INVALID                     # a descriptor of another size
    assert call(d, 65, 5, fstride=1040) == L.SD_OK                # 65 rows of 1 + 5 * 3 bytes
    assert call(d, 65, 5, fstride=1024) == L.SD_ERR_INVALID       # the rows do not fit
    assert call(d, 65, 5, fstride=1377) == L.SD_ERR_INVALID       # not a multiple of 16
    assert call(d, 65, 5, ostride=65 * 5 * 3 - 1) == L.SD_ERR_INVALID
    assert call(d, 65, 5, wsb=need.value - 16) == L.SD_ERR_INVALID
    assert call(d, 65, 5, rows_ptr=dev.data_ptr() + 4) == L.SD_ERR_INVALID
    bad = L.sd_png_frame_desc.from_buffer_copy(d)
    bad.channels = 4
    assert call(bad, 65, 5) == L.SD_ERR_INVALID
    bad = L.sd_png_frame_desc.from_buffer_copy(d)
    bad.palette_entries = 3
    assert call(bad, 65, 5) == L.SD_ERR_INVALID
    assert eng.lib.sd_png_reconstruct_workspace(0, C.byref(need)) == L.SD_ERR_INVALID
    torch.cuda.synchronize()


@pytest.mark.parametrize("form", ["waves16", "wave1"])
def test_palette_index_beyond_the_palette_flags_that_frame_only(engines, refs, form):
    """the frame's word alone is non-zero, its flagged pixel takes palette entry 0, every other byte of the batch is the host decoder's"""
    buf, y, x = P.overflow_case()
    rng = np.random.default_rng(3)
    pal = rng.integers(0, 256, (9, 3), dtype=np.uint8)
    others = [P.make_png(rng.integers(0, 9, (70, 9, 1), dtype=np.uint8), 3, rng.integers(0, 5, 70), palette=pal),
              P.make_png(rng.integers(0, 256, (70, 9, 3), dtype=np.uint8), 2, rng.integers(0, 5, 70))]
    got, status = _call(engines[form], [others[0], buf, others[1]], pad_in=16, pad_out=5)
    assert status[0] == 0 and status[1] != 0 and status[2] == 0
    assert np.array_equal(got[0], frame_io.decode_png(others[0])) and np.array_equal(got[2], frame_io.decode_png(others[1]))
    _, rows, d = P.inflate_rows(buf)
    want, over = P.unfilter_host(rows, d)
    assert over and np.array_equal(got[1], want)
    assert np.array_equal(got[1, y, x], np.ctypeslib.as_array(d.palette).reshape(256, 3)[0][::-1])


def _mixed_directory(tmp_path, refs, with_jpeg=True):
    import jpeg_cases as J
    _, jbuf, jwant = J.golden_files()[2]
    h, w = jwant.shape[:2]
    rng = np.random.default_rng(8)
    pal = rng.integers(0, 256, (40, 3), dtype=np.uint8)
    paths = []
    for i in range(11):
        if with_jpeg and i in (2, 3, 7):
            p = str(tmp_path / f"f{i:03d}.jpg")
            open(p, "wb").write(J.with_orientation(jbuf, (1, 3)[i % 2]))
        else:
            ct = (2, 6, 0, 3, 4)[i % 5]
            img = rng.integers(0, 40 if ct == 3 else 256, (h, w, P.CHANNELS[ct]), dtype=np.uint8)
            p = str(tmp_path / f"f{i:03d}.png")
            open(p, "wb").write(P.make_png(img, ct, rng.integers(0, 5, h), palette=pal if ct == 3 else None))
        paths.append(p)
    return paths, (h, w)


def _feed(paths, batch, eng, **kw):
    got, los = [], []
    with frame_io.FrameFeeder(paths, batch=batch, device="cuda", workers=3, **kw) as feeder:
        for dev, lo in feeder:
            assert dev.is_cuda and dev.is_contiguous()
            got.append(dev.cpu().numpy())
            los.append(lo)
    return got, los


@pytest.mark.parametrize("jpeg", ["host", "device"])
def test_feeder_device_route_equals_host_route_on_a_mixed_directory(eng, refs, tmp_path, jpeg):
    paths, (h, w) = _mixed_directory(tmp_path, refs)
    host, los_h = _feed(paths, 4, eng)
    kw = {"jpeg": "device"} if jpeg == "device" else {}
    devr, los_d = _feed(paths, 4, eng, png="device", engine=eng, **kw)
    assert los_h == los_d == [0, 4, 8] and [g.shape for g in devr] == [g.shape for g in host] == [(4, h, w, 3), (4, h, w, 3), (3, h, w, 3)]
    for a, b in zip(host, devr):
        assert np.array_equal(a, b)
    for i, p in enumerate(paths):
        assert np.array_equal(np.concatenate(devr)[i], frame_io.imread(p)), p


def test_feeder_raises_what_the_host_route_raises(eng, refs, tmp_path):
    paths, (h, w) = _mixed_directory(tmp_path, refs, with_jpeg=False)
    good = open(paths[5], "rb").read()
    rng = np.random.default_rng(9)
    over = rng.integers(0, 4, (h, w, 1), dtype=np.uint8)
    over[h // 2, w // 2] = 4
    corrupt = {"truncated": good[:len(good) // 2],
               "index beyond the palette": P.make_png(over, 3, rng.integers(0, 5, h), palette=rng.integers(0, 256, (4, 3), dtype=np.uint8))}
    for what, data in corrupt.items():
        open(paths[5], "wb").write(data)
        msgs = []
        for kw in ({}, {"png": "device", "engine": eng}):
            with pytest.raises(ValueError, match="could not be read as") as ei:
                _feed(paths, 4, eng, **kw)
            msgs.append(str(ei.value))
        assert msgs[0] == msgs[1], what
    with pytest.raises(ValueError, match="needs engine="):
        frame_io.FrameFeeder(paths, 4, png="device")
    with pytest.raises(ValueError, match="device='cpu' has none"):
        frame_io.FrameFeeder(paths, 4, device="cpu", png="device", engine=eng)
    with pytest.raises(ValueError, match="png must be"):
        frame_io.FrameFeeder(paths, 4, png="gpu")


def test_run_sequence_files_passes_the_route_through(eng, tmp_path):
    """distributed.run_sequence_files(png_in="device") at 64 x 128 returns the record bytes of png_in="host"; the engine comes from engine=
    or from step.engine"""
    import torch
    from semantic_depth_amd import distributed as D
    rng = np.random.default_rng(21)
    paths = []
    for i in range(7):
        ct = (2, 6, 0, 4)[i % 4]
        p = str(tmp_path / f"s{i:03d}.png")
        open(p, "wb").write(P.make_png(rng.integers(0, 256, (64, 128, P.CHANNELS[ct]), dtype=np.uint8), ct, rng.integers(0, 5, 64)))
        paths.append(p)
    seen = []

    def step(frames, first):
        assert frames.is_cuda and tuple(frames.shape[1:]) == (64, 128, 3)
        seen.append((first, frames.shape[0]))
        rows = frames.reshape(frames.shape[0], -1)
        return torch.cat([rows[:, :D.RECORD_BYTES // 2], rows[:, -(D.RECORD_BYTES // 2):]], 1).contiguous()
    host = D.run_sequence_files(paths, step, batch=3, device="cuda", workers=2, png_in="host").cpu().numpy()
    bounds = list(seen)
    del seen[:]
    dev = D.run_sequence_files(paths, step, batch=3, device="cuda", workers=2, png_in="device", engine=eng).cpu().numpy()
    assert seen == bounds == [(0, 3), (3, 3), (6, 1)]
    assert host.shape == (7, D.RECORD_BYTES) and np.array_equal(host, dev)
    step.engine = eng
    assert np.array_equal(D.run_sequence_files(paths, step, batch=3, device="cuda", workers=2, png_in="device").cpu().numpy(), host)
    del step.engine
    with pytest.raises(ValueError, match="needs engine="):
        D.run_sequence_files(paths, step, batch=3, device="cuda", workers=2, png_in="device")
