"""GPU: the device half of the split JPEG route (jpeg_gpu.hip through sd_jpeg_reconstruct_bgr, Engine.jpeg_reconstruct and
FrameFeeder(jpeg="device")) against the existing host decoder sd_jpeg_decode_bgr, byte for byte.  The yardstick is that decoder (the
committed goldens pin it to libjpeg-turbo), never the kernels against themselves.  The file sets are tests/jpeg_cases.py."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as graft
import jpeg_cases as J
from semantic_depth_amd import _lib as L
from semantic_depth_amd import frame_io, outputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    graft.build()
    from semantic_depth_amd.engine import Engine
    e = Engine(128, 256, 2, "resnet50")
    yield e
    e.close()


def _device_decode(eng, bufs):
    """files of ONE size after the orientation -> u8 [n,h,w,3] through Engine.jpeg_reconstruct"""
    import torch
    decoded = [J.coef_decode(b) for b in bufs]
    assert all(st == L.SD_OK for st, _, _ in decoded)
    stride = max(-(-d.coef_elems() // 8) * 8 for _, _, d in decoded)
    coef = np.zeros((len(bufs), stride), np.int16)
    descs = (L.sd_jpeg_frame_desc * len(bufs))()
    for i, (_, c, d) in enumerate(decoded):
        coef[i, :d.coef_elems()] = c[:d.coef_elems()]
        descs[i] = d
    out = eng.jpeg_reconstruct(torch.from_numpy(coef).cuda(), descs)
    return out.cpu().numpy()


def _check(eng, name, buf, want=None):
    _, st, ref = J.host_decode(buf)
    assert st == L.SD_OK, name
    if want is not None:
        assert np.array_equal(ref, want), name
    got = _device_decode(eng, [buf])[0]
    assert got.shape == ref.shape and np.array_equal(got, ref), (name, int((got != ref).sum()))


def test_single_frames_golden_vectors_every_orientation(eng):
    """needs no Pillow: the committed vectors (4:4:4, 4:2:2, 4:2:0, gray, odd sizes) as stored and under the EXIF orientations 2..8,
    and the frame with the reference's progressive scan script"""
    for name, buf, want in J.golden_files():
        _check(eng, name, buf, want)
        for o in range(2, 9):
            _check(eng, f"{name} orientation {o}", J.with_orientation(buf, o))
    _check(eng, "scan_script", J.scan_script_file()[1])


def test_crafted_files_both_routes_accept(eng):
    """sequential files whose scans leave a component out: the one-call decoder keeps that plane at sample 0, and so must the kernels"""
    for name, buf in J.accepted_crafted_jpegs().items():
        _check(eng, name, buf)
    _, _, ref = J.host_decode(J.accepted_crafted_jpegs()["three_components_one_scanned"])
    assert (ref == np.array([0, 91, 0], np.uint8)).all()       # Y = 0, Cb = 128, Cr = 0


def test_single_frames_pillow_matrix(eng):
    PILImage = pytest.importorskip("PIL.Image")
    files = J.pil_matrix(PILImage) + J.pil_orientations(PILImage) + J.pil_orientations(PILImage, 23, 37, 2) + J.pil_orientations(PILImage, 9, 1, 1)
    assert len(files) > 250
    for name, buf in files:
        _check(eng, name, buf)


def test_accepted_mutated_files_agree(eng):
    """the mutated streams the host accepts carry coefficients no encoder writes: the device must still give the host's integers"""
    PILImage = pytest.importorskip("PIL.Image")
    n = 0
    for i, f in enumerate(J.mutated_jpegs(PILImage)):
        st_q, st, ref = J.host_decode(f, cap_limit=1 << 22)
        if st_q != L.SD_OK or st != L.SD_OK:
            continue
        _check(eng, f"mutation {i}", f)
        n += 1
    assert n > 30


def test_mixed_batch_of_one_oriented_size(eng):
    """one batch, one launch group: 4:4:4, 4:2:2, 4:2:0, gray and rotated frames that all are 40 x 24 after the orientation"""
    import io
    PILImage = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(9)
    bufs = []

    def jpeg(h, w, o=1, gray=False, **kw):
        im = PILImage.fromarray(J._img(rng, h, w))
        b = io.BytesIO()
        ex = PILImage.Exif()
        ex[0x0112] = o
        (im.convert("L") if gray else im).save(b, "JPEG", quality=88, exif=ex, **kw)
        return b.getvalue()
    for ss in (0, 1, 2):
        bufs.append(jpeg(40, 24, subsampling=ss))
        bufs.append(jpeg(40, 24, subsampling=ss, progressive=True))
    bufs.append(jpeg(40, 24, gray=True))
    for o in (3, 6, 8, 5, 7):
        bufs.append(jpeg(24, 40, o=o, subsampling=2) if o >= 5 else jpeg(40, 24, o=o, subsampling=1))
    assert len(bufs) == 12                                   # more than one group of eight
    ref = np.stack([J.host_decode(b)[2] for b in bufs])
    assert ref.shape == (12, 40, 24, 3)
    got = _device_decode(eng, bufs)
    for i in range(len(bufs)):
        assert np.array_equal(got[i], ref[i]), i


def test_mixed_sizes_through_the_c_call_and_the_workspace_is_checked(eng):
    """the C entry point takes frames of different sizes (no Pillow: the goldens, some rotated); a workspace one byte short, a
    coefficient stride or an output stride that cannot hold a frame and a descriptor that is not self-consistent are SD_ERR_INVALID,
    and nothing is launched: the output keeps its fill"""
    import torch
    lib = L.load()
    bufs = [b for _, b, _ in J.golden_files()] + [J.with_orientation(J.golden_files()[i][1], o) for i, o in ((1, 6), (2, 5), (3, 8), (5, 7))]
    decoded = [J.coef_decode(b) for b in bufs]
    refs = [J.host_decode(b)[2] for b in bufs]
    B = len(bufs)
    stride = max(-(-d.coef_elems() // 8) * 8 for _, _, d in decoded)
    ostride = max(r.size for r in refs)
    coef = np.zeros((B, stride), np.int16)
    descs = (L.sd_jpeg_frame_desc * B)()
    for i, (_, c, d) in enumerate(decoded):
        coef[i, :d.coef_elems()] = c[:d.coef_elems()]
        descs[i] = d
    need = C.c_size_t()
    assert lib.sd_jpeg_reconstruct_workspace(descs, B, C.byref(need)) == L.SD_OK and need.value > 0
    cdev = torch.from_numpy(coef).cuda()
    ws = torch.empty(need.value, dtype=torch.uint8, device="cuda")
    out = torch.full((B, ostride), 0xA5, dtype=torch.uint8, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(descs_=descs, cstride=stride * 2, ostride_=ostride, wsbytes=need.value):
        return lib.sd_jpeg_reconstruct_bgr(eng.h, C.c_void_p(cdev.data_ptr()), cstride, descs_, B, C.c_void_p(out.data_ptr()), ostride_,
                                           C.c_void_p(ws.data_ptr()), wsbytes, stream)
    assert call(wsbytes=need.value - 1) == L.SD_ERR_INVALID
    assert call(cstride=(max(d.coef_elems() for _, _, d in decoded) * 2 - 16) // 16 * 16) == L.SD_ERR_INVALID
    assert call(ostride_=ostride - 1) == L.SD_ERR_INVALID
    bad = (L.sd_jpeg_frame_desc * B).from_buffer_copy(bytes(descs))
    bad[B - 1].blocks_h[0] += 1
    assert call(descs_=bad) == L.SD_ERR_INVALID
    bad = (L.sd_jpeg_frame_desc * B).from_buffer_copy(bytes(descs))
    bad[0].orientation = 9
    assert call(descs_=bad) == L.SD_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all())
    assert call() == L.SD_OK
    got = out.cpu().numpy()
    for i, r in enumerate(refs):
        assert np.array_equal(got[i, :r.size].reshape(r.shape), r), i
        assert (got[i, r.size:] == 0xA5).all(), i            # nothing beyond a frame's own bytes


def _feed(paths, batch, jpeg, eng):
    got, los = [], []
    kw = {"jpeg": "device", "engine": eng} if jpeg == "device" else {}
    with frame_io.FrameFeeder(paths, batch=batch, device="cuda", workers=3, **kw) as feeder:
        for dev, lo in feeder:
            assert dev.is_cuda and dev.dtype.is_floating_point is False and dev.is_contiguous()
            got.append(dev.cpu().numpy())
            los.append(lo)
    return got, los


def test_feeder_device_route_equals_host_route_on_a_mixed_directory(eng, tmp_path):
    """PNG and JPEG files of one size in one sorted list, batches of 3 over 8 files (a ragged last batch, batches with and without PNGs)"""
    _, buf, want = J.golden_files()[2]
    h, w = want.shape[:2]
    rng = np.random.default_rng(4)
    paths = []
    for i in range(8):
        if i in (1, 6, 7):
            paths.append(outputs.write_png(str(tmp_path / f"f{i:03d}.png"), rng.integers(0, 256, (h, w, 3), dtype=np.uint8)))
        else:
            p = str(tmp_path / f"f{i:03d}.jpg")
            open(p, "wb").write(J.with_orientation(buf, (1, 3, 2, 4)[i % 4]))
            paths.append(p)
    host, los_h = _feed(paths, 3, "host", eng)
    devr, los_d = _feed(paths, 3, "device", eng)
    assert los_h == los_d == [0, 3, 6] and [g.shape for g in devr] == [g.shape for g in host] == [(3, h, w, 3), (3, h, w, 3), (2, h, w, 3)]
    for a, b in zip(host, devr):
        assert np.array_equal(a, b)
    for i, p in enumerate(paths):
        assert np.array_equal(np.concatenate(devr)[i], frame_io.imread(p)), p


def test_feeder_full_size_frame_through_the_cubic_resize(eng, tmp_path):
    """1024 x 2048 frames (4:2:0 baseline and progressive, 4:4:4) through FrameFeeder(jpeg="device") -> Engine.resize_cubic equal the
    host route bit for bit"""
    PILImage = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(12)
    yy, xx = np.mgrid[0:1024, 0:2048]
    base = np.stack([(yy // 3 + xx // 5) % 256, (xx // 2 + yy) % 256, (yy * 3 + xx // 7) % 256], -1).astype(np.uint8)
    paths = []
    for i, kw in enumerate(({"subsampling": 2}, {"subsampling": 2, "progressive": True}, {"subsampling": 0})):
        p = str(tmp_path / f"full{i}.jpg")
        PILImage.fromarray(base ^ rng.integers(0, 16, base.shape, dtype=np.uint8)).save(p, "JPEG", quality=90, **kw)
        paths.append(p)
    res = {}
    for mode in ("host", "device"):
        kw = {"jpeg": "device", "engine": eng} if mode == "device" else {}
        frames, small = [], []
        with frame_io.FrameFeeder(paths, batch=2, device="cuda", workers=3, **kw) as feeder:
            for dev, lo in feeder:
                assert tuple(dev.shape[1:]) == (1024, 2048, 3)
                small.append(eng.resize_cubic(dev).cpu().numpy())
                frames.append(dev.cpu().numpy())
        res[mode] = (np.concatenate(frames), np.concatenate(small))
    assert np.array_equal(res["host"][0], res["device"][0])
    assert res["host"][1].shape == (3, 128, 256, 3) and np.array_equal(res["host"][1], res["device"][1])


def test_run_sequence_files_passes_the_route_through(eng, tmp_path):
    """distributed.run_sequence_files(jpeg="device") feeds the step the frames of jpeg="host": a step that copies each frame's first
    bytes into its record returns the same records in both modes; the engine comes from engine= or from step.engine"""
    import torch
    from semantic_depth_amd import distributed as D
    _, buf, want = J.golden_files()[2]
    h, w = want.shape[:2]
    rng = np.random.default_rng(21)
    paths = []
    for i in range(7):
        if i == 4:
            paths.append(outputs.write_png(str(tmp_path / f"s{i:03d}.png"), rng.integers(0, 256, (h, w, 3), dtype=np.uint8)))
        else:
            p = str(tmp_path / f"s{i:03d}.jpg")
            open(p, "wb").write(J.with_orientation(buf, (1, 2, 3, 4)[i % 4]))
            paths.append(p)
    seen = []

    def step(frames, first):
        assert frames.is_cuda and tuple(frames.shape[1:]) == (h, w, 3)
        seen.append((first, frames.shape[0]))
        rows = frames.reshape(frames.shape[0], -1)
        return torch.cat([rows[:, :D.RECORD_BYTES // 2], rows[:, -(D.RECORD_BYTES // 2):]], 1).contiguous()
    host = D.run_sequence_files(paths, step, batch=3, device="cuda", workers=2).cpu().numpy()
    bounds = list(seen)
    del seen[:]
    dev = D.run_sequence_files(paths, step, batch=3, device="cuda", workers=2, jpeg="device", engine=eng).cpu().numpy()
    assert seen == bounds == [(0, 3), (3, 3), (6, 1)]
    assert host.shape == (7, D.RECORD_BYTES) and np.array_equal(host, dev)
    step.engine = eng                                        # what make_engine_step sets
    del seen[:]
    assert np.array_equal(D.run_sequence_files(paths, step, batch=3, device="cuda", workers=2, jpeg="device").cpu().numpy(), host)
    del step.engine
    with pytest.raises(ValueError, match="needs engine="):
        D.run_sequence_files(paths, step, batch=3, device="cuda", workers=2, jpeg="device")
