"""GPU: the JPEG entropy route (jpeg_entropy_gpu.hip through sd_jpeg_entropy_decode, Engine.jpeg_entropy_decode and
FrameFeeder(jpeg="device_entropy")) against the existing host decoder, element for element and byte for byte.  The kernel sees only
streams the shared function (semantic_depth_amd/csrc/jpeg_entropy.hpp) has already handled on the CPU in the same test: hostile inputs are
the business of tests/test_jpeg_entropy_cpu.py and scripts/fuzz_jpeg_entropy.cpp."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as graft
import jpeg_cases as J
import jpeg_entropy_cases as E
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


def _both(eng, batch):
    """the batch through the CPU statement, then through the kernels: (host coef, host status, device coef, device status)"""
    st, hc, hs = batch.host()
    assert st == L.SD_OK
    st, dc, ds = batch.device(eng)
    assert st == L.SD_OK
    return hc, hs, dc.cpu().numpy(), ds.cpu().numpy()


def _eligible_files():
    files = E.own_files()
    try:
        from PIL import Image as PILImage
        files += E.pil_files(PILImage)
    except ImportError:
        pass
    return files


def test_eligible_files_one_launch_each_and_all_in_one(eng):
    files = _eligible_files()
    plans = [E.Plan(b) for _, b in files]
    assert all(p.eligible for p in plans)
    for (name, _), p in zip(files, plans):
        hc, hs, dc, ds = _both(eng, E.Batch([p]))
        E.check_frame(name, p, dc[0], ds[0])
    hc, hs, dc, ds = _both(eng, E.Batch(plans))                # mixed sizes, samplings and tables in one launch
    for i, (name, _) in enumerate(files):
        E.check_frame(name, plans[i], dc[i], ds[i])
    assert np.array_equal(hc, dc) and np.array_equal(hs, ds)


def _first_refused(PILImage):
    for f in E.damaged_scans(PILImage):
        p = E.Plan(f)
        if p.eligible and J.coef_decode(f)[0] != L.SD_OK:
            return p
    raise AssertionError("no eligible-and-refused stream")


def test_eligible_ineligible_refused_eligible_in_one_launch(eng):
    PILImage = pytest.importorskip("PIL.Image")
    own = E.own_files()
    prog = next(b for name, b in J.pil_matrix(PILImage) if name.endswith("prog"))
    plans = [E.Plan(own[1][1]), E.Plan(prog), _first_refused(PILImage), E.Plan(own[4][1])]
    assert [p.eligible for p in plans] == [True, False, True, True]
    hc, hs, dc, ds = _both(eng, E.Batch(plans))                # (the CPU statement has run this exact stream first)
    assert hs[2] != 0 and ds[2] != 0
    for i in (0, 3):
        E.check_frame(f"frame {i}", plans[i], dc[i], ds[i])
    assert (dc[1] == E.FILL16).all() and ds[1] == 0


def test_accepted_damaged_scans_in_batches_of_32(eng):
    PILImage = pytest.importorskip("PIL.Image")
    plans = []
    for f in E.damaged_scans(PILImage):
        p = E.Plan(f)
        if p.eligible and J.coef_decode(f)[0] == L.SD_OK:
            plans.append(p)
    assert len(plans) >= 290
    for k in range(0, len(plans), 32):
        part = plans[k:k + 32]
        hc, hs, dc, ds = _both(eng, E.Batch(part))
        assert (hs == 0).all()
        for i, p in enumerate(part):
            E.check_frame(f"mutation {k + i}", p, dc[i], ds[i])


def test_argument_checks_through_the_device_entry_point(eng):
    import torch
    files = E.own_files()
    batch = E.Batch([E.Plan(b) for _, b in files])
    big = max(p.desc.coef_elems() for p in batch.plans)
    intervals = batch.copies()[2]
    intervals[4 * batch.interval_stride + 10].end = batch.byte_stride + 1
    bad_frames = batch.copies()[1]
    bad_frames[1].mcus_x += 1
    need = C.c_size_t()
    assert L.load().sd_jpeg_entropy_workspace(batch.B, batch.interval_stride, C.byref(need)) == L.SD_OK
    for over in (dict(intervals=intervals), dict(coef_stride_bytes=(big - 64) * 2), dict(frames=bad_frames), dict(workspace_bytes=need.value - 1),
                 dict(byte_stride=batch.byte_stride + 8)):
        st, coef, status = batch.device(eng, **over)
        assert st == L.SD_ERR_INVALID, over.keys()
        torch.cuda.synchronize()
        assert bool((coef == int(E.FILL16)).all()) and bool((status == -1).all()), over.keys()
    st, coef, status = batch.device(eng)
    assert st == L.SD_OK
    coef, status = coef.cpu().numpy(), status.cpu().numpy()
    for i, (name, _) in enumerate(files):
        E.check_frame(name, batch.plans[i], coef[i], status[i])


def _feed(paths, batch, jpeg, eng):
    got, los = [], []
    kw = {"jpeg": jpeg, "engine": eng} if jpeg != "host" else {}
    with frame_io.FrameFeeder(paths, batch=batch, device="cuda", workers=3, **kw) as feeder:
        for dev, lo in feeder:
            assert dev.is_cuda and dev.is_contiguous()
            got.append(dev.cpu().numpy())
            los.append(lo)
        fallback = list(feeder.entropy_fallback)
    return got, los, fallback


def _feeder_files(tmp_path, PILImage, h=48, w=80):
    """8 files of one size: the project's encoder, Pillow restart files, one progressive JPEG, one baseline JPEG without DRI, one PNG"""
    rng = np.random.default_rng(41)
    paths = []
    for i in range(8):
        img = J._img(rng, h, w)
        p = str(tmp_path / f"f{i:03d}.{'png' if i == 5 else 'jpg'}")
        if i in (0, 3):
            open(p, "wb").write(E.own_jpeg(img, 85))
        elif i in (1, 4, 7):
            PILImage.fromarray(img).save(p, "JPEG", quality=88, subsampling=(0, 1, 2)[i % 3], restart_marker_rows=1)
        elif i == 2:
            PILImage.fromarray(img).save(p, "JPEG", quality=88, progressive=True)
        elif i == 6:
            PILImage.fromarray(img).save(p, "JPEG", quality=88)
        else:
            outputs.write_png(p, img)
        paths.append(p)
    return paths


def test_feeder_entropy_route_equals_host_route_on_a_mixed_directory(eng, tmp_path):
    """batches of 3 over 8 files.  The sub-case "a stream the host decoder ACCEPTS but whose plan-eligible decode flags" is skipped: no
    such stream exists in the damaged set -- tests/test_jpeg_entropy_cpu.py asserts status 0 for every eligible file the host accepts."""
    PILImage = pytest.importorskip("PIL.Image")
    paths = _feeder_files(tmp_path, PILImage)
    host, los_h, _ = _feed(paths, 3, "host", eng)
    devr, los_d, fallback = _feed(paths, 3, "device_entropy", eng)
    assert los_h == los_d == [0, 3, 6] and [g.shape for g in devr] == [g.shape for g in host]
    for a, b in zip(host, devr):
        assert np.array_equal(a, b)
    assert fallback == [(2, "ineligible"), (6, "ineligible")]
    # a stream the kernel flags is refused by the host decoder too: the route raises what the "device" route raises
    bad = str(tmp_path / "f008.jpg")
    refused = _first_refused(PILImage)
    assert E.Batch([refused]).host()[2][0] != 0                # (the CPU statement first)
    open(bad, "wb").write(refused.buf)
    msgs = []
    for mode in ("device", "device_entropy"):
        with pytest.raises(ValueError) as ei:
            _feed([bad], 3, mode, eng)
        msgs.append(str(ei.value))
    assert msgs[0] == msgs[1]


def test_run_sequence_files_passes_the_entropy_route_through(eng, tmp_path):
    import torch
    from semantic_depth_amd import distributed as D
    PILImage = pytest.importorskip("PIL.Image")
    paths = _feeder_files(tmp_path, PILImage)[:7]
    seen = []

    def step(frames, first):
        seen.append((first, frames.shape[0]))
        rows = frames.reshape(frames.shape[0], -1)
        return torch.cat([rows[:, :D.RECORD_BYTES // 2], rows[:, -(D.RECORD_BYTES // 2):]], 1).contiguous()
    host = D.run_sequence_files(paths, step, batch=3, device="cuda", workers=2).cpu().numpy()
    bounds = list(seen)
    del seen[:]
    dev = D.run_sequence_files(paths, step, batch=3, device="cuda", workers=2, jpeg="device_entropy", engine=eng).cpu().numpy()
    assert seen == bounds == [(0, 3), (3, 3), (6, 1)]
    assert host.shape == (7, D.RECORD_BYTES) and np.array_equal(host, dev)
    with pytest.raises(ValueError, match="needs engine="):
        D.run_sequence_files(paths, step, batch=3, device="cuda", workers=2, jpeg="device_entropy")


def test_mjpeg_avi_round_trip(eng, tmp_path):
    """no Pillow: Engine.encode_jpeg on four 96 x 160 frames -> outputs.MjpegAviWriter -> frame_io.avi_frames ->
    Engine.jpeg_entropy_decode + jpeg_reconstruct == frame_io.decode_jpeg of the same byte strings"""
    import torch
    rng = np.random.default_rng(51)
    frames = np.stack([J._img(rng, 96, 160) for _ in range(4)])
    streams, sizes = _encode(eng, torch.from_numpy(frames).cuda())
    path = str(tmp_path / "clip.avi")
    with outputs.MjpegAviWriter(path, 160, 96, 10) as wr:
        for s in streams:
            wr.append(s)
    files = list(frame_io.avi_frames(path))
    assert files == streams
    batch = E.Batch([E.Plan(f) for f in files])
    assert all(p.eligible and p.frame.n_intervals == 6 for p in batch.plans)
    assert batch.host()[0] == L.SD_OK                          # (the CPU statement first)
    coef, status = eng.jpeg_entropy_decode(torch.from_numpy(batch.bytes).cuda(), batch.descs, batch.frames, batch.tables, batch.intervals,
                                           batch.interval_stride)
    got = eng.jpeg_reconstruct(coef, batch.descs).cpu().numpy()
    assert bool((status == 0).all())
    for i, f in enumerate(files):
        assert np.array_equal(got[i], frame_io.decode_jpeg(f)), i


def _encode(eng, frames_dev, quality=90):
    """Engine.encode_jpeg -> ([bytes per frame], sizes)"""
    out = eng.encode_jpeg(frames_dev, quality)
    streams, sizes = out[0].cpu().numpy(), out[1].cpu().numpy()
    return [streams[i, :int(sizes[i])].tobytes() for i in range(frames_dev.shape[0])], sizes


def test_real_size_frames_through_the_feeder_and_the_cubic_resize(eng, tmp_path):
    """two 512 x 1024 4:2:0 frames of Engine.encode_jpeg (q90): the entropy route's frames and their cubic resize to 128 x 256 equal the
    host route's"""
    import torch
    rng = np.random.default_rng(61)
    yy, xx = np.mgrid[0:512, 0:1024]
    base = np.stack([(yy // 3 + xx // 5) % 256, (xx // 2 + yy) % 256, (yy * 3 + xx // 7) % 256], -1).astype(np.uint8)
    frames = np.stack([base ^ rng.integers(0, 16, base.shape, dtype=np.uint8) for _ in range(2)])
    streams, _ = _encode(eng, torch.from_numpy(frames).cuda())
    paths = []
    for i, s in enumerate(streams):
        paths.append(str(tmp_path / f"real{i}.jpg"))
        open(paths[-1], "wb").write(s)
    res = {}
    for mode in ("host", "device_entropy"):
        kw = {"jpeg": mode, "engine": eng} if mode != "host" else {}
        with frame_io.FrameFeeder(paths, batch=2, device="cuda", workers=2, **kw) as feeder:
            (dev, lo), = list(feeder)
            assert tuple(dev.shape) == (2, 512, 1024, 3) and feeder.entropy_fallback == []
            res[mode] = (dev.cpu().numpy(), eng.resize_cubic(dev).cpu().numpy())
    assert np.array_equal(res["host"][0], res["device_entropy"][0])
    assert res["host"][1].shape == (2, 128, 256, 3) and np.array_equal(res["host"][1], res["device_entropy"][1])
