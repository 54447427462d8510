"""GPU: the JPEG sync route (jpeg_sync_gpu.hip through sd_jpeg_sync_decode, Engine.jpeg_sync_decode and FrameFeeder(jpeg="device_sync"))
against its CPU statement element for element -- coefficients, status words and the fill behind each frame -- and against the host
decoder byte for byte.  The kernels see only streams the shared statement (semantic_depth_amd/csrc/jpeg_sync.hpp) has already handled on
the CPU in the same test: hostile inputs are the business of tests/test_jpeg_sync_cpu.py and scripts/fuzz_jpeg_sync.cpp."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as graft
import jpeg_cases as J
import jpeg_entropy_cases as E
import jpeg_sync_cases as S
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


@pytest.mark.parametrize("piece", S.PIECES)
def test_intact_files_and_an_ineligible_one_in_one_batch(eng, piece):
    """files with and without DRI, gray, five workgroups of noise, a scan shorter than a piece, a progressive file among them: one call;
    everything the kernels wrote equals the CPU statement, and every frame equals the host decoder"""
    PILImage = pytest.importorskip("PIL.Image")
    files = S.intact_files(PILImage)
    prog = next(b for name, b in J.pil_matrix(PILImage) if name.endswith("prog"))
    files.insert(7, ("progressive", prog))
    plans = [S.Plan(b, piece) for _, b in files]
    assert [p.eligible for p in plans] == [i != 7 for i in range(len(files))]
    hc, hs, dc, ds = _both(eng, S.Batch(plans))
    assert np.array_equal(hs, ds) and (ds == 0).all()
    assert np.array_equal(hc, dc)
    assert (dc[7] == S.FILL16).all()
    for i, (name, _) in enumerate(files):
        if i != 7:
            S.check_frame(name, plans[i], dc[i], ds[i])


@pytest.mark.parametrize("piece", S.PIECES)
def test_damaged_scans_in_batches_of_64(eng, piece):
    """every third damaged scan (300 files, with and without DRI): the status word is zero exactly where the CPU statement's is, and
    the coefficients are equal there -- which is the host decoder's result (tests/test_jpeg_sync_cpu.py).  The host decoder accepts
    693 and refuses 147 of all eligible files, so every third gives about 230 and 50; the floors keep the test from passing by skipping."""
    PILImage = pytest.importorskip("PIL.Image")
    plans = [p for p in (S.Plan(f, piece) for f in S.damaged_scans(PILImage)[::3]) if p.eligible]
    assert len(plans) >= 250
    zero = flagged = 0
    for k in range(0, len(plans), 64):
        part = plans[k:k + 64]
        hc, hs, dc, ds = _both(eng, S.Batch(part))
        assert np.array_equal(hs == 0, ds == 0), (k, hs, ds)
        ok = hs == 0
        assert np.array_equal(hc[ok], dc[ok])
        zero, flagged = zero + int(ok.sum()), flagged + int((~ok).sum())
    assert zero >= 150 and flagged >= 30, (zero, flagged)


def test_argument_checks_through_the_device_entry_point(eng):
    import torch
    files = E.own_files()
    batch = S.Batch([S.Plan(b, 64) for _, b in files])
    big = max(p.desc.coef_elems() for p in batch.plans)
    intervals = batch.copies()[2]
    intervals[4 * batch.interval_stride + 10].end = batch.frames[4].clean_bytes + 1
    pieces = batch.copies()[2]
    pieces[4 * batch.interval_stride + 3].first_piece += 1
    bad_frames = batch.copies()[1]
    bad_frames[1].n_pieces += 300
    need = C.c_size_t()
    assert L.load().sd_jpeg_sync_workspace(batch.B, batch.interval_stride, batch.max_pieces, C.byref(need)) == L.SD_OK
    for over in (dict(intervals=intervals), dict(intervals=pieces), dict(coef_stride_bytes=(big - 64) * 2), dict(frames=bad_frames),
                 dict(workspace_bytes=need.value - 1), dict(byte_stride=batch.byte_stride + 8), dict(subseq_bytes=32)):
        st, coef, status = batch.device(eng, **over)
        assert st == L.SD_ERR_INVALID, over.keys()
        torch.cuda.synchronize()
        assert bool((coef == int(S.FILL16)).all()) and bool((status == -1).all()), over.keys()
    st, coef, status = batch.device(eng)
    assert st == L.SD_OK
    coef, status = coef.cpu().numpy(), status.cpu().numpy()
    for i, (name, _) in enumerate(files):
        S.check_frame(name, batch.plans[i], coef[i], status[i])


def _feed(paths, batch, jpeg, eng, **more):
    got, los = [], []
    kw = dict(jpeg=jpeg, engine=eng, **more) if jpeg != "host" else {}
    with frame_io.FrameFeeder(paths, batch=batch, device="cuda", workers=3, **kw) as feeder:
        for dev, lo in feeder:
            assert dev.is_cuda and dev.is_contiguous()
            got.append(dev.cpu().numpy())
            los.append(lo)
        fallback = list(feeder.sync_fallback)
    return got, los, fallback


def test_the_stream_that_never_synchronises_takes_the_host_decoder_in_the_feeder(eng, tmp_path):
    """160 x 160 gray: flagged "not synchronised" at 32-byte pieces (the CPU statement first), so the feeder names it in sync_fallback
    and its frame is the host route's; the frame before it is decoded on the GPU"""
    PILImage = pytest.importorskip("PIL.Image")
    buf = S.never_synchronising()
    plan = S.Plan(buf, 32)
    assert S.Batch([plan]).host()[2][0] == L.SD_JPEG_SYNC_NOT_SYNCHRONISED
    rng = np.random.default_rng(43)
    paths = [str(tmp_path / "a.jpg"), str(tmp_path / "b.jpg")]
    PILImage.fromarray(J._img(rng, 160, 160)).save(paths[0], "JPEG", quality=80)
    open(paths[1], "wb").write(buf)
    host, _, _ = _feed(paths, 2, "host", eng)
    devr, _, fallback = _feed(paths, 2, "device_sync", eng, sync_piece=32)
    assert fallback == [(1, "flagged")]
    assert np.array_equal(host[0], devr[0])
    devr, _, fallback = _feed(paths, 2, "device_sync", eng, sync_piece=128)      # one workgroup: its rounds carry the true state through
    assert fallback == [] and np.array_equal(host[0], devr[0])


def _mixed_folder(tmp_path, PILImage, h=48, w=80):
    """8 files of one size: Pillow files without DRI at the three samplings, Pillow restart files, the project's encoder, one
    progressive JPEG, one PNG"""
    rng = np.random.default_rng(42)
    paths = []
    for i in range(8):
        img = J._img(rng, h, w)
        p = str(tmp_path / f"f{i:03d}.{'png' if i == 5 else 'jpg'}")
        if i in (0, 3, 6):
            PILImage.fromarray(img).save(p, "JPEG", quality=88, subsampling={0: 0, 3: 1, 6: 2}[i])
        elif i in (1, 4):
            PILImage.fromarray(img).save(p, "JPEG", quality=88, subsampling=i % 3, restart_marker_rows=1)
        elif i == 2:
            PILImage.fromarray(img).save(p, "JPEG", quality=88, progressive=True)
        elif i == 7:
            open(p, "wb").write(E.own_jpeg(img, 85))
        else:
            outputs.write_png(p, img)
        paths.append(p)
    return paths


def test_feeder_sync_route_equals_the_other_routes_on_a_mixed_folder(eng, tmp_path):
    PILImage = pytest.importorskip("PIL.Image")
    paths = _mixed_folder(tmp_path, PILImage)
    host, los_h, _ = _feed(paths, 3, "host", eng)
    devc, los_c, _ = _feed(paths, 3, "device", eng)
    devs, los_s, fallback = _feed(paths, 3, "device_sync", eng)
    assert los_h == los_c == los_s == [0, 3, 6] and [g.shape for g in devs] == [g.shape for g in host]
    for a, b, c in zip(host, devc, devs):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    assert fallback == [(2, "ineligible")]                     # DRI or not, every sequential file was decoded on the GPU
    devp, _, fallback = _feed(paths, 3, "device_sync", eng, png="device")
    assert fallback == [(2, "ineligible")] and all(np.array_equal(a, b) for a, b in zip(host, devp))
    with pytest.raises(ValueError, match="sync_piece"):
        frame_io.FrameFeeder(paths, 3, jpeg="device_sync", engine=eng, sync_piece=48)


def test_run_sequence_files_passes_the_sync_route_through(eng, tmp_path):
    import torch
    from semantic_depth_amd import distributed as D
    PILImage = pytest.importorskip("PIL.Image")
    paths = _mixed_folder(tmp_path, PILImage)[:7]
    seen = []

    def step(frames, first):
        seen.append((first, frames.shape[0]))
        rows = frames.reshape(frames.shape[0], -1)
        return torch.cat([rows[:, :D.RECORD_BYTES // 2], rows[:, -(D.RECORD_BYTES // 2):]], 1).contiguous()
    res = {}
    for mode in ("host", "device", "device_sync"):
        del seen[:]
        kw = dict(jpeg=mode, engine=eng) if mode != "host" else {}
        res[mode] = D.run_sequence_files(paths, step, batch=3, device="cuda", workers=2, **kw).cpu().numpy()
        assert seen == [(0, 3), (3, 3), (6, 1)]
    assert res["host"].shape == (7, D.RECORD_BYTES)
    assert np.array_equal(res["host"], res["device"]) and np.array_equal(res["host"], res["device_sync"])
    with pytest.raises(ValueError, match="needs engine="):
        D.run_sequence_files(paths, step, batch=3, device="cuda", workers=2, jpeg="device_sync")
