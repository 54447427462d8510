"""GPU: the device route of the result images (png_gpu.hip through sd_png_encode_bgr, Engine.encode_png and
SequenceOutputs(png="device")) against its host statement sd_png_encode_zlib_host, byte for byte.  The yardstick is that function --
tests/test_png_device_cpu.py holds it to zlib's inflater and a numpy statement of the Paeth rows -- never the kernels against themselves.
The frames are those of tests/png_device_cases.py."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import __graft_entry__ as graft
import png_device_cases as P
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


def _compare(eng, imgs):
    """Engine.encode_png on the batch against the host statement on each frame; the stream buffer is filled with 0xA5 behind the sizes"""
    imgs = np.ascontiguousarray(imgs, np.uint8)
    streams, sizes = eng.encode_png(torch.from_numpy(imgs).cuda())
    torch.cuda.synchronize()
    assert streams.dtype == torch.uint8 and sizes.dtype == torch.int64 and tuple(streams.shape) == (len(imgs), P.bound(*imgs.shape[1:3]))
    st, sz = streams.cpu().numpy(), sizes.cpu().numpy()
    for b, img in enumerate(imgs):
        want = P.encode_host(img)
        assert int(sz[b]) == len(want), (b, int(sz[b]), len(want))
        got = st[b, :len(want)].tobytes()
        if got != want:
            first = next(i for i in range(len(want)) if got[i] != want[i])
            raise AssertionError(f"frame {b}: first differing byte {first} of {len(want)}")
    return st, sz


def _frames(seed, B, h, w):
    rng = np.random.default_rng(seed)
    out = np.empty((B, h, w, 3), np.uint8)
    for b in range(B):
        f = (rng.integers(0, 256, (h, w, 3)) // (8 << b) * (8 << b)).astype(np.uint8)       # coarser steps frame by frame: more and longer runs
        f[: h // 4] = (159, 157, 156) if b != 1 else f[: h // 4]
        if b == 2:
            f[:, w // 2:] = rng.integers(0, 256, (h, w - w // 2, 3), dtype=np.uint8)
        out[b] = f
    return out


@pytest.mark.parametrize("h,w", [(37, 53), (96, 700)])
def test_streams_are_the_bytes_of_the_host_statement(eng, h, w):
    _compare(eng, _frames(h + w, 3, h, w))


def test_forced_residual_streams(eng):
    by_shape = {}
    for name, (h, w, flat) in P.forced_cases().items():
        by_shape.setdefault((h, w), []).append(P.forced(h, w, flat)[0])
    assert len(by_shape) >= 5
    for imgs in by_shape.values():
        _compare(eng, np.stack(imgs))


@pytest.mark.parametrize("n", [P.CHUNK - 1, P.CHUNK, P.CHUNK + 1])
def test_frames_at_the_chunk_size(eng, n):
    h, w = P.shape_for(n)
    _compare(eng, _frames(n, 2, h, w))


def test_noise_frame_takes_the_stored_fallback(eng):
    img = np.random.default_rng(5).integers(0, 256, (1, 96, 700, 3), dtype=np.uint8)
    st, sz = _compare(eng, img)
    assert int(sz[0]) == 96 * 2101 + 10 * 7 + 11


def _raw_call(eng, imgs, stride=None, ws_bytes=None, h=None, w=None, fill=0xA5):
    B, ih, iw = imgs.shape[:3]
    h, w = ih if h is None else h, iw if w is None else w
    need, bound = C.c_size_t(), C.c_size_t()
    assert eng.lib.sd_png_encode_workspace(B, ih, iw, C.byref(need), C.byref(bound)) == L.SD_OK
    stride = bound.value if stride is None else stride
    ws_bytes = need.value if ws_bytes is None else ws_bytes
    dev = torch.from_numpy(imgs).cuda()
    streams = torch.full((B, max(stride, bound.value)), fill, dtype=torch.uint8, device="cuda")
    sizes = torch.full((B,), -1, dtype=torch.int64, device="cuda")
    ws = torch.empty((need.value,), dtype=torch.uint8, device="cuda")
    st = eng.lib.sd_png_encode_bgr(eng.h, dev.data_ptr(), ih * iw * 3, B, h, w, streams.data_ptr(), stride, sizes.data_ptr(), ws.data_ptr(), ws_bytes,
                                   torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return st, streams.cpu().numpy(), sizes.cpu().numpy()


def test_bytes_behind_the_size_are_not_written(eng):
    imgs = _frames(11, 3, 37, 53)
    st, streams, sizes = _raw_call(eng, imgs)
    assert st == L.SD_OK
    for b in range(3):
        want = P.encode_host(imgs[b])
        assert int(sizes[b]) == len(want) and streams[b, :len(want)].tobytes() == want
        assert (streams[b, len(want):] == 0xA5).all()


def test_argument_refusals_launch_nothing(eng):
    imgs = _frames(12, 2, 37, 53)
    bound = P.bound(37, 53)
    for kw in (dict(stride=bound - 1), dict(ws_bytes=1024), dict(h=0), dict(w=0), dict(h=16385), dict(w=16385)):
        st, streams, sizes = _raw_call(eng, imgs, **kw)
        assert st == L.SD_ERR_INVALID, kw
        assert (streams == 0xA5).all() and (sizes == -1).all(), kw


def test_run_sequence_files_device_route_writes_the_host_route_s_images(tmp_path):
    """the driver at B = 8 on the geometry of tests/test_gpu_sequence_outputs.py, once per route: same names, same pixels, same records,
    and no device-route file larger than its host-route twin"""
    import test_gpu_sequence_outputs as S
    from semantic_depth_amd import weights as W
    from semantic_depth_amd.distributed import make_engine_step, run_sequence_files
    from semantic_depth_amd.engine import Engine, RoadWidthParams
    frames = S._smooth_frames(np.random.default_rng(21), 8, 2 * S.H, 2 * S.W_, cell=16)
    src = tmp_path / "in"
    src.mkdir()
    paths = [outputs.write_png(str(src / f"city_{i:03d}_leftImg8bit.png"), frames[i], level=1) for i in range(len(frames))]
    e = Engine(S.H, S.W_, 8, "resnet50", precision="bf16x3")
    try:
        e.load_weights(L.SD_NET_FCN8S, W.make_fcn8s_weights(1, decoder_std=0.05))
        wm = W.make_monodepth_weights("resnet50", 2)
        wm["dec/disp1/biases"] = (wm["dec/disp1/biases"] + np.float32(-1.5)).astype(np.float32)
        e.load_weights(L.SD_NET_MONODEPTH, wm)
        prm, names = RoadWidthParams(), outputs.sequence_names(paths)
        rec, man = {}, {}
        for route in ("host", "device"):
            outs = outputs.SequenceOutputs(str(tmp_path / route), names, depth=prm.depth, threads=8, png=route)
            rec[route] = run_sequence_files(paths, make_engine_step(e, lambda i: S.CAM, prm, outputs=outs), batch=8, device="cuda").cpu()
            man[route] = json.load(open(outs.manifest))
    finally:
        e.close()
    assert torch.equal(rec["host"], rec["device"])
    assert man["host"]["files"] == man["device"]["files"] and len(man["host"]["files"]) == 3 * len(names)
    assert man["device"]["status"] == "ok"
    for name in names:
        ph, pd = (str(tmp_path / r / outputs.SEQ_IMG_DIR / (name + ".png")) for r in ("host", "device"))
        assert np.array_equal(frame_io.imread(ph), frame_io.imread(pd)), name
        print(f"{name}: host route {os.path.getsize(ph)} B, device route {os.path.getsize(pd)} B")
        assert os.path.getsize(pd) <= os.path.getsize(ph), name
        for kind, ext in ((outputs.SEQ_IMG_DIR, "_overlay.json"), (outputs.SEQ_PLY_DIR, "_rw.ply")):
            a, b = (open(str(tmp_path / r / kind / (name + ext)), "rb").read() for r in ("host", "device"))
            assert a == b, (name, ext)
