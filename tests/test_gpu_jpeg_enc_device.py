"""GPU: the device JPEG encoder of the result video (jpeg_enc_gpu.hip through sd_jpeg_encode_bgr and Engine.encode_jpeg) against its host
statement sd_jpeg_encode_bgr_host, byte for byte.  The yardstick is that function -- tests/test_jpeg_enc_cpu.py holds it to the project's
coefficient reader, a float64 DCT and PIL -- never the kernels against themselves.  The frames are those of tests/jpeg_enc_cases.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import __graft_entry__ as graft
import jpeg_enc_cases as JC
from semantic_depth_amd import _lib as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    graft.build()
    from semantic_depth_amd.engine import Engine
    e = Engine(128, 256, 2, "resnet50")
    yield e
    e.close()


def _raw_call(eng, imgs, quality, stride=None, ws_bytes=None, h=None, w=None, B=None, fill=0xA5, ws_offset=0, frame_stride=None):
    """sd_jpeg_encode_bgr through the C ABI with every buffer pre-filled: (status, streams [B, stride], sizes, flags)"""
    n, ih, iw = imgs.shape[:3]
    need, bound = C.c_size_t(), C.c_size_t()
    assert eng.lib.sd_jpeg_encode_workspace(n, ih, iw, C.byref(need), C.byref(bound)) == L.SD_OK
    assert bound.value == JC.bound(ih, iw)
    stride = bound.value if stride is None else stride
    dev = torch.from_numpy(np.ascontiguousarray(imgs)).cuda()
    streams = torch.full((n, max(stride, 1)), fill, dtype=torch.uint8, device="cuda")
    sizes = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    flags = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    ws = torch.full((need.value + 16,), fill, dtype=torch.uint8, device="cuda")
    st = eng.lib.sd_jpeg_encode_bgr(eng.h, dev.data_ptr(), ih * iw * 3 if frame_stride is None else frame_stride, n if B is None else B,
                                    ih if h is None else h, iw if w is None else w, quality, streams.data_ptr(), stride, sizes.data_ptr(),
                                    flags.data_ptr(), ws.data_ptr() + ws_offset, need.value if ws_bytes is None else ws_bytes,
                                    torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return st, streams.cpu().numpy(), sizes.cpu().numpy(), flags.cpu().numpy()


def _assert_same(got, want, what):
    if got != want:
        first = next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), min(len(got), len(want)))
        raise AssertionError(f"{what}: first differing byte {first} of {len(want)} (got {len(got)})")


@pytest.mark.parametrize("name", JC.CASE_NAMES)
def test_every_case_is_the_bytes_of_the_host_statement(eng, name):
    img, quality = JC.cases()[name]
    want = JC.host_stream(name)
    streams, sizes, flags = eng.encode_jpeg(torch.from_numpy(img[None]).cuda(), quality=quality)
    torch.cuda.synchronize()
    assert streams.dtype == torch.uint8 and sizes.dtype == torch.int64 and flags.dtype == torch.int32
    assert tuple(streams.shape) == (1, JC.bound(*img.shape[:2]))
    assert int(flags[0]) == 0 and int(sizes[0]) == len(want), (int(flags[0]), int(sizes[0]), len(want))
    _assert_same(streams[0, :len(want)].cpu().numpy().tobytes(), want, name)


def _batch():
    """five frames of one geometry whose files differ in size by orders of magnitude; 3 strips of MCUs per row and 5 MCU rows"""
    h, w = 70, 260
    rng = np.random.default_rng(77)
    imgs = np.stack([
        np.full((h, w, 3), (10, 20, 30), np.uint8),
        rng.integers(0, 256, (h, w, 3), dtype=np.uint8),
        JC.mixed_frame(1, h, w),
        np.ascontiguousarray(JC.smooth_frame(2, h, w)),
        np.ascontiguousarray(np.repeat(np.where((np.add.outer(np.arange(h) >> 3, np.arange(w) >> 3) & 1)[..., None], 255, 0), 3, axis=2)).astype(np.uint8),
    ])
    return imgs, 100


@pytest.fixture(scope="module")
def batch_want():
    imgs, q = _batch()
    want = [JC.encode_host(im, q) for im in imgs]
    assert len(want[1]) > 30 * len(want[0])
    return imgs, q, want


@pytest.mark.parametrize("fill", [0x00, 0xFF])
def test_batch_sizes_flags_streams_whatever_the_buffers_held(eng, batch_want, fill):
    imgs, q, want = batch_want
    st, streams, sizes, flags = _raw_call(eng, imgs, q, fill=fill)
    assert st == L.SD_OK
    assert sizes.tolist() == [len(x) for x in want] and flags.tolist() == [0] * 5
    for b in range(5):
        _assert_same(streams[b, :len(want[b])].tobytes(), want[b], f"frame {b}")
        assert (streams[b, len(want[b]):] == fill).all(), b


def test_a_short_stride_flags_only_the_frames_that_do_not_fit(eng, batch_want):
    imgs, q, want = batch_want
    sizes_want = [len(x) for x in want]
    stride = (sorted(sizes_want)[-1] + sorted(sizes_want)[-2]) // 2                # between the noise frame and every other
    assert sizes_want[1] > stride > max(s for i, s in enumerate(sizes_want) if i != 1) and stride > sizes_want[0]
    st, streams, sizes, flags = _raw_call(eng, imgs, q, stride=stride)
    assert st == L.SD_OK
    assert flags.tolist() == [0, 1, 0, 0, 0] and sizes.tolist() == [s if i != 1 else 0 for i, s in enumerate(sizes_want)]
    assert (streams[1] == 0xA5).all()
    for b in (0, 2, 3, 4):
        _assert_same(streams[b, :len(want[b])].tobytes(), want[b], f"frame {b}")
        assert (streams[b, len(want[b]):] == 0xA5).all()


def test_argument_refusals_launch_nothing(eng, batch_want):
    imgs = batch_want[0][:2]
    h, w = imgs.shape[1:3]
    for kw in (dict(h=0), dict(w=0), dict(h=16385), dict(w=16385), dict(B=0), dict(quality=0), dict(quality=101), dict(frame_stride=h * w * 3 - 1),
               dict(stride=JC.HEADER_LEN - 1), dict(ws_bytes=16), dict(ws_offset=8)):
        kw = dict(kw)
        quality = kw.pop("quality", 90)
        st, streams, sizes, flags = _raw_call(eng, imgs, quality, **kw)
        assert st == L.SD_ERR_INVALID, kw
        assert (streams == 0xA5).all() and (sizes == -1).all() and (flags == -7).all(), kw


def test_engine_stream_stride(eng, batch_want):
    imgs, q, want = batch_want
    stride = len(want[1]) + 3
    streams, sizes, flags = eng.encode_jpeg(torch.from_numpy(imgs).cuda(), quality=q, stream_stride=stride)
    torch.cuda.synchronize()
    assert tuple(streams.shape) == (5, stride) and flags.tolist() == [0] * 5 and sizes.tolist() == [len(x) for x in want]
    _assert_same(streams[1, :len(want[1])].cpu().numpy().tobytes(), want[1], "noise frame")


def test_run_sequence_files_writes_the_video_on_both_png_routes(tmp_path):
    """the driver on the geometry of tests/test_gpu_sequence_outputs.py, 4 frames in batches of 2, text="draw": the AVI of the device route is
    the host route's bytes on either PNG route, and every frame decodes to within 0.5 dB of PIL's own file of the PNG written beside it"""
    import io
    import json
    PILImage = pytest.importorskip("PIL.Image")
    import test_gpu_sequence_outputs as S
    from semantic_depth_amd import frame_io, outputs
    from semantic_depth_amd import weights as W
    from semantic_depth_amd.distributed import make_engine_step, run_sequence_files
    from semantic_depth_amd.engine import Engine, RoadWidthParams
    frames = S._smooth_frames(np.random.default_rng(23), 4, 2 * S.H, 2 * S.W_, cell=16)
    src = tmp_path / "in"
    src.mkdir()
    paths = [outputs.write_png(str(src / f"city_{i:03d}_leftImg8bit.png"), frames[i], level=1) for i in range(len(frames))]
    e = Engine(S.H, S.W_, 2, "resnet50", precision="bf16x3")
    runs = (("host", "device"), ("device", "device"), ("host", "host"))
    man = {}
    try:
        e.load_weights(L.SD_NET_FCN8S, W.make_fcn8s_weights(1, decoder_std=0.05))
        wm = W.make_monodepth_weights("resnet50", 2)
        wm["dec/disp1/biases"] = (wm["dec/disp1/biases"] + np.float32(-1.5)).astype(np.float32)
        e.load_weights(L.SD_NET_MONODEPTH, wm)
        prm, names = RoadWidthParams(), outputs.sequence_names(paths)
        for png, route in runs:
            outs = outputs.SequenceOutputs(str(tmp_path / (png + route)), names, depth=prm.depth, threads=8, ply=False)
            run_sequence_files(paths, make_engine_step(e, lambda i: S.CAM, prm, outputs=outs), batch=2, device="cuda", png=png, text="draw",
                               video=outputs.Video(fps=25, quality=90, route=route))
            man[png + route] = json.load(open(outs.manifest))
    finally:
        e.close()
    avis = {}
    for png, route in runs:
        m = man[png + route]
        assert m["status"] == "ok" and m["video"] == ["result_imgs.avi"] and m["video_fallback"] == []
        avis[png + route] = open(str(tmp_path / (png + route) / "result_imgs.avi"), "rb").read()
    assert avis["hostdevice"] == avis["hosthost"] and avis["devicedevice"] == avis["hosthost"]

    def psnr(a, b):
        return 10.0 * np.log10(255.0 ** 2 / max(1e-12, np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))

    for png in ("host", "device"):
        got = list(frame_io.avi_frames(str(tmp_path / (png + "device") / "result_imgs.avi")))
        assert len(got) == len(names)
        for name, jpg in zip(names, got):
            ref = frame_io.imread(str(tmp_path / (png + "device") / outputs.SEQ_IMG_DIR / (name + ".png")))
            buf = io.BytesIO()
            PILImage.fromarray(ref[..., ::-1]).save(buf, "JPEG", quality=90, subsampling=2)
            ours, pil = psnr(frame_io.decode_jpeg(jpg), ref), psnr(frame_io.decode_jpeg(buf.getvalue()), ref)
            print(f"{png} {name}: ours {ours:.2f} dB, PIL {pil:.2f} dB, {len(jpg)} B")
            assert ours >= pil - 0.5, (name, ours, pil)
