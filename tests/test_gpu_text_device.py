"""GPU: the device route of the result images' banner text (text_gpu.hip through sd_text_draw_rw, Engine.draw_result_text and
make_engine_step(text="draw")) against its host statement, sd_text_draw_host on sd_text_items_rw_host, on every byte.  The yardstick is that
statement -- tests/test_text_cpu.py holds it to Python's formatter and to an independent statement of the raster rule -- never the kernels
against themselves.  The records are those of tests/text_cases.py."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import __graft_entry__ as graft
import text_cases as T
from semantic_depth_amd import _lib as L
from semantic_depth_amd import frame_io, outputs
from semantic_depth_amd.engine import RW_DTYPE

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    graft.build()
    from semantic_depth_amd.engine import Engine
    e = Engine(128, 256, 2, "resnet50")
    yield e
    e.close()


def _dev_records(recs):
    return torch.from_numpy(np.ascontiguousarray(recs).view(np.uint8).reshape(len(recs), RW_DTYPE.itemsize).copy()).cuda()


def _want(img, recs, depth=10.0):
    return np.stack([T.host_draw(img[b], *T.host_items(recs[b], img.shape[1], img.shape[2], depth)) for b in range(len(recs))])


def _batch(B):
    pool = np.concatenate([T.records(), T.special_records()])
    return pool[[i % len(pool) for i in range(B)]] if B <= len(pool) else pool


@pytest.mark.parametrize("B,h,w", [(5, 200, 640), (3, 333, 1001), (2, 1024, 2048), (9, 96, 256)])
def test_draw_result_text_equals_the_host_statement(eng, B, h, w):
    recs = _batch(B)
    img = T.prefilled(h + w, len(recs), h, w, 3)
    dev = torch.from_numpy(img).cuda()
    out = eng.draw_result_text(dev, _dev_records(recs), 10.0)
    assert out is dev
    got, want = out.cpu().numpy(), _want(img, recs)
    for b in range(len(recs)):
        assert np.array_equal(got[b], want[b]), (b, int((got[b] != want[b]).any(-1).sum()))
        assert (got[b] != img[b]).any()
    if h >= 1024:                                                      # the tool's geometry: the banner text of a found frame is not clipped at the top
        assert all(np.array_equal(got[b, 0], img[b, 0]) for b in range(len(recs)) if recs[b]["found"])


def _raw_call(eng, img, recs, fill=0, ws_bytes=None, B=None, depth=b"10.00"):
    need = eng.lib.sd_text_workspace_bytes(len(recs))
    dev = torch.from_numpy(img).cuda()
    ws = torch.full((need,), fill, dtype=torch.uint8, device="cuda")
    st = eng.lib.sd_text_draw_rw(eng.h, dev.data_ptr(), len(recs) if B is None else B, img.shape[1], img.shape[2], _dev_records(recs).data_ptr(), depth,
                                 ws.data_ptr(), need if ws_bytes is None else ws_bytes, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return st, dev.cpu().numpy(), ws.cpu().numpy()


def test_result_does_not_depend_on_the_workspace(eng):
    recs = T.records()[:4]
    img = T.prefilled(31, len(recs), 120, 700, 3)
    st0, a, _ = _raw_call(eng, img, recs, fill=0x00)
    st1, b, _ = _raw_call(eng, img, recs, fill=0xFF)
    assert st0 == st1 == L.SD_OK
    assert np.array_equal(a, b) and np.array_equal(a, _want(img, recs))


def test_argument_refusals_launch_nothing(eng):
    recs = T.records()[:2]
    img = T.prefilled(32, 2, 64, 256, 3)
    need = eng.lib.sd_text_workspace_bytes(2)
    for kw in (dict(ws_bytes=need - 1), dict(B=0), dict(depth=b"1" * 24)):
        st, out, ws = _raw_call(eng, img, recs, fill=0xA5, **kw)
        assert st == L.SD_ERR_INVALID, kw
        assert np.array_equal(out, img) and (ws == 0xA5).all(), kw
    h = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device="cuda")
    assert eng.lib.sd_text_draw_rw(eng.h, h.data_ptr(), 1, 8, 16385, _dev_records(recs).data_ptr(), b"10.00", h.data_ptr(), 1 << 20, None) == L.SD_ERR_INVALID


class _FoundEngine:
    """the engine, except that process_batch's records of frames 0 and 2 of a batch are replaced, on the device, by found records of
    tests/text_cases.py: the seeded weights find no road line on the test's frames, and the route is mainly for frames that have one"""

    def __init__(self, eng):
        self._eng = eng
        self._found = _dev_records(T.records()[[0, 2]])

    def __getattr__(self, name):
        return getattr(self._eng, name)

    def process_batch(self, *a, **k):
        out = self._eng.process_batch(*a, **k)
        out["records"][0].copy_(self._found[0])
        out["records"][2].copy_(self._found[1])
        return out


def test_run_sequence_files_draws_the_text_on_both_png_routes(tmp_path):
    """the driver on the geometry of tests/test_gpu_sequence_outputs.py (4 frames, one batch, two of them made found: _FoundEngine): with
    text="draw" the decoded PNGs of both routes are the composed images (what the default run writes) with the host statement drawn on
    them; with text="json" the files are the bytes of a run without the argument"""
    import test_gpu_sequence_outputs as S
    from semantic_depth_amd import weights as W
    from semantic_depth_amd.distributed import make_engine_step, run_sequence_files
    from semantic_depth_amd.engine import Engine, RoadWidthParams
    frames = S._smooth_frames(np.random.default_rng(21), 4, 2 * S.H, 2 * S.W_, cell=16)
    src = tmp_path / "in"
    src.mkdir()
    paths = [outputs.write_png(str(src / f"city_{i:03d}_leftImg8bit.png"), frames[i], level=1) for i in range(len(frames))]
    e = Engine(S.H, S.W_, 4, "resnet50", precision="bf16x3")
    try:
        e.load_weights(L.SD_NET_FCN8S, W.make_fcn8s_weights(1, decoder_std=0.05))
        wm = W.make_monodepth_weights("resnet50", 2)
        wm["dec/disp1/biases"] = (wm["dec/disp1/biases"] + np.float32(-1.5)).astype(np.float32)
        e.load_weights(L.SD_NET_MONODEPTH, wm)
        prm, names = RoadWidthParams(), outputs.sequence_names(paths)
        rec = {}
        for key, kw in (("plain", {}), ("json", dict(text="json")), ("draw_host", dict(text="draw", png="host")), ("draw_device", dict(text="draw", png="device"))):
            outs = outputs.SequenceOutputs(str(tmp_path / key), names, depth=prm.depth, threads=8, ply=False)
            rec[key] = run_sequence_files(paths, make_engine_step(_FoundEngine(e), lambda i: S.CAM, prm, outputs=outs), batch=4, device="cuda", **kw).cpu()
            assert json.load(open(outs.manifest))["status"] == "ok"
    finally:
        e.close()
    recs = rec["plain"].numpy().view(RW_DTYPE).reshape(-1)
    R_banner_rows = int(0.25 * 2 * S.H) + 1                            # cv2.rectangle's corners are inclusive
    for key in ("json", "draw_host", "draw_device"):
        assert torch.equal(rec[key], rec["plain"])
    assert recs["found"][0] and recs["found"][2] and not recs["found"].all(), recs["found"]          # both layouts go through the driver
    for i, name in enumerate(names):
        files = {k: str(tmp_path / k / outputs.SEQ_IMG_DIR / name) for k in rec}
        assert open(files["json"] + ".png", "rb").read() == open(files["plain"] + ".png", "rb").read(), name
        composed = frame_io.imread(files["plain"] + ".png")
        want = T.host_draw(composed, *T.host_items(recs[i], composed.shape[0], composed.shape[1], prm.depth))
        assert (want != composed).any()
        assert (composed[:R_banner_rows] == [156, 157, 159]).all() == bool(recs[i]["found"])
        for key in ("draw_host", "draw_device"):
            assert np.array_equal(frame_io.imread(files[key] + ".png"), want), (name, key)
            assert open(files[key] + "_overlay.json", "rb").read() == open(files["plain"] + "_overlay.json", "rb").read(), (name, key)
