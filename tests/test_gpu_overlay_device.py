"""GPU: the device route of the measurement lines (overlay_gpu.hip through sd_overlay_draw, Engine.draw_result_lines and
make_engine_step(lines=)) against its host statement, sd_overlay_draw_host on sd_overlay_segments_host, on every byte and every flag.  The
yardstick is that statement -- tests/test_overlay_cpu.py holds it to an independent statement of the rule -- never the kernels against
themselves.  The records, profiles and cameras are those of tests/overlay_cases.py."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import __graft_entry__ as graft
import overlay_cases as O
from semantic_depth_amd import _lib as L
from semantic_depth_amd import frame_io, outputs
from semantic_depth_amd.engine import RW_DTYPE

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    graft.build()
    from semantic_depth_amd.engine import Engine
    e = Engine(O.NET[0], O.NET[1], 2, "resnet50")
    yield e
    e.close()


def _dev(a):
    """a structured array [...] as a u8 [..., itemsize] device tensor; None stays None"""
    if a is None:
        return None
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(a.shape + (a.dtype.itemsize,)).copy()).cuda()


SHAPES = [dict(B=1, h=16, w=64), dict(B=3, h=37, w=130), dict(B=5, h=120, w=700), dict(B=5, h=120, w=700, fence=False),
          dict(B=5, h=120, w=700, D=7), dict(B=5, h=120, w=700, D=7, fence=False), dict(B=5, h=120, w=700, D=256),
          dict(B=5, h=120, w=700, D=256, fence=False), dict(B=11, h=37, w=130, thickness=1), dict(B=4, h=120, w=200, D=7, thickness=32,
                                                                                                  profile_thickness=32, clip_top=60, first=2),
          dict(B=11, h=150, w=333, D=1, first=5, profile_thickness=2, clip_top=17)]


@pytest.mark.parametrize("kw", SHAPES, ids=lambda k: "-".join(f"{a}{b}" for a, b in k.items()))
def test_draw_result_lines_equals_the_host_statement(eng, kw):
    c = O.build(seed=sum(kw.values()), **kw)
    img = O.prefilled(c["h"] + c["w"], c["B"], c["h"], c["w"], 3)
    dev = torch.from_numpy(img).cuda()
    out, flags = eng.draw_result_lines(dev, _dev(c["records"]), c["cams"], c["lines"], f2f=_dev(c["f2f"]), profile=_dev(c["profile"]),
                                       f2f_profile=_dev(c["f2f_profile"]), clip_top=c["clip_top"])
    assert out is dev
    got, want = out.cpu().numpy(), O.host_draw(img, c)
    for b in range(c["B"]):
        assert np.array_equal(got[b], want[0][b]), (b, int((got[b] != want[0][b]).any(-1).sum()))
    assert np.array_equal(flags.cpu().numpy(), want[1]) and np.array_equal(want[1], c["flags"])
    assert (got != img).any() and (got == img).all(-1).any()


def _raw_call(eng, img, c, fill=0, **over):
    """sd_overlay_draw with the case's arguments, `over` replacing some: (status, image, flags, workspace) afterwards"""
    B, D = c["B"], c["D"]
    need = eng.lib.sd_overlay_workspace_bytes(B, D)
    dev = torch.from_numpy(img).cuda()
    ws = torch.full((need,), fill, dtype=torch.uint8, device="cuda")
    flags = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    cams = (L.sd_camera * B)(*[L.sd_camera(k.cx, k.cy, k.f, k.b, k.disp_mult) for k in c["cams"]])
    rec, f2, pr, fpr = _dev(c["records"]), _dev(c["f2f"]), _dev(c["profile"]), _dev(c["f2f_profile"])
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())      # noqa: E731
    style = over.get("style", c["lines"].struct(c["clip_top"]))
    st = eng.lib.sd_overlay_draw(eng.h, dev.data_ptr(), over.get("B", B), c["h"], c["w"], O.NET[0], O.NET[1], cams, ptr(rec), ptr(f2),
                                 None if over.get("no_profile") else ptr(pr), ptr(fpr), over.get("D", D), C.byref(style), flags.data_ptr(),
                                 ws.data_ptr(), over.get("ws_bytes", need), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return st, dev.cpu().numpy(), flags.cpu().numpy(), ws.cpu().numpy()


def test_result_does_not_depend_on_the_workspace(eng):
    c = O.build(B=5, h=120, w=700, D=7, seed=31)
    img = O.prefilled(31, c["B"], c["h"], c["w"], 3)
    st0, a, fa, _ = _raw_call(eng, img, c, fill=0x00)
    st1, b, fb, _ = _raw_call(eng, img, c, fill=0xFF)
    want, wflags = O.host_draw(img, c)
    assert st0 == st1 == L.SD_OK
    assert np.array_equal(a, b) and np.array_equal(fa, fb) and np.array_equal(a, want) and np.array_equal(fa, wflags)


def test_argument_refusals_launch_nothing(eng):
    c = O.build(B=2, h=64, w=256, D=7, seed=32)
    img = O.prefilled(32, c["B"], c["h"], c["w"], 3)
    need = eng.lib.sd_overlay_workspace_bytes(c["B"], c["D"])
    thin = c["lines"].struct(0)
    thin.thickness = 0
    for over in (dict(ws_bytes=need - 1), dict(B=0), dict(D=257), dict(style=thin), dict(no_profile=True)):
        st, out, flags, ws = _raw_call(eng, img, c, fill=0xA5, **over)
        assert st == L.SD_ERR_INVALID, over
        assert np.array_equal(out, img) and (flags == -7).all() and (ws == 0xA5).all(), over
    st, out, flags, _ = _raw_call(eng, img, c, fill=0xA5)
    assert st == L.SD_OK and (out != img).any() and (flags != -7).all()


class _FoundEngine:
    """the engine, except that process_batch's records of frames 0 and 2 of a batch are replaced on the device: the seeded weights find no road
    line on the test's frames.  Frame 0 gets a line in front of the camera (it is drawn), frame 2 tests/text_cases.py's record, whose end
    points lie behind it (Z > 0: the line is skipped and the frame flagged)."""

    def __init__(self, eng):
        import text_cases as T
        self._eng = eng
        front = T.record()
        front["left_pt"], front["right_pt"] = (np.float32(-3.4150002), -1.6, -10.0), (np.float32(0.125), -1.6, -10.0)
        found = np.zeros((2,), RW_DTYPE)
        found[0], found[1] = front, T.records()[2]
        self._found = _dev(found)

    def __getattr__(self, name):
        return getattr(self._eng, name)

    def process_batch(self, *a, **k):
        out = self._eng.process_batch(*a, **k)
        out["records"][0].copy_(self._found[0])
        out["records"][2].copy_(self._found[1])
        return out


def test_run_sequence_files_draws_the_lines_on_both_png_routes(tmp_path):
    """the driver on the geometry of tests/test_gpu_text_device.py (4 frames, one batch, two of them made found: _FoundEngine): with
    lines=OverlayLines() and text="draw" the decoded PNGs of both routes are the composed images (what the default run writes) with the host
    lines and then the host text drawn on them, and the _overlay.json files carry the same segments; with lines=None every file is the
    bytes of a run without the argument"""
    import test_gpu_sequence_outputs as S
    import text_cases as T
    from semantic_depth_amd import weights as W
    from semantic_depth_amd.distributed import make_engine_step, run_sequence_files
    from semantic_depth_amd.engine import Engine, RoadWidthParams
    frames = S._smooth_frames(np.random.default_rng(21), 4, 2 * S.H, 2 * S.W_, cell=16)
    src = tmp_path / "in"
    src.mkdir()
    paths = [outputs.write_png(str(src / f"city_{i:03d}_leftImg8bit.png"), frames[i], level=1) for i in range(len(frames))]
    lines = outputs.OverlayLines()
    e = Engine(S.H, S.W_, 4, "resnet50", precision="bf16x3")
    try:
        e.load_weights(L.SD_NET_FCN8S, W.make_fcn8s_weights(1, decoder_std=0.05))
        wm = W.make_monodepth_weights("resnet50", 2)
        wm["dec/disp1/biases"] = (wm["dec/disp1/biases"] + np.float32(-1.5)).astype(np.float32)
        e.load_weights(L.SD_NET_MONODEPTH, wm)
        prm, names = RoadWidthParams(), outputs.sequence_names(paths)
        rec, manifest = {}, {}
        for key, kw in (("plain", {}), ("none", dict(lines=None)), ("host", dict(lines=lines, text="draw", png="host")),
                        ("device", dict(lines=lines, text="draw", png="device"))):
            outs = outputs.SequenceOutputs(str(tmp_path / key), names, depth=prm.depth, threads=8, ply=False)
            rec[key] = run_sequence_files(paths, make_engine_step(_FoundEngine(e), lambda i: S.CAM, prm, outputs=outs), batch=4, device="cuda", **kw).cpu()
            manifest[key] = json.load(open(outs.manifest))
            assert manifest[key]["status"] == "ok"
    finally:
        e.close()
    recs = rec["plain"].numpy().view(RW_DTYPE).reshape(-1)
    for key in ("none", "host", "device"):
        assert torch.equal(rec[key], rec["plain"])
    assert manifest["none"] == manifest["plain"] and "lines" not in manifest["plain"]
    for key in ("host", "device"):
        assert manifest[key]["lines"] == lines.as_dict() and manifest[key]["lines_flagged"] == [names[2]], manifest[key]
    for i, name in enumerate(names):
        files = {k: str(tmp_path / k / outputs.SEQ_IMG_DIR / name) for k in rec}
        for ext in (".png", "_overlay.json"):
            assert open(files["none"] + ext, "rb").read() == open(files["plain"] + ext, "rb").read(), (name, ext)
        composed = frame_io.imread(files["plain"] + ".png")
        h, w = composed.shape[:2]
        segs, flag = outputs.overlay_segments(recs[i], S.CAM, (S.H, S.W_), (h, w), lines, clip_top=int(0.25 * h))
        if i in (0, 2):                                                    # the drawn line and the skipped one
            assert (len(segs), flag) == ((1, 0) if i == 0 else (0, 1)), (i, len(segs), flag)
        lined = outputs.draw_lines(composed, segs, int(0.25 * h))
        assert (lined != composed).any() == (len(segs) > 0)
        want = T.host_draw(lined, *T.host_items(recs[i], h, w, prm.depth))
        plain_doc = json.load(open(files["plain"] + "_overlay.json"))
        for key in ("host", "device"):
            assert np.array_equal(frame_io.imread(files[key] + ".png"), want), (name, key)
            doc = json.load(open(files[key] + "_overlay.json"))
            assert doc.pop("lines") == outputs.segments_json(segs) and doc == plain_doc, (name, key)
