"""GPU: the device route of the disparity images (disp_image_gpu.hip through sd_disp_image, Engine.disparity_image and
make_engine_step(disp=)) against its host statement, sd_disp_image_host, on every byte and flag.  The yardstick is that statement --
tests/test_disp_image_cpu.py holds it to what scipy.misc.imresize + plt.imsave leave -- never the kernels against themselves."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import __graft_entry__ as graft
from semantic_depth_amd import _lib as L
from semantic_depth_amd import frame_io, outputs

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "disp_image.npz")


@pytest.fixture(scope="module")
def eng():
    graft.build()
    from semantic_depth_amd.engine import Engine
    e = Engine(128, 256, 2, "resnet50")
    yield e
    e.close()


def _maps(seed, B, h, w):
    """B maps of very different ranges (frame b spans about 10^(b - 2)), some negative"""
    rng = np.random.default_rng(seed)
    d = rng.random((B, h, w), dtype=np.float32)
    for b in range(B):
        d[b] = d[b] * np.float32(10.0 ** (b % 5 - 2)) - np.float32(0.3 * (b % 2))
    return d


def _both(eng, disp, oh, ow, cmap, mults=None, out=None):
    """(device images, device flags, host images, host flags) as numpy arrays"""
    got, flags = eng.disparity_image(torch.from_numpy(disp).cuda(), oh, ow, cmap, mults=mults, out=out)
    want, wflags = outputs.disparity_image(disp, oh, ow, cmap, mults)
    return got.cpu().numpy(), flags.cpu().numpy(), want, wflags


def _same(eng, disp, oh, ow, cmap, mults=None):
    got, flags, want, wflags = _both(eng, disp, oh, ow, cmap, mults)
    assert np.array_equal(flags, wflags), (flags, wflags)
    assert np.array_equal(got, want), (disp.shape, (oh, ow), cmap, np.argwhere(got != want)[:3])
    return got


def test_golden_cases_equal_the_host_twin_and_imsave(eng):
    golden = np.load(GOLDEN)
    for name in [str(n) for n in golden["names"]]:
        disp, mults = golden[name + "/disp"], golden[name + "/mults"]
        oh, ow = (int(v) for v in golden[name + "/size"])
        for cmap in outputs.DISP_MAPS:
            got = _same(eng, disp, oh, ow, cmap, mults)
            assert np.array_equal(got[..., ::-1], golden[f"{name}/{cmap}"]), (name, cmap)


@pytest.mark.parametrize("B,h,w,oh,ow", [(1, 64, 128, 100, 260), (5, 64, 128, 100, 260), (1, 128, 256, 128, 256), (5, 128, 256, 128, 256),
                                         (3, 7, 13, 9, 11),         # frames * pixels not divisible by 4: the one-pixel-per-lane forms
                                         (3, 64, 128, 9, 11),       # vector input, byte output; shrink
                                         (2, 9, 13, 20, 40),        # byte input, vector output
                                         (2, 300, 200, 37, 50)])    # more than one workgroup per frame in the input passes
def test_sizes_and_batches_equal_the_host_twin(eng, B, h, w, oh, ow):
    disp = _maps(B * 1000 + h, B, h, w)
    mults = [1.0, 3800.0, 2048.0, 0.5, 3800.0][:B]
    for cmap in outputs.DISP_MAPS:
        _same(eng, disp, oh, ow, cmap, mults)
    _same(eng, disp, oh, ow, "gray", None)


def test_non_finite_pixels(eng):
    disp = _maps(9, 4, 16, 24)
    disp[0, 3, 5], disp[0, 0, 0], disp[0, 15, 23] = np.nan, np.inf, -np.inf
    disp[2] = np.nan                                       # nothing finite: lo = 0, cs = 1, every byte 0, entry 0 of the map
    disp[3, 8, 8] = 3.0e38                                 # finite, but times 3800 it is not
    got, flags, want, wflags = _both(eng, disp, 20, 30, "plasma", [1.0, 1.0, 1.0, 3800.0])
    assert flags.tolist() == [1, 0, 1, 1] and np.array_equal(flags, wflags)
    assert np.array_equal(got, want)
    assert (got[2] == np.array([134, 7, 12], np.uint8)).all()
    # hi - lo beyond the float32 range: scale 0, and the rule's byte 0 for the product that is not a number
    wide = _maps(10, 1, 8, 16)
    wide[0, 0, 0], wide[0, 7, 15] = 3.0e38, -3.0e38
    _same(eng, wide, 8, 16, "gray")


def test_a_frame_alone_and_in_a_batch_and_twice(eng):
    disp = _maps(3, 5, 64, 128)
    mults = [3800.0, 1.0, 2.0, 3800.0, 0.25]
    whole = _same(eng, disp, 100, 260, "plasma", mults)
    again = _same(eng, disp, 100, 260, "plasma", mults)
    assert np.array_equal(whole, again)
    for b in (0, 3, 4):
        alone = _same(eng, disp[b:b + 1], 100, 260, "plasma", mults[b:b + 1])
        assert np.array_equal(alone[0], whole[b]), b
    other = disp[::-1].copy()                              # the same frame among other frames, at another position
    rev = _same(eng, other, 100, 260, "plasma", mults[::-1])
    assert np.array_equal(rev[4], whole[0]) and np.array_equal(rev[1], whole[3])


def test_out_view_at_an_odd_byte_offset(eng):
    disp = _maps(4, 2, 16, 32)
    want, _ = outputs.disparity_image(disp, 20, 40, "plasma")
    n = want.size
    for offset in (1, 2, 3, 4):
        buf = torch.full((n + 16,), 0xA5, dtype=torch.uint8, device="cuda")
        view = buf[offset:offset + n].view(2, 20, 40, 3)
        assert view.data_ptr() % 4 == offset % 4
        got, flags = eng.disparity_image(torch.from_numpy(disp).cuda(), 20, 40, "plasma", out=view)
        assert got.data_ptr() == view.data_ptr()
        host = buf.cpu().numpy()
        assert np.array_equal(host[offset:offset + n].reshape(want.shape), want), offset
        assert (host[:offset] == 0xA5).all() and (host[offset + n:] == 0xA5).all(), offset      # nothing outside the view is written


def test_refusals(eng):
    d = torch.zeros((1, 8, 8), dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError):
        eng.disparity_image(d, 8, 8, "jet")
    with pytest.raises(ValueError):
        eng.disparity_image(d, 8, 8, mults=[1.0, 2.0])
    with pytest.raises(L.SdError):
        eng.disparity_image(d, 0, 8)
    with pytest.raises(L.SdError):
        eng.disparity_image(d, 8, 16385)
    with pytest.raises(L.SdError):
        eng.disparity_image(torch.zeros((1, 66, 8), dtype=torch.float32, device="cuda"), 2, 8)
    # the C entry itself: a bad map, a short workspace and an unaligned one, before any launch (the output keeps its fill)
    need = C.c_size_t()
    assert eng.lib.sd_disp_image_workspace(1, 8, 8, 16, 16, C.byref(need)) == L.SD_OK
    ws = torch.empty((need.value + 16,), dtype=torch.uint8, device="cuda")
    out = torch.full((1, 16, 16, 3), 0xA5, dtype=torch.uint8, device="cuda")
    flags = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(cmap, ws_ptr, ws_bytes, B=1):
        return eng.lib.sd_disp_image(eng.h, C.c_void_p(d.data_ptr()), None, B, 8, 8, 16, 16, cmap, C.c_void_p(out.data_ptr()), C.c_void_p(flags.data_ptr()),
                                     C.c_void_p(ws_ptr), ws_bytes, stream)
    assert call(2, ws.data_ptr(), need.value) == L.SD_ERR_INVALID
    assert call(-1, ws.data_ptr(), need.value) == L.SD_ERR_INVALID
    assert call(0, ws.data_ptr(), need.value - 1) == L.SD_ERR_INVALID
    assert call(0, ws.data_ptr() + 8, need.value) == L.SD_ERR_INVALID
    assert call(0, ws.data_ptr(), need.value, B=0) == L.SD_ERR_INVALID
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0xA5).all() and flags.cpu().tolist() == [7]
    assert call(0, ws.data_ptr(), need.value) == L.SD_OK
    torch.cuda.synchronize()
    assert flags.cpu().tolist() == [0] and (out.cpu().numpy() == 0).all()          # a constant map: entry 0 of gray


class _DispEngine:
    """the engine, keeping every batch's disp_pp (copied to the host) and camera multipliers for the test to apply the host statement to"""

    def __init__(self, eng):
        self._eng, self.seen = eng, []

    def __getattr__(self, name):
        return getattr(self._eng, name)

    def process_batch(self, frames, cams, *a, **k):
        out = self._eng.process_batch(frames, cams, *a, **k)
        self.seen.append((out["disp_pp"].cpu().numpy().copy(), [c.disp_mult for c in cams]))
        return out


def test_make_engine_step_writes_the_disparity_images_on_both_png_routes(tmp_path):
    """the driver on a 128 x 256 engine, four frames of 256 x 512 in batches of two: every _disp.png of both PNG routes decodes to the host
    statement applied to that step's disp_pp; every other file is the disp=None run's"""
    import sequence_all_routes_cases as A
    import test_gpu_sequence_outputs as S
    from semantic_depth_amd import weights as W
    from semantic_depth_amd.distributed import make_engine_step, run_sequence_files
    from semantic_depth_amd.engine import Engine, RoadWidthParams
    H, W_ = 128, 256
    frames = S._smooth_frames(np.random.default_rng(33), 4, 2 * H, 2 * W_, cell=16)
    src = tmp_path / "in"
    src.mkdir()
    paths = [outputs.write_png(str(src / f"city_{i:03d}_leftImg8bit.png"), frames[i], level=1) for i in range(len(frames))]
    e = Engine(H, W_, 2, "resnet50", precision="bf16x3")
    trees, manifests, seen = {}, {}, {}
    try:
        e.load_weights(L.SD_NET_FCN8S, W.make_fcn8s_weights(1, decoder_std=0.05))
        e.load_weights(L.SD_NET_MONODEPTH, W.make_monodepth_weights("resnet50", 2))
        prm, names = RoadWidthParams(), outputs.sequence_names(paths)
        for png in ("host", "device"):
            for disp in (None, "plasma"):
                key = (png, disp)
                outs = outputs.SequenceOutputs(str(tmp_path / f"{png}_{disp}"), names, depth=prm.depth, threads=8, png=png)
                de = _DispEngine(e)
                run_sequence_files(paths, make_engine_step(de, lambda i: S.CAM, prm, outputs=outs, disp=disp), batch=2, device="cuda")
                manifests[key] = json.load(open(outs.manifest))
                assert manifests[key]["status"] == "ok"
                trees[key], seen[key] = A.tree(tmp_path / f"{png}_{disp}"), de.seen
    finally:
        e.close()
    rel = [os.path.join(outputs.SEQ_DISP_DIR, f"{nm}_disp.png") for nm in names]
    for png in ("host", "device"):
        off, on = trees[(png, None)], trees[(png, "plasma")]
        assert "disp" not in manifests[(png, None)] and not any(k.startswith(outputs.SEQ_DISP_DIR) for k in off)
        assert manifests[(png, "plasma")]["disp"] == rel and manifests[(png, "plasma")]["disp_nonfinite"] == []
        assert set(on) == set(off) | set(rel)
        for k in off:                                      # every other file is the disp=None run's
            if k != "manifest_rank0.json":
                assert on[k] == off[k], (png, k)
        assert len(seen[(png, "plasma")]) == 2
        maps = np.concatenate([m for m, _ in seen[(png, "plasma")]])
        mults = [v for _, mu in seen[(png, "plasma")] for v in mu]
        assert mults == [3800.0] * 4 and maps.shape == (4, H, W_)
        want, flags = outputs.disparity_image(maps, 2 * H, 2 * W_, "plasma", mults)
        assert not flags.any() and len(np.unique(want.reshape(-1, 3), axis=0)) > 100
        for i, r in enumerate(rel):
            assert np.array_equal(frame_io.imread(str(tmp_path / f"{png}_plasma" / r)), want[i]), (png, r)
