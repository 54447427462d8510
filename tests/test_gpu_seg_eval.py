"""GPU: the kernels of seg_eval_gpu.hip (Engine.resize_pil, Engine.seg_confusion) against their host twins and np.bincount, byte for byte
and count for count, and evaluate_files' device route against its host route.  Inputs come from tests/seg_eval_cases.py and
tests/golden/ (Pillow's recorded outputs, two label images)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import __graft_entry__ as graft
import seg_eval_cases as S
from semantic_depth_amd import _lib as L
from semantic_depth_amd import evaluate as E

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine_and_weights():
    """the seeded-weight f16x2 engine at 256 x 512 (FCN-8s loaded), shared through gpu_common's cache"""
    graft.build()
    import gpu_common as G
    eng, wf, _ = G.engine(256, 512, max_batch=2, load=("fcn",), precision="f16x2")
    return eng, wf


@pytest.fixture(scope="module")
def eng(engine_and_weights):
    return engine_and_weights[0]


@pytest.fixture(scope="module")
def golden():
    g = np.load(S.GOLDEN)
    return {name: (g[name + "/src"], g[name + "/dst"]) for name in S.GEOMETRIES}


@pytest.fixture(scope="module")
def tree(tmp_path_factory, golden_dir):
    """the two-frame fixture set: the committed label images beside seeded frames, 1200 x 1600"""
    return S.write_fixture_tree(str(tmp_path_factory.mktemp("seg_eval")), golden_dir)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check_resize(eng, frames, dh, dw, **kw):
    st, want = S.host_resize(frames, dh, dw, **kw)
    assert st == L.SD_OK
    got = eng.resize_pil(dev(frames), dh, dw, **kw).cpu().numpy()
    assert got.shape == want.shape and np.array_equal(got, want), (frames.shape, dh, dw, kw, int((got != want).sum()))
    return got


# ---- the resample ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(S.GEOMETRIES))
def test_resample_kernel_on_the_golden_geometries(eng, golden, name):
    src, dst = golden[name]
    got = check_resize(eng, src[None], dst.shape[0], dst.shape[1])
    assert np.array_equal(got[0], dst)                                  # and so Pillow's bytes


def test_resample_kernel_three_frames_in_one_call(eng):
    rng = np.random.default_rng(11)
    frames = rng.integers(0, 256, (3, 37, 53, 3), dtype=np.uint8)       # rows of 159 bytes: no row starts on a dword but the first
    got = check_resize(eng, frames, 16, 24)
    assert not np.array_equal(got[0], got[1]) and not np.array_equal(got[1], got[2])
    check_resize(eng, frames, 70, 53)                                   # vertical pass only, upscaling, odd row length
    check_resize(eng, frames[:, :, :, :1], 37, 131)                     # horizontal pass only, upscaling: windows of one and two taps


def test_resample_kernel_pixel_stride_and_reverse(eng):
    rng = np.random.default_rng(12)
    frames = rng.integers(0, 256, (2, 37, 53, 3), dtype=np.uint8)
    plain = check_resize(eng, frames, 16, 24)
    ch0 = check_resize(eng, frames, 16, 24, channels=1, pixel_stride=3)
    assert np.array_equal(ch0, check_resize(eng, np.ascontiguousarray(frames[..., :1]), 16, 24))       # against the contiguous copy
    rev = check_resize(eng, frames, 16, 24, reverse=True)
    assert np.array_equal(rev, plain[..., ::-1])
    four = rng.integers(0, 256, (1, 20, 45, 4), dtype=np.uint8)
    assert np.array_equal(check_resize(eng, four, 7, 13, channels=3, pixel_stride=4), check_resize(eng, np.ascontiguousarray(four[..., :3]), 7, 13))


def test_resample_kernel_widest_window(eng):
    """factor 32 on both axes: 65 taps, the longest span a column tile stages (more than one tile, partial last tile)"""
    rng = np.random.default_rng(13)
    check_resize(eng, rng.integers(0, 256, (1, 96, 2112, 3), dtype=np.uint8), 3, 66)
    check_resize(eng, rng.integers(0, 256, (2, 64, 2200, 1), dtype=np.uint8), 2, 69)


@pytest.mark.parametrize("channels", [3, 1])
def test_resample_kernel_at_the_real_geometry(eng, channels):
    rng = np.random.default_rng(14 + channels)
    check_resize(eng, rng.integers(0, 256, (1, 1200, 1600, channels), dtype=np.uint8), 256, 512)


def test_resample_limits_by_status_without_a_launch(eng):
    lib = eng.lib
    need = C.c_size_t(0)
    ok = lambda *a: lib.sd_resize_pil_workspace(*a, C.byref(need))     # noqa: E731
    assert ok(1, 64, 64, 2, 2, 1) == L.SD_OK and need.value > 0
    assert ok(1, 16384, 16384, 512, 512, 3) == L.SD_OK
    for bad in [(1, 65, 64, 2, 2, 1), (1, 64, 65, 2, 2, 1), (1, 16385, 4, 16385, 4, 1), (1, 4, 4, 4, 16385, 1), (0, 4, 4, 4, 4, 1), (65536, 4, 4, 4, 4, 1),
                (1, 4, 4, 4, 4, 2)]:
        assert ok(*bad) == L.SD_ERR_INVALID, bad
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    p, s = C.c_void_p(buf.data_ptr()), eng._stream()
    call = lambda sh, sw, ps, ch, dh, dw, ws=p, nws=1 << 16: lib.sd_resize_pil_bilinear_u8(eng.h, p, 1, sh, sw, ps, ch, 0, p, dh, dw, ws, nws, s)      # noqa: E731
    assert call(65, 8, 1, 1, 2, 8) == L.SD_ERR_INVALID and call(8, 65, 1, 1, 8, 2) == L.SD_ERR_INVALID
    assert call(8, 8, 2, 3, 4, 4) == L.SD_ERR_INVALID and call(8, 8, 5, 3, 4, 4) == L.SD_ERR_INVALID
    assert call(8, 8, 1, 1, 4, 4, nws=16) == L.SD_ERR_INVALID                                # workspace too small
    assert call(8, 8, 1, 1, 4, 4, ws=C.c_void_p(buf.data_ptr() + 4)) == L.SD_ERR_INVALID     # not 16-byte aligned
    with pytest.raises(L.SdError):
        eng.resize_pil(torch.zeros((1, 40, 40, 1), dtype=torch.uint8, device="cuda"), 1, 40)
    torch.cuda.synchronize()
    assert not buf.any()                                                                     # nothing was launched


# ---- the confusion counts --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,h,w", [(1, 1, 1), (2, 7, 13), (5, 256, 512), (3, 31, 33)])
def test_confusion_kernel_matches_bincount(eng, B, h, w):
    for k, tab in enumerate([("robo", "test"), ("city", "train")]):
        t = E.label_table(*tab)
        pred, labels = S.confusion_inputs(h, w, B=B, seed=k)
        got = eng.seg_confusion(dev(pred), dev(labels), t).cpu().numpy()
        assert np.array_equal(got, S.bincount_confusion(pred, labels, t)), (B, h, w, tab)
        assert np.array_equal(got, S.host_confusion(pred, labels, t)[1])


def test_confusion_kernel_single_class_accumulation_and_the_tenth_counter(eng):
    t = E.label_table("robo")
    pred = np.full((2, 256, 512), 1, np.uint8)                          # every lane of every wave votes for one cell
    labels = np.full((2, 256, 512), 13, np.uint8)
    got = eng.seg_confusion(dev(pred), dev(labels), t)
    want = np.zeros((2, 10), np.int64)
    want[:, 4] = 256 * 512
    assert np.array_equal(got.cpu().numpy(), want)
    p2, l2 = S.confusion_inputs(256, 512, B=2, seed=9)
    p2[1, 100, 200:203] = 3
    p2[0, 255, 511] = 255
    again = eng.seg_confusion(dev(p2), dev(l2), t, out=got)             # a second call adds into the same counts
    assert again is got
    total = want + S.bincount_confusion(p2, l2, t)
    assert np.array_equal(got.cpu().numpy(), total) and total[:, 9].tolist() == [1, 3]
    # a view of one frame of a larger count tensor, as evaluate_files hands it over
    big = torch.zeros((4, 10), dtype=torch.int64, device="cuda")
    eng.seg_confusion(dev(p2[:1]), dev(l2[:1]), t, out=big[2:3])
    assert np.array_equal(big.cpu().numpy()[2], S.bincount_confusion(p2[:1], l2[:1], t)[0]) and not big.cpu().numpy()[[0, 1, 3]].any()
    wrong = t.copy()
    wrong[0] = 3
    with pytest.raises(L.SdError):
        eng.seg_confusion(dev(pred), dev(labels), wrong)


# ---- the routes -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def device_route(eng, tree, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("overlay_device"))
    return E.evaluate_files(tree[0], tree[1], eng, dataset="robo", route="device", images_dir=out, batch=2), out


def test_routes_agree(eng, tree, device_route, tmp_path):
    dres, ddir = device_route
    hdir = str(tmp_path / "overlay_host")
    hres = E.evaluate_files(tree[0], tree[1], eng, dataset="robo", route="host", images_dir=hdir, batch=2)
    assert dres["per_frame"].shape == (2, 3, 3) and np.array_equal(dres["per_frame"], hres["per_frame"])
    assert (dres["per_frame"].sum((1, 2)) == 256 * 512).all()
    assert E.iou_file_text(dres) == E.iou_file_text(hres) and E.iou_file_text(dres).count("\n") == 2
    names = sorted(os.listdir(ddir))
    assert names == sorted(os.listdir(hdir)) == ["berlin_00125_leftImg8bit.png", "berlin_00126_leftImg8bit.png"]
    for n in names:
        assert open(os.path.join(ddir, n), "rb").read() == open(os.path.join(hdir, n), "rb").read(), n
    # the labels the score saw are the committed images through the rule: the row sums of a frame's matrix are its label classes
    from semantic_depth_amd import frame_io
    t = E.label_table("robo")
    for i, (gt_file, _) in enumerate(dres["pairs"]):
        lab = S.host_resize(frame_io.imread(gt_file)[None], 256, 512, channels=1, pixel_stride=3)[1][0, :, :, 0]
        assert np.array_equal(dres["per_frame"][i].sum(1), np.bincount(t[lab].ravel(), minlength=3)), i


def test_counts_do_not_depend_on_the_arena_contents(engine_and_weights, tree, device_route):
    from semantic_depth_amd.engine import Engine
    eng, wf = engine_and_weights
    other = Engine(256, 512, 2, "resnet50", precision="f16x2", arena_fill=0xFF)
    try:
        other.load_weights(L.SD_NET_FCN8S, wf)
        res = E.evaluate_files(tree[0], tree[1], other, dataset="robo", route="device", batch=2)
        assert np.array_equal(res["per_frame"], device_route[0]["per_frame"])
        rng = np.random.default_rng(21)
        frames = rng.integers(0, 256, (2, 37, 53, 3), dtype=np.uint8)
        assert np.array_equal(other.resize_pil(dev(frames), 16, 24).cpu().numpy(), eng.resize_pil(dev(frames), 16, 24).cpu().numpy())
    finally:
        other.close()
