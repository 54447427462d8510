"""CPU: the host twins of the segmentation score (sd_resize_pil_bilinear_u8_host, sd_seg_confusion_host) against Pillow -- recorded in
tests/golden/pil_bilinear.npz and, where Pillow is installed, directly -- and np.bincount; the numpy restatement of the resample rule
with three seeded mistakes; semantic_depth_amd.evaluate's table, file walk, mean IoU, file text and host route.  No GPU."""
import os

import numpy as np
import pytest

import __graft_entry__ as graft
import seg_eval_cases as S
from semantic_depth_amd import _lib as L
from semantic_depth_amd import evaluate as E


@pytest.fixture(scope="module", autouse=True)
def built():
    graft.build()


@pytest.fixture(scope="module")
def golden():
    g = np.load(S.GOLDEN)
    out = {name: (g[name + "/src"], g[name + "/dst"]) for name in S.GEOMETRIES}
    for s, d in out.values():
        s.setflags(write=False)
        d.setflags(write=False)
    return out


# ---- the resample ---------------------------------------------------------------------------------------------------------------------
def test_golden_holds_the_seeded_inputs_and_the_named_geometries(golden):
    for name, (h, w, c, dh, dw) in S.GEOMETRIES.items():
        src, dst = golden[name]
        assert src.shape == (h, w, c) and dst.shape == (dh, dw, c) and np.array_equal(src, S.source(name)), name
    blocks = golden["label_blocks_75x100_c1"]
    assert set(np.unique(blocks[0])) == {0, 7, 13}
    # the quirk the issue names: interpolated label ids that are neither road nor fence
    assert len(set(np.unique(blocks[1])) - {0, 7, 13}) > 0


@pytest.mark.parametrize("name", sorted(S.GEOMETRIES))
def test_host_twin_matches_the_recorded_pillow_output(golden, name):
    src, dst = golden[name]
    st, out = S.host_resize(src[None], dst.shape[0], dst.shape[1])
    assert st == L.SD_OK and np.array_equal(out[0], dst)


@pytest.mark.parametrize("name", sorted(S.GEOMETRIES))
def test_numpy_restatement_matches_the_recorded_pillow_output(golden, name):
    src, dst = golden[name]
    assert np.array_equal(S.pil_resize_np(src, dst.shape[0], dst.shape[1]), dst)


def test_host_twin_matches_pillow_directly(golden):
    pytest.importorskip("PIL")
    for name, (src, dst) in golden.items():
        assert np.array_equal(S.pillow_resize(src, dst.shape[0], dst.shape[1]), dst), name      # the golden is this Pillow's
    rng = np.random.default_rng(5)
    for h, w, c, dh, dw in [(61, 47, 3, 9, 23), (9, 23, 1, 61, 47), (40, 640, 3, 40, 20), (64, 3, 1, 2, 3), (1, 1, 3, 5, 4), (300, 400, 3, 64, 128)]:
        src = rng.integers(0, 256, (2, h, w, c), dtype=np.uint8)
        st, out = S.host_resize(src, dh, dw)
        assert st == L.SD_OK
        for b in range(2):
            assert np.array_equal(out[b], S.pillow_resize(src[b], dh, dw)), (h, w, c, dh, dw, b)


def test_pixel_stride_channel_choice_and_reverse():
    rng = np.random.default_rng(6)
    src = rng.integers(0, 256, (3, 37, 53, 3), dtype=np.uint8)
    _, plain = S.host_resize(src, 16, 24)
    st, rev = S.host_resize(src, 16, 24, reverse=True)
    assert st == L.SD_OK and np.array_equal(rev, plain[..., ::-1])
    st, ch0 = S.host_resize(src, 16, 24, channels=1, pixel_stride=3)
    assert st == L.SD_OK and np.array_equal(ch0, plain[..., :1])
    assert not np.array_equal(plain[0], plain[1])                      # the frames of a batch are resampled each for itself


def test_limits_are_refused_by_status():
    one = np.zeros((1, 40, 40, 1), np.uint8)
    assert S.host_resize(one, 1, 40)[0] == L.SD_ERR_INVALID             # factor 40 > 32
    assert S.host_resize(np.zeros((1, 64, 64, 1), np.uint8), 2, 2)[0] == L.SD_OK      # factor 32: 65 taps
    assert S.host_resize(one, 16385, 40)[0] == L.SD_ERR_INVALID
    assert S.host_resize(np.zeros((1, 4, 4, 2), np.uint8), 2, 2)[0] == L.SD_ERR_INVALID            # two channels
    assert S.host_resize(np.zeros((1, 4, 4, 3), np.uint8), 2, 2, channels=3, pixel_stride=2)[0] == L.SD_ERR_INVALID


@pytest.mark.parametrize("mistake", S.MISTAKES)
def test_each_seeded_mistake_is_caught_by_the_golden(golden, mistake):
    """the restatement with one mistake differs from Pillow on at least one geometry -- and on the one built to show it"""
    shows = {"no_round_between": "down_37x53_c3",            # needs both passes
             "floor_xmin_no_clamp": "cols_only_100x77_c3",   # the first windows of a downscaled axis reach in front of the image
             "unnormalised": "up_16x24_c1"}[mistake]         # even where most windows sum to 1: the clipped windows at the borders
    src, dst = golden[shows]
    assert not np.array_equal(S.pil_resize_np(src, dst.shape[0], dst.shape[1], mistake), dst)
    differs = [n for n, (s, d) in golden.items() if not np.array_equal(S.pil_resize_np(s, d.shape[0], d.shape[1], mistake), d)]
    assert len(differs) >= 2, differs


def test_floor_and_truncation_agree_while_the_clamp_is_kept():
    """why the second mistake is stated without the clamp: with it, floor(v) and (int)v are both <= 0 or equal"""
    for n_in, n_out in [(53, 24), (24, 53), (1600, 512), (77, 33)]:
        scale = n_in / n_out
        for d in range(n_out):
            v = (d + 0.5) * scale - max(scale, 1.0) + 0.5
            assert max(int(np.floor(v)), 0) == max(int(v), 0)


# ---- the confusion counts --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(1, 1), (7, 13), (64, 64)])
@pytest.mark.parametrize("table", [("robo", "test"), ("city", "test"), ("city", "train")])
def test_confusion_twin_matches_bincount(hw, table):
    t = E.label_table(*table)
    pred, labels = S.confusion_inputs(*hw, B=2, seed=len(table[0]) + len(table[1]))
    st, got = S.host_confusion(pred, labels, t)
    assert st == L.SD_OK and np.array_equal(got, S.bincount_confusion(pred, labels, t))
    assert got[:, :9].sum() == 2 * hw[0] * hw[1] and not got[:, 9].any()


def test_confusion_twin_class_absent_bad_prediction_and_accumulation():
    t = E.label_table("robo")
    pred, labels = S.confusion_inputs(7, 13, B=1, seed=3, absent=1)
    st, got = S.host_confusion(pred, labels, t)
    assert st == L.SD_OK and np.array_equal(got, S.bincount_confusion(pred, labels, t))
    assert not got[0, :9].reshape(3, 3)[:, 1].any()                      # nobody predicted the fence
    bad = pred.copy()
    bad[0, 2, 5] = 3
    bad[0, 6, 12] = 255
    st, got3 = S.host_confusion(bad, labels, t)
    assert st == L.SD_OK and got3[0, 9] == 2 and got3[0, :9].sum() == 7 * 13 - 2
    assert np.array_equal(got3, S.bincount_confusion(bad, labels, t))
    st, twice = S.host_confusion(pred, labels, t, counts=got.copy())     # the call ADDS
    assert st == L.SD_OK and np.array_equal(twice, 2 * got)
    wrong = t.copy()
    wrong[40] = 3
    assert S.host_confusion(pred, labels, wrong)[0] == L.SD_ERR_INVALID


def test_label_tables():
    robo, city_test, city_train = E.label_table("robo"), E.label_table("cityscapes", "test"), E.label_table("cityscapes", "train")
    assert np.array_equal(robo, city_test) and robo.dtype == np.uint8 and robo.shape == (256,)
    assert robo[7] == 0 and robo[13] == 1 and (np.delete(robo, [7, 13]) == 2).all()
    assert city_train[7] == 0 and (city_train[11:17] == 1).all() and (np.delete(city_train, [7, 11, 12, 13, 14, 15, 16]) == 2).all()
    with pytest.raises(ValueError):
        E.label_table("kitti")


# ---- mean IoU, the running list, the file -------------------------------------------------------------------------------------------------
def test_mean_iou_by_hand():
    cm = np.array([[50, 2, 3], [4, 30, 6], [7, 8, 90]])
    # float32 by hand: 50 / (55 + 61 - 50), 30 / (40 + 40 - 30), 90 / (105 + 99 - 90)
    f = np.float32
    want = f(f(f(f(50) / f(66)) + f(f(30) / f(50))) + f(f(90) / f(114))) / f(3)
    got = E.mean_iou(cm)
    assert isinstance(got, np.float32) and got == want
    iou, valid = E.class_iou(cm)
    assert valid.all() and iou.dtype == np.float32 and iou[1] == f(0.6)


def test_mean_iou_leaves_out_absent_classes_and_is_zero_for_nothing():
    cm = np.array([[10, 0, 5], [0, 0, 0], [5, 0, 20]])                  # the fence: in no label, in no prediction
    iou, valid = E.class_iou(cm)
    assert valid.tolist() == [True, False, True] and iou[1] == 0
    f = np.float32
    assert E.mean_iou(cm) == f(f(f(10) / f(20)) + f(f(20) / f(30))) / f(2)
    assert E.mean_iou(np.zeros((3, 3), np.int64)) == 0 and isinstance(E.mean_iou(np.zeros((3, 3))), np.float32)
    # a class that is predicted but never labelled IS valid, with IoU 0
    assert E.mean_iou(np.array([[10, 5, 0], [0, 0, 0], [0, 0, 0]])) == f(f(f(10) / f(15)) + f(0)) / f(2)


def test_running_values_and_file_text_of_three_frames(tmp_path):
    frames = np.array([[[8, 0, 0], [0, 0, 0], [0, 0, 8]],
                       [[4, 4, 0], [0, 6, 2], [0, 0, 0]],
                       [[0, 0, 3], [1, 0, 0], [2, 0, 10]]])
    res = E.summarise(frames)
    f = np.float32
    c2 = np.array([[12, 4, 0], [0, 6, 2], [0, 0, 8]])
    c3 = c2 + frames[2]
    run = [f(1.0),
           f(f(f(f(12) / f(16)) + f(f(6) / f(12))) + f(f(8) / f(10))) / f(3),
           f(f(f(f(12) / f(22)) + f(f(6) / f(13))) + f(f(18) / f(25))) / f(3)]
    assert np.array_equal(res["total"], c3) and [float(v) for v in res["running_mean_iou"]] == [float(v) for v in run]
    assert res["mean_iou"] == run[2] == E.mean_iou(c3)
    mean = f(f(f(run[0] + run[1]) + run[2]) / f(3))
    assert res["mean_of_running"] == mean and res["mean_of_running"] != res["mean_iou"]
    text = "1.0\n{}\n{}\nIoU metric of Testing set: {}".format(run[1], run[2], mean)
    assert "".join("{}\n".format(v) for v in run[:1]) == "1.0\n"
    path = E.write_test_set_iou(str(tmp_path / "test_set_iou.txt"), res)
    assert open(path, "rb").read() == text.encode() and not text.endswith("\n")
    # "{}".format of a numpy float32 goes through Python's float: the digits of the float32 value (12/16 + 6/12 + 8/10) / 3 as a double
    assert text.splitlines()[1] == "0.6833333373069763"


# ---- the file walk and the host route -------------------------------------------------------------------------------------------------
def test_labelled_pairs_on_a_cityscapes_tree(tmp_path):
    gt, im = tmp_path / "gtFine" / "test", tmp_path / "leftImg8bit" / "test"
    for city, ids in (("munich", (3, 1)), ("berlin", (2,))):
        (gt / city).mkdir(parents=True)
        (im / city).mkdir(parents=True)
        for i in ids:
            (gt / city / f"{city}_{i:05d}_gtFine_labelIds.png").write_bytes(b"")
            (gt / city / f"{city}_{i:05d}_gtFine_polygons.json").write_bytes(b"")
            (gt / city / f"{city}_{i:05d}_gtFine_color.png").write_bytes(b"")
            (im / city / f"{city}_{i:05d}_leftImg8bit.png").write_bytes(b"")
    pairs = E.labelled_pairs(str(gt), str(im))
    assert [(os.path.basename(a), os.path.basename(b)) for a, b in pairs] == [
        ("berlin_00002_gtFine_labelIds.png", "berlin_00002_leftImg8bit.png"),
        ("munich_00001_gtFine_labelIds.png", "munich_00001_leftImg8bit.png"),
        ("munich_00003_gtFine_labelIds.png", "munich_00003_leftImg8bit.png")]
    (im / "berlin" / "berlin_00009_leftImg8bit.png").write_bytes(b"")
    with pytest.raises(ValueError):
        E.labelled_pairs(str(gt), str(im))


class StubEngine:
    """fcn8s_forward returns a prescribed argmax: class 0 in the lower half, 1 in a band, 2 elsewhere; frame b shifts the band"""
    H, W, max_batch, device = 64, 128, 2, "cpu"

    def __init__(self):
        self.seen = []

    def prescribed(self, i):
        a = np.full((self.H, self.W), 2, np.uint8)
        a[self.H // 2:] = 0
        a[10 + 4 * i:20 + 4 * i, 30:90] = 1
        return a

    def fcn8s_forward(self, frames):
        import torch
        assert frames.dtype == torch.uint8 and tuple(frames.shape[1:]) == (self.H, self.W, 3)
        n0 = len(self.seen)
        self.seen += [frames[b].numpy().copy() for b in range(frames.shape[0])]
        amax = torch.from_numpy(np.stack([self.prescribed(n0 + b) for b in range(frames.shape[0])]))
        return dict(argmax=amax, road=(amax == 0).to(torch.uint8), fence=(amax == 1).to(torch.uint8), logits=None)


@pytest.mark.parametrize("batch", [1, 2])
def test_evaluate_files_host_route_with_a_stub_engine(tmp_path, golden_dir, batch):
    from semantic_depth_amd import frame_io
    gt, im = S.write_fixture_tree(str(tmp_path), golden_dir, frame_hw=(1200, 1600))
    eng = StubEngine()
    res = E.evaluate_files(gt, im, eng, dataset="robo", route="host", batch=batch)
    assert [os.path.basename(p[0]) for p in res["pairs"]] == list(S.LABEL_FILES) and res["per_frame"].shape == (2, 3, 3)
    table = E.label_table("robo")
    for i, (gt_file, img_file) in enumerate(res["pairs"]):
        label = frame_io.imread(gt_file)
        assert label.shape == (1200, 1600, 3) and np.array_equal(label[..., 0], label[..., 2])
        lab = S.pil_resize_np(label[..., :1], eng.H, eng.W)[..., 0]
        want = S.bincount_confusion(eng.prescribed(i)[None], lab[None], table)[0, :9].reshape(3, 3)
        assert np.array_equal(res["per_frame"][i], want), i
        # the network saw the frame as RGB, resampled by the same rule
        rgb = S.pil_resize_np(frame_io.imread(img_file)[..., ::-1], eng.H, eng.W)
        assert np.array_equal(eng.seen[i], rgb), i
    assert np.array_equal(res["total"], res["per_frame"].sum(0)) and res["total"].sum() == 2 * eng.H * eng.W
    assert res["running_mean_iou"][0] == E.mean_iou(res["per_frame"][0]) and res["running_mean_iou"][1] == res["mean_iou"]
    assert set(np.unique(frame_io.imread(res["pairs"][0][0]))) >= {7, 13}          # the fixtures hold road and fence
