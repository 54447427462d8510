"""GPU: the sequence tool's result images and road PLYs from the batched driver (semantic_depth_cityscapes_sequence.py:303-361).
sd_compose_result_frames is bit-identical to the host composition PIL paste -> sd_resize_cubic_u8 -> draw_overlay banner, and
run_sequence_files with outputs on computes the records it computes with outputs off and writes the files of exactly those frames."""
import glob
import json
import os

import numpy as np
import pytest
import torch

import __graft_entry__ as graft
from semantic_depth_amd import _lib as L
from semantic_depth_amd import frame_io, outputs
from semantic_depth_amd import weights as W
from semantic_depth_amd.distributed import RECORD_BYTES, make_engine_step, run_sequence_files
from semantic_depth_amd.engine import RW_DTYPE, Camera, Engine, RoadWidthParams
from tests import sequence_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def small_engine():
    graft.build()
    eng = Engine(128, 256, 1, "resnet50", precision="f32")         # (the compose call needs a bound workspace only: no weights)
    yield eng
    eng.close()


def _records(found):
    rec = np.zeros(len(found), RW_DTYPE)
    rec["found"] = found
    rec["width"] = 6.5
    return torch.from_numpy(rec.view(np.uint8).reshape(-1, RECORD_BYTES).copy()).cuda()


def _smooth_frames(rng, B, h, w, cell=8):
    base = rng.integers(0, 256, (B, (h + cell - 1) // cell, (w + cell - 1) // cell, 3), dtype=np.uint8)
    f = np.repeat(np.repeat(base, cell, axis=1), cell, axis=2)[:, :h, :w]
    return (f.astype(np.int16) + rng.integers(-16, 17, f.shape, dtype=np.int16)).clip(0, 255).astype(np.uint8)


@pytest.mark.parametrize("sh,sw,dh,dw", [(512, 1024, 1024, 2048), (256, 512, 375, 1242), (256, 512, 99, 203), (256, 512, 256, 512),
                                         (37, 61, 37, 61)])
@pytest.mark.parametrize("fence_color", [R.FENCE_SEQ, R.FENCE_SINGLE])
def test_compose_is_bit_identical_to_paste_resize_banner(small_engine, sh, sw, dh, dw, fence_color):
    eng = small_engine
    rng = np.random.default_rng(sh + dw)
    found = [1, 0, 1, 0] if sh < 512 else [0, 1, 1]
    B = len(found)
    frames = _smooth_frames(rng, B, sh, sw) if sh >= 64 else rng.integers(0, 256, (B, sh, sw, 3), dtype=np.uint8)
    road = (rng.random((B, sh, sw)) < 0.45).astype(np.uint8)
    fence = (rng.random((B, sh, sw)) < 0.25).astype(np.uint8) * 3          # (non-zero = set)
    got = eng.compose_result_frames(torch.from_numpy(frames).cuda(), torch.from_numpy(road).cuda(), torch.from_numpy(fence).cuda(), _records(found),
                                    dh, dw, R.ROAD, fence_color, R.ALPHA).cpu().numpy()
    over = np.stack([R.pil_paste(frames[b], road[b], fence[b], fence_color=fence_color) for b in range(B)])
    rs = eng.resize_cubic(torch.from_numpy(over).cuda(), dh, dw).cpu().numpy()
    for b in range(B):
        banner, _ = outputs.overlay_items_sequence(dw, dh, 10.0, bool(found[b]), [[-1.0, 0, 0]], [[1.0, 0, 0]], 2.0)
        want, _ = outputs.draw_overlay(rs[b], banner, [])
        assert np.array_equal(got[b], want), (b, int((got[b] != want).any(-1).sum()))
    rows = R.banner_rows(dh)
    assert (got[np.array(found, bool), :rows] == [156, 157, 159]).all()


def test_compose_rejects_bad_arguments(small_engine):
    eng = small_engine
    fr = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device="cuda")
    m = torch.zeros((1, 8, 8), dtype=torch.uint8, device="cuda")
    with pytest.raises(L.SdError):
        eng.compose_result_frames(fr, m, m, _records([0]), 8, 20000)
    with pytest.raises(L.SdError):
        eng.compose_result_frames(fr, m, m, _records([0]), 8, 8, alpha=256)


# ------------------------------------------------------------------------------------------------ the driver, outputs on / off
H, W_ = 512, 1024
CAM = Camera(1048.64 / 2, 519.277 / 2, 1000.0, 1.0, 3800.0)         # the sequence tool's camera at 512 x 1024 (seq:500-508, :105)


@pytest.fixture(scope="module")
def seq_engine():
    graft.build()
    eng = Engine(H, W_, 8, "resnet50", precision="bf16x3")
    eng.load_weights(L.SD_NET_FCN8S, W.make_fcn8s_weights(1, decoder_std=0.05))
    wm = W.make_monodepth_weights("resnet50", 2)
    wm["dec/disp1/biases"] = (wm["dec/disp1/biases"] + np.float32(-1.5)).astype(np.float32)    # (median depth near the measuring depth)
    eng.load_weights(L.SD_NET_MONODEPTH, wm)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def frame_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("seq_in")
    frames = _smooth_frames(np.random.default_rng(21), 12, 2 * H, 2 * W_, cell=16)
    paths = [outputs.write_png(str(d / f"city_{i:03d}_leftImg8bit.png"), frames[i], level=1) for i in range(len(frames))]
    return paths


class _Spy(outputs.SequenceOutputs):
    """keeps a host copy of what every batch submitted (the kernel's images and the final road clouds)"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.kept = {}

    def submit(self, lo, records, size, images=None, final=None):
        n = records.shape[0]
        for i in range(n):
            cnt = int(final["n"][i])
            self.kept[lo + i] = (images[i].cpu().numpy(), final["xyz"][i, :cnt].cpu().numpy(), final["rgb"][i, :cnt].cpu().numpy(),
                                 records[i:i + 1].cpu().numpy().view(RW_DTYPE)[0])
        super().submit(lo, records, size, images=images, final=final)


def test_run_sequence_files_with_outputs_keeps_the_records_and_writes_every_frame(seq_engine, frame_dir, tmp_path):
    eng = seq_engine
    prm = RoadWidthParams()
    off = run_sequence_files(frame_dir, make_engine_step(eng, lambda i: CAM, prm), batch=8, device="cuda")
    names = outputs.sequence_names(frame_dir)
    outs = _Spy(str(tmp_path), names, depth=prm.depth, threads=8)
    on = run_sequence_files(frame_dir, make_engine_step(eng, lambda i: CAM, prm, outputs=outs), batch=8, device="cuda")
    assert torch.equal(on.cpu(), off.cpu())
    recs = off.cpu().numpy().view(RW_DTYPE).reshape(-1)
    m = json.load(open(os.path.join(str(tmp_path), "manifest_rank0.json")))
    assert m["status"] == "ok" and m["frames"] == [0, len(names)] and len(m["files"]) == 3 * len(names)
    assert sorted(outs.kept) == list(range(len(names)))
    for i, name in enumerate(names):
        img, xyz, rgb, rec = outs.kept[i]
        assert rec.tobytes() == recs[i].tobytes()
        assert img.shape == (2 * H, 2 * W_, 3)
        assert np.array_equal(frame_io.imread(os.path.join(str(tmp_path), outputs.SEQ_IMG_DIR, name + ".png")), img)
        left = rec["left_pt"].astype(np.float64)[None, :] if rec["found"] else None
        right = rec["right_pt"].astype(np.float64)[None, :] if rec["found"] else None
        ply = open(os.path.join(str(tmp_path), outputs.SEQ_PLY_DIR, name + "_rw.ply"), "rb").read()
        assert ply == outputs.rw_ply_bytes(xyz.astype(np.float64), rgb, left, right)
        ov = json.load(open(os.path.join(str(tmp_path), outputs.SEQ_IMG_DIR, name + "_overlay.json")))
        assert (ov["banner"] is not None) == bool(rec["found"])
        if rec["found"]:
            assert (img[:R.banner_rows(2 * H)] == [156, 157, 159]).all()
    assert len(glob.glob(os.path.join(str(tmp_path), "*", "*"))) == 3 * len(names)
    print(f"frames with the road line found: {int(recs['found'].sum())} of {len(recs)}")
