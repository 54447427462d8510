"""CPU side of the per-frame fp16 range recompute (Engine(on_range='recompute')): the splice bookkeeping on CPU tensors and the argument
checks of sd_saturation_frames."""
import ctypes as C

import numpy as np
import pytest
import torch

from semantic_depth_amd import _lib as L
from semantic_depth_amd import recompute as RC

SD_ERR_INVALID = -1      # include/semdepth.h


def test_flagged_frames_are_the_nonzero_counts_in_order():
    assert RC.flagged_frames(np.array([0, 3, 0, 1], np.uint32)) == [1, 3]
    assert RC.flagged_frames(np.zeros(5, np.uint32)) == []


def test_modes_are_checked():
    assert RC.check_mode("raise") == "raise" and RC.check_mode("recompute") == "recompute"
    with pytest.raises(ValueError):
        RC.check_mode("clamp")


def test_splice_replaces_exactly_the_flagged_frames_of_every_output():
    B, cap = 4, 6
    g = torch.Generator().manual_seed(0)
    dst = dict(seg=dict(road=torch.zeros(B, 2, 3, dtype=torch.uint8), logits=None),
               disp_pp=torch.zeros(B, 2, 3),
               fuse=dict(road_xyz=torch.zeros(B, cap, 3), n_road=torch.zeros(B, dtype=torch.int32), dense=None),
               records=torch.zeros(B, 104, dtype=torch.uint8), f2f=None,
               pair=(torch.zeros(B, 2), torch.zeros(B, 1, 2)))
    idx = torch.tensor([1, 3])
    src = dict(seg=dict(road=torch.ones(2, 2, 3, dtype=torch.uint8), logits=torch.ones(2, 2, 3, 3)),
               disp_pp=torch.rand(2, 2, 3, generator=g),
               fuse=dict(road_xyz=torch.rand(2, cap, 3, generator=g), n_road=torch.tensor([5, 2], dtype=torch.int32), dense=None,
                         disp_pp=torch.rand(2, 2, 3)),     # (a subset that fits one pass returns more: ignored)
               records=torch.full((2, 104), 7, dtype=torch.uint8), f2f=None,
               pair=(torch.ones(2, 2), torch.ones(2, 1, 2)))
    before = {k: v.clone() for k, v in (("disp", dst["disp_pp"]),)}
    out = RC.splice(dst, src, idx)
    assert out is dst and dst["seg"]["logits"] is None and dst["f2f"] is None
    for i, j in ((1, 0), (3, 1)):
        assert torch.equal(dst["disp_pp"][i], src["disp_pp"][j])
        assert torch.equal(dst["fuse"]["road_xyz"][i], src["fuse"]["road_xyz"][j])
        assert int(dst["fuse"]["n_road"][i]) == int(src["fuse"]["n_road"][j])
        assert torch.equal(dst["records"][i], src["records"][j])
        assert torch.equal(dst["pair"][1][i], src["pair"][1][j])
        assert dst["seg"]["road"][i].all()
    for i in (0, 2):
        assert torch.equal(dst["disp_pp"][i], before["disp"][i])
        assert not dst["seg"]["road"][i].any() and not dst["records"][i].any() and int(dst["fuse"]["n_road"][i]) == 0


def test_splice_refuses_mismatched_results():
    dst = dict(a=torch.zeros(3, 2))
    with pytest.raises(ValueError):
        RC.splice(dst, dict(a=torch.zeros(2, 3)), torch.tensor([0, 1]))
    with pytest.raises(KeyError):
        RC.splice(dst, dict(b=torch.zeros(2, 2)), torch.tensor([0, 1]))
    with pytest.raises(ValueError):
        RC.splice(dict(a=torch.zeros(3, 2)), dict(a=torch.zeros(2, 2, dtype=torch.int32)), torch.tensor([0, 1]))


def test_saturation_frames_rejects_bad_arguments():
    lib = L.load()
    assert lib.sd_saturation_frames(None, None, 1, 0, None) == SD_ERR_INVALID
    h = C.c_void_p()
    assert lib.sd_create(C.byref(h), 0, 64, 128, 2, L.SD_ENC_RESNET50, L.SD_PREC_F16X2) == 0
    try:
        buf = (C.c_uint32 * 4)()
        assert lib.sd_saturation_frames(h, None, 1, 0, None) == SD_ERR_INVALID
        assert lib.sd_saturation_frames(h, buf, 0, 0, None) == SD_ERR_INVALID
        assert lib.sd_saturation_frames(h, buf, 3, 0, None) == SD_ERR_INVALID        # n > max_batch
    finally:
        lib.sd_destroy(h)


def test_saturation_settle_rejects_bad_arguments():
    lib = L.load()
    assert lib.sd_saturation_settle(None, 1, None) == SD_ERR_INVALID
    h = C.c_void_p()
    assert lib.sd_create(C.byref(h), 0, 64, 128, 2, L.SD_ENC_RESNET50, L.SD_PREC_F16X2) == 0
    try:
        assert lib.sd_saturation_settle(h, 0, None) == SD_ERR_INVALID
        assert lib.sd_saturation_settle(h, 3, None) == SD_ERR_INVALID
    finally:
        lib.sd_destroy(h)
