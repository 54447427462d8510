"""CPU: which kernel runs every conv layer of a handle (sd_conv_forms) against tests/golden/conv_forms.json.

The golden was recorded while the listing was still a thin extraction beside the launch path's own per-call choice (and that path's per-layer profile
labels were checked against it on the GPU); csrc/conv_form.cpp, the one resolver the launch path now reads too, must keep giving it.  The
configurations are in conv_forms_cases.py: both networks, both encoders, the six precisions, four geometries, the small-batch levels, every
SEMDEPTH_DISABLE switch one at a time, a full pass and a call of one frame."""
import ctypes as C

import pytest

import __graft_entry__ as graft
import conv_forms_cases as cc
from semantic_depth_amd import _lib as L


@pytest.fixture(scope="module")
def lib():
    graft.build()
    return L.load()


@pytest.fixture(scope="module")
def golden():
    return cc.golden()


def test_the_golden_holds_every_configuration(golden):
    assert sorted(golden) == sorted(cc.key(c) for c in cc.configurations())


@pytest.mark.parametrize("cfg", cc.configurations(), ids=cc.key)
def test_listing_and_workspace_equal_the_golden(lib, golden, cfg):
    assert cc.entry(lib, cfg) == golden[cc.key(cfg)]


@pytest.mark.parametrize("cfg", [c for c in cc.configurations() if c[5]], ids=cc.key)
def test_small_batch_plan_is_the_split_lines_of_the_listing(lib, cfg):
    with cc.handle(lib, cfg) as h:
        split = 0
        for net in cc.NETS.values():
            buf = C.create_string_buffer(8192)
            assert lib.sd_small_batch_plan(h, net, buf, 8192) == 0
            plan = dict((k, int(v)) for k, v in (s.rsplit(":", 1) for s in buf.value.decode().split(",") if s))
            assert plan == {k: s for k, (_, s) in L.conv_forms(lib, h, net).items() if s > 1}
            split += len(plan)
        assert split > 0            # (one frame never fills the chip)


def test_a_call_of_one_frame_differs_only_where_a_rule_reads_the_call(golden):
    """Two rules read the image count of the call.  The row groups of conv_dma3 (N % (256 / Wout) == 0) change ConvParams::rowgrp, never the kernel.
    conv_split's 128 x 256 tile needs 512 tiles of the call, so a conv_split layer with Cout % 256 == 0 may fall back to 128 x 128: in the golden's
    configurations these are the res2 / res3 block tails of the bf16x3 monodepth without the LDS-DMA kernels (SEMDEPTH_DISABLE=dma), nothing else."""
    differs = {k: e["frames=1"] for k, e in golden.items() if any(e["frames=1"].values())}
    assert differs == {"resnet50 bf16x3 256x512x8 small_batch=0 disable=dma": {"fcn8s": {}, "monodepth": {
        f"enc/{blk}/conv3": "conv_split_x3_kernel<2,2,2,2>" for blk in ("res2_1", "res2_2", "res3_1", "res3_2", "res3_3")}}}
    full = golden["resnet50 bf16x3 256x512x8 small_batch=0 disable=dma"]["monodepth"]
    assert set(differs["resnet50 bf16x3 256x512x8 small_batch=0 disable=dma"]["monodepth"]) <= set(full["conv_split_x3_kernel<2,4,2,2>"])


def test_bad_arguments(lib):
    with cc.handle(lib, ("resnet50", "f16x2", 128, 256, 2, 0, None)) as h:
        buf = C.create_string_buffer(1 << 16)
        assert lib.sd_conv_forms(None, 0, 0, buf, len(buf)) == L.SD_ERR_INVALID
        assert lib.sd_conv_forms(h, 0, 3, buf, len(buf)) == L.SD_ERR_INVALID          # more frames than a pass holds
        assert lib.sd_conv_forms(h, 0, -1, buf, len(buf)) == L.SD_ERR_INVALID
        assert lib.sd_conv_forms(h, 0, 0, buf, 16) == L.SD_ERR_INVALID and len(buf.value) == 15      # cut at cap - 1, as sd_small_batch_plan
        assert lib.sd_conv_forms(h, 0, 2, buf, len(buf)) == 0 and buf.value.decode().startswith("conv1_1 conv_stem_hs_kernel 1\n")
