"""CPU: the chunk-split rule of small-batch level 2 (sd_small_batch_split_direct, sd_set_small_batch(h, 2) before any memory is bound).

The 3x3 direct kernel walks work items = (16 x 32-pixel tile) x (pass of 64 output channels), each over the layer's whole chunk axis (a chunk =
16 input channels x 9 taps).  Level 2 cuts an under-filled layer's chunk axis into S contiguous ranges per item:

    S = 1                  when items >= CUs (the layer fills the chip)
    S = smallest value with items * S >= CUs, capped at 16 and at nchunks / 4 (a slice keeps at least 4 chunks)
    the slices are as even as possible, the longer ones first, and cover the chunk axis exactly once.

Which fill fraction below the CU count admits a layer is what the measurement decides (include/semdepth.h states it); nothing here pins it
beyond "items >= CUs is never split" and the one-frame conv5_x layers (8 items for 256 CUs) being split."""
import ctypes as C

import pytest

import __graft_entry__ as graft
from semantic_depth_amd import _lib as L


@pytest.fixture(scope="module")
def lib():
    graft.build()
    return L.load()


def split(lib, items, nchunks, cus=256):
    lens = (C.c_int * 16)()
    s = lib.sd_small_batch_split_direct(items, nchunks, cus, lens)
    assert s == lib.sd_small_batch_split_direct(items, nchunks, cus, None)        # (the lengths are optional)
    return s, list(lens[:s])


def test_rule_invariants_over_a_grid(lib):
    split_somewhere = 0
    for cus in (64, 256, 304):
        for items in (1, 2, 4, 8, 12, 16, 31, 32, 33, 64, 100, 128, 152, 255, 256, 257, 304, 512, 4096):
            for nchunks in (1, 3, 4, 7, 8, 9, 16, 17, 24, 32, 33, 48, 63, 64, 96, 200):
                s, lens = split(lib, items, nchunks, cus)
                assert 1 <= s <= 16, (items, nchunks, cus, s)
                if items >= cus:
                    assert s == 1, (items, nchunks, cus, s)
                if s > 1:
                    split_somewhere += 1
                    assert len(lens) == s and sum(lens) == nchunks and min(lens) >= 4 and max(lens) - min(lens) <= 1, (items, nchunks, cus, lens)
                    assert sorted(lens, reverse=True) == lens            # the longer slices first: slice i starts where i - 1 ended
                    # the smallest S that covers the chip, unless a cap stopped it
                    assert items * (s - 1) < cus, (items, nchunks, cus, s)
                    assert items * s >= cus or s == 16 or nchunks // (s + 1) < 4, (items, nchunks, cus, s)
                else:
                    assert lens == [nchunks]
    assert split_somewhere > 100


def test_the_one_frame_conv5_layers_fill_the_chip_as_far_as_the_slice_floor_allows(lib):
    # conv5_x of a 256 x 512 frame: 1 tile x 8 passes, 512 input channels = 32 chunks: 8 * S >= 256 asks for 32, the 4-chunk floor leaves 8
    s, lens = split(lib, 8, 32)
    assert s == 8 and lens == [4] * 8
    # the same layers at 512 x 1024: 32 items
    s, lens = split(lib, 32, 32)
    assert s == 8 and lens == [4] * 8


def test_bad_arguments_give_one(lib):
    assert split(lib, 0, 32)[0] == 1
    assert split(lib, -8, 32)[0] == 1
    assert split(lib, 8, 0)[0] == 1
    assert split(lib, 8, -32)[0] == 1
    assert split(lib, 8, 32, cus=0)[0] == 1
    assert split(lib, 8, 32, cus=-256)[0] == 1
    assert split(lib, 8, 7)[0] == 1                   # two slices would fall below 4 chunks


def _ws(lib, h):
    fw, mw, ws = C.c_size_t(), C.c_size_t(), C.c_size_t()
    assert lib.sd_query_memory(h, C.byref(fw), C.byref(mw), C.byref(ws)) == 0
    return fw.value, mw.value, ws.value


def _plan(lib, h, net):
    buf = C.create_string_buffer(8192)
    assert lib.sd_small_batch_plan(h, net, buf, 8192) == 0
    return dict((k, int(v)) for k, v in (s.rsplit(":", 1) for s in buf.value.decode().split(",") if s))


def _is_vgg_conv(name):
    return name.startswith("conv") and "_" in name


def test_level_two_is_guarded_like_level_one(lib):
    for prec in (L.SD_PREC_F32, L.SD_PREC_BF16X3, L.SD_PREC_BF16X2, L.SD_PREC_PLAN):
        h = C.c_void_p()
        assert lib.sd_create(C.byref(h), 0, 256, 512, 1, L.SD_ENC_RESNET50, prec) == 0
        assert lib.sd_set_small_batch(h, 2) == L.SD_ERR_INVALID
        lib.sd_destroy(h)
    assert lib.sd_set_small_batch(None, 2) == L.SD_ERR_INVALID
    h = C.c_void_p()
    assert lib.sd_create(C.byref(h), 0, 256, 512, 1, L.SD_ENC_RESNET50, L.SD_PREC_F16X2) == 0
    assert lib.sd_set_small_batch(h, 3) == L.SD_ERR_INVALID
    assert _plan(lib, h, L.SD_NET_FCN8S) == {}                   # (a refused level changes nothing)
    lib.sd_destroy(h)


def test_level_two_adds_the_direct_layers_to_the_level_one_plan(lib):
    h = C.c_void_p()
    assert lib.sd_create(C.byref(h), 0, 256, 512, 1, L.SD_ENC_RESNET50, L.SD_PREC_F16X2) == 0
    base = _ws(lib, h)
    assert _plan(lib, h, L.SD_NET_FCN8S) == {} and _plan(lib, h, L.SD_NET_MONODEPTH) == {}
    assert lib.sd_set_small_batch(h, 1) == 0
    one = {n: _plan(lib, h, n) for n in (L.SD_NET_FCN8S, L.SD_NET_MONODEPTH)}
    ws1 = _ws(lib, h)
    # level 1 is what it was: the GEMM layers, no direct conv layer, 4 <= S <= 16
    assert one[L.SD_NET_FCN8S].get("fc6", 1) > 1 and one[L.SD_NET_FCN8S].get("fc7", 1) > 1
    assert not [k for k in one[L.SD_NET_FCN8S] if _is_vgg_conv(k)], one
    assert all(4 <= s <= 16 for p in one.values() for s in p.values()), one
    # ... literally: the plan of this handle before level 2 existed (256 CUs; res5_x/conv2 at 8 x 16 pixels are GEMM layers, not direct ones)
    assert one[L.SD_NET_FCN8S] == {"fc6": 16, "fc7": 16}
    assert one[L.SD_NET_MONODEPTH] == {
        "enc/res4_2/conv3": 5, "enc/res4_3/conv3": 5, "enc/res4_4/conv3": 5, "enc/res4_5/conv3": 5, "enc/res4_6/conv1": 4, "enc/res4_6/conv3": 5,
        "enc/res5_1/conv1": 4, "enc/res5_1/conv2": 16, "enc/res5_1/conv3": 6, "enc/res5_2/conv1": 8, "enc/res5_2/conv2": 16, "enc/res5_2/conv3": 10,
        "enc/res5_3/conv1": 8, "enc/res5_3/conv3": 10}
    assert lib.sd_set_small_batch(h, 2) == 0
    two = {n: _plan(lib, h, n) for n in (L.SD_NET_FCN8S, L.SD_NET_MONODEPTH)}
    ws2 = _ws(lib, h)
    for n in one:
        assert all(two[n].get(k) == s for k, s in one[n].items()), (one[n], two[n])
    for layer in ("conv5_1", "conv5_2", "conv5_3"):
        assert two[L.SD_NET_FCN8S].get(layer, 1) > 1, two
    assert all(2 <= s <= 16 for p in two.values() for s in p.values()), two
    assert ws2[:2] == ws1[:2] == base[:2] and ws2[2] >= ws1[2] >= base[2]
    # the partial sums of conv5_x at conv resolution: [S][16 x 32 pixels][512] f32
    assert ws2[2] >= base[2] + two[L.SD_NET_FCN8S]["conv5_1"] * 16 * 32 * 512 * 4
    assert lib.sd_set_small_batch(h, 1) == 0
    assert {n: _plan(lib, h, n) for n in one} == one and _ws(lib, h) == ws1
    assert lib.sd_set_small_batch(h, 0) == 0
    assert _ws(lib, h) == base and _plan(lib, h, L.SD_NET_FCN8S) == {} and _plan(lib, h, L.SD_NET_MONODEPTH) == {}
    lib.sd_destroy(h)


def test_level_two_changes_nothing_on_a_handle_whose_full_pass_fills_the_chip(lib):
    # max_batch = 32 at 256 x 512: every direct layer has at least 256 items, every GEMM layer more than an eighth of the CUs in tiles
    h = C.c_void_p()
    assert lib.sd_create(C.byref(h), 0, 256, 512, 32, L.SD_ENC_RESNET50, L.SD_PREC_F16X2) == 0
    base = _ws(lib, h)
    assert lib.sd_set_small_batch(h, 2) == 0
    assert _plan(lib, h, L.SD_NET_FCN8S) == {} and _plan(lib, h, L.SD_NET_MONODEPTH) == {} and _ws(lib, h) == base
    lib.sd_destroy(h)
