"""CPU: the split-K rule of the small-batch switch (sd_small_batch_split, sd_set_small_batch before any memory is bound).  The rule is a pure
function of what a handle fixes -- the rows of a full pass, the layer's Cout and padded K, the CU count -- so it is checked here without a GPU.

    tiles = ceil(rows / 256) * (cout / 256)           (the 256 x 256 block of conv_dma3.hip)
    a layer is split when 8 * tiles <= CUs            (below the CU count is necessary; the eighth is what the measurement left in the rule:
                                                       profiles/latency_b1*.json -- every layer that gained has 16 or 32 tiles of 256 CUs, the
                                                       layers with 64-128 tiles gained nothing, nothing in between was measured)
    S     = smallest value with tiles * S >= CUs, capped at 16 and at (kpad / 32) / 8 (a slice keeps at least 8 k-tiles of 32);
            a layer the caps leave below S = 4 is not split (measured as well: the S = 2 and S = 3 layers lost to their unsplit launch)
    the slices are contiguous k-tile ranges, as even as possible: they cover kpad / 32 exactly once.

Where the cap binds, tiles * S stays below the CU count: the ResNet-50 res5 block tails at one frame + flip (1024 rows, Cout 2048: 32
tiles) have K = 512 + 1024 = 1536 (res5_1: conv3 + projection, 48 k-tiles -> S = 6) or 512 + 2048 = 2560 (res5_2, res5_3: 80 k-tiles -> S = 8
at 32 tiles, 10 at the 16 tiles of the strided last block), so "tiles * S >= CUs" and "no slice below 8 k-tiles" cannot both hold for
res5_1; the cap is the rule, and the test holds these shapes to S > 1 and to the cap being what stopped them."""
import ctypes as C

import pytest

import __graft_entry__ as graft
from semantic_depth_amd import _lib as L

CUS = 256


@pytest.fixture(scope="module")
def lib():
    graft.build()
    return L.load()


def split(lib, rows, cout, kpad, cus=CUS):
    lens = (C.c_int * 16)()
    s = lib.sd_small_batch_split(rows, cout, kpad, cus, lens)
    assert s == lib.sd_small_batch_split(rows, cout, kpad, cus, None)        # (the lengths are optional)
    return s, list(lens[:s])


def tiles(rows, cout):
    return -(-rows // 256) * (cout // 256)


def test_a_layer_that_fills_the_chip_is_not_split(lib):
    assert split(lib, 32 * 512, 4096, 25088)[0] == 1             # fc6 at max_batch = 32, 512 x 1024
    assert split(lib, 256 * 256, 256, 4096)[0] == 1              # exactly 256 tiles
    assert split(lib, 8 * 512, 4096, 4096)[0] == 1               # 256 tiles
    assert split(lib, 512, 4096 + 64, 4096)[0] == 1              # Cout not a multiple of 256: not a candidate
    assert split(lib, 512, 4096, 4096, cus=32)[0] == 1           # a chip of 32 CUs is full with 32 tiles
    assert split(lib, 4096, 1024, 1280)[0] == 1                  # 64 tiles (res4 block tails of one frame + flip): measured, no gain
    assert split(lib, 2 * 4096, 512, 640)[0] == 1                # 64 tiles (res3 block tails)
    assert split(lib, 3 * 1024, 1024, 1280)[0] == 1              # 48 tiles: the unmeasured band between an eighth and a quarter


@pytest.mark.parametrize("rows,cout,kpad", [(512, 4096, 25088), (512, 4096, 4096)])
def test_fc6_and_fc7_of_one_frame_fill_the_chip_when_split(lib, rows, cout, kpad):
    s, lens = split(lib, rows, cout, kpad)
    assert s > 1 and tiles(rows, cout) * s >= CUS, (s, lens)
    assert tiles(rows, cout) * (s - 1) < CUS                     # the smallest such S
    assert sum(lens) == kpad // 32 and min(lens) >= 8 and max(lens) - min(lens) <= 1


@pytest.mark.parametrize("kpad", [1536, 2560])
def test_res5_block_tails_are_split_as_far_as_the_slice_floor_allows(lib, kpad):
    rows, cout = 1024, 2048
    s, lens = split(lib, rows, cout, kpad)
    assert s > 1, (s, lens)
    assert sum(lens) == kpad // 32 and min(lens) >= 8
    # either the chip is covered, or one more slice would push a slice below 8 k-tiles
    assert tiles(rows, cout) * s >= CUS or (kpad // 32) // (s + 1) < 8


def test_slices_cover_k_exactly_once_and_respect_both_caps(lib):
    for rows in (128, 256, 512, 1024, 2048, 4096):
        for cout in (256, 512, 1024, 2048, 4096):
            for kt in (2, 7, 8, 15, 16, 17, 48, 64, 100, 128, 144, 784, 2000):
                for cus in (64, 256, 304):
                    s, lens = split(lib, rows, cout, kt * 32, cus)
                    assert 1 <= s <= 16
                    t = tiles(rows, cout)
                    if 8 * t > cus:
                        assert s == 1
                    if s > 1:
                        assert len(lens) == s and sum(lens) == kt and min(lens) >= 8 and max(lens) - min(lens) <= 1
                        assert sorted(lens, reverse=True) == lens            # the longer slices first: slice i starts where i - 1 ended
                    if 8 * t <= cus:
                        want = min(-(-cus // t), 16, kt // 8)
                        want = want if want >= 4 else 1
                        assert s == want, (rows, cout, kt, cus, s, want)


def test_bad_arguments_give_one(lib):
    assert split(lib, 0, 4096, 4096)[0] == 1
    assert split(lib, 512, 0, 4096)[0] == 1
    assert split(lib, 512, 4096, 0)[0] == 1
    assert split(lib, 512, 4096, 4096 + 16)[0] == 1              # K not padded to k-tiles of 32
    assert split(lib, 512, 4096, 4096, cus=0)[0] == 1


def test_the_switch_is_refused_on_other_precisions_and_grows_the_workspace(lib):
    def ws_of(h):
        fw, mw, ws = C.c_size_t(), C.c_size_t(), C.c_size_t()
        assert lib.sd_query_memory(h, C.byref(fw), C.byref(mw), C.byref(ws)) == 0
        return fw.value, mw.value, ws.value

    def plan(h, net):
        buf = C.create_string_buffer(8192)
        assert lib.sd_small_batch_plan(h, net, buf, 8192) == 0
        return dict((k, int(v)) for k, v in (s.rsplit(":", 1) for s in buf.value.decode().split(",") if s))

    for prec in (L.SD_PREC_F32, L.SD_PREC_BF16X3, L.SD_PREC_BF16X2, L.SD_PREC_PLAN):
        h = C.c_void_p()
        assert lib.sd_create(C.byref(h), 0, 256, 512, 1, L.SD_ENC_RESNET50, prec) == 0
        assert lib.sd_set_small_batch(h, 1) == L.SD_ERR_INVALID
        lib.sd_destroy(h)
    assert lib.sd_set_small_batch(None, 1) == L.SD_ERR_INVALID
    h = C.c_void_p()
    assert lib.sd_create(C.byref(h), 0, 512, 1024, 1, L.SD_ENC_RESNET50, L.SD_PREC_F16X2) == 0
    base = ws_of(h)
    assert plan(h, L.SD_NET_FCN8S) == {} and plan(h, L.SD_NET_MONODEPTH) == {}
    assert lib.sd_set_small_batch(h, 1) == 0
    on = ws_of(h)
    fcn = plan(h, L.SD_NET_FCN8S)
    assert fcn.get("fc6", 1) > 1 and fcn.get("fc7", 1) > 1, fcn
    # the partial sums of the largest split layer: at least fc6's [S][512][4096] f32
    assert on[:2] == base[:2] and on[2] >= base[2] + fcn["fc6"] * 512 * 4096 * 4, (base, on, fcn)
    mono = plan(h, L.SD_NET_MONODEPTH)
    assert mono and all(4 <= s <= 16 for s in mono.values()), mono
    assert lib.sd_set_small_batch(h, 0) == 0 and ws_of(h) == base and plan(h, L.SD_NET_FCN8S) == {}
    lib.sd_destroy(h)
    # a handle whose full pass fills the chip: switching it on changes nothing
    h = C.c_void_p()
    assert lib.sd_create(C.byref(h), 0, 512, 1024, 32, L.SD_ENC_RESNET50, L.SD_PREC_F16X2) == 0
    base = ws_of(h)
    assert lib.sd_set_small_batch(h, 1) == 0
    assert plan(h, L.SD_NET_FCN8S) == {} and plan(h, L.SD_NET_MONODEPTH) == {} and ws_of(h) == base
    lib.sd_destroy(h)
