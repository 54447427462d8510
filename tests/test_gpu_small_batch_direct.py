"""GPU: level 2 of the small-batch switch (Engine(small_batch=2), sd_set_small_batch(h, 2)): the under-filled 3x3 direct conv layers of a one- or
two-frame f16x2 handle run as S contiguous chunk ranges per work item (conv_direct_splitc_hs_kernel, raw f32 partial sums at conv resolution)
plus a reduce launch (splitc_reduce_kernel) that adds the slices in ascending order and applies the layer's epilogue: alpha, bias, activation,
the fused 2x2 max pool, the HS split with the per-frame clamp attribution, NHWC or sub-planar output.

Shapes are the smallest on which each path exists:
  128 x 256   conv3_x = 1 tile x 4 passes, conv4_x = 1 tile x 8 passes (conv5_x is 8 x 16 pixels: not on the direct kernel)
  192 x 256   conv4_x has 24 rows: its second 16-row tile is half empty (no partial sum of a row >= H may reach the output)
  256 x 512   conv5_x = 1 tile x 8 passes; monodepth res4 conv2 (resnet50) / conv4a, conv5a and the concatenated-source iconv layers (vgg)
Every engine is small_batch=2 with max_batch 1 or 2, held to the frozen bounds of the exact-f32 engine like every other f16x2 path."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import nets
from semantic_depth_amd import _lib as L
from semantic_depth_amd import api
from semantic_depth_amd import weights as Wt
from semantic_depth_amd.engine import Engine, RangeError
from gpu_common import assert_close, dev, err_report

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def keep_activations():
    # as test_gpu_small_batch.py: hand the cached engines' memory back, keep the layer taps intact after a forward
    import gc
    import gpu_common
    for entry in list(gpu_common._cache.values()):
        entry[0].close()
    gpu_common._cache.clear()
    api.release_engines()
    gc.collect()
    torch.cuda.empty_cache()
    os.environ["SEMDEPTH_KEEP_ACTIVATIONS"] = "1"
    yield
    os.environ.pop("SEMDEPTH_KEEP_ACTIVATIONS", None)


def _frames(B, H, W, seed):
    """blocky noise + fine noise: frames that differ from each other and exercise every channel"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (B, H // 8, W // 8, 3), dtype=np.uint8)
    fr = np.repeat(np.repeat(base, 8, axis=1), 8, axis=2).astype(np.int16)
    return (fr + rng.integers(-16, 17, fr.shape, dtype=np.int16)).clip(0, 255).astype(np.uint8)


def _pair(frame):
    f = frame.astype(np.float32) / 255
    return np.stack((f, np.fliplr(f)), 0)


_weights = {}


def _fcn_weights():
    if "fcn" not in _weights:
        _weights["fcn"] = Wt.make_fcn8s_weights(1, decoder_std=0.05, bias_std=0.1)
    return _weights["fcn"]


def _mono_weights(enc):
    if enc not in _weights:
        _weights[enc] = Wt.make_monodepth_weights(enc, 2, bias_std=0.05)
    return _weights[enc]


def _engine(H, W, B=1, enc="resnet50", nets_=("fcn", "mono"), **kw):
    eng = Engine(H, W, B, enc, precision=kw.pop("precision", "f16x2"), small_batch=kw.pop("small_batch", 2), **kw)
    if "fcn" in nets_:
        eng.load_weights(L.SD_NET_FCN8S, _fcn_weights())
    if "mono" in nets_:
        eng.load_weights(L.SD_NET_MONODEPTH, _mono_weights(enc))
    return eng


def _direct_layers(H, W, B, enc):
    """{net: {layer: S}}: what level 2 adds to the level-1 plan of such a handle -- the chunk-split direct layers (unbound handles: no memory)"""
    lib = L.load()
    h = C.c_void_p()
    assert lib.sd_create(C.byref(h), 0, H, W, B, {"vgg": L.SD_ENC_VGG, "resnet50": L.SD_ENC_RESNET50}[enc], L.SD_PREC_F16X2) == 0
    plans = []
    for level in (1, 2):
        assert lib.sd_set_small_batch(h, level) == 0
        per = {}
        for name, net in (("fcn8s", L.SD_NET_FCN8S), ("monodepth", L.SD_NET_MONODEPTH)):
            buf = C.create_string_buffer(8192)
            assert lib.sd_small_batch_plan(h, net, buf, 8192) == 0
            per[name] = {k: int(v) for k, v in (s.rsplit(":", 1) for s in buf.value.decode().split(",") if s)}
        plans.append(per)
    lib.sd_destroy(h)
    for net in plans[0]:
        assert all(plans[1][net].get(k) == s for k, s in plans[0][net].items()), plans          # level 2 keeps level 1's layers and slice counts
    return {net: {k: s for k, s in plans[1][net].items() if k not in plans[0][net]} for net in plans[1]}


@pytest.mark.parametrize("H,W", [(128, 256), (256, 512), (192, 256)])
def test_fcn8s_taps_and_logits_of_a_one_frame_handle_match_the_oracle(H, W):
    """layer3_out / layer4_out are the pooled reduce of conv3_3 / conv4_3, layer7_out sits behind conv5_x; 192 x 256 is the partial-tile case"""
    eng = _engine(H, W, nets_=("fcn",))
    plan = eng.small_batch_plan()["fcn8s"]
    direct = _direct_layers(H, W, 1, "resnet50")["fcn8s"]
    print("split layers", H, W, plan, "direct", direct)
    behind = ["conv3_2", "conv3_3", "conv4_1", "conv4_2", "conv4_3"] + (["conv5_1", "conv5_2", "conv5_3"] if W >= 512 else [])
    assert all(direct.get(k, 1) > 1 and plan.get(k) == direct[k] for k in behind), (plan, direct)
    fr = _frames(1, H, W, seed=51)
    lg = eng.fcn8s_forward(dev(fr), want_logits=True)["logits"].cpu().numpy()
    got = {k: eng.net_tensor(L.SD_NET_FCN8S, k + "_out").cpu().numpy() for k in ("layer3", "layer4", "layer7")}
    eng.check_range()
    ref, taps = nets.fcn8s_forward(fr, _fcn_weights(), return_taps=True)
    print("logits", err_report(lg, ref))
    for k, v in got.items():
        print(k, err_report(v, taps[k]))
    for k, v in got.items():
        assert v.shape == taps[k].shape
        assert_close(v, taps[k], "f16x2", what=k + "_out")
    assert_close(lg, ref, "f16x2", what="logits")
    eng.close()


def _mono_tap_oracle(pair, wm, enc):
    """an encoder tap behind split direct layers, from oracle/nets.py's own blocks (NHWC): resnet50 -> enc/conv4 (the res4 stage, whose conv2 layers are
    split), vgg -> enc/conv5a (behind conv4a)"""
    m = nets._Mono(wm, torch.float32)
    x = nets._t(pair, torch.float32).permute(0, 3, 1, 2).contiguous()
    if enc == "resnet50":
        conv1 = m.conv(x, "enc/conv1", 7, 2)
        t = m.resblock(m.resblock(m.resblock(m.maxpool3(conv1), 2, 64, 3), 3, 128, 4), 4, 256, 6)
    else:
        for i, k in enumerate([7, 5, 3, 3], start=1):
            x = m.conv_block(x, f"enc/conv{i}", k)
        t = m.conv(x, "enc/conv5a", 3, 1)
    return t.permute(0, 2, 3, 1).contiguous().numpy()


@pytest.mark.parametrize("enc", ["resnet50", "vgg"])
def test_monodepth_disparities_and_an_encoder_tap_match_the_oracle(enc):
    H, W = 256, 512
    eng = _engine(H, W, enc=enc, nets_=("mono",))
    plan = eng.small_batch_plan()["monodepth"]
    direct = _direct_layers(H, W, 1, enc)["monodepth"]
    print("split layers", enc, plan, "direct", direct)
    assert direct and all(plan.get(k) == s and s > 1 for k, s in direct.items()), (plan, direct)       # no split monodepth layer: the test would say nothing
    if enc == "resnet50":
        tap = "enc/conv4"
        assert any(k.startswith("enc/res4_") and k.endswith("/conv2") for k in direct), direct
    else:
        tap = "enc/conv5a"
        assert "enc/conv4a" in direct and "enc/conv5a" in direct and any(k.startswith("dec/iconv") for k in direct), direct
    fr = _frames(1, H, W, seed=52)
    _, raw = eng.monodepth_forward(dev(fr), want_raw=True)
    raw = raw[0].cpu().numpy()
    got = eng.net_tensor(L.SD_NET_MONODEPTH, tap).cpu().numpy()
    eng.check_range()
    pair = _pair(fr[0])
    wm = _mono_weights(enc)
    ref = nets.monodepth_forward(pair, wm, enc)[..., 0]
    reft = _mono_tap_oracle(pair, wm, enc)
    print("disparity", enc, err_report(raw, ref), tap, err_report(got, reft))
    assert got.shape == reft.shape
    assert_close(got, reft, "f16x2", what=tap)
    assert_close(raw, ref, "f16x2", what="disparity", kind="disp")
    eng.close()


def test_results_are_deterministic_and_do_not_depend_on_the_size_of_the_call():
    H, W = 128, 256
    eng = _engine(H, W, B=2)
    direct = _direct_layers(H, W, 2, "resnet50")
    assert direct["fcn8s"].get("conv4_2", 1) > 1 and direct["monodepth"], direct
    fr = dev(_frames(2, H, W, seed=53))
    two = eng.fcn8s_forward(fr, want_logits=True)["logits"].clone()
    p2 = eng.monodepth_forward(fr).clone()
    for _ in range(2):          # three identical calls
        assert torch.equal(eng.fcn8s_forward(fr, want_logits=True)["logits"], two)
        assert torch.equal(eng.monodepth_forward(fr), p2)
    one = eng.fcn8s_forward(fr[:1].contiguous(), want_logits=True)["logits"]
    p1 = eng.monodepth_forward(fr[:1].contiguous())
    assert torch.equal(one[0], two[0]) and torch.equal(p1[0], p2[0])
    assert not torch.equal(two[0], two[1]) and not torch.equal(p2[0], p2[1])
    eng.close()


def test_range_violations_in_a_split_direct_layer_are_attributed_to_their_frames():
    """bias 1e5 on conv4_2, a chunk-split layer: every value of it leaves the fp16 range, and the clamps happen in the reduce kernel's epilogue"""
    H, W, B = 128, 256, 2
    wf = dict(_fcn_weights())
    wf["vgg/conv4_2/biases"] = np.full_like(wf["vgg/conv4_2/biases"], 1.0e5)
    fr = dev(_frames(B, H, W, seed=54))
    eng = Engine(H, W, B, "resnet50", precision="f16x2", small_batch=2)
    assert _direct_layers(H, W, B, "resnet50")["fcn8s"].get("conv4_2", 1) > 1 and eng.small_batch_plan()["fcn8s"].get("conv4_2", 1) > 1
    eng.load_weights(L.SD_NET_FCN8S, wf)
    lg = eng.fcn8s_forward(fr, want_logits=True)["logits"].cpu().numpy()
    assert np.isfinite(lg).all()
    assert eng.saturated_frames().tolist() == [True, True]
    counts = eng._frame_counts(B, reset=False)
    print("clamps per frame", counts, "total", eng.saturation_count())
    assert counts.min() >= (H // 8) * (W // 8) * 512 * 0.99 and int(counts.sum()) == eng.saturation_count(), counts
    with pytest.raises(RangeError):
        eng.check_range()
    eng.close()
    rec = Engine(H, W, B, "resnet50", precision="f16x2", small_batch=2, on_range="recompute")
    rec.load_weights(L.SD_NET_FCN8S, wf)
    with pytest.warns(RuntimeWarning):
        got = rec.fcn8s_forward(fr, want_logits=True)
    assert rec.last_recomputed == [0, 1]
    rec.check_range()
    e3 = Engine(H, W, B, "resnet50", precision="bf16x3")
    e3.load_weights(L.SD_NET_FCN8S, wf)
    want = e3.fcn8s_forward(fr, want_logits=True)
    for k in ("logits", "road", "fence", "argmax"):
        assert torch.equal(got[k], want[k]), k
    assert rec._companion.small_batch_plan() == {"fcn8s": {}, "monodepth": {}}       # the companion is not split
    rec.close()
    e3.close()


def test_api_classes_take_the_level_and_the_c_abi_guards_it():
    H, W = 128, 256
    wf = _fcn_weights()
    fr = _frames(1, H, W, seed=55)
    try:
        seg = api.SegmentFrame((H, W), wf, small_batch=2)
        road, fence, _ = seg.segment_frame(fr[0])
        e = seg.engine
        assert e.small_batch and e.small_batch_level == 2 and e.small_batch_plan()["fcn8s"].get("conv4_2", 1) > 1
        # the level is part of the registry key; True and 1 are one engine
        assert api.shared_engine(H, W, small_batch=2) is e
        one = api.shared_engine(H, W, small_batch=True)
        assert one is not e and api.shared_engine(H, W, small_batch=1) is one and api.shared_engine(H, W) is not e
        assert "conv4_2" not in one.small_batch_plan()["fcn8s"]
        # sd_set_small_batch after sd_bind_memory: SD_ERR_STATE, whatever the level
        for level in (0, 1, 2):
            assert e.lib.sd_set_small_batch(e.h, level) == L.SD_ERR_STATE
        d = api.DepthFrame(encoder="resnet50", input_height=H, input_width=W, checkpoint_path=_mono_weights("resnet50"), small_batch=2)
        assert d.engine.small_batch_level == 2 and d.engine.small_batch_plan()["monodepth"]
        assert d.compute_disparity(fr[0]).shape == (H, W)
    finally:
        api.release_engines()
    eng = Engine(H, W, 1, "resnet50", precision="f16x2", small_batch=2)
    eng.load_weights(L.SD_NET_FCN8S, wf)
    out = eng.fcn8s_forward(dev(fr))
    assert np.array_equal(out["road"][0].cpu().numpy().astype(bool)[..., None], road)
    assert np.array_equal(out["fence"][0].cpu().numpy().astype(bool)[..., None], fence)
    eng.close()
    with pytest.raises(ValueError):
        Engine(64, 128, 1, "resnet50", precision="f16x2", small_batch=3)
    with pytest.raises(ValueError):
        Engine(64, 128, 1, "resnet50", precision="bf16x3", small_batch=2)
