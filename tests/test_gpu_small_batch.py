"""GPU: the opt-in split-K forms of the small-batch f16x2 handles (Engine(small_batch=True), sd_set_small_batch).

On a handle whose full pass is one or two frames the deep GEMM layers (fc6 / fc7, the res5 1x1 layers, res4_6's) have 16-32 output tiles of
256 x 256 for 256 CUs, at most an eighth of the chip; with the switch they run as S k-slices per tile (conv_splitk_hs_kernel) plus a reduce launch (splitk_reduce_kernel)
that adds the slices in ascending order and applies the layer's epilogue.  Held to the frozen bounds of the exact-f32 engine like every other
f16x2 path, to the fp32-grade gate of test_gpu_nets.py, and to determinism / call-size independence / per-frame range attribution.
Every test builds its engines with small_batch=True."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from oracle import nets
from semantic_depth_amd import _lib as L
from semantic_depth_amd import api
from semantic_depth_amd import weights as Wt
from semantic_depth_amd.engine import Engine, RangeError
from gpu_common import assert_close, dev

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def keep_activations():
    # the engines other modules left in the shared caches hold most of the card by the time this module runs in a whole-suite session:
    # close them (a later user rebuilds its engine on a cache miss) and hand the memory back before the first arena here is allocated
    import gc
    import gpu_common
    for entry in list(gpu_common._cache.values()):
        entry[0].close()
    gpu_common._cache.clear()
    api.release_engines()
    gc.collect()
    torch.cuda.empty_cache()
    os.environ["SEMDEPTH_KEEP_ACTIVATIONS"] = "1"      # layer taps stay intact after a forward
    yield
    os.environ.pop("SEMDEPTH_KEEP_ACTIVATIONS", None)


def _grade():
    spec = importlib.util.spec_from_file_location("f32_grade_check", os.path.join(ROOT, "scripts", "f32_grade_check.py"))
    gc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gc)
    return gc


def _frames(B, H, W, seed=0):
    """the bench's frame recipe (scripts/f32_grade_check.py frame): low-pass of uniform noise + a little noise"""
    gc = _grade()
    return np.concatenate([gc.frame(seed + i, H, W) for i in range(B)], 0)


def _pair(frame):
    f = frame.astype(np.float32) / 255
    return np.stack((f, np.fliplr(f)), 0)


def _fcn_weights():
    return Wt.make_fcn8s_weights(1, decoder_std=0.05, bias_std=0.1)


def _mono_weights(enc):
    return Wt.make_monodepth_weights(enc, 2, bias_std=0.05)


def _engine(H, W, B=1, enc="resnet50", nets_=("fcn", "mono"), small_batch=True, **kw):
    eng = Engine(H, W, B, enc, precision=kw.pop("precision", "f16x2"), small_batch=small_batch, **kw)
    wf = wm = None
    if "fcn" in nets_:
        wf = _fcn_weights()
        eng.load_weights(L.SD_NET_FCN8S, wf)
    if "mono" in nets_:
        wm = _mono_weights(enc)
        eng.load_weights(L.SD_NET_MONODEPTH, wm)
    return eng, wf, wm


def _res5_oracle(pair, wm):
    """the encoder of oracle/nets.py monodepth_forward (resnet50) up to conv5, NHWC"""
    m = nets._Mono(wm, torch.float32)
    x = nets._t(pair, torch.float32).permute(0, 3, 1, 2).contiguous()
    conv1 = m.conv(x, "enc/conv1", 7, 2)
    conv5 = m.resblock(m.resblock(m.resblock(m.resblock(m.maxpool3(conv1), 2, 64, 3), 3, 128, 4), 4, 256, 6), 5, 512, 3)
    return conv5.permute(0, 2, 3, 1).contiguous().numpy()


@pytest.mark.parametrize("H,W", [(256, 512), (512, 1024)])
def test_fcn8s_logits_and_layer7_of_a_one_frame_handle_match_the_oracle(H, W):
    """parity + taps: fc6 and fc7 must be listed as split, or the test says nothing about the split path"""
    eng, wf, _ = _engine(H, W, nets_=("fcn",))
    plan = eng.small_batch_plan()["fcn8s"]
    print("split layers", H, W, plan)
    assert plan.get("fc6", 1) > 1 and plan.get("fc7", 1) > 1, plan
    fr = _frames(1, H, W, seed=41)
    lg = eng.fcn8s_forward(dev(fr), want_logits=True)["logits"].cpu().numpy()
    l7 = eng.net_tensor(L.SD_NET_FCN8S, "layer7_out").cpu().numpy()
    eng.check_range()
    ref, taps = nets.fcn8s_forward(fr, wf, return_taps=True)
    from gpu_common import err_report
    print("logits", err_report(lg, ref), "layer7", err_report(l7, taps["layer7"]))
    assert l7.shape == taps["layer7"].shape
    assert_close(l7, taps["layer7"], "f16x2", what="layer7_out")
    assert_close(lg, ref, "f16x2", what="logits")
    eng.close()


@pytest.mark.parametrize("enc,H,W", [("resnet50", 512, 1024), ("vgg", 256, 512)])
def test_monodepth_disparities_of_a_one_frame_handle_match_the_oracle(enc, H, W):
    eng, _, wm = _engine(H, W, enc=enc, nets_=("mono",))
    plan = eng.small_batch_plan()["monodepth"]
    print("split layers", enc, H, W, plan)
    if enc == "resnet50":
        assert any(k.startswith("enc/res5") for k in plan) and all(s > 1 for s in plan.values()), plan
    else:
        assert plan.get("enc/conv6a", 1) > 1 and plan.get("enc/conv7a", 1) > 1, plan
    fr = _frames(1, H, W, seed=42)
    _, raw = eng.monodepth_forward(dev(fr), want_raw=True)
    raw = raw[0].cpu().numpy()
    eng.check_range()
    pair = _pair(fr[0])
    ref = nets.monodepth_forward(pair, wm, enc)[..., 0]
    from gpu_common import err_report
    print("disparity", enc, err_report(raw, ref))
    if enc == "resnet50":
        c5 = eng.net_tensor(L.SD_NET_MONODEPTH, "enc/conv5").cpu().numpy()
        ref5 = _res5_oracle(pair, wm)
        print("enc/conv5", err_report(c5, ref5))
        assert c5.shape == ref5.shape
        assert_close(c5, ref5, "f16x2", what="enc/conv5")
    assert_close(raw, ref, "f16x2", what="disparity", kind="disp")
    eng.close()


def test_split_handle_is_fp32_grade_against_a_float64_oracle():
    """the gate of test_f16x2_is_fp32_grade_on_every_seed (scripts/f32_grade_check.py verdicts: every figure within 1.5 x the exact-f32 engine's,
    the single worst element within 2 x) on one (weight seed, frame seed) pair per net, the f16x2 engine being a small_batch handle"""
    gc = _grade()
    H, W = 512, 1024
    (ws, fs) = gc.PAIRS[0]
    fr = gc.frame(fs, H, W)
    pair = _pair(fr[0])
    rows = {}
    for enc in ("resnet50", "vgg"):
        wf = Wt.make_fcn8s_weights(ws, decoder_std=0.05, bias_std=0.1)
        wm = Wt.make_monodepth_weights(enc, ws + 100, bias_std=0.05)
        ref_d = nets.monodepth_forward(pair, wm, enc, dtype=torch.float64)[..., 0]
        ref_l = nets.fcn8s_forward(fr, wf, dtype=torch.float64) if enc == "resnet50" else None
        for prec in ("f32", "f16x2"):
            eng = Engine(H, W, 1, enc, precision=prec, small_batch=prec == "f16x2")
            if prec == "f16x2":
                plan = eng.small_batch_plan()
                assert plan["fcn8s"].get("fc6", 1) > 1 and plan["fcn8s"].get("fc7", 1) > 1, plan
            eng.load_weights(L.SD_NET_MONODEPTH, wm)
            _, raw = eng.monodepth_forward(dev(fr), want_raw=True)
            rows[("mono-" + enc, ws, fs, prec)] = gc.stats(raw[0].cpu().numpy(), ref_d)
            if ref_l is not None:
                eng.load_weights(L.SD_NET_FCN8S, wf)
                lg = eng.fcn8s_forward(dev(fr), want_logits=True)["logits"].cpu().numpy()
                rows[("fcn8s", ws, fs, prec)] = gc.stats(lg, ref_l)
            eng.check_range()
            eng.close()
    v = gc.verdicts(rows, "f16x2")
    for r in v:
        print(r)
    assert len(v) == 3 * 4
    assert not [r for r in v if not r[-1]], [r for r in v if not r[-1]]
    for key, st in rows.items():
        assert st["max"] < 1e-5, (key, st)


def test_two_runs_of_the_same_call_are_bit_equal():
    H, W = 256, 512
    eng, _, _ = _engine(H, W)
    assert eng.small_batch_plan()["fcn8s"] and eng.small_batch_plan()["monodepth"]
    fr = dev(_frames(1, H, W, seed=43))
    a = eng.fcn8s_forward(fr, want_logits=True)["logits"].clone()
    pa = eng.monodepth_forward(fr).clone()
    for _ in range(2):
        assert torch.equal(eng.fcn8s_forward(fr, want_logits=True)["logits"], a)
        assert torch.equal(eng.monodepth_forward(fr), pa)
    eng.close()


def test_a_frames_result_does_not_depend_on_the_size_of_the_call():
    H, W = 256, 512
    eng, _, _ = _engine(H, W, B=2)
    plan = eng.small_batch_plan()
    assert plan["fcn8s"].get("fc6", 1) > 1 and plan["monodepth"], plan
    fr = dev(_frames(2, H, W, seed=44))
    two = eng.fcn8s_forward(fr, want_logits=True)["logits"].clone()
    p2 = eng.monodepth_forward(fr).clone()
    one = eng.fcn8s_forward(fr[:1].contiguous(), want_logits=True)["logits"]
    p1 = eng.monodepth_forward(fr[:1].contiguous())
    assert torch.equal(one[0], two[0]) and torch.equal(p1[0], p2[0])
    assert not torch.equal(two[0], two[1])
    eng.close()


def test_the_switch_changes_nothing_on_a_handle_whose_full_pass_fills_the_chip(monkeypatch):
    """max_batch = 32 at 256 x 512 (fc6: 256 tiles; the res4 / res5 1x1 layers 64-256): no candidate is down to an eighth of the CUs, the plan
    lists no layer, the workspace and the bits are the default handle's.  (No layer taps are read: the arenas are laid out with liveness reuse,
    a quarter of the bytes.)"""
    monkeypatch.delenv("SEMDEPTH_KEEP_ACTIVATIONS", raising=False)
    H, W = 256, 512
    fr = dev(_frames(2, H, W, seed=45))
    outs = []
    for sb in (False, True):
        eng, _, _ = _engine(H, W, B=32, small_batch=sb)
        assert eng.small_batch_plan() == {"fcn8s": {}, "monodepth": {}}
        outs.append((eng.fcn8s_forward(fr, want_logits=True)["logits"].cpu(), eng.monodepth_forward(fr).cpu(), eng.bytes["workspace"]))
        eng.close()
        del eng
        torch.cuda.empty_cache()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]) and outs[0][2] == outs[1][2]


def test_range_violations_in_a_split_layer_are_attributed_to_their_frames():
    """the bias-1e5 construction of test_a_value_beyond_the_fp16_range_is_an_error_not_a_counter on fc7, a split layer: the clamps happen in the
    reduce kernel's epilogue"""
    H, W, B = 64, 128, 2
    wf = Wt.make_fcn8s_weights(1, decoder_std=0.05)
    wf["vgg/fc7/biases"] = np.full_like(wf["vgg/fc7/biases"], 1.0e5)
    fr = dev(_frames(B, H, W, seed=46))
    eng = Engine(H, W, B, "resnet50", precision="f16x2", small_batch=True)
    assert eng.small_batch_plan()["fcn8s"].get("fc7", 1) > 1
    eng.load_weights(L.SD_NET_FCN8S, wf)
    lg = eng.fcn8s_forward(fr, want_logits=True)["logits"].cpu().numpy()
    assert np.isfinite(lg).all()
    assert eng.saturated_frames().tolist() == [True, True]
    counts = eng._frame_counts(B, reset=False)
    # at least every fc7 value of each frame (bias 1e5 behind a ReLU), and no clamp that is not on one of the two frames
    assert counts.min() >= (H // 32) * (W // 32) * 4096 * 0.99 and int(counts.sum()) == eng.saturation_count(), counts
    with pytest.raises(RangeError):
        eng.check_range()
    eng.close()
    rec = Engine(H, W, B, "resnet50", precision="f16x2", small_batch=True, on_range="recompute")
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


def test_api_classes_take_the_switch_and_the_c_abi_guards_it():
    H, W = 256, 512
    wf = _fcn_weights()
    fr = _frames(1, H, W, seed=47)
    try:
        seg = api.SegmentFrame((H, W), wf, small_batch=True)
        road, fence, _ = seg.segment_frame(fr[0])
        e = seg.engine
        assert e.small_batch and e.small_batch_plan()["fcn8s"].get("fc6", 1) > 1
        assert api.shared_engine(H, W) is not e                   # the switch is part of the registry key
        assert api.shared_engine(H, W, small_batch=True) is e
        # sd_set_small_batch after sd_bind_memory: SD_ERR_STATE
        assert e.lib.sd_set_small_batch(e.h, 0) == L.SD_ERR_STATE
        assert e.lib.sd_set_small_batch(e.h, 1) == L.SD_ERR_STATE
    finally:
        api.release_engines()
    eng = Engine(H, W, 1, "resnet50", precision="f16x2", small_batch=True)
    eng.load_weights(L.SD_NET_FCN8S, wf)
    out = eng.fcn8s_forward(dev(fr))
    assert np.array_equal(out["road"][0].cpu().numpy().astype(bool)[..., None], road)
    assert np.array_equal(out["fence"][0].cpu().numpy().astype(bool)[..., None], fence)
    eng.close()
    e3 = Engine(64, 128, 1, "resnet50", precision="bf16x3")
    assert e3.lib.sd_set_small_batch(e3.h, 1) == L.SD_ERR_INVALID
    e3.close()
    with pytest.raises(ValueError):
        Engine(64, 128, 1, "resnet50", precision="bf16x3", small_batch=True)
    d = api.DepthFrame(encoder="resnet50", input_height=H, input_width=W, checkpoint_path=_mono_weights("resnet50"), small_batch=True)
    try:
        assert d.engine.small_batch and d.engine.small_batch_plan()["monodepth"]
        assert d.compute_disparity(fr[0]).shape == (H, W)
    finally:
        api.release_engines()
