"""Per-frame attribution of fp16 range violations and their recompute on bf16x3 (Engine(on_range='recompute')).

Frames that leave the fp16 range are made by constant first-layer weights: the FCN-8s subtracts the VGG means, so a grey frame of those
means gives ~0 after conv1_1 while a white one exceeds 65504 tenfold; monodepth reads frame / 255, so black gives the bias, white overflows.
"""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import nets
from semantic_depth_amd import _lib as L
from semantic_depth_amd import api, outputs
from semantic_depth_amd import weights as Wt
from semantic_depth_amd.distributed import make_engine_step, run_sequence_files
from semantic_depth_amd.engine import RW_DTYPE, Camera, Engine, RangeError

pytestmark = pytest.mark.gpu

H, W = 128, 256          # (monodepth-vgg needs multiples of 128)
FP16_MAX = 65504.0
MONO_FIRST = {"vgg": "enc/conv1a", "resnet50": "enc/conv1"}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _grey():
    return np.broadcast_to(np.round(np.array(nets.VGG_MEAN_BGR)[::-1]).astype(np.uint8), (H, W, 3)).copy()


def _white():
    return np.full((H, W, 3), 255, np.uint8)


def _fcn_weights():
    """conv1_1 = +c with c chosen on the CPU oracle: white frames >= 10 x 65504 inside the image, grey ones <= 65504 / 10 everywhere"""
    wf = Wt.make_fcn8s_weights(1, decoder_std=0.05)
    frames = np.stack([_grey(), _white()])
    x = nets.vgg_preprocess(frames)
    unit = F.conv2d(x, torch.ones(64, 3, 3, 3), None, padding=1)
    c = float(np.ceil(10 * FP16_MAX / unit[1, :, 1:-1, 1:-1].min().item()))
    wf["vgg/conv1_1/filter"] = np.full_like(wf["vgg/conv1_1/filter"], c)
    y = F.conv2d(x, torch.full((64, 3, 3, 3), c), torch.from_numpy(wf["vgg/conv1_1/biases"]).float(), padding=1)
    assert y[1, :, 1:-1, 1:-1].min().item() >= 10 * FP16_MAX and y[0].abs().max().item() <= FP16_MAX / 10
    lg, taps = nets.fcn8s_forward(frames[:1], wf, return_taps=True)
    for k, v in taps.items():
        assert np.abs(v).max() <= FP16_MAX / 10, k
    return wf


def _mono_weights(enc):
    wm = Wt.make_monodepth_weights(enc, 2)
    k = MONO_FIRST[enc]
    w = wm[f"{k}/weights"]
    c = float(np.ceil(10 * FP16_MAX / (w.shape[0] * w.shape[1] * w.shape[2])))         # white: every tap 1.0 (inside the image)
    wm[f"{k}/weights"] = np.full_like(w, c)
    assert np.abs(wm[f"{k}/biases"]).max() <= FP16_MAX / 10
    return wm


def _mixed(kind="fcn"):
    lo = _grey() if kind == "fcn" else np.zeros((H, W, 3), np.uint8)
    return np.stack([lo, _white(), lo, _white()])


CAMS = [Camera(W / 2, H / 2, 1000.0, 1.0, float(W))] * 4


@pytest.mark.parametrize("chunk", [None, "1"])
def test_fcn_overflow_is_attributed_to_its_frames(chunk, monkeypatch):
    if chunk:
        monkeypatch.setenv("SEMDEPTH_CHUNK", chunk)
    eng = Engine(H, W, 4, "resnet50", precision="f16x2")
    assert eng.pass_frames == (1 if chunk else 4)
    eng.load_weights(L.SD_NET_FCN8S, _fcn_weights())
    eng.fcn8s_forward(dev(_mixed()))
    assert eng.saturated_frames().tolist() == [False, True, False, True]
    assert eng.saturated_frames(reset=True).tolist() == [False, True, False, True]
    assert not eng.saturated_frames().any()
    eng.saturation_count(reset=True)
    eng.close()


@pytest.mark.parametrize("enc", ["vgg", "resnet50"])
@pytest.mark.parametrize("chunk", [None, "1"])
def test_monodepth_overflow_and_its_flip_count_on_their_frame(enc, chunk, monkeypatch):
    if chunk:
        monkeypatch.setenv("SEMDEPTH_CHUNK", chunk)
    eng = Engine(H, W, 4, enc, precision="f16x2")
    eng.load_weights(L.SD_NET_MONODEPTH, _mono_weights(enc))
    before = eng.saturation_count()
    eng.monodepth_forward(dev(_mixed("mono")))
    counts = eng._frame_counts(4, reset=False)
    assert (counts > 0).tolist() == [False, True, False, True]
    # the frame and its fliplr copy are one frame's images: every clamp is on frames 1 and 3 (a flip attributed elsewhere would land on
    # another frame's slot), and the two white frames clamp alike
    assert int(counts.sum()) == eng.saturation_count() - before
    assert counts[1] == counts[3]
    eng.saturation_count(reset=True)
    eng.close()


def _layer_kernels(eng, frames, capfd, net):
    """{conv op: kernel} of one call, from the SEMDEPTH_PROFILE_VERBOSE lines of sd_profile_read"""
    eng.profile(True)
    (eng.fcn8s_forward if net == L.SD_NET_FCN8S else eng.monodepth_forward)(frames)
    capfd.readouterr()
    eng.profile_read()
    eng.profile(False)
    err = capfd.readouterr().err
    out = {}
    for line in err.splitlines():
        if line.startswith("[sd_profile]"):
            parts = line.split()
            m = int(parts[2].split("=")[1])
            out[parts[1]] = (line.split("TF/s", 1)[1].strip(), m)
    return out


def _family(kernel):
    for f in ("conv_stem", "conv_dma3", "conv_dma", "conv_split", "conv_direct3", "conv_direct"):
        if kernel.startswith(f):
            return f
    return None


def test_every_epilogue_family_counts_per_frame_what_it_counts_in_total(monkeypatch, capfd):
    monkeypatch.setenv("SEMDEPTH_PROFILE_VERBOSE", "1")
    rng = np.random.default_rng(3)
    frames = dev(rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8))
    covered = {}
    for enc in ("resnet50", "vgg"):
        eng = Engine(H, W, 2, enc, precision="f16x2")
        base = {L.SD_NET_FCN8S: Wt.make_fcn8s_weights(1, decoder_std=0.05), L.SD_NET_MONODEPTH: Wt.make_monodepth_weights(enc, 2)}
        for net, w in base.items():
            eng.load_weights(net, w)
        for net in (L.SD_NET_FCN8S, L.SD_NET_MONODEPTH):
            kern = _layer_kernels(eng, frames, capfd, net)
            table = eng.weight_table(net)
            pick = {}
            for op, (k, m) in kern.items():
                fam = _family(k)
                bias = [n for n in table if n.rsplit("/", 1)[0].split("/")[-1] == op.split("/")[-1] and n.rsplit("/", 1)[1] in ("biases", "bias")]
                # (a layer whose GEMM rows end in a partial tile clamps rows no image owns: they count in total only)
                if fam and fam not in covered and fam not in pick and len(bias) == 1 and m % 512 == 0:
                    pick[fam] = (op, bias[0])
            for fam, (op, bname) in pick.items():
                w = dict(base[net])
                w[bname] = np.full_like(w[bname], 1.0e6)
                eng.load_weights(net, w)
                eng.saturation_count(reset=True)
                eng.saturated_frames(reset=True)
                (eng.fcn8s_forward if net == L.SD_NET_FCN8S else eng.monodepth_forward)(frames)
                total = eng.saturation_count()
                per = eng._frame_counts(2, reset=True)
                assert total > 0, (fam, op)
                assert int(per.sum()) == total and (per > 0).all(), (fam, op, per, total)
                covered[fam] = op
                eng.load_weights(net, base[net])
            eng.saturation_count(reset=True)
        eng.close()
    assert {"conv_stem", "conv_dma", "conv_direct"} <= set(covered), covered


def _bits(t):
    return t.detach().cpu().numpy().tobytes()


def _cmp_frame(a, ia, b, ib):
    """every per-frame output of process_batch: frame ia of result a == frame ib of result b, bit for bit (clouds up to their counts)"""
    for k in ("road", "fence", "argmax"):
        assert _bits(a["seg"][k][ia]) == _bits(b["seg"][k][ib]), k
    assert _bits(a["disp_pp"][ia]) == _bits(b["disp_pp"][ib])
    assert _bits(a["records"][ia]) == _bits(b["records"][ib])
    assert _bits(a["f2f"][ia]) == _bits(b["f2f"][ib])
    for kind in ("road", "fence"):
        n = int(a["fuse"][f"n_{kind}"][ia])
        assert n == int(b["fuse"][f"n_{kind}"][ib])
        assert _bits(a["fuse"][f"{kind}_xyz"][ia, :n]) == _bits(b["fuse"][f"{kind}_xyz"][ib, :n])
        assert _bits(a["fuse"][f"{kind}_rgb"][ia, :n]) == _bits(b["fuse"][f"{kind}_rgb"][ib, :n])
    n = int(a["road_final"]["n"][ia])
    assert n == int(b["road_final"]["n"][ib])
    assert _bits(a["road_final"]["xyz"][ia, :n]) == _bits(b["road_final"]["xyz"][ib, :n])
    cnt = Engine.f2f_records(a["f2f"][ia:ia + 1])[0]["counts"]
    for side, c in (("left", int(cnt[5])), ("right", int(cnt[6]))):
        assert _bits(a["fence_final"][f"{side}_xyz"][ia, :c]) == _bits(b["fence_final"][f"{side}_xyz"][ib, :c])


def test_recompute_splices_bf16x3_frames_into_the_f16x2_batch():
    wf, wm = _fcn_weights(), Wt.make_monodepth_weights("resnet50", 2)
    fr = dev(_mixed())

    def run(precision, frames, on_range="raise"):
        e = Engine(H, W, 4, "resnet50", precision=precision, on_range=on_range)
        e.load_weights(L.SD_NET_FCN8S, wf)
        e.load_weights(L.SD_NET_MONODEPTH, wm)
        return e, e.process_batch(frames, CAMS[:frames.shape[0]], approach="both", want_final=True)

    eng = Engine(H, W, 4, "resnet50", precision="f16x2", on_range="recompute")
    eng.load_weights(L.SD_NET_FCN8S, wf)
    eng.load_weights(L.SD_NET_MONODEPTH, wm)
    with pytest.warns(RuntimeWarning):
        out = eng.process_batch(fr, CAMS, approach="both", want_final=True)
    assert eng.last_recomputed == [1, 3]
    eng.check_range()                                                  # no RangeError: every clamped frame was recomputed
    e_x3, alone = run("bf16x3", fr[1:2].contiguous())
    _cmp_frame(out, 1, alone, 0)
    _cmp_frame(out, 3, alone, 0)                                       # (frames 1 and 3 are the same white frame)
    e_x3.close()
    e_f16, greys = run("f16x2", fr[0::2].contiguous())
    _cmp_frame(out, 0, greys, 0)
    _cmp_frame(out, 2, greys, 1)
    e_f16.close()
    again = eng.process_batch(fr[0::2].contiguous(), CAMS[:2], approach="both", want_final=True)
    assert eng.last_recomputed == []
    eng.check_range()
    _cmp_frame(again, 0, greys, 0)
    eng.close()


def test_raise_mode_still_raises_on_the_same_batch():
    eng = Engine(H, W, 4, "resnet50", precision="f16x2")
    eng.load_weights(L.SD_NET_FCN8S, _fcn_weights())
    eng.fcn8s_forward(dev(_mixed()))
    with pytest.raises(RangeError):
        eng.check_range()
    eng.close()


def test_segment_frame_recompute_matches_bf16x3_where_f16x2_raised():
    """f16x2 must not be able to fail where the reference cannot (conv4_1's bias of 1e5, as in test_gpu_nets)"""
    wf = Wt.make_fcn8s_weights(1, decoder_std=0.05)
    wf["vgg/conv4_1/biases"] = np.full_like(wf["vgg/conv4_1/biases"], 1.0e5)
    fr = np.random.default_rng(2).integers(0, 256, (H, W, 3), dtype=np.uint8)
    try:
        rec = api.SegmentFrame((H, W), wf, precision="f16x2", on_range="recompute")
        ref = api.SegmentFrame((H, W), wf, precision="bf16x3")
        with pytest.warns(RuntimeWarning):
            road, fence, ov = rec.segment_frame(fr)
        assert rec.engine.last_recomputed == [0] and rec.engine.on_range == "recompute"
        r2, f2, o2 = ref.segment_frame(fr)
        assert np.array_equal(road, r2) and np.array_equal(fence, f2) and np.array_equal(ov, o2)
        assert api.shared_engine(H, W, precision="f16x2", on_range="recompute") is rec.engine
        assert api.shared_engine(H, W, precision="f16x2") is not rec.engine
    finally:
        api.release_engines()


def test_sequence_driver_writes_the_spliced_outputs_and_names_the_recomputed_frames(tmp_path):
    wf, wm = _fcn_weights(), Wt.make_monodepth_weights("resnet50", 2)
    frames = _mixed()
    frame_dir = tmp_path / "in"
    frame_dir.mkdir()
    paths = []
    for i, f in enumerate(frames):
        p = str(frame_dir / f"f_{i:03d}.png")
        outputs.write_png(p, f)
        paths.append(p)
    cam = CAMS[0]
    eng = Engine(H, W, 4, "resnet50", precision="f16x2", on_range="recompute")
    eng.load_weights(L.SD_NET_FCN8S, wf)
    eng.load_weights(L.SD_NET_MONODEPTH, wm)
    names = outputs.sequence_names(paths)
    outs = outputs.SequenceOutputs(str(tmp_path / "out"), names, threads=2, ply=False)
    step = make_engine_step(eng, lambda i: cam, outputs=outs, on_range="recompute")
    with pytest.warns(RuntimeWarning):
        recs = run_sequence_files(paths, step, batch=4, device="cuda", workers=1)
    assert step.recomputed == [1, 3]
    m = json.load(open(os.path.join(str(tmp_path / "out"), "manifest_rank0.json")))
    assert m["status"] == "ok" and m["recomputed"] == [names[1], names[3]]
    # the per-frame mix: white frames as bf16x3 computes them, grey ones as f16x2
    ex3 = Engine(H, W, 4, "resnet50", precision="bf16x3")
    ef16 = Engine(H, W, 4, "resnet50", precision="f16x2")
    for e in (ex3, ef16):
        e.load_weights(L.SD_NET_FCN8S, wf)
        e.load_weights(L.SD_NET_MONODEPTH, wm)
    fr = dev(frames)
    want_x3 = ex3.process_batch(fr, CAMS)
    want_f16 = ef16.process_batch(fr[0::2].contiguous(), CAMS[:2])
    got = recs.cpu().numpy().view(RW_DTYPE).reshape(-1)
    x3 = Engine.records(want_x3["records"])
    f16 = Engine.records(want_f16["records"])
    assert got[1].tobytes() == x3[1].tobytes() and got[3].tobytes() == x3[3].tobytes()
    assert got[0].tobytes() == f16[0].tobytes() and got[2].tobytes() == f16[1].tobytes()
    img_dir = os.path.join(str(tmp_path / "out"), outputs.SEQ_IMG_DIR)
    from semantic_depth_amd import frame_io
    im_x3 = ex3.compose_result_frames(fr, want_x3["seg"]["road"], want_x3["seg"]["fence"], want_x3["records"], H, W,
                                      outs.road_color, outs.fence_color, outs.alpha).cpu().numpy()
    im_f16 = ef16.compose_result_frames(fr[0::2].contiguous(), want_f16["seg"]["road"], want_f16["seg"]["fence"], want_f16["records"], H, W,
                                        outs.road_color, outs.fence_color, outs.alpha).cpu().numpy()
    for i, want in ((0, im_f16[0]), (1, im_x3[1]), (2, im_f16[1]), (3, im_x3[3])):
        assert np.array_equal(frame_io.imread(os.path.join(img_dir, names[i] + ".png")), want), i
    for e in (eng, ex3, ef16):
        e.close()


def test_clamps_of_padding_rows_do_not_outlive_the_recompute():
    """an fp16-range bias on a layer whose GEMM rows end in a partial tile (fc7: 4 x 8 px per frame at this geometry): the zero-padded rows
    output the bias and clamp too, but no frame owns them.  'raise' still counts them; 'recompute' takes them out with the frame's own, so
    check_range stays quiet on this call and every later one (the sequence driver's next batch included)."""
    wf = Wt.make_fcn8s_weights(1, decoder_std=0.05)
    wf["vgg/fc7/biases"] = np.full_like(wf["vgg/fc7/biases"], 1.0e5)
    fr = np.random.default_rng(4).integers(0, 256, (1, H, W, 3), dtype=np.uint8)
    eng = Engine(H, W, 1, "resnet50", precision="f16x2")
    eng.load_weights(L.SD_NET_FCN8S, wf)
    eng.fcn8s_forward(dev(fr))
    per = int(eng._frame_counts(1, reset=True).sum())
    total = eng.saturation_count(reset=True)
    assert 0 < per < total                                 # (the padding rows clamped: the case exists at this geometry)
    eng.close()
    rec = Engine(H, W, 1, "resnet50", precision="f16x2", on_range="recompute")
    rec.load_weights(L.SD_NET_FCN8S, wf)
    ref = Engine(H, W, 1, "resnet50", precision="bf16x3")
    ref.load_weights(L.SD_NET_FCN8S, wf)
    want = ref.fcn8s_forward(dev(fr), want_logits=True)
    for i in range(3):
        if i == 0:
            with pytest.warns(RuntimeWarning):
                got = rec.fcn8s_forward(dev(fr), want_logits=True)
        else:
            got = rec.fcn8s_forward(dev(fr), want_logits=True)
        assert rec.last_recomputed == [0]
        rec.check_range()
        assert rec.saturation_count() == 0
        for k in ("logits", "road", "fence", "argmax"):
            assert _bits(got[k]) == _bits(want[k]), k
    seg = api.SegmentFrame((H, W), wf, engine=rec, precision="f16x2")
    seg.segment_frame(fr[0])                               # (calls check_range: quiet)
    rec.close()
    ref.close()


def test_full_size_eight_frame_pass_attributes_to_the_right_frames():
    """at 512 x 1024 a pass of 8 frames: the deep layers' 256-row tiles then hold the rows of several frames (fc6: 16 x 32 px per frame), so
    an image mapping that is off by a frame would flag grey frames"""
    global H, W
    h0, w0 = H, W
    wf = _fcn_weights()                                    # (chosen at the small geometry: a constant frame's values do not depend on it)
    try:
        H, W = 512, 1024
        frames = np.stack([_grey(), _white()] * 4)
        eng = Engine(H, W, 8, "resnet50", precision="f16x2")
        eng.load_weights(L.SD_NET_FCN8S, wf)
        eng.fcn8s_forward(dev(frames))
        assert eng.saturated_frames(n=8).tolist() == [False, True] * 4
        eng.saturation_count(reset=True)
        eng.close()
    finally:
        H, W = h0, w0
