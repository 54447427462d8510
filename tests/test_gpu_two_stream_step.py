"""GPU: the two-stream pipelined step of bench.py (--overlap: the two networks of step i+1 on the main stream, the tail of step i on a
high-priority side stream, one handle, one workspace arena) held to the one-stream results, bit for bit.

The benchmark feeds every timed step the same frames, so a stale or early read of a region the two streams share would return the same bytes
there.  Here three DIFFERENT frame batches A, B, C go through tests/two_stream_cases.pipelined_steps (the benchmark's step restated;
tests/test_two_stream_step_cpu.py holds it to bench.py's source) as A, B, C, A, B, C with no host synchronisation inside, and every step's
outputs must equal what Engine.process_batch gave the same frames on one stream: masks, disparity, point counts, both clouds with their
colours, the record bytes and the fence-to-fence bytes.  No tolerance: a frame's bits do not depend on call history
(test_gpu_state_independence.py), so any difference is an ordering defect between the streams -- in the library or in the choreography.
The one-stream records are in turn tied to oracle.pipeline.frame_tail (first case), so the overlapped bytes are the CPU restatement's too.

What the comparison can see, measured once on an MI355X with pipelined_steps edited by hand: without `side.wait_event(ev[3])` the record bytes of all
six steps differ, at 128 x 256 and at 256 x 512 (the fusion reads the raw pair of the batch before); without the main stream's wait on ev[4] nothing
differs at these sizes -- the fusion is a few microseconds, the next monodepth pass writes its output tensor milliseconds later -- so that edge is
held by the happens-before check of test_two_stream_step_cpu.py alone.

Conditions on the one-stream reference alone are asserted first: every frame has >= 1000 road points, at least half the frames have a road
width, and the records of A, B and C differ pairwise on every frame (otherwise stale data could pass)."""
import numpy as np
import pytest
import torch

from semantic_depth_amd.engine import Camera, Engine, RoadWidthParams
from gpu_common import _check_records_against_oracle, dev, engine
from test_gpu_pipeline import _smooth_frames
from two_stream_cases import pipelined_steps

pytestmark = pytest.mark.gpu

SEEDS = (201, 202, 203)            # frame batches A, B, C
# 128 x 256, resnet50, max_batch 4: the smallest geometry at which both networks and all three tail stages run their usual kernel families.
# 256 x 512, max_batch 8 with 32 CUs reserved: the persistent launches have more tiles than CUs there, so the reserved-CU grid really differs.
CASES = {
    "f16x2-both-colours": dict(precision="f16x2", approach="both", colours=True, priority=-1, H=128, W=256, max_batch=4, reserve=0),
    "bf16x3-rw-colours": dict(precision="bf16x3", approach="rw", colours=True, priority=-1, H=128, W=256, max_batch=4, reserve=0),
    "plan-both-plain-prio0": dict(precision="plan", approach="both", colours=False, priority=0, H=128, W=256, max_batch=4, reserve=0),
    "f16x2-rw-plain-256x512-reserved32": dict(precision="f16x2", approach="rw", colours=False, priority=-1, H=256, W=512, max_batch=8, reserve=32),
}
_setups = {}


def _camera_at_10m(disp_pp, H, W):
    """test_gpu_pipeline._camera_at_10m at this geometry: the median disparity lies at the measuring depth"""
    d0 = float(disp_pp.median().item()) * float(W)
    return Camera(W / 2 - 0.5, H / 2 - 0.5, 10.0 * d0, 1.0, float(W))


def _bits(t):
    return t.contiguous().view(torch.uint8)


def _one_stream(eng, fr, s):
    """Engine.process_batch on the current stream, then the raw pair of the same frames"""
    out = eng.process_batch(fr, s["cams"][:fr.shape[0]], s["prm"], approach=s["approach"], colours=s["colours"])
    _, raw = eng.monodepth_forward(fr, want_raw=True)
    return out, raw


def _setup(name):
    """engine, the frame batches, the camera and the one-stream reference of a case, with the conditions on the reference alone (once per case)"""
    if name in _setups:
        return _setups[name]
    c = CASES[name]
    H, W, mb = c["H"], c["W"], c["max_batch"]
    eng, _, _ = engine(H, W, mb, "resnet50", fcn_kw=dict(decoder_std=0.05), precision=c["precision"])
    frames_np = [_smooth_frames(mb, H, W, seed=s_) for s_ in SEEDS]
    frames = [dev(f) for f in frames_np]
    s = dict(c, eng=eng, frames_np=frames_np, frames=frames, prm=RoadWidthParams())
    eng.reserve_cus(c["reserve"])
    try:
        s["cams"] = [_camera_at_10m(eng.monodepth_forward(frames[0]), H, W)] * mb
        ref = [_one_stream(eng, fr, s) for fr in frames]
        torch.cuda.synchronize()
    finally:
        eng.reserve_cus(0)
    s["ref"], s["raw"] = [r[0] for r in ref], [r[1] for r in ref]
    recs = [Engine.records(o["records"]) for o in s["ref"]]
    print(name, "n_road", [r["n_road"].tolist() for r in recs], "n_ror", [r["n_ror"].tolist() for r in recs], "found", [r["found"].tolist() for r in recs])
    for r in recs:
        assert (r["n_road"] >= 1000).all(), r["n_road"]
    assert sum(int((r["found"] != 0).sum()) for r in recs) * 2 >= 3 * mb
    rb = [o["records"].cpu().numpy() for o in s["ref"]]
    for i, j in ((0, 1), (0, 2), (1, 2)):
        for b in range(mb):
            assert rb[i][b].tobytes() != rb[j][b].tobytes(), (i, j, b)
    _setups[name] = s
    return s


def _assert_step_equals(got, ref, s, what):
    """every output of a pipelined step against the one-stream outputs of the same frames, byte for byte"""
    B = ref["records"].shape[0]
    for k in ("road", "fence", "argmax"):
        assert torch.equal(got["seg"][k], ref["seg"][k]), (what, k)
    assert got["disp_pp"].shape == ref["disp_pp"].shape and torch.equal(_bits(got["disp_pp"]), _bits(ref["disp_pp"])), (what, "disp_pp")
    for k in ("road", "fence"):
        n_got, n_ref = got["fuse"][f"n_{k}"], ref["fuse"][f"n_{k}"]
        assert torch.equal(n_got, n_ref), (what, f"n_{k}", n_got.tolist(), n_ref.tolist())
        for b, n in enumerate(n_ref.tolist()):
            assert torch.equal(_bits(got["fuse"][f"{k}_xyz"][b, :n]), _bits(ref["fuse"][f"{k}_xyz"][b, :n])), (what, f"{k}_xyz", b)
            if s["colours"]:
                assert torch.equal(got["fuse"][f"{k}_rgb"][b, :n], ref["fuse"][f"{k}_rgb"][b, :n]), (what, f"{k}_rgb", b)
            else:
                assert got["fuse"][f"{k}_rgb"] is None and ref["fuse"][f"{k}_rgb"] is None
    assert got["records"].shape == (B, ref["records"].shape[1]) and torch.equal(got["records"], ref["records"]), \
        (what, "records", Engine.records(got["records"])[["n_road", "n_ror", "found", "width"]], Engine.records(ref["records"])[["n_road", "n_ror", "found", "width"]])
    if s["approach"] == "both":
        assert torch.equal(got["f2f"], ref["f2f"]), (what, "f2f", Engine.f2f_records(got["f2f"])["counts"], Engine.f2f_records(ref["f2f"])["counts"])
    else:
        assert got["f2f"] is None and ref["f2f"] is None


def _pipelined(s, batches):
    eng = s["eng"]
    eng.reserve_cus(s["reserve"])
    try:
        torch.cuda.synchronize()
        outs = pipelined_steps(eng, batches, s["cams"], s["prm"], s["approach"], s["colours"], s["priority"])
        torch.cuda.synchronize()                    # the one synchronisation: nothing inside the region waited on the host
    finally:
        eng.reserve_cus(0)
    return outs


@pytest.mark.parametrize("name", list(CASES))
def test_pipelined_steps_equal_the_one_stream_results(name):
    s = _setup(name)
    eng = s["eng"]
    order = [0, 1, 2, 0, 1, 2]
    outs = _pipelined(s, [s["frames"][i] for i in order])
    assert len(outs) == 6
    for step, i in enumerate(order):
        _assert_step_equals(outs[step], s["ref"][i], s, f"{name}: step {step} (batch {'ABC'[i]})")
    # the handle is left as one-stream use expects it
    eng.reserve_cus(s["reserve"])
    try:
        again, _ = _one_stream(eng, s["frames"][0], s)
        torch.cuda.synchronize()
    finally:
        eng.reserve_cus(0)
    _assert_step_equals(again, s["ref"][0], s, f"{name}: process_batch(A) after the pipelined region")
    if s["precision"] == "f16x2":
        assert eng.saturation_count() == 0
    eng.check_range()


def test_overlapped_records_equal_the_oracle_tail():
    """the oracle tie: the records of batch A as the OVERLAPPED step 3 produced them (A again, between the tails of C and the networks of B),
    through oracle.pipeline.frame_tail fed the GPU's own masks and raw pair"""
    name = next(iter(CASES))
    s = _setup(name)
    outs = _pipelined(s, [s["frames"][i] for i in (0, 1, 2, 0, 1)])
    recs, found = _check_records_against_oracle(s["eng"], s["frames_np"][0], outs[3], s["raw"][0], s["cams"][0], s["prm"], colours=True)
    _check_records_against_oracle(s["eng"], s["frames_np"][0], s["ref"][0], s["raw"][0], s["cams"][0], s["prm"], colours=True)
    print(name, "oracle tie: n_road", recs["n_road"].tolist(), "n_ror", recs["n_ror"].tolist(), "found", found)
    assert found * 2 >= len(recs)


def test_ragged_steps_equal_the_one_stream_results():
    """steps of 4, 3, 4, 2 frames on the first engine: sd_handle::last_mono_frames, the per-frame look-back words and tickets of the one-pass
    fusion and the camera upload across a changing B.  Each step against process_batch on the same frames."""
    name = next(iter(CASES))
    s = _setup(name)
    eng = s["eng"]
    batches = [s["frames"][0], s["frames"][1][:3].contiguous(), s["frames"][2], s["frames"][0][:2].contiguous()]
    refs = [s["ref"][0], _one_stream(eng, batches[1], s)[0], s["ref"][2], _one_stream(eng, batches[3], s)[0]]
    outs = _pipelined(s, batches)
    for step, (got, ref) in enumerate(zip(outs, refs)):
        assert got["records"].shape[0] == batches[step].shape[0]
        _assert_step_equals(got, ref, s, f"{name}: ragged step {step} ({batches[step].shape[0]} frames)")
    assert eng.saturation_count() == 0
    eng.check_range()
