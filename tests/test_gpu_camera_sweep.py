"""GPU: the camera sweep -- T trial cameras per frame behind one compaction (sd_fuse_backproject_sweep), the batched chains over the
(trial, frame) slots (Engine.sweep_tail) and one network pass per frame batch (Engine.camera_sweep) -- against the calls they batch
(Engine.fuse_backproject, road_width, fence_to_fence, process_batch: bit for bit) and against the oracle."""
from dataclasses import replace

import numpy as np
import pytest
import torch

from oracle import fusion, pipeline
from gpu_common import Camera, RoadWidthParams, dev, engine
from semantic_depth_amd.engine import Engine, FenceParams

pytestmark = pytest.mark.gpu

H, W = 128, 256                      # 32 blocks of 1024 pixels (128 of 256): the scan is multi-block
NPIX = H * W


@pytest.fixture(scope="module")
def eng():
    return engine(H, W, 4, "resnet50", load=())[0]


@pytest.fixture(scope="module", autouse=True)
def _release_own_engines():
    """the engines only this module asks gpu_common for are closed and dropped from its cache when the module is done, and the freed
    blocks go back to the device: the rest of the suite starts with the memory it had before"""
    import gc

    import gpu_common
    before = set(gpu_common._cache)
    yield
    for key in set(gpu_common._cache) - before:
        if key[:3] != (H, W, 4):                                            # (test_gpu_fusion.py shares the 128 x 256, max_batch 4 engine)
            gpu_common._cache.pop(key)[0].close()
    gc.collect()
    torch.cuda.empty_cache()


def _cam_dict(c):
    return dict(cx=c.cx, cy=c.cy, f=c.f, b=c.b, disp_mult=c.disp_mult)


def _trial_cams(base):
    """T = 3 trials of len(base) frames: no field is shared between two cameras; trial 1 has the other rig (b = 0.6, multiplier 3800, shifted
    principal point) of test_gpu_fusion.py"""
    rows = []
    for t, (f, b_, mult) in enumerate(((250.0, 1.0, None), (300.0, 0.6, 3800.0), (410.0, 0.8, 512.0))):
        rows.append([Camera(c.cx + 2.25 * t + 0.5 * i, c.cy - 1.5 * t - 0.25 * i, f + 7.0 * i, b_ + i / 64.0, (mult or c.disp_mult) + 16.0 * i)
                     for i, c in enumerate(base)])
    return rows


class _Case:
    """two fence scenes, their device tensors, and per trial the existing call's result (computed once, shared)"""

    def __init__(self, e):
        self.scenes = [pipeline.synthetic_scene(H, W, seed=s, f=250.0, fences=True) for s in (3, 4)]
        self.cams = _trial_cams([Camera(**s[4]) for s in self.scenes])
        self.pp = e.post_process(dev(np.stack([s[0] for s in self.scenes])))
        self.road = dev(np.stack([s[1] for s in self.scenes]).astype(np.uint8))
        self.fence = dev(np.stack([s[2] for s in self.scenes]).astype(np.uint8))
        self.frames = dev(np.stack([s[3] for s in self.scenes]))
        self.plain = [e.fuse_backproject(self.pp, self.road, self.fence, self.frames, row) for row in self.cams]
        self.oracle = [[fusion.fuse(s[0], s[1], s[2], s[3], **_cam_dict(c)) for s, c in zip(self.scenes, row)] for row in self.cams]


@pytest.fixture(scope="module")
def case(eng):
    return _Case(eng)


def _assert_slots_equal_plain(out, plain_per_trial, B, cap=None, rgb=True, fence=True):
    """slot t * B + b == frame b of the existing call with trial t's cameras: counts, and rows [:min(n, cap)] of xyz and rgb"""
    for t, ref in enumerate(plain_per_trial):
        for b in range(B):
            s = t * B + b
            for k in ("road", "fence") if fence else ("road",):
                n = int(out[f"n_{k}"][s])
                assert n == int(ref[f"n_{k}"][b]), (t, b, k)
                m = n if cap is None else min(n, cap)
                assert np.array_equal(out[f"{k}_xyz"][s, :m].cpu().numpy(), ref[f"{k}_xyz"][b, :m].cpu().numpy(), equal_nan=True), (t, b, k)
                if rgb:
                    assert np.array_equal(out[f"{k}_rgb"][s, :m].cpu().numpy(), ref[f"{k}_rgb"][b, :m].cpu().numpy()), (t, b, k)


# ------------------------------------------------------------------------------------------------ the launch against the existing call
@pytest.mark.parametrize("one_pixel_per_thread", [False, True])
def test_sweep_slots_equal_the_plain_call_and_the_oracle(eng, case, one_pixel_per_thread, monkeypatch):
    """B = 2 frames, T = 3 trials: every slot is the existing call's frame and the oracle's, in both forms of the write kernel"""
    e = eng
    if one_pixel_per_thread:
        monkeypatch.setenv("SEMDEPTH_DISABLE", "fuse4")            # switches are latched when the handle is created
        e = Engine(H, W, 4, "resnet50")
    out = e.fuse_backproject_sweep(case.pp, case.road, case.fence, case.frames, case.cams)
    assert tuple(out["road_xyz"].shape) == (6, NPIX, 3) and tuple(out["n_fence"].shape) == (6,) and out["road_rgb"].dtype == torch.uint8
    _assert_slots_equal_plain(out, case.plain, 2)
    for t in range(3):
        for b in range(2):
            s, ref = t * 2 + b, case.oracle[t][b]
            nr, nf = int(out["n_road"][s]), int(out["n_fence"][s])
            assert nr == len(ref["road3d"]) > 0 and nf == len(ref["fence3d"]) > 0
            assert np.array_equal(out["road_xyz"][s, :nr].cpu().numpy(), ref["road3d"])
            assert np.array_equal(out["road_rgb"][s, :nr].cpu().numpy(), ref["road_rgb"])
            assert np.array_equal(out["fence_xyz"][s, :nf].cpu().numpy(), ref["fence3d"])
            assert np.array_equal(out["fence_rgb"][s, :nf].cpu().numpy(), ref["fence_rgb"])
    # the trials do differ: a launch that ignored the camera could not have passed
    assert not torch.equal(out["road_xyz"][0, :100], out["road_xyz"][2, :100])


def test_sweep_without_colours_and_without_the_fence_group(eng, case):
    out = eng.fuse_backproject_sweep(case.pp, case.road, case.fence, case.frames, case.cams, want_rgb=False)
    assert out["road_rgb"] is None and out["fence_rgb"] is None
    _assert_slots_equal_plain(out, case.plain, 2, rgb=False)
    out = eng.fuse_backproject_sweep(case.pp, case.road, case.fence, None, case.cams)          # no frames: no colours either
    assert out["road_rgb"] is None
    _assert_slots_equal_plain(out, case.plain, 2, rgb=False)
    out = eng.fuse_backproject_sweep(case.pp, case.road, case.fence, case.frames, case.cams, want_fence=False)
    assert out["fence_xyz"] is None and out["fence_rgb"] is None and out["n_fence"] is None
    _assert_slots_equal_plain(out, case.plain, 2, fence=False)


def test_one_trial_is_the_plain_call(eng, case):
    out = eng.fuse_backproject_sweep(case.pp, case.road, case.fence, case.frames, case.cams[1:2])
    assert out["road_xyz"].shape[0] == 2
    _assert_slots_equal_plain(out, case.plain[1:2], 2)


# ------------------------------------------------------------------------------------------------ edges of the same launch
def test_empty_full_and_block_straddling_masks(eng, case):
    """frame 0: no road, every pixel fence; frame 1: every pixel road, and a fence mask whose kept pixels are the last pixel of every
    1024-pixel block and the first of the next (and of every 256-pixel block), with the image's first and last pixel"""
    road = np.zeros((2, NPIX), np.uint8)
    fence = np.ones((2, NPIX), np.uint8)
    road[1] = 1
    fence[1] = 0
    edge = np.arange(256, NPIX, 256)
    fence[1, edge] = fence[1, edge - 1] = 1
    fence[1, 0] = fence[1, NPIX - 1] = 200                                  # any non-zero byte is "set"
    road_d, fence_d = dev(road.reshape(2, H, W)), dev(fence.reshape(2, H, W))
    cams = case.cams[:2]
    out = eng.fuse_backproject_sweep(case.pp, road_d, fence_d, case.frames, cams)
    n_edge = int((fence[1] != 0).sum())
    assert out["n_road"].tolist() == [0, NPIX, 0, NPIX] and out["n_fence"].tolist() == [NPIX, n_edge, NPIX, n_edge]
    plain = [eng.fuse_backproject(case.pp, road_d, fence_d, case.frames, row) for row in cams]
    _assert_slots_equal_plain(out, plain, 2)
    # the straddling mask against the oracle's row-major gather
    for t in range(2):
        ref = fusion.fuse(case.scenes[1][0], road[1].reshape(H, W).astype(bool), fence[1].reshape(H, W).astype(bool), case.scenes[1][3],
                          **_cam_dict(cams[t][1]))
        assert np.array_equal(out["fence_xyz"][t * 2 + 1, :n_edge].cpu().numpy(), ref["fence3d"])
        assert np.array_equal(out["fence_rgb"][t * 2 + 1, :n_edge].cpu().numpy(), ref["fence_rgb"])


def test_capacity_below_the_count_and_untouched_rows(eng, case):
    """cap = 1000 under a full road mask: the count is reported in full and rows < cap are the uncapped launch's; a slot's rows behind
    its count and an empty slot's first row keep the sentinel they were filled with"""
    cap, few = 1000, 10
    road = np.zeros((2, NPIX), np.uint8)
    fence = np.zeros((2, NPIX), np.uint8)
    road[0] = fence[0] = 1                                                  # frame 0: both clouds overflow the capacity
    road[1, np.arange(few) * 1500 + 1023] = 1                               # frame 1: ten road pixels, no fence pixel
    road_d, fence_d = dev(road.reshape(2, H, W)), dev(fence.reshape(2, H, W))
    cams = case.cams
    buf = eng._sweep_buffers(6, 2, 3, cap, True, True)
    for k in ("road_xyz", "fence_xyz"):
        buf[k].fill_(-777.0)
    for k in ("road_rgb", "fence_rgb"):
        buf[k].fill_(201)
    out = eng._fuse_sweep_into(buf, case.pp, road_d, fence_d, case.frames, cams)
    full = eng.fuse_backproject_sweep(case.pp, road_d, fence_d, case.frames, cams)
    plain = [eng.fuse_backproject(case.pp, road_d, fence_d, case.frames, row, cap=cap) for row in cams]
    assert out["n_road"].tolist() == [NPIX, few] * 3 and out["n_fence"].tolist() == [NPIX, 0] * 3
    assert torch.equal(out["n_road"], full["n_road"]) and torch.equal(out["n_fence"], full["n_fence"])
    _assert_slots_equal_plain(out, plain, 2, cap=cap)
    for t in range(3):
        s0, s1 = t * 2, t * 2 + 1
        for k in ("road", "fence"):
            assert torch.equal(out[f"{k}_xyz"][s0], full[f"{k}_xyz"][s0, :cap]) and torch.equal(out[f"{k}_rgb"][s0], full[f"{k}_rgb"][s0, :cap])
        assert torch.equal(out["road_xyz"][s1, :few], full["road_xyz"][s1, :few])
        assert bool((out["road_xyz"][s1, few:] == -777.0).all()) and bool((out["road_rgb"][s1, few:] == 201).all())
        assert bool((out["fence_xyz"][s1] == -777.0).all()) and bool((out["fence_rgb"][s1] == 201).all())     # the slot behind an overflowing one


def test_zero_infinite_and_nan_disparities(eng, case):
    """a row of zero, +-inf and NaN disparities under a full mask: +-inf / NaN exactly like IEEE division in the oracle, for a sparse
    Q (the shortcut's guard) in every trial"""
    pp0 = case.pp[:1].clone()
    vals = torch.tensor([0.0, float("inf"), float("nan"), -0.0, float("-inf"), 0.25], device=pp0.device)
    pp0[0, 5, :] = vals.repeat(W // 6 + 1)[:W]
    ones = dev(np.ones((1, H, W), np.uint8))
    cams = [row[:1] for row in case.cams]
    out = eng.fuse_backproject_sweep(pp0, ones, None, None, cams, want_fence=False)
    plain = [eng.fuse_backproject(pp0, ones, None, None, row, want_fence=False) for row in cams]
    _assert_slots_equal_plain(out, plain, 1, rgb=False, fence=False)
    seen_nonfinite = False
    for t, row in enumerate(cams):
        c = row[0]
        d0 = pp0[0].cpu().numpy() * np.float32(c.disp_mult)
        with np.errstate(all="ignore"):
            ref = fusion.reproject(d0, fusion.make_Q(c.cx, c.cy, c.f, c.b))
        assert int(out["n_road"][t]) == NPIX
        assert np.array_equal(out["road_xyz"][t].cpu().numpy().reshape(H, W, 3), ref, equal_nan=True), t
        seen_nonfinite |= not np.isfinite(ref[5]).all()
    assert seen_nonfinite


# ------------------------------------------------------------------------------------------------ sweep_tail
TRIAL_F = (200.0, 300.0, 380.0)
RW_COUNTS = ("n_road", "n_zcut", "n_mad_y", "n_mad_x", "n_plane", "n_sor", "n_ror")
PLANE_TOL = dict(rtol=1e-8, atol=1e-10)          # as in test_gpu_pcl_chains.py


class _TailCase:
    def __init__(self):
        self.scenes = [pipeline.synthetic_scene(H, W, seed=s, f=250.0, fences=True) for s in (3, 4, 5)]
        self.cams = [[replace(Camera(**s[4]), f=f) for s in self.scenes] for f in TRIAL_F]        # [t][frame]
        self.rw, self.ft = {}, {}
        for t in range(3):
            for i, s in enumerate(self.scenes):
                ref = pipeline.frame_tail(s[0], s[1], s[2], s[3], _cam_dict(self.cams[t][i]))
                self.rw[(t, i)] = ref["rw"]
                self.ft[(t, i)] = pipeline.fence_tail(ref["fence3d"], ref["fence_rgb"], ref["rw"]["plane"])

    def tensors(self, e, idx):
        sc = [self.scenes[i] for i in idx]
        return (e.post_process(dev(np.stack([s[0] for s in sc]))), dev(np.stack([s[1] for s in sc]).astype(np.uint8)),
                dev(np.stack([s[2] for s in sc]).astype(np.uint8)), dev(np.stack([s[3] for s in sc])))


@pytest.fixture(scope="module")
def tail_case():
    return _TailCase()


def _check_against_oracle(rec, f2, rw, ft, tag):
    got = [int(rec[k]) for k in RW_COUNTS]
    want = [rw[k] for k in ("n_in", "n_zcut", "n_mad_y", "n_mad_x", "n_plane", "n_sor", "n_ror")]
    assert got == want, (tag, got, want)
    assert bool(rec["found"]) == rw["found"], tag
    if rw["found"]:
        assert float(rec["width"]) == rw["width"] and float(rec["x_left"]) == rw["x_left"] and float(rec["x_right"]) == rw["x_right"], tag
        assert np.array_equal(rec["left_pt"].astype(np.float64), rw["left_pt"]) and np.array_equal(rec["right_pt"].astype(np.float64), rw["right_pt"]), tag
    else:
        assert np.isnan(rec["width"]), tag
    np.testing.assert_allclose(rec["plane"], [rw["plane"][k] for k in ("Cx", "Cy", "Cz", "C")], **PLANE_TOL)
    assert [int(c) for c in f2["counts"]] == [ft["n_fence"], ft["n_mad_y"], ft["n_thr"], ft["n_left"], ft["n_right"], ft["n_left_final"],
                                              ft["n_right_final"]], tag
    assert bool(f2["ok"]), tag
    np.testing.assert_allclose(f2["dist"], ft["dist"], rtol=1e-9)
    np.testing.assert_allclose(f2["left_pt"], ft["left_pt"], rtol=1e-9, atol=1e-9)
    for side in ("left", "right"):
        pl = ft["plane_" + side]
        np.testing.assert_allclose(f2["plane_" + side], [pl[k] for k in ("Cx", "Cy", "Cz", "C")], **PLANE_TOL)


def test_sweep_tail_equals_the_chains_per_trial_and_the_oracle(eng, tail_case):
    """seeds 3, 4 as one call of B = 2 (T * B = 6: two chunks on max_batch = 4) and seed 5 as a call of B = 1 (one chunk); trials
    f = 200, 300, 380, approach 'both'.  The oracle's own spread over the trials first, then the records' bytes against the chains run
    per trial, their fields against the oracle, a T * B = 4 call, and an engine with max_batch = 2 (other chunking)."""
    tc = tail_case
    for i in range(3):                                                      # a sweep that ignored f could not reproduce this
        assert [tc.rw[(t, i)]["found"] for t in range(3)] == [False, True, True]
        nz = [tc.rw[(t, i)]["n_zcut"] for t in range(3)]
        assert 4000 < nz[0] < 4300 and 9200 < nz[1] < 9400 and nz[2] == 10158, nz
        assert all(6.3 < tc.rw[(t, i)]["width"] < 6.8 for t in (1, 2)) and tc.rw[(1, i)]["width"] != tc.rw[(2, i)]["width"]
        dist = [tc.ft[(t, i)]["dist"] for t in range(3)]
        assert all(8.2 < d < 8.35 for d in dist) and len(set(dist)) == 3, dist
    prm, fp = RoadWidthParams(), FenceParams()
    small = engine(H, W, 2, "resnet50", load=())[0]
    for idx in ((0, 1), (2,)):
        B = len(idx)
        pp, road, fence, frames = tc.tensors(eng, idx)
        cams = [[row[i] for i in idx] for row in tc.cams]
        out = eng.sweep_tail(pp, road, fence, frames, cams, prm, approach="both", fence_params=fp)
        assert tuple(out["records"].shape) == (3 * B, 104) and out["records"].is_cuda and out["f2f"].shape[0] == 3 * B
        rec_b, f2f_b = out["records"].cpu().numpy(), out["f2f"].cpu().numpy()
        recs, f2s = Engine.records(out["records"]), Engine.f2f_records(out["f2f"])
        for t in range(3):
            fz = eng.fuse_backproject(pp, road, fence, None, cams[t])
            rw = eng.road_width(fz["road_xyz"], fz["n_road"], prm)
            f2 = eng.fence_to_fence(fz["fence_xyz"], fz["n_fence"], rw, fp)
            assert rec_b[t * B:(t + 1) * B].tobytes() == rw.cpu().numpy().tobytes(), (idx, t)
            assert f2f_b[t * B:(t + 1) * B].tobytes() == f2.cpu().numpy().tobytes(), (idx, t)
            for b, i in enumerate(idx):
                _check_against_oracle(recs[t * B + b], f2s[t * B + b], tc.rw[(t, i)], tc.ft[(t, i)], (i, t))
        # colours carried through the chains change no record
        col = eng.sweep_tail(pp, road, fence, frames, cams, prm, approach="both", fence_params=fp, colours=True)
        assert col["records"].cpu().numpy().tobytes() == rec_b.tobytes() and col["f2f"].cpu().numpy().tobytes() == f2f_b.tobytes()
        # T * B = 4 (B = 2: one chunk): the last two trials alone are the same slots
        two = eng.sweep_tail(pp, road, fence, frames, cams[1:], prm, approach="both", fence_params=fp)
        assert two["records"].cpu().numpy().tobytes() == rec_b[B:].tobytes() and two["f2f"].cpu().numpy().tobytes() == f2f_b[B:].tobytes()
        # another chunking: max_batch = 2 walks B = 2 one trial at a time, B = 1 two trials at a time
        pp2, road2, fence2, frames2 = tc.tensors(small, idx)
        oth = small.sweep_tail(pp2, road2, fence2, frames2, cams, prm, approach="both", fence_params=fp)
        assert oth["records"].cpu().numpy().tobytes() == rec_b.tobytes() and oth["f2f"].cpu().numpy().tobytes() == f2f_b.tobytes()
        rw_only = eng.sweep_tail(pp, road, fence, frames, cams, prm)
        assert rw_only["f2f"] is None and rw_only["records"].cpu().numpy().tobytes() == rec_b.tobytes()
    with pytest.raises(ValueError):
        pp, road, fence, frames = tc.tensors(small, (0, 1, 2))
        small.sweep_tail(pp, road, fence, frames, tc.cams, prm)              # B = 3 > max_batch = 2


# ------------------------------------------------------------------------------------------------ camera_sweep
def test_camera_sweep_runs_each_network_once_and_equals_process_batch(monkeypatch):
    """128 x 128 (the smallest geometry the vgg monodepth plan accepts: H and W multiples of 128), two frames, three focal lengths on the
    f32 engine with its synthetic weights: records and f2f are process_batch's bytes per trial -- whatever those weights segment -- and
    each network ran once"""
    e = engine(128, 128, 4, "vgg", precision="f32")[0]
    frames = dev(np.stack([pipeline.synthetic_scene(128, 128, seed=s, f=125.0)[3] for s in (1, 2)]))
    cams = [[Camera(64.8, 59.8, f, 1.0, 128.0), Camera(63.1, 61.4, f + 3.0, 1.0, 130.0)] for f in (100.0, 125.0, 160.0)]
    want = [e.process_batch(frames, row, approach="both") for row in cams]
    calls = dict(fcn=0, mono=0)
    fcn, mono = Engine._fcn8s, Engine._mono

    def count_fcn(self, *a, **k):
        calls["fcn"] += 1
        return fcn(self, *a, **k)

    def count_mono(self, *a, **k):
        calls["mono"] += 1
        return mono(self, *a, **k)

    monkeypatch.setattr(Engine, "_fcn8s", count_fcn)
    monkeypatch.setattr(Engine, "_mono", count_mono)
    out = e.camera_sweep(frames, cams, approach="both")
    assert calls == dict(fcn=1, mono=1)
    assert torch.equal(out["disp_pp"], want[0]["disp_pp"]) and torch.equal(out["seg"]["road"], want[0]["seg"]["road"])
    rec, f2f = out["records"].cpu().numpy(), out["f2f"].cpu().numpy()
    assert rec.shape == (6, 104)
    for t in range(3):
        assert rec[2 * t:2 * t + 2].tobytes() == want[t]["records"].cpu().numpy().tobytes(), t
        assert f2f[2 * t:2 * t + 2].tobytes() == want[t]["f2f"].cpu().numpy().tobytes(), t
