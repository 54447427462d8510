"""GPU: the depth profile on the device (Engine.road_width_profile / f2f_profile: rw_profile_partial_kernel + rw_profile_merge_kernel,
f2f_profile_kernel) against its host statement byte for byte on the crafted clouds of tests/depth_profile_cases.py -- which
tests/test_depth_profile_cpu.py holds to the oracle --, against the single-depth calls the tool has always had, and through
process_batch, the engine step and the sequence writer.

The clouds run on the 256 x 512 handle of the chain tests although one of them has more rows than that handle's cap and a batch more
frames than a 4-frame handle's max_batch: the call depends on neither.  The network-backed tests use the 128 x 128 vgg f32 engine of
the camera sweep test (the smallest geometry the monodepth plan accepts) with its synthetic weights."""
import ctypes as C
import functools
import glob
import json
import os
from dataclasses import asdict

import numpy as np
import pytest
import torch

import depth_profile_cases as dc
import pcl_chain_cases as cc
from gpu_common import Camera, RoadWidthParams, dev, engine
from oracle import pipeline
from semantic_depth_amd import _lib as L
from semantic_depth_amd import outputs
from semantic_depth_amd.distributed import make_engine_step
from semantic_depth_amd.engine import F2F_DTYPE, F2FP_DTYPE, RW_DTYPE, RWP_DTYPE, Engine, FenceParams

pytestmark = pytest.mark.gpu

PRM = RoadWidthParams(window=dc.WINDOW, depth_offset=dc.OFFSET)
SHARED = 44          # bytes an sd_rw_depth_result shares with the head of an sd_rw_result: width .. found


@pytest.fixture(scope="module")
def eng():
    return engine(256, 512, 8, "resnet50", load=())[0]


@pytest.fixture(scope="module")
def net_eng():
    return engine(128, 128, 4, "vgg", precision="f32")[0]


@pytest.fixture(scope="module", autouse=True)
def _release_own_engines():
    """the engines only this module asks gpu_common for are closed and dropped from its cache when the module is done (the 256 x 512
    handle stays: tests/test_gpu_pcl_chains.py asks for the same one), and the clouds go back to the device"""
    import gc

    import gpu_common
    before = set(gpu_common._cache)
    yield
    for key in set(gpu_common._cache) - before:
        if key[:3] != (256, 512, 8):
            gpu_common._cache.pop(key)[0].close()
    _cloud.cache_clear()
    gc.collect()
    torch.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def _cloud(name):
    bt = dc.batches()[name]
    return dev(bt.xyz), dev(bt.n)


@functools.lru_cache(maxsize=None)
def _host(name, lname):
    """the host statement's records of a batch, [B, D]; its buffers start at 0x5A where the device's start at 0xA5, so equal bytes also
    say that both sides wrote every byte"""
    bt = dc.batches()[name]
    return np.stack([dc.host_profile(bt.rows(b), dc.depth_lists()[lname], fill=0x5A) for b in range(len(bt.labels))])


def _profile(eng, xyz, n, depths):
    out = torch.full((xyz.shape[0], len(depths), RWP_DTYPE.itemsize), 0xA5, dtype=torch.uint8, device=xyz.device)
    assert eng.road_width_profile(xyz, n, depths, PRM, out=out) is out
    return out.cpu().numpy()


# ------------------------------------------------------------------------------------------ road profile
@pytest.mark.parametrize("name", sorted(dc.batches()))
def test_device_profile_equals_host_byte_for_byte(eng, name):
    bt = dc.batches()[name]
    xyz, n = _cloud(name)
    for lname in bt.lists:
        got = _profile(eng, xyz, n, dc.depth_lists()[lname])
        want = _host(name, lname)
        assert got.shape == (len(bt.labels), len(dc.depth_lists()[lname]), 48)
        for b, label in enumerate(bt.labels):
            rec = got[b].view(RWP_DTYPE).reshape(-1)
            bad = [i for i in range(len(rec)) if rec[i].tobytes() != want[b, i].tobytes()]
            assert not bad, (name, label, lname, bad[:4], rec[bad[0]], want[b, bad[0]])
        print(name, lname, "found", int(got.view(RWP_DTYPE)["found"].sum()), "of", got.shape[0] * got.shape[1])


@pytest.mark.parametrize("name", ["sizes", "edges"])
def test_device_profile_equals_the_single_cloud_call(eng, name):
    """sd_pcl_get_end_points_of_road (end_points_kernel, what sd_road_width's last step launches) per (frame, depth) of the nine-depth
    list: the fields the two records share, byte for byte"""
    bt = dc.batches()[name]
    xyz, n = _cloud(name)
    depths = dc.depth_lists()["nine"]
    got = _profile(eng, xyz, n, depths)
    B, D = len(bt.labels), len(depths)
    single = torch.full((B * D, RW_DTYPE.itemsize), 0xA5, dtype=torch.uint8, device=xyz.device)
    for b in range(B):
        rows = min(int(bt.n[b]), bt.cap)
        for i, d in enumerate(depths):
            st = eng.lib.sd_pcl_get_end_points_of_road(eng.h, C.c_void_p(xyz[b].data_ptr()), rows, float(d) - dc.OFFSET, dc.WINDOW,
                                                       C.c_void_p(single[b * D + i].data_ptr()), eng._stream())
            assert st == L.SD_OK
    single = single.cpu().numpy().reshape(B, D, -1)
    assert np.array_equal(got[:, :, :SHARED], single[:, :, :SHARED]), np.argwhere((got[:, :, :SHARED] != single[:, :, :SHARED]).any(-1))[:4]
    assert RWP_DTYPE.fields["found"][1] == RW_DTYPE.fields["found"][1] == SHARED - 4


def test_device_profile_does_not_depend_on_call_history(eng, net_eng):
    """the same batch twice, after a smaller batch, in reversed frame order, and on another handle: equal bytes per frame"""
    xyz, n = _cloud("edges")
    depths = dc.depth_lists()["nine"]
    first = _profile(eng, xyz, n, depths)
    again = _profile(eng, xyz, n, depths)
    small = _profile(eng, xyz[2:4].contiguous(), n[2:4].contiguous(), depths[:5])
    third = _profile(eng, xyz, n, depths)
    other = _profile(net_eng, xyz, n, depths)
    rev = _profile(eng, xyz.flip(0).contiguous(), n.flip(0).contiguous(), depths)
    assert first.tobytes() == again.tobytes() == third.tobytes() == other.tobytes() == rev[::-1].tobytes()
    assert small.tobytes() == first[2:4, :5].tobytes()
    # the reversed twin of the tie frame: the same extremes (other rows of the tie come first), the same counts
    e = dict(zip(dc.batches()["edges"].labels, range(6)))
    a, r = (first[e[k]].view(RWP_DTYPE).reshape(-1) for k in ("ties", "ties_reversed"))
    for k in ("found", "n_window", "x_left", "x_right", "width"):
        assert np.array_equal(a[k], r[k], equal_nan=True), k


# ------------------------------------------------------------------------------------------ fence profile
def _pack(frames, cap):
    xyz = np.full((len(frames), cap, 3), 777.0, np.float32)
    for b, fr in enumerate(frames):
        xyz[b, :len(fr.xyz)] = fr.xyz
    return dev(xyz), dev(np.int32([fr.n_passed for fr in frames]))


def test_f2f_profile_equals_host_and_the_chain_per_depth(eng):
    frames = cc.fence_main_frames()
    rx, rn = _pack(cc.fence_road_frames(len(frames)), eng.cap)
    rw = eng.road_width(rx, rn, RoadWidthParams(**asdict(cc.FENCE_ROAD_PARAMS)))
    fx, fn = _pack(frames, eng.cap)
    f2 = eng.fence_to_fence(fx, fn, rw, FenceParams())
    depths = dc.depth_lists()["nine"]
    out = torch.full((len(frames), len(depths), F2FP_DTYPE.itemsize), 0xA5, dtype=torch.uint8, device=fx.device)
    assert eng.f2f_profile(rw, f2, depths, out=out) is out
    got = Engine.f2f_profile_records(out)
    road_rec, f2f_rec = Engine.records(rw), Engine.f2f_records(f2)
    n_ok = 0
    for b, fr in enumerate(frames):
        want = dc.host_f2f_profile(road_rec[b], f2f_rec[b], depths)
        assert got[b].tobytes() == want.tobytes(), (fr.label, got[b], want)
        n_ok += int(got[b]["ok"].all())
    assert n_ok >= 4 and (got["ok"] == 0).any() and (got["reserved"] == 0).all()
    for i, d in enumerate(depths):
        chain = Engine.f2f_records(eng.fence_to_fence(fx, fn, rw, FenceParams(depth=float(d))))
        for k in ("dist", "left_pt", "right_pt"):
            assert np.array_equal(got[:, i][k], chain[k], equal_nan=True), (d, k, got[:, i][k], chain[k])
        assert np.array_equal(got[:, i]["ok"], chain["ok"]), d


# ------------------------------------------------------------------------------------------ process_batch, the step, the writer
def _frames(nf):
    return np.stack([pipeline.synthetic_scene(128, 128, seed=s, f=125.0)[3] for s in range(1, nf + 1)])


CAMS = [Camera(64.8, 59.8, 125.0, 1.0, 128.0), Camera(63.1, 61.4, 128.0, 1.0, 130.0), Camera(64.0, 60.0, 120.0, 1.0, 127.0)]
DEPTHS = [4.0, 10.0, 2.5, 6.0, 10.0, 3.0]


def _flat(out, prefix=""):
    for k, v in sorted(out.items()):
        if isinstance(v, dict):
            yield from _flat(v, prefix + k + ".")
        elif v is not None:
            yield prefix + k, v


def _valid_rows(out):
    """{flat key of a cloud tensor: its per-frame row counts}: the rows behind a cloud's count are never written"""
    cnt = Engine.f2f_records(out["f2f"])["counts"]
    fz, cap = out["fuse"], out["fuse"]["road_xyz"].shape[1]
    rows = {"fuse.road_": fz["n_road"].cpu().numpy().clip(0, cap), "fuse.fence_": fz["n_fence"].cpu().numpy().clip(0, cap),
            "road_final.": out["road_final"]["n"].cpu().numpy(), "fence_final.left_": cnt[:, 5], "fence_final.right_": cnt[:, 6]}
    return {p + k: v for p, v in rows.items() for k in ("xyz", "rgb")}


def _same_tensor(a, b, rows):
    if rows is None:
        return torch.equal(a, b)
    return all(torch.equal(a[i, :int(r)], b[i, :int(r)]) for i, r in enumerate(rows))


def test_process_batch_with_depths(net_eng):
    e = net_eng
    frames = dev(_frames(2))
    prm = RoadWidthParams()
    plain = e.process_batch(frames, CAMS[:2], prm, approach="both", want_final=True)
    out = e.process_batch(frames, CAMS[:2], prm, approach="both", want_final=True, depths=DEPTHS)
    assert set(out) == set(plain) | {"profile", "f2f_profile"} and "profile" not in plain
    rows = _valid_rows(plain)
    for (ka, a), (kb, b) in zip(_flat(plain), _flat({k: v for k, v in out.items() if k not in ("profile", "f2f_profile")})):
        assert ka == kb and _same_tensor(a, b, rows.get(ka)), ka
    fin = out["road_final"]
    assert torch.equal(out["profile"], e.road_width_profile(fin["xyz"], fin["n"], DEPTHS, prm))
    assert torch.equal(out["f2f_profile"], e.f2f_profile(out["records"], out["f2f"], DEPTHS))
    prof, rec = Engine.profile_records(out["profile"]), Engine.records(out["records"])
    fprof, frec = Engine.f2f_profile_records(out["f2f_profile"]), Engine.f2f_records(out["f2f"])
    assert prof.shape == (2, len(DEPTHS)) and fprof.shape == (2, len(DEPTHS))
    for i in (1, 4):                                     # DEPTHS[i] == prm.depth: the record's own fields
        assert DEPTHS[i] == prm.depth
        assert out["profile"][:, i, :SHARED].cpu().numpy().tobytes() == out["records"][:, :SHARED].cpu().numpy().tobytes()
        for k in ("dist", "left_pt", "right_pt"):
            assert np.array_equal(fprof[:, i][k], frec[k], equal_nan=True), k
        assert np.array_equal(fprof[:, i]["ok"], frec["ok"])
    print("found per depth", prof["found"].tolist(), "n_window", prof["n_window"].tolist(), "records found", rec["found"].tolist())
    # without want_final the clouds stay inside, the profile is the same
    lean = e.process_batch(frames, CAMS[:2], prm, approach="rw", depths=DEPTHS)
    assert "road_final" not in lean and "f2f_profile" not in lean and torch.equal(lean["profile"], out["profile"])


def test_frame_processor_profile(net_eng):
    from semantic_depth_amd import api
    e, wf, wm = engine(128, 128, 4, "vgg", precision="f32")
    seg = api.SegmentFrame((128, 128), wf, engine=e)
    dep = api.DepthFrame(encoder="vgg", input_height=128, input_width=128, checkpoint_path=wm, engine=e)
    frame = _frames(1)[0]
    plain = api.FrameProcessor(seg, dep, depth=10.0, approach="both").process_frame(frame)
    res = api.FrameProcessor(seg, dep, depth=10.0, approach="both", depths=DEPTHS).process_frame(frame)
    assert "profile" not in plain and plain["record"].tobytes() == res["record"].tobytes()
    rows = res["profile"]
    assert [r["depth"] for r in rows] == DEPTHS and all(set(r) == {"depth", "found", "width", "x_left", "x_right", "n_window", "dist_f2f"} for r in rows)
    for i in (1, 4):
        assert rows[i]["found"] == int(res["record"]["found"]) and rows[i]["dist_f2f"] == res["dist_f2f"]
        if rows[i]["found"]:
            assert rows[i]["width"] == res["dist_rw"] and rows[i]["n_window"] >= 1
    rw_only = api.FrameProcessor(seg, dep, depth=10.0, depths=DEPTHS[:2]).process_frame(frame)["profile"]
    assert len(rw_only) == 2 and "dist_f2f" not in rw_only[0]


def _tree(root):
    return {os.path.relpath(p, root): open(p, "rb").read() for p in glob.glob(os.path.join(root, "**", "*"), recursive=True) if os.path.isfile(p)}


def test_sequence_writer_profile_files(net_eng, tmp_path):
    e = net_eng
    frames = _frames(3)
    names = ["f000", "f001", "f002"]
    prm = RoadWidthParams()
    runs = {}
    for tag, depths in (("on", DEPTHS), ("off", None)):
        root = str(tmp_path / tag)
        outs = outputs.SequenceOutputs(root, names, depth=prm.depth, threads=2, profile=depths)
        step = make_engine_step(e, lambda i: CAMS[i], prm, approach="both", outputs=outs, depths=depths)
        rec = step(frames, 0)
        outs.close()
        runs[tag] = (_tree(root), rec.cpu().numpy())
    on, off = runs["on"][0], runs["off"][0]
    assert runs["on"][1].tobytes() == runs["off"][1].tobytes()
    prof_files = sorted(k for k in on if k.startswith(outputs.SEQ_PROFILE_DIR + os.sep))
    assert prof_files == [os.path.join(outputs.SEQ_PROFILE_DIR, nm + ".txt") for nm in names]
    assert not any(k.startswith(outputs.SEQ_PROFILE_DIR) for k in off) and not os.path.isdir(os.path.join(str(tmp_path / "off"), outputs.SEQ_PROFILE_DIR))
    rest = {k: v for k, v in on.items() if k not in prof_files and not k.startswith("manifest")}
    assert rest == {k: v for k, v in off.items() if not k.startswith("manifest")}
    m_on, m_off = (json.loads(t["manifest_rank0.json"]) for t in (on, off))
    assert m_on["profile_depths"] == DEPTHS and sorted(m_on["profile"]) == prof_files and "profile_depths" not in m_off and "profile" not in m_off
    assert m_on["status"] == m_off["status"] == "ok"
    out = e.process_batch(dev(frames), CAMS, prm, approach="both", depths=DEPTHS)
    prof, fprof = Engine.profile_records(out["profile"]), Engine.f2f_profile_records(out["f2f_profile"])
    for b, nm in enumerate(names):
        want = outputs.write_profile(str(tmp_path / "want.txt"), DEPTHS, prof[b], fprof[b])
        assert on[prof_files[b]] == open(want, "rb").read(), nm
    with pytest.raises(ValueError):
        make_engine_step(e, lambda i: CAMS[i], prm, outputs=outputs.SequenceOutputs(str(tmp_path / "x"), names, profile=[1.0]), depths=[2.0])


# ------------------------------------------------------------------------------------------ refusals
def test_device_calls_refuse_bad_arguments(eng):
    lib, h, s = eng.lib, eng.h, eng._stream()
    B, cap, D = 2, 64, 3
    xyz = torch.zeros((B, cap, 3), dtype=torch.float32, device=eng.device)
    n = torch.full((B,), cap, dtype=torch.int32, device=eng.device)
    need = lib.sd_rw_profile_workspace(B, cap, D)
    ws = torch.full((need + 32,), 0xA5, dtype=torch.uint8, device=eng.device)
    res = torch.full((B * D * 48 + 16,), 0xA5, dtype=torch.uint8, device=eng.device)
    good = np.array([3.0, 4.0, 5.0])
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)      # noqa: E731
    hp = lambda a: a.ctypes.data_as(C.c_void_p)               # noqa: E731
    base = dict(h=h, xyz=p(xyz), n=p(n), B=B, cap=cap, d=hp(good), D=D, w=0.05, off=0.02, res=p(res), ws=p(ws), wsb=need)

    def rw(**kw):
        a = {**base, **kw}
        return lib.sd_road_width_profile(a["h"], a["xyz"], a["n"], a["B"], a["cap"], a["d"], a["D"], a["w"], a["off"], a["res"], a["ws"], a["wsb"], s)
    assert ws.data_ptr() % 16 == 0 and res.data_ptr() % 8 == 0
    big = np.full(L.SD_PROFILE_MAX_DEPTHS + 1, 3.0)
    cases = [dict(h=None), dict(xyz=None), dict(n=None), dict(d=None), dict(res=None), dict(ws=None), dict(B=0), dict(B=65536), dict(cap=0),
             dict(D=0), dict(d=hp(big), D=len(big)), dict(d=hp(np.array([3.0, np.nan, 4.0]))), dict(d=hp(np.array([3.0, 4.0, np.inf]))),
             dict(w=0.0), dict(w=-0.05), dict(w=float("nan")), dict(w=float("inf")), dict(off=float("nan")), dict(off=float("-inf")),
             dict(wsb=need - 1), dict(ws=p(ws, 8)), dict(xyz=p(xyz, 2)), dict(n=p(n, 2)), dict(res=p(res, 4))]
    for bad in cases:
        assert rw(**bad) == L.SD_ERR_INVALID, bad
    road = torch.zeros((B, RW_DTYPE.itemsize), dtype=torch.uint8, device=eng.device)
    f2f = torch.zeros((B, F2F_DTYPE.itemsize), dtype=torch.uint8, device=eng.device)
    fres = torch.full((B * D * 64 + 16,), 0xA5, dtype=torch.uint8, device=eng.device)
    fbase = dict(h=h, road=p(road), f2f=p(f2f), B=B, d=hp(good), D=D, res=p(fres))

    def ff(**kw):
        a = {**fbase, **kw}
        return lib.sd_f2f_profile(a["h"], a["road"], a["f2f"], a["B"], a["d"], a["D"], a["res"], s)
    for bad in (dict(h=None), dict(road=None), dict(f2f=None), dict(d=None), dict(res=None), dict(B=0), dict(B=65536), dict(D=0),
                dict(d=hp(big), D=len(big)), dict(d=hp(np.array([3.0, np.nan, 4.0]))), dict(res=p(fres, 4))):
        assert ff(**bad) == L.SD_ERR_INVALID, bad
    torch.cuda.synchronize()
    assert bool((res == 0xA5).all()) and bool((fres == 0xA5).all()) and bool((ws == 0xA5).all())        # nothing was launched
    assert rw() == L.SD_OK and ff() == L.SD_OK
    torch.cuda.synchronize()
    assert bool((res[:B * D * 48] != 0xA5).any()) and bool((res[B * D * 48:] == 0xA5).all()) and bool((fres[B * D * 64:] == 0xA5).all())
    with pytest.raises(ValueError):
        eng.road_width_profile(xyz, n, [])
    with pytest.raises(ValueError):
        eng.road_width_profile(xyz, n, [3.0] * 257)
    with pytest.raises(L.SdError):
        eng.road_width_profile(xyz, n, [3.0, float("nan")])
