"""GPU: the scene PLY route.  Chain level: the boxes of sd_road_width_boxes / sd_fence_to_fence_boxes against np.amin / np.amax of the
oracle chain's entering clouds, every other output bit-equal to the calls without boxes.  Formatter: sd_scene_format (scene_gpu.hip)
against sd_scene_format_host byte for byte, workspace and text buffer pre-filled with garbage.  Sequence level: the files of
Scene(route="device") equal those of route="host", and scene=None changes nothing.  (The CPU half is tests/test_scene_cpu.py.)"""
import ctypes as C
import json
import os
import warnings
from dataclasses import asdict

import numpy as np
import pytest
import torch

import __graft_entry__ as graft
import pcl_chain_cases as cc
import ply_device_cases as P
import scene_cases as S
from oracle import pcl as oracle_pcl
from semantic_depth_amd import _lib as L
from semantic_depth_amd import outputs
from semantic_depth_amd.engine import BOX_DTYPE, F2F_DTYPE, RW_DTYPE, FenceParams, RoadWidthParams

pytestmark = pytest.mark.gpu

B, CAP, LATTICE_CAP = 3, 1024, 4096


@pytest.fixture(scope="module")
def eng():
    graft.build()
    from semantic_depth_amd.engine import Engine
    e = Engine(128, 256, B, "resnet50")
    yield e
    e.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------ chain level
def _pack_chain(frames):
    """the first CAP rows of every crafted frame; the count handed over stays the frame's own (the kernels clamp it to CAP)"""
    xyz, rgb = np.full((len(frames), CAP, 3), 777.0, np.float32), np.full((len(frames), CAP, 3), 201, np.uint8)
    for b, fr in enumerate(frames):
        k = min(len(fr.xyz), CAP)
        xyz[b, :k], rgb[b, :k] = fr.xyz[:k], fr.rgb[:k]
    return dev(xyz), dev(rgb), dev(np.int32([fr.n_passed for fr in frames]))


def _want_box(pts, ia, ib):
    b = np.zeros((), BOX_DTYPE)
    if len(pts):
        b["lo_a"], b["hi_a"], b["lo_b"], b["hi_b"] = np.amin(pts[:, ia]), np.amax(pts[:, ia]), np.amin(pts[:, ib]), np.amax(pts[:, ib])
    b["n"] = len(pts)
    return b


def _mad(pts, col, axis, thr):
    if not len(pts):
        return pts, col
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return oracle_pcl.remove_noise_by_mad(pts, col, axis, thr)[:2]


def _road_frames():
    cases = cc.road_cases()
    pick = {("mixed", "hit16384_nanx"), ("mixed", "zcut0"), ("sloped", "small2500")}
    frames = [fr for name, label in sorted(pick) for fr in cases[name].frames if fr.label == label]
    assert len(frames) == B
    return frames, cases["mixed"].params


def test_road_boxes_and_unchanged_outputs(eng):
    frames, p = _road_frames()
    xyz, rgb, n = _pack_chain(frames)
    prm = RoadWidthParams(**asdict(p))
    plain = eng.road_width(xyz, n, prm, want_final=True, road_rgb=rgb)
    boxes = torch.full((B, 24), 0xA5, dtype=torch.uint8, device="cuda")
    withb = eng.road_width(xyz, n, prm, want_final=True, road_rgb=rgb, boxes=boxes)
    torch.cuda.synchronize()
    assert torch.equal(plain[0], withb[0]) and torch.equal(plain[3], withb[3])      # records and counts: the same bytes
    for b, m in enumerate(plain[3].cpu().numpy()):                    # final cloud and colours (rows behind the count are scratch of the chain)
        assert plain[1][b, :m].cpu().numpy().tobytes() == withb[1][b, :m].cpu().numpy().tobytes() and torch.equal(plain[2][b, :m], withb[2][b, :m])
    got = boxes.cpu().numpy().view(BOX_DTYPE).reshape(-1)
    some = 0
    for b, fr in enumerate(frames):
        pts, col = fr.xyz[:CAP], fr.rgb[:CAP]
        keep = pts[:, 2] < -p.z_cut
        pts, col = pts[keep], col[keep]
        pts, col = _mad(pts, col, 1, p.mad_y)
        pts, col = _mad(pts, col, 0, p.mad_x)
        want = _want_box(pts, 0, 2)
        assert got[b].tobytes() == want.tobytes(), (fr.label, got[b], want)
        assert int(eng.records(withb[0])[b]["n_mad_x"]) == int(want["n"])
        some += int(want["n"]) > 0
    assert some >= 2 and any(int(g["n"]) == 0 for g in got)           # full boxes and an empty one (its four floats are 0)


def test_fence_boxes_and_unchanged_outputs(eng):
    cases = cc.fence_cases()
    frames = [cases["keep_all"].frames[1], cases["main"].frames[5], cases["main"].frames[6]]     # plain3000, no_fence, right_const
    p = cases["main"].params
    roads = cc.fence_road_frames(B)
    rx, _, rn = _pack_chain(roads)
    rw = eng.road_width(rx, rn, RoadWidthParams(**asdict(cc.FENCE_ROAD_PARAMS)))
    xyz, rgb, n = _pack_chain(frames)
    fp = FenceParams(**asdict(p))
    res0, cl0 = eng.fence_to_fence(xyz, n, rw, fp, fence_rgb=rgb, want_clouds=True)
    boxes = torch.full((B, 2, 24), 0xA5, dtype=torch.uint8, device="cuda")
    res1, cl1 = eng.fence_to_fence(xyz, n, rw, fp, fence_rgb=rgb, want_clouds=True, boxes=boxes)
    torch.cuda.synchronize()
    assert res0.cpu().numpy().tobytes() == res1.cpu().numpy().tobytes()
    rec = eng.f2f_records(res1)
    for k, j in (("left_xyz", 5), ("left_rgb", 5), ("right_xyz", 6), ("right_rgb", 6)):
        for b in range(B):                                           # (rows behind a side's count are scratch of the chain)
            m = int(rec[b]["counts"][j])
            assert torch.equal(cl0[k][b, :m], cl1[k][b, :m]), (k, b)
    got = boxes.cpu().numpy().view(BOX_DTYPE).reshape(B, 2)
    some = 0
    for b, fr in enumerate(frames):
        pts, col = fr.xyz[:CAP], fr.rgb[:CAP]
        pts, col = _mad(pts, col, 1, p.mad_y)
        sides = (pts[:0], pts[:0])
        if len(pts):
            pts, col = oracle_pcl.threshold_complete(pts, col, 2, p.z_max)
        if len(pts):
            l, lc, r, rc = oracle_pcl.extract_pcls(pts, col)
            sides = (_mad(l, lc, 0, p.mad_left)[0], _mad(r, rc, 0, p.mad_right)[0])
        for s in range(2):
            want = _want_box(sides[s], 1, 2)
            assert got[b, s].tobytes() == want.tobytes(), (fr.label, s, got[b, s], want)
            some += int(want["n"]) > 0
    assert some >= 3


# ------------------------------------------------------------------------------------------------ formatter
_frames = S.gpu_frames


def _lattice_rows(f, k):
    box, plane, axis = ((f["road_box"], f["record"]["plane"], 1), (f["fence_boxes"][0], f["f2f"]["plane_left"], 0),
                        (f["fence_boxes"][1], f["f2f"]["plane_right"], 0))[k]
    na, nb = C.c_uint32(), C.c_uint32()
    pl = np.ascontiguousarray(plane, np.float64)
    assert L.load().sd_scene_lattice_host(np.ascontiguousarray(box).ctypes.data_as(C.c_void_p), pl.ctypes.data_as(C.c_void_p), axis, C.byref(na),
                                          C.byref(nb), None, 0) == L.SD_OK
    return na.value, nb.value


def _device(eng, frames, mask, fence=True, capacity=None):
    """sd_scene_format on the batch, called through the C ABI with a workspace and a text buffer full of garbage"""
    n = len(frames)
    cnt = np.int32([len(f["road_xyz"]) for f in frames])
    rng = np.random.default_rng(77)
    road_xyz, road_rgb = np.full((n, CAP, 3), np.nan, np.float32), np.full((n, CAP, 3), 0xA5, np.uint8)
    fx = {k: (np.full((n, CAP, 3), np.nan, np.float32) if k.endswith("xyz") else np.full((n, CAP, 3), 0xA5, np.uint8))
          for k in ("left_xyz", "left_rgb", "right_xyz", "right_rgb")}
    for i, f in enumerate(frames):
        road_xyz[i, :cnt[i]], road_rgb[i, :cnt[i]] = f["road_xyz"], f["road_rgb"]
        for k in fx:
            fx[k][i, :len(f["fence"][k])] = f["fence"][k]
    rec = dev(np.stack([np.frombuffer(f["record"].tobytes(), np.uint8) for f in frames]))
    f2f = dev(np.stack([np.frombuffer(f["f2f"].tobytes(), np.uint8) for f in frames]))
    rbox = dev(np.stack([np.frombuffer(f["road_box"].tobytes(), np.uint8) for f in frames]))
    fbox = dev(np.stack([np.frombuffer(f["fence_boxes"].tobytes(), np.uint8) for f in frames]))
    final = dict(xyz=dev(road_xyz), rgb=dev(road_rgb), n=dev(cnt))
    fd = {k: dev(v) for k, v in fx.items()} if fence else {k: None for k in fx}
    need, bound = C.c_size_t(), C.c_size_t()
    assert eng.lib.sd_scene_workspace(n, CAP, CAP if fence else 0, LATTICE_CAP, mask, C.byref(need), C.byref(bound)) == L.SD_OK
    capacity = bound.value if capacity is None else capacity
    text = dev(rng.integers(0, 256, max(capacity, 1) + 64, dtype=np.uint8))
    before = text.cpu().numpy().copy()
    ws = dev(rng.integers(0, 256, need.value, dtype=np.uint8))
    offsets = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    flags = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    st = eng.lib.sd_scene_format(eng.h, ptr(final["xyz"]), ptr(final["rgb"]), ptr(final["n"]), CAP, ptr(fd["left_xyz"]), ptr(fd["left_rgb"]),
                                 ptr(fd["right_xyz"]), ptr(fd["right_rgb"]), CAP if fence else 0, n, ptr(rec), ptr(f2f) if fence else None,
                                 ptr(rbox), ptr(fbox) if fence else None, mask, LATTICE_CAP, ptr(text), capacity, ptr(offsets), ptr(flags), ptr(ws),
                                 need.value, eng._stream())
    L.check(eng.lib, eng.h, st, "sd_scene_format")
    torch.cuda.synchronize()
    t, o, fl = text.cpu().numpy(), offsets.cpu().numpy(), flags.cpu().numpy()
    assert o[0] == 0 and (np.diff(o) >= 0).all() and o[-1] <= capacity
    assert np.array_equal(t[o[-1]:], before[o[-1]:])                  # nothing at or behind offsets[B] is written
    return [t[o[i]:o[i + 1]].tobytes() for i in range(n)], fl


def _host(f, mask, fence=True):
    return outputs.scene_format_host(mask=mask, lattice_cap=LATTICE_CAP, **S.args(f, fence))


@pytest.mark.parametrize("middle", (False, True))
@pytest.mark.parametrize("variant", ("flag1", "flag3", "flag2"))
def test_formatter_equals_the_host_statement(eng, variant, middle):
    f0, f1, f2 = _frames(variant)
    assert _lattice_rows(f0, 0) == (16, 32) and _lattice_rows(f1, 0)[0] == 1
    if variant == "flag3":
        assert _lattice_rows(f2, 2) == (17, 241)
    frames = [f0, f2, f1] if middle else [f0, f1, f2]
    flagged = 1 if middle else 2
    for key, mask in S.FILE_MASKS.items():
        want = [_host(f, mask) for f in frames]
        capacity = None
        if variant == "flag2":                                        # one byte short for the flagged frame; the (shorter) frame behind it still packs
            assert want[flagged][1] == 0 and all(len(w[0]) < len(want[flagged][0]) for w in want[flagged + 1:])
            capacity = sum(len(w[0]) for w in want[:flagged]) + len(want[flagged][0]) - 1
            want[flagged] = (b"", 2)
        elif key != "road" and not (variant == "flag3" and key == "fence"):
            assert want[flagged] == (b"", int(variant[-1])), (key, want[flagged][1])
        files, flags = _device(eng, frames, mask, capacity=capacity)
        for i, (data, flag) in enumerate(want):
            assert flags[i] == flag, (key, i, flags, flag)
            diff = P.first_difference(files[i], data)
            assert diff is None, f"{key} frame {i}: {diff}"


def test_formatter_with_null_fence_inputs(eng):
    frames = list(_frames("plain"))
    for key, mask in S.FILE_MASKS.items():
        files, flags = _device(eng, frames, mask, fence=False)
        for i, f in enumerate(frames):
            data, flag = _host(f, mask, fence=False)
            assert flags[i] == flag == 0 and P.first_difference(files[i], data) is None, (key, i, P.first_difference(files[i], data))


def test_engine_method_and_refusals(eng):
    """Engine.format_scene_ply is the call above; an invalid call launches nothing"""
    frames = list(_frames("plain"))
    n = len(frames)
    cnt = np.int32([len(f["road_xyz"]) for f in frames])
    xyz, rgb = np.zeros((n, CAP, 3), np.float32), np.zeros((n, CAP, 3), np.uint8)
    side = {k: np.zeros((n, CAP, 3), np.float32 if k.endswith("xyz") else np.uint8) for k in ("left_xyz", "left_rgb", "right_xyz", "right_rgb")}
    for i, f in enumerate(frames):
        xyz[i, :cnt[i]], rgb[i, :cnt[i]] = f["road_xyz"], f["road_rgb"]
        for k in side:
            side[k][i, :len(f["fence"][k])] = f["fence"][k]
    rec = dev(np.stack([np.frombuffer(f["record"].tobytes(), np.uint8) for f in frames]))
    f2f = dev(np.stack([np.frombuffer(f["f2f"].tobytes(), np.uint8) for f in frames]))
    boxes = dict(road=dev(np.stack([np.frombuffer(f["road_box"].tobytes(), np.uint8) for f in frames])),
                 fence=dev(np.stack([np.frombuffer(f["fence_boxes"].tobytes(), np.uint8) for f in frames]).reshape(n, 2, 24)))
    final = dict(xyz=dev(xyz), rgb=dev(rgb), n=dev(cnt))
    text, offsets, flags = eng.format_scene_ply(final, {k: dev(v) for k, v in side.items()}, rec, f2f, boxes, lattice_cap=LATTICE_CAP)
    torch.cuda.synchronize()
    o, t = offsets.cpu().numpy(), text.cpu().numpy()
    assert (flags.cpu().numpy() == 0).all()
    for i, f in enumerate(frames):
        assert P.first_difference(t[o[i]:o[i + 1]].tobytes(), _host(f, S.ALL)[0]) is None
    with pytest.raises(L.SdError):
        eng.format_scene_ply(final, None, rec, None, boxes, mask=256)
    assert eng.lib.sd_scene_workspace(0, CAP, CAP, LATTICE_CAP, S.ALL, None, None) != L.SD_OK
    assert eng.lib.sd_scene_workspace(1, 1 << 30, 1 << 30, 1 << 28, S.ALL, None, None) != L.SD_OK
    assert eng.lib.sd_scene_workspace(1, CAP, CAP, LATTICE_CAP, 256, None, None) != L.SD_OK
    # the grid, the workspace and the text bound follow the mask: the _ROAD and _FENCE files carry no lattice and no line
    bounds = {}
    for key, mask in S.FILE_MASKS.items():
        need, bound = C.c_size_t(), C.c_size_t()
        assert eng.lib.sd_scene_workspace(B, CAP, CAP, LATTICE_CAP, mask, C.byref(need), C.byref(bound)) == L.SD_OK
        bounds[key] = (need.value, bound.value)
    assert bounds["scene"][1] == B * (209 + (2 * CAP + 3 * LATTICE_CAP + 2002) * 69)
    assert bounds["road"][1] == bounds["fence"][1] == B * (209 + CAP * 69) and bounds["road"][0] < bounds["scene"][0] // 4


# ------------------------------------------------------------------------------------------------ sequence level
def test_sequence_routes_agree_and_none_changes_nothing(tmp_path):
    """make_engine_step on three 64 x 128 frames, approach 'both': the files of Scene(route="device") are those of route="host"; without
    scene= the run writes the same manifest and the same bytes in every other file, and no scene key.  The monodepth bias is calibrated
    (as bench.py does) so that the median depth is the measuring depth: the frames have road points, so the road cloud, the road plane
    lattice and the road box travel on both routes, and the scene file holds more than the _ROAD and _FENCE files together"""
    import test_gpu_sequence_outputs as SO
    from semantic_depth_amd import weights as W
    from semantic_depth_amd.distributed import make_engine_step, run_sequence_files
    from semantic_depth_amd.engine import Camera, Engine
    frames = SO._smooth_frames(np.random.default_rng(31), B, 64, 128, cell=8)
    src = tmp_path / "in"
    src.mkdir()
    paths = [outputs.write_png(str(src / f"city_{i:03d}_leftImg8bit.png"), frames[i], level=1) for i in range(B)]
    cam = Camera(1048.64 / 8, 519.277 / 8, 250.0, 1.0, 3800.0)
    e = Engine(128, 256, B, "resnet50", precision="bf16x3")
    try:
        e.load_weights(L.SD_NET_FCN8S, W.make_fcn8s_weights(1, decoder_std=0.05))
        wm = W.make_monodepth_weights("resnet50", 2)
        e.load_weights(L.SD_NET_MONODEPTH, wm)
        prm, names = RoadWidthParams(z_cut=2.0, use_o3d=False), outputs.sequence_names(paths)
        d0 = float(e.monodepth_forward(e.resize_cubic(torch.from_numpy(frames).cuda())).median().item())
        logit = lambda p: float(np.log(p / (1.0 - p)))
        target = cam.f * cam.b / prm.depth / cam.disp_mult
        bias = round((logit(target / 0.3) - logit(min(max(d0, 1e-4), 0.2999) / 0.3)) * 64.0) / 64.0
        e.load_weights(L.SD_NET_MONODEPTH, {"dec/disp1/biases": (wm["dec/disp1/biases"] + np.float32(bias)).astype(np.float32)})
        rec, man = {}, {}
        for route in ("none", "host", "device"):
            outs = outputs.SequenceOutputs(str(tmp_path / route), names, depth=prm.depth, threads=4)
            scene = None if route == "none" else outputs.Scene(route=route, lattice_cap=1 << 16, capacity_per_frame=4 << 20)
            step = make_engine_step(e, lambda i: cam, prm, approach="both", outputs=outs, scene=scene)
            rec[route] = run_sequence_files(paths, step, batch=B, device="cuda").cpu()
            man[route] = json.load(open(outs.manifest))
    finally:
        e.close()
    assert torch.equal(rec["none"], rec["host"]) and torch.equal(rec["none"], rec["device"])
    assert "scene" not in man["none"] and "scene_fallback" not in man["none"]
    want = sorted(os.path.join(outputs.SEQ_PLY_DIR, nm + sfx) for nm in names for sfx, _ in outputs.SCENE_FILES.values())
    for route in ("host", "device"):
        m = dict(man[route])
        assert m.pop("scene") == want and m["status"] == "ok"
        fallback = m.pop("scene_fallback")
        assert fallback == [] if route == "host" else set(fallback) <= set(names)
        m["files"] = [f for f in m["files"] if f not in want]
        assert m == man["none"]                                       # scene= adds its keys and its files, nothing else
        for f in man["none"]["files"]:
            assert open(tmp_path / "none" / f, "rb").read() == open(tmp_path / route / f, "rb").read(), f
    for f in want:
        a, b = (open(tmp_path / r / f, "rb").read() for r in ("host", "device"))
        diff = P.first_difference(b, a)
        assert diff is None, f"{f}: {diff}"
        assert a.startswith(b"ply\n")

    def vertices(nm, sfx):
        data = open(tmp_path / "device" / outputs.SEQ_PLY_DIR / (nm + sfx), "rb").read()
        return int(data.split(b"element vertex ")[1].split(b"\n")[0])

    counts = {nm: tuple(vertices(nm, outputs.SCENE_FILES[k][0]) for k in ("scene", "road", "fence")) for nm in names}
    n_final = rec["none"].numpy().view(RW_DTYPE).reshape(-1)["n_ror"]
    # road points reached the files, and the scene holds segments the other two files lack (the lattices, the lines)
    assert (n_final > 1).any() and all(c[1] <= max(int(n) - 1, 0) for c, n in zip(counts.values(), n_final)), (counts, n_final)
    assert any(c[1] > 0 and c[0] > c[1] + c[2] + 1 for c in counts.values()), counts
