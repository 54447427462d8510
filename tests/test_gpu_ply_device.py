"""GPU: the device route of the road PLYs (ply_gpu.hip through sd_ply_format_rw, Engine.format_rw_ply and SequenceOutputs(ply="device"))
against outputs.rw_ply_bytes, byte for byte.  The yardstick is that function (and the host statement sd_ply_format_rw_host, which
tests/test_ply_device_cpu.py holds to it) -- never the kernels against themselves.  The frames are those of tests/ply_device_cases.py."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import __graft_entry__ as graft
import ply_device_cases as P
from semantic_depth_amd import _lib as L
from semantic_depth_amd import outputs

pytestmark = pytest.mark.gpu

GROUPS = P.batches(P.good_cases())
GOOD = {c["name"]: c for c in P.good_cases()}
FLAGGED = {c["name"]: c for c in P.flagged_cases()}


@pytest.fixture(scope="module")
def eng():
    graft.build()
    from semantic_depth_amd.engine import Engine
    e = Engine(128, 256, 2, "resnet50")
    yield e
    e.close()


def _pack(cases, cap=None, n=None):
    """device tensors of one batch; rows behind a frame's n hold NaN / 0xA5 and must not be read"""
    B = len(cases)
    cap = max(len(c["xyz"]) for c in cases) if cap is None else cap
    xyz, rgb = np.full((B, cap, 3), np.nan, np.float32), np.full((B, cap, 3), 0xA5, np.uint8)
    cnt = np.array([len(c["xyz"]) for c in cases], np.int32)
    for i, c in enumerate(cases):
        xyz[i, :cnt[i]], rgb[i, :cnt[i]] = c["xyz"], c["rgb"]
    if n is not None:
        cnt = np.asarray(n, np.int32)
    rec = np.stack([np.frombuffer(c["rec"].tobytes(), np.uint8) for c in cases]).copy()
    final = dict(xyz=torch.from_numpy(xyz).cuda(), rgb=torch.from_numpy(rgb).cuda(), n=torch.from_numpy(cnt).cuda())
    return final, torch.from_numpy(rec).cuda()


def _files(text, offsets, flags):
    torch.cuda.synchronize()
    t, o, f = text.cpu().numpy(), offsets.cpu().numpy(), flags.cpu().numpy()
    assert text.dtype == torch.uint8 and offsets.dtype == torch.int64 and flags.dtype == torch.int32
    assert o[0] == 0 and (np.diff(o) >= 0).all() and o[-1] <= len(t)
    return [t[o[i]:o[i + 1]].tobytes() for i in range(len(f))], o, f


def _check(cases, files, flags, expect_flags=None):
    for i, c in enumerate(cases):
        if expect_flags is not None and expect_flags[i]:
            assert flags[i] == expect_flags[i] and files[i] == b"", (c["name"], flags[i], len(files[i]))
            continue
        assert flags[i] == 0, (c["name"], flags[i])
        diff = P.first_difference(files[i], P.want(c))
        assert diff is None, f"frame {i} ({c['name']}): {diff}"


@pytest.mark.parametrize("g", range(len(GROUPS)))
def test_text_is_the_bytes_of_rw_ply_bytes(eng, g):
    cases = GROUPS[g]
    final, rec = _pack(cases)
    out = torch.full((len(cases) * P.bound(final["xyz"].shape[1]) + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    text, offsets, flags = eng.format_rw_ply(final, rec, out=out)
    files, o, f = _files(text, offsets, flags)
    _check(cases, files, f)
    assert (out.cpu().numpy()[o[-1]:] == 0xA5).all()                 # nothing at or behind offsets[B] is written


def test_default_capacity_is_the_bound(eng):
    cases = [GOOD["seam_257"], GOOD["line_long_fractions"]]
    final, rec = _pack(cases)
    text, offsets, flags = eng.format_rw_ply(final, rec)
    assert text.numel() == 2 * P.bound(257)
    files, _, f = _files(text, offsets, flags)
    _check(cases, files, f)
    with pytest.raises(ValueError):
        eng.format_rw_ply(dict(final, rgb=None), rec)


@pytest.mark.parametrize("names,flags", [
    (["line_long_fractions", "nan_in_cloud", "inf_in_cloud", "seam_256"], [0, 1, 1, 0]),
    (["two_to_the_31", "rounding_2", "nan_end_point", "one_point_line"], [1, 0, 1, 0]),
    (["inf_end_point", "right_end_at_2_31", "last_255", "empty_line"], [1, 1, 0, 0])])
def test_frames_outside_the_range_are_flagged_and_the_others_still_pack(eng, names, flags):
    cases = [GOOD.get(nm) or FLAGGED[nm] for nm in names]
    final, rec = _pack(cases)
    files, o, f = _files(*eng.format_rw_ply(final, rec))
    _check(cases, files, f, flags)
    for i, c in enumerate(cases):                                    # the host statement gives the same verdicts
        assert P.host(c)[2] == flags[i]


def test_a_count_outside_the_cloud_is_flagged(eng):
    cases = [GOOD["last_256"], GOOD["seam_255"], GOOD["shared_minimum_line"], GOOD["one_point"]]
    final, rec = _pack(cases, cap=256, n=[256, 257, -1, 1])
    files, o, f = _files(*eng.format_rw_ply(final, rec))
    _check(cases, files, f, [0, 1, 1, 0])


def test_a_capacity_that_cuts_one_frame(eng):
    cases = [GOOD["line_mixed_signs"], GOOD["last_257"], GOOD["seam_512"], GOOD["one_point_line"]]
    want = [P.want(c) for c in cases]
    assert len(want[3]) < len(want[2])
    capacity = len(want[0]) + len(want[1]) + len(want[2]) - 1      # frames 0-1 fit, frame 2 is one byte too long, frame 3 fits behind frame 1
    final, rec = _pack(cases)
    out = torch.full((capacity + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
    text, offsets, flags = eng.format_rw_ply(final, rec, capacity=capacity, out=out)
    assert text.numel() == capacity
    files, o, f = _files(text, offsets, flags)
    _check(cases, files, f, [0, 0, 2, 0])
    assert list(o) == [0, len(want[0]), len(want[0]) + len(want[1]), len(want[0]) + len(want[1]), len(want[0]) + len(want[1]) + len(want[3])]
    assert (out.cpu().numpy()[o[-1]:] == 0xA5).all()
    final1, rec1 = _pack(cases[:1])                                   # no room at all: flag 2, nothing written
    out = torch.full((64,), 0xA5, dtype=torch.uint8, device="cuda")
    files, o, f = _files(*eng.format_rw_ply(final1, rec1, capacity=0, out=out))
    assert list(f) == [2] and list(o) == [0, 0] and (out.cpu().numpy() == 0xA5).all()


def _raw_call(eng, final, rec, ws_fill=0, ws_bytes=None, ws_shift=0, B=None, cap=None, null=None, stream=None):
    """sd_ply_format_rw on a workspace filled with ``ws_fill`` -> (status, text, offsets, flags) as numpy, all pre-filled"""
    rB, rcap = (int(v) for v in final["xyz"].shape[:2])
    need, bound = C.c_size_t(), C.c_size_t()
    assert eng.lib.sd_ply_format_workspace(rB, rcap, C.byref(need), C.byref(bound)) == L.SD_OK
    if isinstance(ws_fill, int):
        ws = torch.full((need.value + 16,), ws_fill, dtype=torch.uint8, device="cuda")
    else:
        ws = torch.from_numpy(np.random.default_rng(ws_fill[0]).integers(0, 256, need.value + 16, dtype=np.uint8)).cuda()
    text = torch.full((bound.value,), 0xA5, dtype=torch.uint8, device="cuda")
    offsets = torch.full((rB + 1,), -1, dtype=torch.int64, device="cuda")
    flags = torch.full((rB,), -1, dtype=torch.int32, device="cuda")
    ptrs = [final["xyz"].data_ptr(), final["rgb"].data_ptr(), final["n"].data_ptr(), rec.data_ptr(), text.data_ptr(), offsets.data_ptr(),
            flags.data_ptr(), ws.data_ptr() + ws_shift]
    if null is not None:
        ptrs[null] = None
    s = torch.cuda.current_stream() if stream is None else stream
    s.wait_stream(torch.cuda.current_stream())                       # (the fills above ran on the current stream)
    st = eng.lib.sd_ply_format_rw(eng.h, ptrs[0], ptrs[1], ptrs[2], rB if B is None else B, rcap if cap is None else cap, ptrs[3], ptrs[4],
                                  bound.value, ptrs[5], ptrs[6], ptrs[7], need.value if ws_bytes is None else ws_bytes, s.cuda_stream)
    torch.cuda.synchronize()
    return st, text.cpu().numpy(), offsets.cpu().numpy(), flags.cpu().numpy()


def test_the_result_does_not_depend_on_the_workspace_or_the_stream(eng):
    cases = [GOOD["rounding_0"], GOOD["seam_512"], FLAGGED["nan_in_cloud"], GOOD["empty_line"]]
    final, rec = _pack(cases)
    runs = [_raw_call(eng, final, rec, ws_fill=0x00), _raw_call(eng, final, rec, ws_fill=0xFF), _raw_call(eng, final, rec, ws_fill=(3,))]
    side = torch.cuda.Stream()
    runs.append(_raw_call(eng, final, rec, ws_fill=(4,), stream=side))
    st, text, o, f = runs[0]
    assert st == L.SD_OK and list(f) == [0, 0, 1, 0]
    _check(cases, [text[o[i]:o[i + 1]].tobytes() for i in range(4)], f, [0, 0, 1, 0])
    assert (text[o[-1]:] == 0xA5).all()
    for st2, text2, o2, f2 in runs[1:]:
        assert st2 == L.SD_OK and np.array_equal(o, o2) and np.array_equal(f, f2) and np.array_equal(text, text2)


def test_argument_refusals_launch_nothing(eng):
    final, rec = _pack([GOOD["seam_255"], GOOD["one_point"]])
    for kw in (dict(B=0), dict(B=-1), dict(cap=-1), dict(ws_bytes=64), dict(ws_shift=4), dict(null=0), dict(null=1), dict(null=2), dict(null=3),
               dict(null=4), dict(null=5), dict(null=6), dict(null=7)):
        st, text, o, f = _raw_call(eng, final, rec, **kw)
        assert st == L.SD_ERR_INVALID, kw
        assert (text == 0xA5).all() and (o == -1).all() and (f == -1).all(), kw


def test_run_sequence_files_device_route_writes_the_host_route_s_plys(tmp_path):
    """the driver on four synthetic frames, once per route: same records, same manifest apart from 'ply_fallback', same bytes in every file"""
    import test_gpu_sequence_outputs as S
    from semantic_depth_amd import weights as W
    from semantic_depth_amd.distributed import make_engine_step, run_sequence_files
    from semantic_depth_amd.engine import Engine, RoadWidthParams
    frames = S._smooth_frames(np.random.default_rng(23), 4, S.H, S.W_, cell=16)
    src = tmp_path / "in"
    src.mkdir()
    paths = [outputs.write_png(str(src / f"city_{i:03d}_leftImg8bit.png"), frames[i], level=1) for i in range(len(frames))]
    e = Engine(S.H, S.W_, 4, "resnet50", precision="bf16x3")
    try:
        e.load_weights(L.SD_NET_FCN8S, W.make_fcn8s_weights(1, decoder_std=0.05))
        wm = W.make_monodepth_weights("resnet50", 2)
        wm["dec/disp1/biases"] = (wm["dec/disp1/biases"] + np.float32(-1.5)).astype(np.float32)
        e.load_weights(L.SD_NET_MONODEPTH, wm)
        prm, names = RoadWidthParams(), outputs.sequence_names(paths)
        rec, man = {}, {}
        for route in ("host", "device"):
            outs = outputs.SequenceOutputs(str(tmp_path / route), names, depth=prm.depth, threads=4, images=False)
            rec[route] = run_sequence_files(paths, make_engine_step(e, lambda i: S.CAM, prm, outputs=outs, ply=route), batch=4, device="cuda").cpu()
            assert outs.ply_route == route
            man[route] = json.load(open(outs.manifest))
    finally:
        e.close()
    assert torch.equal(rec["host"], rec["device"])
    fallback = man["device"].pop("ply_fallback")
    assert "ply_fallback" not in man["host"] and man["host"] == man["device"] and man["device"]["status"] == "ok"
    assert len(man["host"]["files"]) == 2 * len(names) and set(fallback) <= set(names)
    for name in names:
        a, b = (open(str(tmp_path / r / outputs.SEQ_PLY_DIR / (name + "_rw.ply")), "rb").read() for r in ("host", "device"))
        print(f"{name}: {len(a)} B, fallback {name in fallback}")
        diff = P.first_difference(b, a)
        assert diff is None, f"{name}: {diff}"
