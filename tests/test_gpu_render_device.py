"""GPU: the device route of the rendered clouds (render_gpu.hip through sd_render_rw, Engine.render_rw and make_engine_step(render=))
against its host statement, sd_render_rw_host, on every byte.  The yardstick is that statement -- tests/test_render_cpu.py holds it to an
independent numpy statement of the rule -- never the kernels against themselves.  The frames are those of tests/render_cases.py."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import __graft_entry__ as graft
import render_cases as R
from semantic_depth_amd import _lib as L
from semantic_depth_amd import frame_io, outputs
from semantic_depth_amd.engine import RW_DTYPE

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    graft.build()
    from semantic_depth_amd.engine import Engine
    e = Engine(128, 256, 2, "resnet50")
    yield e
    e.close()


def _pack(cases, cap, counts=None, seed=0):
    """the cases as one batch of capacity ``cap``: (final dict of host arrays, records u8 [B,104]); the rows behind a frame's count hold
    values that would show if they were read (NaN, huge and ordinary points, colours of the line)"""
    B = len(cases)
    rng = np.random.default_rng(seed)
    xyz = (rng.random((B, cap, 3)) * [12.0, 0.4, 30.0] + [-6.0, 0.2, 5.0]).astype(np.float32)
    xyz[:, ::3, 0] = np.nan
    xyz[:, 1::7, 2] = -1e30
    rgb = np.full((B, cap, 3), [250, 0, 0], np.uint8)
    n = np.zeros(B, np.int32)
    for b, c in enumerate(cases):
        k = len(c["xyz"])
        assert k <= cap
        xyz[b, :k], rgb[b, :k], n[b] = c["xyz"], c["rgb"], k
    if counts is not None:
        n[:] = counts
    recs = np.array([c["rec"] for c in cases], RW_DTYPE)
    return dict(xyz=xyz, rgb=rgb, n=n), recs.view(np.uint8).reshape(B, RW_DTYPE.itemsize).copy()


def _dev(final, recs):
    return {k: torch.from_numpy(v).cuda() for k, v in final.items()}, torch.from_numpy(recs).cuda()


def _want(cases):
    out = []
    for c in cases:
        st, img, flag = R.host(c)
        assert st == L.SD_OK and flag == 0
        out.append(img)
    return np.stack(out)


def _frames(B, cap, cam, counts, seed):
    cases = []
    for b in range(B):
        p = R.cloud(seed + b, counts[b])
        if counts[b] > 20:                                               # rows the rule skips, a shared minimum and a tie in depth
            p[3, 1], p[4, 0], p[5, 2], p[6] = np.nan, np.inf, -np.inf, [0.0, 1e30, 20.0]
            p[[7, 8, 9], 2] = p[np.isfinite(p).all(1), 2].min()
            p[11] = p[10]
        cases.append(R.case(f"frame_{b}", p, cam, rec=R.LINE if b % 2 == 0 else None, seed=seed + b))
    return cases


SHAPES = [(3, 64, 96, 300, [0, 300, 150]), (2, 37, 53, 1000, [1000, 333]), (5, 128, 128, 2048, [2048, 0, 1, 1000, 257])]


@pytest.mark.parametrize("B,h,w,cap,counts", SHAPES)
@pytest.mark.parametrize("view", ["slanted", "top"])
def test_render_rw_equals_the_host_statement(eng, B, h, w, cap, counts, view):
    cam = R.slanted_camera(w, h, point_size=4) if view == "slanted" else R.top(w, h)
    cases = _frames(B, cap, cam, counts, seed=h + w)
    final, recs = _dev(*_pack(cases, cap, seed=cap))
    images, flags = eng.render_rw(final, recs, cam)
    assert tuple(images.shape) == (B, h, w, 3) and images.dtype == torch.uint8
    got, want = images.cpu().numpy(), _want(cases)
    assert flags.cpu().tolist() == [0] * B
    for b in range(B):
        assert np.array_equal(got[b], want[b]), (b, counts[b], int((got[b] != want[b]).any(-1).sum()))
    assert any((want[b] != 255).any() for b in range(B))
    assert (B * h * w) % 4 == (2 if (h, w) == (37, 53) else 0)           # the odd shape ends in a partial group of four pixels


def test_the_shared_cases_equal_the_host_statement(eng):
    """every case of tests/render_cases.py, batched by camera: point sizes, ties, depth order, the near plane, the borders and corners,
    non-finite rows, shared minima, the line in front of and behind the cloud"""
    groups = {}
    for c in R.all_cases():
        groups.setdefault(c["cam"], []).append(c)
    assert len(groups) >= 12
    for k, (cam, cases) in enumerate(groups.items()):
        cap = max(len(c["xyz"]) for c in cases) + 5
        final, recs = _dev(*_pack(cases, cap, seed=k))
        images, flags = eng.render_rw(final, recs, cam)
        got, want = images.cpu().numpy(), _want(cases)
        assert not flags.cpu().any()
        for b, c in enumerate(cases):
            assert np.array_equal(got[b], want[b]), (c["name"], int((got[b] != want[b]).any(-1).sum()))


def test_a_count_outside_the_cloud_flags_the_frame(eng):
    cam = R.top(53, 37, background=(7, 8, 9))
    cases = _frames(4, 300, cam, [300, 300, 300, 120], seed=5)
    final, recs = _dev(*_pack(cases, 300, counts=[-1, 301, 2 ** 31 - 1, 120]))
    images, flags = eng.render_rw(final, recs, cam)
    got = images.cpu().numpy()
    assert flags.cpu().tolist() == [1, 1, 1, 0]
    assert (got[:3] == [7, 8, 9]).all()
    st, img, flag = R.host(cases[0], n=-1)
    assert st == L.SD_OK and flag == 1 and np.array_equal(img, got[0])
    assert np.array_equal(got[3], _want(cases[3:])[0]) and (got[3] != [7, 8, 9]).any()


def _raw_call(eng, cases, cap, cam, fill=0, ws_bytes=None, B=None, cap_arg=None, cam_struct=None, ws_shift=0, rec_shift=0, null=None):
    final, recs = _pack(cases, cap)
    fin, _ = _dev(final, recs)
    rbuf = torch.zeros((recs.size + 8,), dtype=torch.uint8, device="cuda")
    rbuf[rec_shift:rec_shift + recs.size] = torch.from_numpy(recs.reshape(-1)).cuda()
    cs = cam.struct() if cam_struct is None else cam_struct
    need = C.c_size_t()
    assert eng.lib.sd_render_workspace(len(cases), cap, C.byref(cam.struct()), C.byref(need)) == L.SD_OK
    dst = torch.full((len(cases), cam.height, cam.width, 3), 0x5A, dtype=torch.uint8, device="cuda")
    flags = torch.full((len(cases),), -7, dtype=torch.int32, device="cuda")
    ws = torch.full((need.value + 16,), fill, dtype=torch.uint8, device="cuda")
    ptr = dict(xyz=fin["xyz"].data_ptr(), rgb=fin["rgb"].data_ptr(), n=fin["n"].data_ptr(), rec=rbuf.data_ptr() + rec_shift, cam=C.byref(cs),
               dst=dst.data_ptr(), flags=flags.data_ptr(), ws=ws.data_ptr() + ws_shift)
    if null:
        ptr[null] = None
    st = eng.lib.sd_render_rw(eng.h, ptr["xyz"], ptr["rgb"], ptr["n"], len(cases) if B is None else B, cap if cap_arg is None else cap_arg, ptr["rec"],
                              ptr["cam"], ptr["dst"], ptr["flags"], ptr["ws"], need.value if ws_bytes is None else ws_bytes,
                              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return st, dst.cpu().numpy(), flags.cpu().numpy(), ws.cpu().numpy(), need.value


def test_result_does_not_depend_on_the_workspace(eng):
    cam = R.slanted_camera(53, 37)
    cases = _frames(3, 400, cam, [400, 0, 77], seed=9)
    st0, a, fa, _, _ = _raw_call(eng, cases, 400, cam, fill=0x00)
    st1, b, fb, _, _ = _raw_call(eng, cases, 400, cam, fill=0xFF)
    assert st0 == st1 == L.SD_OK
    assert np.array_equal(a, b) and np.array_equal(fa, fb) and np.array_equal(a, _want(cases)) and (a != 255).any()


def test_argument_refusals_launch_nothing(eng):
    cam = R.top(40, 24)
    cases = _frames(2, 100, cam, [100, 50], seed=3)
    bad_w, bad_z, bad_s, bad_e = cam.struct(), cam.struct(), cam.struct(), cam.struct()
    bad_w.width, bad_z.z_near, bad_s.point_size = 16385, float("nan"), 17
    bad_e.ext[7] = float("inf")
    need = _raw_call(eng, cases, 100, cam)[4]
    refusals = [dict(ws_bytes=need - 1), dict(B=0), dict(B=65536), dict(cap_arg=-1), dict(cam_struct=bad_w), dict(cam_struct=bad_z), dict(cam_struct=bad_s),
                dict(cam_struct=bad_e), dict(ws_shift=8), dict(rec_shift=4)] + [dict(null=k) for k in ("xyz", "rgb", "n", "rec", "cam", "dst", "flags", "ws")]
    for kw in refusals:
        st, dst, flags, ws, _ = _raw_call(eng, cases, 100, cam, fill=0xA5, **kw)
        assert st == L.SD_ERR_INVALID, kw
        assert (dst == 0x5A).all() and (flags == -7).all() and (ws == 0xA5).all(), kw
    st, dst, flags, _, _ = _raw_call(eng, cases, 100, cam, fill=0xA5)
    assert st == L.SD_OK and (flags == 0).all() and np.array_equal(dst, _want(cases))


class _CloudEngine:
    """the engine, except that process_batch's final road clouds and records are replaced, on the device, by frames of tests/render_cases.py
    (the seeded weights leave the final clouds of the test's frames empty, and the route is for frames that have a road); every batch's
    substitutes are kept, copied to the host, for the test to apply the host statement to"""

    def __init__(self, eng, cam):
        self._eng, self._cam, self.seen = eng, cam, []

    def __getattr__(self, name):
        return getattr(self._eng, name)

    def process_batch(self, *a, **k):
        out = self._eng.process_batch(*a, **k)
        assert k.get("want_final") and out.get("road_final") is not None  # render= asks for the final clouds although no PLY is written
        B, first = int(out["records"].shape[0]), len(self.seen) * 2
        cases = [R.case(f"f{first + b}", R.cloud(50 + first + b, (700, 0, 333, 1)[(first + b) % 4]), self._cam, rec=R.LINE if (first + b) % 4 < 2 else None)
                 for b in range(B)]
        final, recs = _pack(cases, 1000, seed=first)
        fin, rec = _dev(final, recs)
        out["road_final"] = fin
        out["records"].copy_(rec)
        self.seen.append(cases)
        return out


def test_run_sequence_files_writes_the_renders_on_both_png_routes(tmp_path):
    """the driver on a 128 x 256 engine, four frames in batches of two: every _render.png of both PNG routes decodes to the host statement
    applied to that batch's final clouds and records; without render= the run writes what it wrote before"""
    import test_gpu_sequence_outputs as S
    from semantic_depth_amd import weights as W
    from semantic_depth_amd.distributed import make_engine_step, run_sequence_files
    from semantic_depth_amd.engine import Engine, RoadWidthParams
    H, W_ = 128, 256
    frames = S._smooth_frames(np.random.default_rng(21), 4, 2 * H, 2 * W_, cell=16)
    src = tmp_path / "in"
    src.mkdir()
    paths = [outputs.write_png(str(src / f"city_{i:03d}_leftImg8bit.png"), frames[i], level=1) for i in range(len(frames))]
    cam = outputs.top_camera(96, 80)
    e = Engine(H, W_, 2, "resnet50", precision="bf16x3")
    seen = {}
    try:
        e.load_weights(L.SD_NET_FCN8S, W.make_fcn8s_weights(1, decoder_std=0.05))
        e.load_weights(L.SD_NET_MONODEPTH, W.make_monodepth_weights("resnet50", 2))
        prm, names = RoadWidthParams(), outputs.sequence_names(paths)
        manifests = {}
        for key, kw in (("plain", {}), ("host", dict(render=cam, png="host")), ("device", dict(render=cam, png="device"))):
            outs = outputs.SequenceOutputs(str(tmp_path / key), names, depth=prm.depth, threads=8, ply=False)
            ce = _CloudEngine(e, cam) if kw else e
            run_sequence_files(paths, make_engine_step(ce, lambda i: S.CAM, prm, outputs=outs), batch=2, device="cuda", **kw)
            manifests[key] = json.load(open(outs.manifest))
            assert manifests[key]["status"] == "ok"
            seen[key] = [c for batch in getattr(ce, "seen", []) for c in batch]
    finally:
        e.close()
    assert "render" not in manifests["plain"] and not os.path.exists(tmp_path / "plain" / outputs.SEQ_RENDER_DIR)
    assert not any("render" in f for f in manifests["plain"]["files"])
    for key in ("host", "device"):
        rel = [os.path.join(outputs.SEQ_RENDER_DIR, f"{nm}_render.png") for nm in names]
        assert manifests[key]["render"] == rel and set(rel) <= set(manifests[key]["files"])
        assert len(seen[key]) == 4
        want = _want(seen[key])
        for i, r in enumerate(rel):
            assert np.array_equal(frame_io.imread(str(tmp_path / key / r)), want[i]), (key, r)
        assert (want[0] != 255).any() and (want[2] != 255).any() and R.line_pixels(want[1]) > 0
        assert len(manifests[key]["files"]) == len(manifests["plain"]["files"]) + 4
