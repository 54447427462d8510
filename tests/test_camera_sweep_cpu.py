"""CPU: the camera sweep (trial cameras as a batch axis behind one network pass) above the kernel -- the batched sweep driver against
outputs.focal_sweep fed the same table of distances, the chunking plan of Engine.sweep_tail, and the bindings and argument checks of
sd_fuse_backproject_sweep (no launch: there is no GPU here)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import __graft_entry__ as graft
from semantic_depth_amd import _lib as L
from semantic_depth_amd import api, outputs
from semantic_depth_amd.engine import F2F_DTYPE, RW_DTYPE, Camera, Engine, sweep_chunks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 8, 16


# ------------------------------------------------------------------------------------------------ the driver
class _Calls:
    def __init__(self):
        self.sweeps, self.resized = [], []


def _operators(monkeypatch, table, max_batch, calls):
    """a SegmentFrame and a DepthFrame over an Engine that was never created (no GPU): camera_sweep answers from ``table``:
    (focal length, frame id) -> (dist_rw or None, dist_f2f or None); a frame's id is its pixel [0, 0, 0]"""
    eng = Engine.__new__(Engine)
    eng.H, eng.W, eng.max_batch, eng.encoder, eng.device, eng.h = H, W, max_batch, "vgg", torch.device("cpu"), None
    wf, wm = {}, {}
    eng._api_loaded = {L.SD_NET_FCN8S: wf, L.SD_NET_MONODEPTH: wm}

    def camera_sweep(self, frames, cams, params=None, approach="rw", fence_params=None, colours=False):
        B, T = frames.shape[0], len(cams)
        assert tuple(frames.shape[1:]) == (H, W, 3) and all(len(row) == B for row in cams) and B <= self.max_batch
        calls.sweeps.append((frames.clone(), cams, approach))
        recs, f2f = np.zeros(T * B, RW_DTYPE), np.zeros(T * B, F2F_DTYPE)
        for t in range(T):
            for b in range(B):
                rw, ff = table[(cams[t][b].f, int(frames[b, 0, 0, 0]))]
                recs[t * B + b]["found"], recs[t * B + b]["width"] = rw is not None, np.nan if rw is None else rw
                f2f[t * B + b]["ok"], f2f[t * B + b]["dist"] = ff is not None, np.nan if ff is None else ff
        as_bytes = lambda a: torch.from_numpy(a.view(np.uint8).reshape(T * B, -1).copy())
        return dict(seg=None, disp_pp=None, records=as_bytes(recs), f2f=as_bytes(f2f) if approach == "both" else None)

    def resize_cubic(self, frames, out_h=None, out_w=None):
        calls.resized.append(tuple(frames.shape))
        return frames[:, :H, :W].contiguous()

    monkeypatch.setattr(Engine, "camera_sweep", camera_sweep)
    monkeypatch.setattr(Engine, "resize_cubic", resize_cubic)
    monkeypatch.setattr(Engine, "check_range", lambda self: None)
    seg = api.SegmentFrame((H, W), wf, engine=eng)
    dep = api.DepthFrame(encoder="vgg", input_height=H, input_width=W, checkpoint_path=wm, engine=eng)
    return seg, dep


def _frame(idx, h=H, w=W):
    f = np.full((h, w, 3), 7, np.uint8)
    f[0, 0, 0] = idx
    return f


def _tree(root):
    return {os.path.relpath(os.path.join(d, f), root): open(os.path.join(d, f), "rb").read() for d, _, fs in os.walk(root) for f in fs}


@pytest.mark.parametrize("max_batch", [1, 2, 8])
def test_batched_driver_writes_the_files_of_focal_sweep(golden_dir, tmp_path, monkeypatch, max_batch):
    """the table of the byte-pinned focal_sweep test through both drivers: the same data.txt files, the same best_focal_lengths.txt,
    the same returned dict -- whatever the frame batching (max_batch = 1: one frame per camera_sweep, legal)"""
    import json
    txt = json.load(open(os.path.join(golden_dir, "ref_text_outputs.json")))
    rows = {int(k): v for k, v in txt["sweep_rows"].items()}
    gt = txt["sweep_gt"]
    names = sorted(gt)
    focal = [380, 580]

    class Depther:
        f = None

    d = Depther()
    old_dir, new_dir = tmp_path / "old", tmp_path / "new"
    old = outputs.focal_sweep(lambda name: tuple(rows[d.f][names.index(name)][1:]), gt, d, focal_lengths=focal, results_directory=str(old_dir))
    assert open(old_dir / "380" / "data.txt").read() == txt["data_380"]

    calls = _Calls()
    table = {(f, i): tuple(rows[f][i][1:]) for f in focal for i in range(len(names))}
    seg, dep = _operators(monkeypatch, table, max_batch, calls)
    f_before = dep.f
    frames = {name: _frame(i) for i, name in enumerate(names)}
    new = outputs.focal_sweep_batched(frames, gt, seg, dep, focal_lengths=focal, results_directory=str(new_dir))
    assert _tree(old_dir) == _tree(new_dir) and len(_tree(new_dir)) == 3
    assert new == old
    assert dep.f == f_before                                                   # the trial focal lengths never touch the operator
    assert len(calls.sweeps) == -(-len(names) // max_batch) and not calls.resized
    assert all(a == "both" for _, _, a in calls.sweeps)


def test_batched_driver_refuses_a_missing_distance_before_writing(tmp_path, monkeypatch):
    gt = {"a": 6.0, "b": 7.0, "c": 6.5}
    table = {(f, i): (6.1 + i, 8.0 + i) for f in (400, 500) for i in range(3)}
    table[(500, 1)] = (None, 9.0)                                            # found == 0
    calls = _Calls()
    seg, dep = _operators(monkeypatch, table, 2, calls)
    frames = {n: _frame(i) for i, n in enumerate(sorted(gt))}
    with pytest.raises(ValueError, match=r"500.*'b'"):
        outputs.focal_sweep_batched(frames, gt, seg, dep, focal_lengths=[400, 500], results_directory=str(tmp_path / "r"))
    assert _tree(tmp_path) == {}
    table[(500, 1)] = (7.1, 9.0)
    table[(400, 2)] = (8.1, None)                                            # ok == 0
    with pytest.raises(ValueError, match=r"400.*'c'"):
        outputs.focal_sweep_batched(frames, gt, seg, dep, focal_lengths=[400, 500], results_directory=str(tmp_path / "r"))
    assert _tree(tmp_path) == {}


def test_batched_driver_builds_one_camera_per_trial_and_frame(tmp_path, monkeypatch):
    """f per trial; the multiplier is each frame's ORIGINAL width (frames of other sizes are resized first), or the constant"""
    gt = {"a": 6.0, "b": 7.0, "c": 6.5}
    focal = [380, 470.5, 580]
    table = {(f, i): (6.0, 8.0) for f in focal for i in range(3)}
    calls = _Calls()
    seg, dep = _operators(monkeypatch, table, 2, calls)
    frames = {"a": _frame(0), "b": _frame(1, 2 * H, 2 * W), "c": _frame(2, H + 3, 40)}
    outputs.focal_sweep_batched(frames, gt, seg, dep, focal_lengths=focal, results_directory=str(tmp_path / "w"))
    assert calls.resized == [(1, 2 * H, 2 * W, 3), (1, H + 3, 40, 3)]
    (fr0, cams0, _), (fr1, cams1, _) = calls.sweeps
    assert fr0.shape[0] == 2 and fr1.shape[0] == 1 and [int(fr0[0, 0, 0, 0]), int(fr0[1, 0, 0, 0]), int(fr1[0, 0, 0, 0])] == [0, 1, 2]
    for cams, widths in ((cams0, (W, 2 * W)), (cams1, (40,))):
        assert len(cams) == 3
        for t, row in enumerate(cams):
            assert row == [Camera(dep.cx, dep.cy, focal[t], dep.b, float(w)) for w in widths]
    calls.sweeps.clear()
    outputs.focal_sweep_batched(frames, gt, seg, dep, focal_lengths=focal, results_directory=str(tmp_path / "c"), disp_multiplier=3800)
    assert all(c.disp_mult == 3800.0 and c.f == focal[t] for _, cams, _ in calls.sweeps for t, row in enumerate(cams) for c in row)
    assert outputs.sweep_cameras(dep, [1, 2], [5])[1][0] == Camera(dep.cx, dep.cy, 2, dep.b, 5.0) and dep.f == 380


# ------------------------------------------------------------------------------------------------ the chunking plan
def test_sweep_chunks():
    assert sweep_chunks(2, 5, 4) == [(0, 2), (2, 4), (4, 5)]                 # chunks of 2, 2, 1 trials: 4, 4, 2 slots
    assert sweep_chunks(1, 3, 1) == [(0, 1), (1, 2), (2, 3)]
    assert sweep_chunks(4, 3, 4) == [(0, 1), (1, 2), (2, 3)]
    assert sweep_chunks(3, 2, 32) == [(0, 2)]
    for B, T, mb in ((2, 5, 4), (3, 7, 8), (1, 20, 32), (5, 20, 32)):
        ch = sweep_chunks(B, T, mb)
        assert ch[0][0] == 0 and ch[-1][1] == T and all(a[1] == b[0] for a, b in zip(ch, ch[1:]))
        assert all(0 < (t1 - t0) * B <= mb for t0, t1 in ch)
    with pytest.raises(ValueError):
        sweep_chunks(5, 3, 4)                                                # a chain call takes at most max_batch slots
    with pytest.raises(ValueError):
        sweep_chunks(2, 0, 4)


# ------------------------------------------------------------------------------------------------ the bindings
@pytest.fixture(scope="module")
def lib():
    graft.build()
    return L.load()


def test_sweep_symbols_are_declared_exported_and_bound(lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "semdepth.h")).read(), flags=re.S)
    ctype = {"sd_handle*": C.c_void_p, "int": C.c_int, "size_t": C.c_size_t, "void*": C.c_void_p, "const sd_camera*": C.POINTER(L.sd_camera),
             "const float*": C.c_void_p, "const uint8_t*": C.c_void_p, "float*": C.c_void_p, "uint8_t*": C.c_void_p, "int32_t*": C.c_void_p}
    for name, ret in (("sd_fuse_sweep_workspace", C.c_size_t), ("sd_fuse_backproject_sweep", C.c_int)):
        m = re.search(r"(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, name + " is not declared in semdepth.h"
        args = [ctype[re.sub(r"\s*\w+$", "", a.strip()).replace(" *", "*")] for a in m.group(2).split(",")]
        fn = getattr(lib, name)
        assert fn.restype is ret and list(fn.argtypes) == args, name
        assert L.SIGNATURES[name] == (ret, args)


def test_sweep_argument_checks(lib):
    """every refusal of the header comment, on a handle that was never bound: SD_ERR_INVALID before anything is launched"""
    assert lib.sd_fuse_sweep_workspace(0, 1, 128, 256) == 0 and lib.sd_fuse_sweep_workspace(1, 0, 128, 256) == 0
    assert lib.sd_fuse_sweep_workspace(256, 256, 128, 256) == 0                 # T * B = 65536
    need = lib.sd_fuse_sweep_workspace(2, 3, 256, 512)
    # 6 cameras of 136 bytes, then block counts and block offsets: two int32 per 256-pixel block and frame, each region 16-byte aligned
    assert need == 6 * 136 + 2 * (2 * 512 * 2 * 4) and need % 16 == 0
    assert lib.sd_fuse_sweep_workspace(255, 257, 256, 512) > 0                  # T * B = 65535
    h = C.c_void_p()
    assert lib.sd_create(C.byref(h), 0, 256, 512, 2, L.SD_ENC_VGG, L.SD_PREC_F32) == 0
    try:
        cams = (L.sd_camera * 6)(*[L.sd_camera(256.0, 128.0, 380.0 + i, 1.0, 512.0) for i in range(6)])
        p = C.c_void_p(4096)                                                # never dereferenced: every call below is refused
        good = dict(disp=p, road=p, fence=p, frames=p, cams=cams, B=2, T=3, cap=100, rx=p, rc=p, rn=p, fx=p, fc=p, fn=p, ws=p, nbytes=need)

        def call(**kw):
            a = dict(good, **kw)
            return lib.sd_fuse_backproject_sweep(h, a["disp"], a["road"], a["fence"], a["frames"], a["cams"], a["B"], a["T"], a["cap"], a["rx"],
                                                 a["rc"], a["rn"], a["fx"], a["fc"], a["fn"], a["ws"], a["nbytes"], None)
        for bad in (dict(disp=None), dict(road=None), dict(cams=None), dict(rx=None), dict(rn=None), dict(ws=None), dict(B=0), dict(T=0),
                    dict(cap=0), dict(B=256, T=256), dict(nbytes=need - 1), dict(ws=C.c_void_p(4096 + 8)), dict(frames=None),
                    dict(frames=None, rc=None), dict(fence=None), dict(fn=None), dict(fx=None)):
            assert call(**bad) == L.SD_ERR_INVALID, bad
            assert b"sd_fuse_backproject_sweep" in lib.sd_last_error(h)
    finally:
        lib.sd_destroy(h)
