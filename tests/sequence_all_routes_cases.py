"""Shared by tests/test_sequence_all_routes_cpu.py and tests/test_gpu_sequence_all_routes.py: three batches (3, 2 and 3 frames of
24 x 32) for one SequenceOutputs with every route on -- png="device", ply="device", text="draw", render=, video route "device", disp=,
profile=, lines=, items -- built from the host statements of the device routes (sd_png_encode_zlib_host, sd_ply_format_rw_host,
sd_jpeg_encode_bgr_host, outputs.render_rw, outputs.disparity_image, outputs.overlay_segments), so that submit() gets what the step of
make_engine_step would hand it.  Both staging slots are reused, once by a smaller and once by a larger batch.  Frame 1's cloud holds a
NaN (PLY flag 1), frame 6 is noise whose video stream is withheld (size 0, flag 1), frame 3 has found = 0, frame 5's cloud is empty,
frame 2's disparity map holds a NaN (disp flag 1) and frame 4 comes with a non-zero lines flag."""
import functools
import os

import numpy as np
import torch

import jpeg_enc_cases as JC
import overlay_cases as O
import ply_device_cases as PD
import png_device_cases as PN
from semantic_depth_amd import outputs
from semantic_depth_amd.engine import RW_DTYPE, RWP_DTYPE, Camera

H, W = 24, 32
BATCHES = ((0, 3), (3, 2), (5, 3))                       # (first frame, frames)
NAMES = [f"f{i:02d}" for i in range(8)]
NAN_FRAME, NOISE_FRAME, NOT_FOUND_FRAME, EMPTY_FRAME = 1, 6, 3, 5
POINTS = [40, 25, 33, 12, 40, 0, 7, 19]
CAP = 40
QUALITY = 90
VIDEO_STRIDE = 1024 + H * W * 3 // 2                     # the stride the step of make_engine_step gives Engine.encode_jpeg
CAMERA = outputs.top_camera(48, 40)
DISP_NAN_FRAME, LINES_FLAGGED_FRAME = 2, 4
NET = (12, 16)                                           # the network size: of the disparity maps, and what the cameras belong to
PROFILE = [8.0, 10.0]
LINES = outputs.OverlayLines()
# the keywords of the routes that came first; run(every=False) turns on only those
BASE_KEYWORDS = ("records", "images", "final", "png_streams", "ply_text", "render_streams", "video_streams")


def _rows(blobs, stride):
    """(u8 [n,stride] filled with 0xA5 behind every blob, i64 [n] sizes)"""
    out = np.full((len(blobs), stride), 0xA5, np.uint8)
    for i, b in enumerate(blobs):
        out[i, :len(b)] = np.frombuffer(b, np.uint8)
    return out, np.array([len(b) for b in blobs], np.int64)


@functools.lru_cache(maxsize=None)
def frames():
    """per frame: dict(image, case (ply_device_cases: xyz, rgb, rec), render, jpeg, disp (the disparity image), disp_flag, cam, profile
    (RWP_DTYPE [2]: found at both depths, the end points in front of the camera), lines_flag)"""
    PD.lib()
    rng = np.random.default_rng(5)
    maps = (rng.random((len(NAMES), *NET), dtype=np.float32) * np.float32(0.08)).astype(np.float32)
    maps[DISP_NAN_FRAME, 3, 4] = np.nan
    disp, disp_flags = outputs.disparity_image(maps, H, W, "gray", np.full(len(NAMES), 3800.0, np.float32))
    assert disp_flags.tolist() == [int(i == DISP_NAN_FRAME) for i in range(len(NAMES))]
    out = []
    for i in range(len(NAMES)):
        if i == NOISE_FRAME:
            image = np.random.default_rng(900).integers(0, 256, (H, W, 3), dtype=np.uint8)
        else:
            image = np.ascontiguousarray(PN.smooth_frame(300 + i, H, W, sigma=3.0))
        xyz = PD.cloud(60 + i, POINTS[i])
        if i == NAN_FRAME:
            xyz[11, 1] = np.nan
        rec = PD.record() if i == NOT_FOUND_FRAME else PD.record((-3.5 + 0.1 * i, 1.5, 9.0), (3.25, 1.5, 9.5 + 0.1 * i))
        c = PD.case(NAMES[i], xyz, rec=rec, seed=i)
        found = bool(rec["found"])
        render = outputs.render_rw(c["xyz"], c["rgb"], rec["left_pt"] if found else None, rec["right_pt"] if found else None, CAMERA)
        cam = Camera(cx=NET[1] / 2 + 0.01 * i, cy=NET[0] / 2 + 0.003, f=5.0001 + 0.1 * i, b=0.22, disp_mult=3800.0)
        profile = np.zeros(len(PROFILE), RWP_DTYPE)
        for k, d in enumerate(PROFILE):
            profile[k]["found"], profile[k]["width"], profile[k]["n_window"] = 1, 6.0 - 0.25 * k + 0.01 * i, 5 + i
            profile[k]["left_pt"] = O.point_at(cam, (H, W), 0.2 + 0.05 * k, 0.9 - 0.2 * k, d, net=NET).astype(np.float32)
            profile[k]["right_pt"] = O.point_at(cam, (H, W), 0.8 - 0.05 * k, 0.9 - 0.2 * k, d, net=NET).astype(np.float32)
            profile[k]["x_left"], profile[k]["x_right"] = profile[k]["left_pt"][0], profile[k]["right_pt"][0]
        out.append(dict(image=image, case=c, render=render, jpeg=JC.encode_host(image, QUALITY), disp=disp[i], disp_flag=int(disp_flags[i]),
                        cam=cam, profile=profile, lines_flag=int(i == LINES_FLAGGED_FRAME)))
    return out


@functools.lru_cache(maxsize=None)
def batches():
    """per batch: (lo, the keywords of SequenceOutputs.submit as host numpy arrays)"""
    fr = frames()
    out = []
    for lo, n in BATCHES:
        part = fr[lo:lo + n]
        records = np.stack([f["case"]["rec"] for f in part]).view(np.uint8).reshape(n, RW_DTYPE.itemsize).copy()
        xyz, rgb = np.zeros((n, CAP, 3), np.float32), np.zeros((n, CAP, 3), np.uint8)
        for i, f in enumerate(part):
            xyz[i, :len(f["case"]["xyz"])], rgb[i, :len(f["case"]["rgb"])] = f["case"]["xyz"], f["case"]["rgb"]
        count = np.array([len(f["case"]["xyz"]) for f in part], np.int32)
        texts, flags = [], []
        for f in part:
            st, text, flag = PD.host(f["case"])
            assert st == 0 and flag == (1 if f is fr[NAN_FRAME] else 0)
            texts.append(b"" if flag else text)
            flags.append(flag)
        offsets = np.concatenate([[0], np.cumsum([len(t) for t in texts])]).astype(np.int64)
        text = np.full(int(offsets[-1]) + 1000, 0xA5, np.uint8)                   # (nothing at or behind offsets[n] is the files')
        text[:offsets[-1]] = np.frombuffer(b"".join(texts), np.uint8)
        jpegs = [b"" if f is fr[NOISE_FRAME] else f["jpeg"] for f in part]
        assert all(len(j) <= VIDEO_STRIDE for j in jpegs)
        vflags = np.array([int(f is fr[NOISE_FRAME]) for f in part], np.int32)
        out.append((lo, dict(records=records, images=np.stack([f["image"] for f in part]), final=dict(xyz=xyz, rgb=rgb, n=count),
                             png_streams=_rows([PN.encode_host(f["image"]) for f in part], PN.bound(H, W)),
                             ply_text=(text, offsets, np.array(flags, np.int32)),
                             render_streams=_rows([PN.encode_host(f["render"]) for f in part], PN.bound(CAMERA.height, CAMERA.width)),
                             video_streams=_rows(jpegs, VIDEO_STRIDE) + (vflags,),
                             disp_streams=_rows([PN.encode_host(f["disp"]) for f in part], PN.bound(H, W)),
                             disp_flags=np.array([f["disp_flag"] for f in part], np.int32),
                             profile=np.stack([f["profile"] for f in part]).view(np.uint8).reshape(n, len(PROFILE), RWP_DTYPE.itemsize).copy(),
                             lines_flags=np.array([f["lines_flag"] for f in part], np.int32), cams=[f["cam"] for f in part], net_size=NET)))
    return out


def _tensors(v, to):
    """the numpy arrays of ``v`` as tensors placed by ``to``; the host values (the cameras, the network size) as they are"""
    if isinstance(v, dict):
        return {k: _tensors(x, to) for k, x in v.items()}
    if isinstance(v, tuple):
        return tuple(_tensors(x, to) for x in v)
    return to(torch.from_numpy(v)) if isinstance(v, np.ndarray) else v


def base(kw: dict) -> dict:
    """the keywords of a batch that run(every=False) needs"""
    return {k: kw[k] for k in BASE_KEYWORDS}


def run(directory, to=lambda t: t, spoil=None, every=True):
    """all batches through one SequenceOutputs with every route on (``every`` False: only png="device", ply="device", render= and the
    video, the run this file made before text, disp, profile and lines were added to it); ``to`` places every tensor
    (``lambda t: t.cuda()``); ``spoil`` = the index of a batch whose png_streams sizes get one entry too many.  Returns the
    SequenceOutputs, not closed."""
    more = dict(text="draw", disp="gray", profile=PROFILE, lines=LINES) if every else {}
    outs = outputs.SequenceOutputs(str(directory), NAMES, threads=2, png="device", ply="device", render=CAMERA,
                                   video=outputs.Video(fps=25, quality=QUALITY, route="device"), **more)
    outs.begin(0, 1, 0, len(NAMES))
    for k, (lo, kw) in enumerate(batches()):
        kw = dict(kw) if every else base(kw)
        if k == spoil:
            kw["png_streams"] = (kw["png_streams"][0], np.append(kw["png_streams"][1], 0))
        kw = _tensors(kw, to)
        outs.submit(lo, kw.pop("records"), (H, W), **kw)
    return outs


def tree(directory):
    """relative path -> bytes of every file below ``directory``"""
    return {os.path.relpath(os.path.join(r, f), directory): open(os.path.join(r, f), "rb").read() for r, _, fs in os.walk(directory) for f in fs}
