"""CPU: the container of the result video (outputs.MjpegAviWriter, frame_io.avi_frames, outputs.join_mjpeg_avi) against an independent
struct-based RIFF walk, and SequenceOutputs(video=Video(route="host")) fed host tensors: the frames of result_imgs.avi are the bytes of
sd_jpeg_encode_bgr_host of the submitted images, in frame order."""
import json
import os
import struct

import numpy as np
import pytest
import torch

import jpeg_enc_cases as JC
from semantic_depth_amd import frame_io, outputs


def _walk(data, start, end):
    out, pos = [], start
    while pos < end:
        cc, size = data[pos:pos + 4], struct.unpack("<I", data[pos + 4:pos + 8])[0]
        out.append((cc, pos + 8, size))
        pos += 8 + size + (size & 1)
    assert pos == end, (pos, end)
    return out


def _check_avi(path, frames, width, height, rate, scale):
    """every size field, count, fourcc and index entry of one file, by a RIFF walk of its own"""
    data = open(path, "rb").read()
    assert data[:4] == b"RIFF" and data[8:12] == b"AVI "
    assert struct.unpack("<I", data[4:8])[0] == len(data) - 8
    top = _walk(data, 12, len(data))
    assert [c for c, _, _ in top] == [b"LIST", b"LIST", b"idx1"]
    (_, hoff, hsize), (_, moff, msize), (_, ioff, isize) = top
    assert data[hoff:hoff + 4] == b"hdrl" and data[moff:moff + 4] == b"movi"
    hdrl = _walk(data, hoff + 4, hoff + hsize)
    assert [c for c, _, _ in hdrl] == [b"avih", b"LIST"] and hdrl[0][2] == 56
    avih = struct.unpack("<14I", data[hdrl[0][1]:hdrl[0][1] + 56])
    assert avih[0] == round(1e6 * scale / rate) and avih[3] == 0x10 and avih[4] == len(frames) and avih[6] == 1 and avih[8:10] == (width, height)
    assert avih[7] == max(len(f) for f in frames)
    assert data[hdrl[1][1]:hdrl[1][1] + 4] == b"strl"
    strl = _walk(data, hdrl[1][1] + 4, hdrl[1][1] + hdrl[1][2])
    assert [(c, s) for c, _, s in strl] == [(b"strh", 56), (b"strf", 40)]
    strh = struct.unpack("<4s4sIHHIIIIIIII4h", data[strl[0][1]:strl[0][1] + 56])
    assert strh[0] == b"vids" and strh[1] == b"MJPG" and (strh[6], strh[7]) == (scale, rate) and strh[9] == len(frames)
    assert strh[13:] == (0, 0, width, height)
    strf = struct.unpack("<IiiHH4sIiiII", data[strl[1][1]:strl[1][1] + 40])
    assert strf[:7] == (40, width, height, 1, 24, b"MJPG", width * height * 3)
    chunks = _walk(data, moff + 4, moff + msize)
    assert [c for c, _, _ in chunks] == [b"00dc"] * len(frames)
    for (_, off, size), fr in zip(chunks, frames):
        assert data[off:off + size] == fr
        if size & 1:
            assert data[off + size] == 0
    assert isize == 16 * len(frames)
    for k, (_, off, size) in enumerate(chunks):
        cc, flags, rel, n = struct.unpack("<4sIII", data[ioff + 16 * k:ioff + 16 * k + 16])
        assert (cc, flags, n) == (b"00dc", 0x10, size) and moff + rel + 8 == off
    assert list(frame_io.avi_frames(path)) == list(frames)
    info = frame_io.avi_info(path)
    assert (info["width"], info["height"], info["frames"], info["rate"], info["scale"]) == (width, height, len(frames), rate, scale)


def _fake_frames(n=5):
    rng = np.random.default_rng(3)
    sizes = [40, 33, 52, 18, 27][:n]                            # (33 and 27: odd lengths, a pad byte each)
    return [b"\xff\xd8" + rng.integers(0, 255, s - 4, dtype=np.uint8).tobytes() + b"\xff\xd9" for s in sizes]


def test_avi_structure(tmp_path):
    frames = _fake_frames()
    assert any(len(f) & 1 for f in frames)
    path = str(tmp_path / "v.avi")
    wr = outputs.MjpegAviWriter(path, 70, 50, 30000 / 1001)
    for f in frames:
        wr.append(f)
    assert wr.close() == [path] and wr.close() == [path]
    _check_avi(path, frames, 70, 50, 30000, 1001)
    with pytest.raises(RuntimeError):
        wr.append(frames[0])


def test_avi_rolls_over_and_joins(tmp_path):
    frames = _fake_frames()
    path = str(tmp_path / "v.avi")
    limit = 224 + sum(8 + len(f) + (len(f) & 1) + 16 for f in frames[:3]) + 8 - 8       # the RIFF payload of exactly three frames
    with outputs.MjpegAviWriter(path, 70, 50, 25, _max_riff_bytes=limit) as wr:
        for f in frames:
            wr.append(f)
    assert wr.paths == [path, str(tmp_path / "v_part1.avi")]
    _check_avi(wr.paths[0], frames[:3], 70, 50, 25, 1)
    _check_avi(wr.paths[1], frames[3:], 70, 50, 25, 1)
    assert os.path.getsize(wr.paths[0]) - 8 <= limit
    joined = outputs.join_mjpeg_avi(wr.paths, str(tmp_path / "all.avi"))
    assert joined == [str(tmp_path / "all.avi")]
    _check_avi(joined[0], frames, 70, 50, 25, 1)


def test_video_is_validated():
    assert outputs.Video() == outputs.Video(30.0, 90, "device")
    for kw in (dict(fps=0), dict(fps=-1), dict(fps=float("nan")), dict(quality=0), dict(quality=101), dict(route="gpu")):
        with pytest.raises(ValueError):
            outputs.Video(**kw)
    with pytest.raises(dataclasses_error()):
        outputs.Video().fps = 3


def dataclasses_error():
    import dataclasses
    return dataclasses.FrozenInstanceError


def _records(n):
    from semantic_depth_amd.engine import RW_DTYPE
    return torch.zeros((n, RW_DTYPE.itemsize), dtype=torch.uint8)


@pytest.mark.parametrize("images", [True, False])
def test_sequence_outputs_host_route(tmp_path, images):
    JC.lib()
    h, w = 40, 56
    imgs = np.stack([JC.mixed_frame(50 + i, h, w) for i in range(5)])
    names = [f"f{i:02d}" for i in range(5)]
    so = outputs.SequenceOutputs(str(tmp_path), names, images=images, ply=False, items=False, video=outputs.Video(fps=12.5, quality=80, route="host"))
    so.begin(0, 1, 0, 5)
    so.submit(0, _records(3), (h, w), images=torch.from_numpy(imgs[:3]))
    so.submit(3, _records(2), (h, w), images=torch.from_numpy(imgs[3:]))
    man = json.load(open(so.close()))
    assert man["video"] == ["result_imgs.avi"] and man["video_fallback"] == [] and man["status"] == "ok"
    assert "result_imgs.avi" in man["files"]
    path = str(tmp_path / "result_imgs.avi")
    got = list(frame_io.avi_frames(path))
    assert got == [JC.encode_host(im, 80) for im in imgs]
    info = frame_io.avi_info(path)
    assert (info["width"], info["height"], info["rate"], info["scale"]) == (w, h, 25, 2)
    assert os.path.exists(tmp_path / "result_sequence_imgs" / "f00.png") == images


def test_sequence_outputs_device_route_from_host_tensors_with_a_flagged_frame(tmp_path):
    """submit(video_streams=) with host tensors: the streams are written as they are, a flagged frame is encoded from its raw image"""
    JC.lib()
    h, w = 24, 40
    imgs = np.stack([JC.mixed_frame(70 + i, h, w) for i in range(3)])
    want = [JC.encode_host(im, 90) for im in imgs]
    stride = max(len(x) for x in want)
    streams = np.zeros((3, stride), np.uint8)
    for i in (0, 2):
        streams[i, :len(want[i])] = np.frombuffer(want[i], np.uint8)
    sizes = np.array([len(want[0]), 0, len(want[2])], np.int64)
    flags = np.array([0, 1, 0], np.int32)
    so = outputs.SequenceOutputs(str(tmp_path), ["a", "b", "c"], images=False, ply=False, items=False, video=outputs.Video())
    with pytest.raises(ValueError):
        so.submit(0, _records(3), (h, w), images=torch.from_numpy(imgs))
    so.submit(0, _records(3), (h, w), images=torch.from_numpy(imgs), video_streams=tuple(torch.from_numpy(a) for a in (streams, sizes, flags)))
    man = json.load(open(so.close()))
    assert man["video_fallback"] == ["b"]
    assert list(frame_io.avi_frames(str(tmp_path / "result_imgs.avi"))) == want


def test_without_video_the_manifest_is_what_it_was(tmp_path):
    so = outputs.SequenceOutputs(str(tmp_path), ["a"], images=False, ply=False, items=False)
    so.submit(0, _records(1), (8, 8))
    man = json.load(open(so.close()))
    assert "video" not in man and "video_fallback" not in man
    assert not os.path.exists(tmp_path / "result_imgs.avi")


def test_host_route_refuses_the_device_png_route(tmp_path):
    with pytest.raises(ValueError):
        outputs.SequenceOutputs(str(tmp_path), ["a"], png="device", video=outputs.Video(route="host"))
    so = outputs.SequenceOutputs(str(tmp_path), ["a"], video=outputs.Video(route="host"))
    with pytest.raises(ValueError):
        so.set_png("device")
    so2 = outputs.SequenceOutputs(str(tmp_path), ["a"], png="device")
    with pytest.raises(ValueError):
        so2.set_video(outputs.Video(route="host"))
    so2.set_video(outputs.Video(route="device"))
    with pytest.raises(ValueError):
        so2.set_video("yes")
    so.close()
    so2.close()
