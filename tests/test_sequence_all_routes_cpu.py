"""CPU: one SequenceOutputs with every route on at once (tests/sequence_all_routes_cases.py) fed host arrays: three batches of changing
size through the two staging slots, a PLY fallback frame and a video fallback frame together; and a failing batch in the middle, which
passes its turn in the video on exactly once."""
import json
import os

import numpy as np
import pytest

import ply_device_cases as PD
import sequence_all_routes_cases as A
from semantic_depth_amd import frame_io, outputs


def test_every_route_in_one_run(tmp_path):
    manifest = A.run(tmp_path).close()
    fr = A.frames()
    for i, name in enumerate(A.NAMES):
        assert np.array_equal(frame_io.imread(str(tmp_path / outputs.SEQ_IMG_DIR / f"{name}.png")), fr[i]["image"]), name
        assert np.array_equal(frame_io.imread(str(tmp_path / outputs.SEQ_RENDER_DIR / f"{name}_render.png")), fr[i]["render"]), name
        got = open(tmp_path / outputs.SEQ_PLY_DIR / f"{name}_rw.ply", "rb").read()
        assert got == PD.want(fr[i]["case"]), (name, PD.first_difference(got, PD.want(fr[i]["case"])))
    want = [outputs.encode_jpeg_host(f["image"], A.QUALITY) for f in fr]
    assert want == [f["jpeg"] for f in fr] and len(want[A.NOISE_FRAME]) > max(len(w) for i, w in enumerate(want) if i != A.NOISE_FRAME)
    assert list(frame_io.avi_frames(str(tmp_path / "result_imgs.avi"))) == want
    m = json.load(open(manifest))
    on_disk = sorted(set(A.tree(tmp_path)) - {"manifest_rank0.json"})
    # per frame: the result image, its _overlay.json, the PLY, the render, the disparity image and the profile; and the video
    assert m["files"] == on_disk and len(on_disk) == 6 * len(A.NAMES) + 1
    assert m["status"] == "ok" and m["valid"] is True and m["frames"] == [0, len(A.NAMES)]
    assert m["ply_fallback"] == [A.NAMES[A.NAN_FRAME]] and m["video_fallback"] == [A.NAMES[A.NOISE_FRAME]]
    assert m["video"] == ["result_imgs.avi"] and m["render"] == [f for f in on_disk if f.startswith(outputs.SEQ_RENDER_DIR + os.sep)]
    assert len(m["render"]) == len(A.NAMES)
    for i, name in enumerate(A.NAMES):
        assert np.array_equal(frame_io.imread(str(tmp_path / outputs.SEQ_DISP_DIR / f"{name}_disp.png")), fr[i]["disp"]), name
        assert open(tmp_path / outputs.SEQ_PROFILE_DIR / f"{name}.txt").read() == outputs.profile_text(A.PROFILE, fr[i]["profile"]), name
        doc = json.load(open(tmp_path / outputs.SEQ_IMG_DIR / f"{name}_overlay.json"))
        segs, _ = outputs.overlay_segments(fr[i]["case"]["rec"], fr[i]["cam"], A.NET, (A.H, A.W), A.LINES, profile=fr[i]["profile"],
                                           clip_top=int(0.25 * A.H))
        assert doc["lines"] == outputs.segments_json(segs) and len(doc["lines"]) >= 2 * len(A.PROFILE), name
    assert m["disp"] == [os.path.join(outputs.SEQ_DISP_DIR, f"{name}_disp.png") for name in A.NAMES]
    assert m["profile"] == [os.path.join(outputs.SEQ_PROFILE_DIR, f"{name}.txt") for name in A.NAMES] and m["profile_depths"] == A.PROFILE
    assert m["disp_nonfinite"] == [A.NAMES[A.DISP_NAN_FRAME]] and m["lines_flagged"] == [A.NAMES[A.LINES_FLAGGED_FRAME]]
    assert m["lines"] == A.LINES.as_dict()
    assert list(m) == ["rank", "world", "frames", "status", "valid", "files", "recomputed", "ply_fallback", "render", "video", "video_fallback",
                       "profile_depths", "profile", "disp", "disp_nonfinite", "lines", "lines_flagged"]


def test_a_failing_batch_passes_its_video_turn_on_once(tmp_path):
    outs = A.run(tmp_path, spoil=1)
    with pytest.raises(ValueError):
        outs.close()
    m = json.load(open(tmp_path / "manifest_rank0.json"))
    assert m["status"] == "error" and m["valid"] is False
    fr = A.frames()
    lo, n = A.BATCHES[2]
    for i in range(lo, lo + n):
        assert np.array_equal(frame_io.imread(str(tmp_path / outputs.SEQ_IMG_DIR / f"{A.NAMES[i]}.png")), fr[i]["image"])
        assert os.path.join(outputs.SEQ_IMG_DIR, f"{A.NAMES[i]}.png") in m["files"]
    kept = [i for k in (0, 2) for i in range(A.BATCHES[k][0], sum(A.BATCHES[k]))]
    assert list(frame_io.avi_frames(str(tmp_path / "result_imgs.avi"))) == [fr[i]["jpeg"] for i in kept]
