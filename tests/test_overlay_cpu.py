"""CPU: the host statement of the measurement lines (sd_overlay_segments_host, sd_overlay_draw_host; csrc/overlay_rule.hpp) against an
independent statement of the rule of include/semdepth.h (tests/overlay_cases.py), integer for integer and byte for byte, and the host-side
plumbing of lines= (SequenceOutputs, save_frame_outputs)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import __graft_entry__ as graft
import overlay_cases as O
from semantic_depth_amd import _lib as L
from semantic_depth_amd import frame_io, outputs
from semantic_depth_amd.engine import RW_DTYPE, Camera


@pytest.fixture(scope="module", autouse=True)
def lib():
    graft.build()
    return L.load()


@pytest.fixture(scope="module")
def drawn():
    """name -> (case, pre-filled frames, the independent statement's frames and flags): computed once, never modified"""
    out = {}
    for i, name in enumerate(O.CASES):
        c = O.case(name)
        img = O.prefilled(100 + i, c["B"], c["h"], c["w"], 3)
        out[name] = (c, img) + O.py_frames(img, c)
    return out


def _tuples(segs):
    return [(int(s["ax"]), int(s["ay"]), int(s["bx"]), int(s["by"]), tuple(int(v) for v in s["bgr"]), int(s["thickness"])) for s in segs]


@pytest.mark.parametrize("name", list(O.CASES))
def test_segments_equal_the_independent_statement(name):
    c = O.case(name)
    total = 0
    for b in range(c["B"]):
        segs, flag = O.host_segments(c, b)
        want, wflag = O.py_segments(c, b)
        assert _tuples(segs) == want, (name, b)
        assert flag == wflag == c["flags"][b], (name, b, flag, wflag, c["flags"][b])
        assert len(segs) <= 4 * c["D"] + 2
        total += len(segs)
    assert total > 0


@pytest.mark.parametrize("name", list(O.CASES))
def test_draw_host_equals_the_independent_statement(drawn, name):
    c, img, want, wflags = drawn[name]
    got, flags = O.host_draw(img, c)
    for b in range(c["B"]):
        assert np.array_equal(got[b], want[b]), (name, b, int((got[b] != want[b]).any(-1).sum()))
    assert np.array_equal(flags, c["flags"]) and np.array_equal(wflags, c["flags"])
    # the conditions of the case set: something is painted, something is left alone, rows above clip_top are never touched
    assert (got != img).any() and (got == img).all(-1).any()
    assert np.array_equal(got[:, :c["clip_top"]], img[:, :c["clip_top"]])


def test_the_case_set_covers_what_it_names(drawn):
    flags = np.concatenate([drawn[n][0]["flags"] for n in O.CASES])
    assert flags.any() and not flags.all()
    assert {O.CASES[n]["D"] for n in O.CASES} >= {0, 1, 7, 256}
    assert {drawn[n][0]["lines"].thickness for n in O.CASES} >= {1, 32}
    c, img, want, _ = drawn["thick_and_clipped"]                        # clip_top cuts through the thick line of frame 0
    assert (want[0, c["clip_top"]] != img[0, c["clip_top"]]).any() and np.array_equal(want[0, c["clip_top"] - 1], img[0, c["clip_top"] - 1])
    c = drawn["profile_seven"][0]
    assert not c["profile"]["found"].all() and not c["f2f_profile"]["ok"].all()      # the holes
    # two segments of different colours cross on frame 3 of the mixed batch: both colours are in the image
    c, img, want, _ = drawn["mixed_partial_tiles"]
    for colour in (c["lines"].rw_bgr, c["lines"].f2f_bgr):
        assert ((want[3] == colour).all(-1) & (img[3] != colour).any(-1)).any()


@pytest.mark.parametrize("mistake", ["no_centre", "flip_y", "first_wins", "clip_off_by_one"])
def test_a_seeded_mistake_changes_a_byte(drawn, mistake):
    """the restatement with one mistake is no longer what the host statement gives, somewhere on the case set"""
    changed = 0
    for name in O.CASES:
        c, img, want, _ = drawn[name]
        if c["D"] > 7:
            continue
        changed += int((O.py_frames(img, c, (mistake,))[0] != want).any(-1).sum())
    assert changed > 0


def test_round_trip_through_the_reprojection():
    """points that oracle.fusion.reproject makes from a seeded 64 x 128 disparity map come back, at 256 x 512, within one unit of 1/256 pixel
    of (x + 0.5) * 4 - 0.5: three float32 roundings (about 1.8e-7 relative) on |x - cx| <= 128 at scale 4 stay below 1e-3 pixel, plus the
    half unit of the quantisation"""
    from oracle import fusion
    rng = np.random.default_rng(11)
    cam = Camera(cx=1048.64 / 16, cy=519.277 / 16, f=580.0 / 16 * 1.37, b=0.22, disp_mult=3800.0)
    disp = (rng.uniform(0.02, 0.3, (64, 128)) * 128).astype(np.float32)
    pts = fusion.reproject(disp, fusion.make_Q(cam.cx, cam.cy, cam.f, cam.b))
    pixels = [(0, 0), (127, 63), (0, 63), (127, 0), (64, 32), (13, 57), (100, 5), (63, 31)]
    for (x0, y0), (x1, y1) in zip(pixels, pixels[1:] + pixels[:1]):
        rec = np.zeros((), RW_DTYPE)
        rec["found"] = 1
        rec["left_pt"], rec["right_pt"] = pts[y0, x0], pts[y1, x1]
        segs, flag = outputs.overlay_segments(rec, cam, (64, 128), (256, 512))
        assert flag == 0 and len(segs) == 1
        want = [((v + 0.5) * 4 - 0.5) * 256 for v in (x0, y0, x1, y1)]
        got = [int(segs[0][k]) for k in ("ax", "ay", "bx", "by")]
        assert all(abs(g - w) <= 1 for g, w in zip(got, want)), (got, want)


def test_refusals_write_nothing(lib):
    c = O.case("profile_seven")
    rec = L.sd_rw_result.from_buffer_copy(c["records"][0].tobytes())
    cam = L.sd_camera(64.0, 32.0, 70.0, 0.22, 1.0)
    prof = np.ascontiguousarray(c["profile"][0])
    segs = (L.sd_overlay_segment * (4 * 7 + 2))()
    C.memset(segs, 0xA5, C.sizeof(segs))
    n, flag = C.c_int(-7), C.c_int32(-7)

    def call(D=7, profile=prof, cam=cam, net=(64, 128), dst=(120, 300), style=None, record=rec, out=segs):
        st = style if style is not None else outputs.OverlayLines().struct(0)
        return lib.sd_overlay_segments_host(C.byref(record) if record is not None else None, None,
                                            None if profile is None else profile.ctypes.data_as(C.c_void_p), None, D, C.byref(cam), net[0], net[1],
                                            dst[0], dst[1], C.byref(st), out, C.byref(n), C.byref(flag))

    def style(**kw):
        s = outputs.OverlayLines().struct(kw.pop("clip_top", 0))
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    bad = [dict(D=257), dict(D=-1), dict(profile=None), dict(net=(0, 128)), dict(dst=(120, 16385)), dict(net=(64, 16385)),
           dict(style=style(thickness=0)), dict(style=style(thickness=33)), dict(style=style(profile_thickness=0)), dict(style=style(clip_top=121)),
           dict(style=style(clip_top=-1)), dict(cam=L.sd_camera(float("nan"), 32.0, 70.0, 0.22, 1.0)), dict(cam=L.sd_camera(64.0, float("inf"), 70.0, 0.22, 1.0)),
           dict(cam=L.sd_camera(64.0, 32.0, 1e39, 0.22, 1.0)), dict(record=None), dict(out=None)]
    for kw in bad:
        assert call(**kw) == L.SD_ERR_INVALID, kw
        assert n.value == -7 and flag.value == -7 and bytes(segs) == b"\xa5" * C.sizeof(segs), kw
    assert call() == L.SD_OK and n.value > 0
    assert call(D=0, profile=None) == L.SD_OK and n.value == 1

    img = np.full((8, 16, 3), 7, np.uint8)
    p = img.ctypes.data_as(C.c_void_p)

    def seg(**kw):
        s = L.sd_overlay_segment(256, 1024, 3000, 1024, (1, 2, 3), 2)
        for k, v in kw.items():
            setattr(s, k, v)
        return (L.sd_overlay_segment * 1)(s)

    cap = L.SD_OVERLAY_MAX_COORD * 256
    for arr, kw in ((seg(thickness=0), {}), (seg(thickness=33), {}), (seg(ax=cap + 1), {}), (seg(by=-cap - 1), {}), (seg(), dict(clip_top=9)),
                    (seg(), dict(clip_top=-1)), (seg(), dict(h=0)), (seg(), dict(w=16385)), (None, dict(n=1)), (seg(), dict(n=-1))):
        assert lib.sd_overlay_draw_host(p, kw.get("h", 8), kw.get("w", 16), arr, kw.get("n", 1), kw.get("clip_top", 0)) == L.SD_ERR_INVALID, kw
    assert lib.sd_overlay_draw_host(None, 8, 16, seg(), 1, 0) == L.SD_ERR_INVALID
    assert (img == 7).all()
    assert lib.sd_overlay_draw_host(p, 8, 16, seg(ax=cap, bx=-cap), 1, 0) == L.SD_OK and (img[4] == (1, 2, 3)).all() and (img[0] == 7).all()
    assert lib.sd_overlay_draw_host(p, 8, 16, None, 0, 8) == L.SD_OK
    assert lib.sd_overlay_workspace_bytes(0, 0) == 0 and lib.sd_overlay_workspace_bytes(1, 257) == 0 and lib.sd_overlay_workspace_bytes(1, -1) == 0
    assert lib.sd_overlay_workspace_bytes(3, 7) > lib.sd_overlay_workspace_bytes(3, 0) > 0
    for kw in (dict(thickness=0), dict(profile_thickness=33), dict(rw_bgr=(0, 0)), dict(edge_bgr=(0, 0, 256))):
        with pytest.raises(ValueError):
            outputs.OverlayLines(**kw)
    with pytest.raises(ValueError):
        outputs.draw_lines(img, np.zeros((1,), outputs.SEG_DTYPE))      # thickness 0


def _submit(outs, c, **more):
    rec = torch.from_numpy(np.ascontiguousarray(c["records"]).view(np.uint8).reshape(c["B"], RW_DTYPE.itemsize).copy())
    outs.submit(0, rec, (c["h"], c["w"]), **more)
    return outs.close()


def test_sequence_outputs_lines_choice(tmp_path):
    c = O.case("profile_seven")
    names = [f"frame_{i}" for i in range(c["B"])]
    kw = dict(images=False, ply=False, threads=2)
    plain = outputs.SequenceOutputs(str(tmp_path / "plain"), names, **kw)
    off = outputs.SequenceOutputs(str(tmp_path / "off"), names, lines=None, **kw)
    off.configure(lines=None)
    m0, m1 = json.load(open(_submit(plain, c))), json.load(open(_submit(off, c)))
    assert m0 == m1 and "lines" not in m0 and "lines_flagged" not in m0
    for nm in names:
        a, b = (open(os.path.join(str(tmp_path / k), outputs.SEQ_IMG_DIR, nm + "_overlay.json"), "rb").read() for k in ("plain", "off"))
        assert a == b and b"lines" not in a
    for bad in ("draw", True, dict(thickness=3)):
        with pytest.raises(ValueError):
            outputs.SequenceOutputs(str(tmp_path / "bad"), names, lines=bad, **kw)
        with pytest.raises(ValueError):
            outputs.SequenceOutputs(str(tmp_path / "bad2"), names, **kw).configure(lines=bad)
    on = outputs.SequenceOutputs(str(tmp_path / "on"), names, profile=list(np.linspace(5.0, 40.0, 7)), **kw)
    on.set_lines(c["lines"])
    with pytest.raises(ValueError):                                      # the cameras and the network size are needed
        on.submit(0, torch.zeros((c["B"], RW_DTYPE.itemsize), dtype=torch.uint8), (c["h"], c["w"]),
                  profile=torch.zeros((c["B"], 7, 48), dtype=torch.uint8))
    raw = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(a.shape + (a.dtype.itemsize,)).copy())      # noqa: E731
    m = json.load(open(_submit(on, c, profile=raw(c["profile"]), f2f_profile=raw(c["f2f_profile"]), f2f=raw(c["f2f"]), cams=c["cams"], net_size=O.NET)))
    with pytest.raises(RuntimeError):
        on.set_lines(c["lines"])                                         # after the first batch
    assert m["lines"] == c["lines"].as_dict() and m["lines_flagged"] == [names[b] for b in range(c["B"]) if c["flags"][b]]
    assert {k: v for k, v in m.items() if k not in ("lines", "lines_flagged", "profile", "profile_depths", "files")} == \
        {k: v for k, v in m0.items() if k != "files"}
    clip = int(0.25 * c["h"])
    for b, nm in enumerate(names):
        doc = json.load(open(os.path.join(str(tmp_path / "on"), outputs.SEQ_IMG_DIR, nm + "_overlay.json")))
        c2 = dict(c, clip_top=clip)
        assert doc["lines"] == outputs.segments_json(O.host_segments(c2, b)[0]) and len(doc["lines"]) > 0
        plain_doc = json.load(open(os.path.join(str(tmp_path / "plain"), outputs.SEQ_IMG_DIR, nm + "_overlay.json")))
        assert {k: v for k, v in doc.items() if k != "lines"} == plain_doc


def test_save_frame_outputs_draws_the_lines(tmp_path):
    rng = np.random.default_rng(3)
    size = (256, 512)                                                    # the segmented frame comes at the size of the files: no resize, no GPU
    cam = Camera(cx=1048.64 / 4, cy=519.277 / 4, f=145.0, b=0.22, disp_mult=3800.0)
    frame = O.prefilled(4, *size, 3)
    rec = np.zeros((), RW_DTYPE)
    rec["found"], rec["width"] = 1, 4.41
    rec["left_pt"] = O.point_at(cam, size, 0.2, 0.6, 10.0, net=size).astype(np.float32)
    rec["right_pt"] = O.point_at(cam, size, 0.8, 0.6, 10.0, net=size).astype(np.float32)
    pts = rng.normal(size=(50, 3)).astype(np.float32) + np.float32([0, 1.5, 9])
    res = dict(record=rec, dist_rw=4.41, road3D_final=pts, road_colors_final=rng.integers(0, 256, (50, 3), dtype=np.uint8))
    runs = {}
    for key, kw in (("default", {}), ("off", dict(lines=None, camera=cam)), ("on", dict(lines=outputs.OverlayLines(), camera=cam)),
                    ("on_text", dict(lines=outputs.OverlayLines(), camera=cam, text="draw"))):
        d = tmp_path / key
        d.mkdir()
        files = outputs.save_frame_outputs(str(d / "f"), res, 10.0, segmented_frame=frame, is_city=True, **kw)
        runs[key] = {os.path.basename(p): open(p, "rb").read() for p in files}
    assert runs["default"] == runs["off"]
    for name, data in runs["on"].items():
        assert (data == runs["default"][name]) == (name not in ("f.png", "f_overlay.json")), name
    plain = frame_io.imread(str(tmp_path / "default" / "f.png"))
    segs, flag = outputs.overlay_segments(rec, cam, size, size, clip_top=int(0.2 * 256))
    want = outputs.draw_lines(plain, segs, int(0.2 * 256))
    assert flag == 0 and len(segs) == 1 and (want != plain).any()
    assert np.array_equal(frame_io.imread(str(tmp_path / "on" / "f.png")), want)
    doc = json.load(open(str(tmp_path / "on" / "f_overlay.json")))
    assert doc["lines"] == outputs.segments_json(segs)
    items = outputs.overlay_items(512, 256, 10.0, True, rec["left_pt"].astype(np.float64)[None, :], rec["right_pt"].astype(np.float64)[None, :], 4.41)[1]
    assert np.array_equal(frame_io.imread(str(tmp_path / "on_text" / "f.png")), outputs.draw_text(want, items))      # the text goes over the lines
    for kw in (dict(lines=outputs.OverlayLines()), dict(lines=outputs.OverlayLines(), camera=cam, segmented_frame=None), dict(lines="on", camera=cam)):
        with pytest.raises(ValueError):
            outputs.save_frame_outputs(str(tmp_path / "x"), res, 10.0, **dict(dict(segmented_frame=frame), **kw))
    assert not [p for p in os.listdir(tmp_path) if p.startswith("x")]
