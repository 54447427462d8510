"""CPU: what the step of make_engine_step launches, and in which order, for every combination of the output choices -- the contract of
its docstring, checked against a recording stand-in for the Engine; and the keywords SequenceOutputs.submit gets from it.  The rules are
written out here from that docstring; nothing is computed by running the step twice."""
import itertools

import numpy as np
import torch

from semantic_depth_amd import outputs
from semantic_depth_amd.distributed import make_engine_step
from semantic_depth_amd.engine import Camera

N, H, W = 2, 8, 16                                         # frames per batch, the network size
SIZE = (2 * H, 2 * W)                                      # the original frames: the step resizes them
CAMS = [Camera(cx=8.0, cy=4.0, f=10.0, b=0.22, disp_mult=3800.0), Camera(cx=8.5, cy=4.5, f=11.0, b=0.22, disp_mult=2048.0)]
RENDER = outputs.top_camera(12, 10)
CHOICES = dict(png=("host", "device"), ply=(False, "host", "device"), text=("json", "draw"), render=(None, RENDER),
               video=(None, "host", "device"), disp=(None, "gray"), lines=(None, outputs.OverlayLines()), profile=(None, [8.0, 10.0]),
               images=(True, False), approach=("rw", "both"))


class RecordingEngine:
    """an Engine that launches nothing: every method returns new small tensors of the right shapes for N frames and appends
    (its name, the label of its image argument, what else the rules ask about) to ``log``"""
    device, H, W, on_range = "cpu", H, W, "raise"

    def __init__(self):
        self.log, self._labels, self._kept = [], {}, []

    def made(self, label, *shape, dtype=torch.uint8):
        t = torch.zeros(shape, dtype=dtype)
        self._labels[id(t)] = label
        self._kept.append(t)                               # (alive, so that no id comes twice)
        return t

    def _note(self, name, image, **more):
        self.log.append((name, self._labels.get(id(image), "?"), more))

    def resize_cubic(self, fr):
        self._note("resize_cubic", fr)
        return self.made("resized", N, H, W, 3)

    def process_batch(self, fr, cams, prm, approach="rw", want_final=False, depths=None):
        self._note("process_batch", fr, want_final=want_final, depths=depths, approach=approach)
        out = dict(records=self.made("records", N, 104), seg=dict(road=self.made("road", N, H, W), fence=self.made("fence", N, H, W)),
                   disp_pp=self.made("disp_pp", N, H, W, dtype=torch.float32), f2f=None)
        if want_final:
            out["road_final"] = dict(xyz=self.made("xyz", N, 5, 3, dtype=torch.float32), rgb=self.made("rgb", N, 5, 3),
                                     n=self.made("n", N, dtype=torch.int32))
            self._labels[id(out["road_final"])] = "road_final"
            self._kept.append(out["road_final"])
        if depths is not None:
            out["profile"] = self.made("profile", N, len(depths), 48)
        if approach == "both":
            out["f2f"] = self.made("f2f", N, 152)
            if depths is not None:
                out["f2f_profile"] = self.made("f2f_profile", N, len(depths), 64)
        return out

    def format_rw_ply(self, final, rec):
        self._note("format_rw_ply", final)
        return self.made("ply_text", 64), self.made("ply_offsets", N + 1, dtype=torch.int64), self.made("ply_flags", N, dtype=torch.int32)

    def render_rw(self, final, rec, camera):
        self._note("render_rw", final, camera=camera)
        return self.made("renders", N, camera.height, camera.width, 3), self.made("render_flags", N, dtype=torch.int32)

    def disparity_image(self, disp, h, w, cmap, mults=None):
        self._note("disparity_image", disp, size=(h, w), cmap=cmap, mults=list(mults))
        return self.made("disp_images", N, h, w, 3), self.made("disp_flags", N, dtype=torch.int32)

    def compose_result_frames(self, fr, road, fence, rec, h, w, *colours):
        self._note("compose_result_frames", fr, size=(h, w))
        return self.made("composed", N, h, w, 3)

    def draw_result_lines(self, images, rec, cams, lines, f2f=None, profile=None, f2f_profile=None, clip_top=0):
        self._note("draw_result_lines", images, clip_top=clip_top, f2f=f2f is not None, profile=profile is not None,
                   f2f_profile=f2f_profile is not None)
        return images, self.made("lines_flags", N, dtype=torch.int32)

    def draw_result_text(self, images, rec, depth):
        self._note("draw_result_text", images)
        return images

    def encode_jpeg(self, images, quality, stream_stride=0):
        self._note("encode_jpeg", images, stride=stream_stride, quality=quality)
        return self.made("jpeg_streams", N, 8), self.made("jpeg_sizes", N, dtype=torch.int64), self.made("jpeg_flags", N, dtype=torch.int32)

    def encode_png(self, images):
        label = self._labels.get(id(images), "?")
        self._note("encode_png", images)
        return self.made("png_of_" + label, N, 8), self.made("png_sizes_of_" + label, N, dtype=torch.int64)

    def label(self, value):
        """the label of a tensor this engine made; of a tuple of them, its first one's"""
        return self._labels.get(id(value[0] if isinstance(value, tuple) else value), "?")


def cases():
    for values in itertools.product(*CHOICES.values()):
        yield dict(zip(CHOICES, values))


def run_case(cfg, directory):
    """one batch through the step for the choices ``cfg``.  Returns (the engine's log, keyword -> label of what submit got under it, None
    for a keyword given as None), or None when configure refuses the combination"""
    video = cfg["video"] and outputs.Video(fps=25, quality=80, route=cfg["video"])
    try:
        outs = outputs.SequenceOutputs(str(directory), ["a", "b"], images=cfg["images"], ply=cfg["ply"], png=cfg["png"], text=cfg["text"],
                                       render=cfg["render"], video=video, disp=cfg["disp"], lines=cfg["lines"], profile=cfg["profile"])
    except ValueError:
        return None
    engine, got = RecordingEngine(), {}

    def submit(lo, records, size, **kw):
        assert (lo, tuple(size)) == (0, SIZE) and engine.label(records) == "records"
        got.update({k: None if v is None else "cams" if k == "cams" else tuple(v) if k == "net_size" else engine.label(v) for k, v in kw.items()})

    outs.submit = submit
    try:
        rec = make_engine_step(engine, lambda i: CAMS[i], approach=cfg["approach"], outputs=outs)(engine.made("frames", N, *SIZE, 3), 0)
        assert engine.label(rec) == "records"
    finally:
        outs.close()
    return engine.log, got


def expected(cfg):
    """(the launches in order as (name, label of the image argument), the non-None submit keywords -> label), from the docstring of
    make_engine_step and SequenceOutputs.submit"""
    device_png, both = cfg["png"] == "device", cfg["approach"] == "both"
    calls = [("resize_cubic", "frames"), ("process_batch", "resized")]
    kw = {}
    if cfg["ply"]:
        kw["final"] = "road_final"
    if cfg["profile"]:
        kw["profile"] = "profile"
        if both:
            kw["f2f_profile"] = "f2f_profile"
    if cfg["ply"] == "device":
        calls.append(("format_rw_ply", "road_final"))
        kw["ply_text"] = "ply_text"
    for on, launch, source, label, raw, streams in ((cfg["render"], "render_rw", "road_final", "renders", "renders", "render_streams"),
                                                    (cfg["disp"], "disparity_image", "disp_pp", "disp_images", "disp_images", "disp_streams")):
        if on:
            calls.append((launch, source))
            if device_png:
                calls.append(("encode_png", label))
                kw[streams] = "png_of_" + label
            else:
                kw[raw] = label
    if cfg["disp"]:
        kw["disp_flags"] = "disp_flags"
    if cfg["images"] or cfg["video"]:
        calls.append(("compose_result_frames", "resized"))
        kw["images"] = "composed"
        if cfg["lines"]:
            calls.append(("draw_result_lines", "composed"))
            kw["lines_flags"] = "lines_flags"
        if cfg["text"] == "draw":
            calls.append(("draw_result_text", "composed"))
        if cfg["video"] == "device":
            calls.append(("encode_jpeg", "composed"))
            kw["video_streams"] = "jpeg_streams"
        if cfg["images"] and device_png:
            calls.append(("encode_png", "composed"))
            kw["png_streams"] = "png_of_composed"
    if cfg["lines"]:
        kw.update(cams="cams", net_size=(H, W))
        if both:
            kw["f2f"] = "f2f"
    return calls, kw


def test_the_step_launches_what_its_docstring_promises_in_that_order(tmp_path):
    ran = refused = 0
    for cfg in cases():
        result = run_case(cfg, tmp_path)
        if result is None:                                 # configure refuses exactly: no raw image reaches the host for the host video route
            assert cfg["png"] == "device" and cfg["video"] == "host", cfg
            refused += 1
            continue
        assert not (cfg["png"] == "device" and cfg["video"] == "host"), cfg
        ran += 1
        log, got = result
        calls, kw = expected(cfg)
        assert [(name, image) for name, image, _ in log] == calls, cfg
        assert {k: v for k, v in got.items() if v is not None} == kw, cfg
        more = {name: m for name, _, m in log}             # (encode_png, the one name that comes more than once, carries nothing more)
        assert more["process_batch"] == dict(want_final=bool(cfg["ply"]) or cfg["render"] is not None, depths=cfg["profile"],
                                             approach=cfg["approach"]), cfg
        if cfg["render"]:
            assert more["render_rw"]["camera"] is RENDER
        if cfg["disp"]:
            assert more["disparity_image"] == dict(size=SIZE, cmap="gray", mults=[3800.0, 2048.0]), cfg
        if "compose_result_frames" in more:
            assert more["compose_result_frames"]["size"] == SIZE
        if "draw_result_lines" in more:
            assert more["draw_result_lines"] == dict(clip_top=int(0.25 * SIZE[0]), f2f=cfg["approach"] == "both", profile=bool(cfg["profile"]),
                                                     f2f_profile=bool(cfg["profile"]) and cfg["approach"] == "both"), cfg
        if "encode_jpeg" in more:
            assert more["encode_jpeg"] == dict(stride=1024 + SIZE[0] * SIZE[1] * 3 // 2, quality=80), cfg
    total = int(np.prod([len(v) for v in CHOICES.values()]))
    assert total == 2304 and refused == total // 6 and ran == total - refused
