"""CPU: save_frame_outputs(text="draw") writes the annotated image with its items rasterised (outputs.draw_text); the default call's files
are what they were."""
import os

import numpy as np
import pytest

import __graft_entry__ as graft
import text_cases as T
from semantic_depth_amd import frame_io, outputs


def _result():
    rng = np.random.default_rng(3)
    pts = rng.normal(size=(50, 3)).astype(np.float32) + np.float32([0, 1.5, 9])
    return dict(record=T.record(), dist_rw=4.41000023, road3D_final=pts, road_colors_final=rng.integers(0, 256, (50, 3), dtype=np.uint8))


@pytest.mark.parametrize("is_city", [True, False])
def test_save_frame_outputs_draws_the_items(tmp_path, is_city):
    graft.build()
    frame = T.prefilled(4, 256, 1024, 3) if is_city else T.prefilled(4, 600, 2000, 3)
    res = _result()
    runs = {}
    for key, kw in (("default", {}), ("json", dict(text="json")), ("draw", dict(text="draw"))):
        d = tmp_path / key
        d.mkdir()
        files = outputs.save_frame_outputs(str(d / "f"), res, 10.0, segmented_frame=frame, is_city=is_city, **kw)
        runs[key] = {os.path.basename(p): open(p, "rb").read() for p in files}
    assert runs["default"] == runs["json"]
    assert sorted(runs["draw"]) == sorted(runs["default"])
    for name, data in runs["draw"].items():
        assert (data == runs["default"][name]) == (name != "f.png"), name
    h, w = frame.shape[:2]
    banner, items = outputs.overlay_items(w, h, 10.0, is_city, res["record"]["left_pt"].astype(np.float64)[None, :],
                                          res["record"]["right_pt"].astype(np.float64)[None, :], res["dist_rw"])
    plain, _ = outputs.draw_overlay(frame, banner, items)
    want = outputs.draw_text(plain, items)
    assert items[0]["thickness"] == (2 if is_city else 5) and (want != plain).any()
    assert np.array_equal(frame_io.imread(str(tmp_path / "draw" / "f.png")), want)
    assert np.array_equal(frame_io.imread(str(tmp_path / "default" / "f.png")), plain)
    assert np.array_equal(want, T.reference_draw(plain, items))
    with pytest.raises(ValueError):
        outputs.save_frame_outputs(str(tmp_path / "x"), res, 10.0, segmented_frame=frame, text="putText")


@pytest.mark.parametrize("name,found", T.SAMPLES)
def test_the_rendered_samples_are_what_the_rasteriser_draws(golden_dir, name, found):
    """tests/golden/text_sample_*.png show both layouts at 1024 x 2048; they stay the pixels of today's font and rule"""
    graft.build()
    assert np.array_equal(frame_io.imread(os.path.join(golden_dir, name)), T.sample_image(found))
