"""CPU: the host statement of the rendered clouds (sd_render_rw_host through csrc/render_rule.hpp) against an independent numpy statement
of the rule of include/semdepth.h on every byte (tests/render_cases.py), the camera file, top_camera, the refusals, the struct's size, the
single-frame tool's file, and the guard that a run without render= writes what it wrote before."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import __graft_entry__ as graft
import render_cases as R
from semantic_depth_amd import _lib as L
from semantic_depth_amd import frame_io, outputs
from semantic_depth_amd.engine import RW_DTYPE


@pytest.fixture(scope="module")
def results():
    """every case once: (host image, host flag, reference image)"""
    graft.build()
    out = {}
    for c in R.all_cases():
        st, img, flag = R.host(c)
        assert st == L.SD_OK, c["name"]
        out[c["name"]] = (img, flag, R.reference(c), c)
    return out


def test_host_statement_equals_the_numpy_statement_on_every_case(results):
    assert len(results) == len(R.all_cases())                            # (the names are unique)
    for name, (img, flag, ref, c) in results.items():
        assert flag == 0, name
        assert np.array_equal(img, ref), (name, int((img != ref).any(-1).sum()))


def _drawn(img, cam):
    return (img != np.asarray(cam.background, np.uint8)).any(-1)


def test_the_cases_show_what_they_are_about(results):
    def get(name):
        img, _, _, c = results[name]
        return img, c

    for name in ("slanted_0", "top_0", "all_rows_one_z", "rows_behind_the_camera"):
        img, c = get(name)
        if name == "rows_behind_the_camera":
            assert 0 < _drawn(img, c["cam"]).sum()                       # the other half of the cloud is in view
        else:
            assert not _drawn(img, c["cam"]).any(), name
    for name in ("slanted_1", "top_1"):                                  # the only row is the minimum
        assert not _drawn(*[get(name)[0], get(name)[1]["cam"]]).any()
    for name in ("slanted_300", "top_300", f"slanted_{R.CAP}", f"top_{R.CAP}"):
        img, c = get(name)
        assert _drawn(img, c["cam"]).sum() > 200 and R.line_pixels(img) == 0, name
    for name in ("slanted_0_line", "top_0_line", "top_300_line", "one_z_line_above"):
        assert R.line_pixels(get(name)[0]) > 50, name
    # the square grows with the point size
    drawn = [int(_drawn(*[get(f"point_size_{s}_top")[0], get(f"point_size_{s}_top")[1]["cam"]]).sum()) for s in (1, 4, 5, 16)]
    assert drawn == sorted(drawn) and drawn[0] < drawn[1] < drawn[2] < drawn[3]
    # equal depth: the lower row index; different depth: the nearer row, in both orders
    red, green = [10, 10, 200], [10, 200, 10]                            # BGR
    assert (get("tie_lower_index_wins")[0][23, 31] == red).all() and (get("tie_lower_index_wins_swapped")[0][23, 31] == green).all()
    assert (get("near_then_far")[0][23, 31] == red).all() and (get("far_then_near")[0][23, 31] == green).all()
    for name in ("tie_lower_index_wins", "near_then_far", "far_then_near"):
        img, c = get(name)
        assert _drawn(img, c["cam"]).sum() == 16 and _drawn(img, c["cam"])[22:26, 30:34].all()          # point size 4: one before, two behind
    assert _drawn(*[get("z_at_the_near_plane")[0], get("z_at_the_near_plane")[1]["cam"]]).sum() == 9
    assert not _drawn(*[get("z_below_the_near_plane")[0], get("z_below_the_near_plane")[1]["cam"]]).any()
    # the borders: what shows of a square of side s around px
    w, h = 23, 17
    for s in (1, 4, 5, 16):
        lo, hi = (s - 1) // 2, s // 2
        shown = [int(_drawn(*[get(f"border_x_{s}_{k}")[0], get(f"border_x_{s}_{k}")[1]["cam"]]).any(0).sum()) for k in range(10)]
        # u = -s (px = -s: out of reach), beyond the rule, the first column alone by one pixel less than reach, ..., the last column, beyond
        assert shown[0] == 0 and shown[1] == 0 and shown[9] == 0 and shown[8] == 0, (s, shown)
        assert shown[2] == 0 and shown[3] == 1 and shown[4] == hi + 1 and shown[5] == lo + 1 and shown[6] == 1 and shown[7] == 0, (s, shown)
        rows = [int(_drawn(*[get(f"border_y_{s}_{k}")[0], get(f"border_y_{s}_{k}")[1]["cam"]]).any(1).sum()) for k in range(10)]
        assert rows == shown, (s, rows, shown)
        img, c = get(f"corners_{s}")
        d = _drawn(img, c["cam"])
        assert d.sum() == 4 and d[0, 0] and d[0, w - 1] and d[h - 1, 0] and d[h - 1, w - 1], s
        assert (img[0, 0] == [3, 2, 1]).all() and (img[h - 1, w - 1] == [12, 11, 10]).all()
    # the line over the cloud hides it; under the cloud it shows only where the cloud has no point
    over, under = R.line_pixels(get("line_in_front_of_the_cloud")[0]), R.line_pixels(get("line_behind_the_cloud")[0])
    assert under > 0 and over > 2 * under and R.line_pixels(get("no_line_found_0")[0]) == 0, (over, under)
    # a non-finite row is skipped and flags nothing; the finite rows of the frame are drawn
    img, c = get("non_finite_rows")
    assert _drawn(img, c["cam"]).sum() > 200 and R.line_pixels(img) > 50
    assert R.line_pixels(get("nan_end_point")[0]) == 0


def test_a_count_outside_the_cloud_flags_the_frame():
    c = R.case("bad_count", R.cloud(1, 20), R.top(40, 30, background=(1, 2, 3)), rec=R.LINE)
    st, img, flag = R.host(c, n=-1)
    assert st == L.SD_OK and flag == 1 and (img == [1, 2, 3]).all()
    st, img, flag = R.host(c)
    assert st == L.SD_OK and flag == 0 and (img != [1, 2, 3]).any()


def test_camera_json_round_trip_is_column_major(tmp_path):
    cam = R.slanted_camera(53, 37, z_near=0.25, point_size=3, background=(1, 2, 3))
    path = cam.to_open3d_json(str(tmp_path / "view.json"))
    d = json.load(open(path))
    e = np.asarray(cam.ext).reshape(3, 4)
    assert d["class_name"] == "PinholeCameraParameters" and len(d["extrinsic"]) == 16 and len(d["intrinsic"]["intrinsic_matrix"]) == 9
    # column by column: the first four numbers are the first COLUMN of the 4 x 4 matrix, the last four the translation and 1
    assert d["extrinsic"][:4] == [e[0, 0], e[1, 0], e[2, 0], 0.0] and d["extrinsic"][12:] == [e[0, 3], e[1, 3], e[2, 3], 1.0]
    assert not np.allclose(e[:, :3], e[:, :3].T)                         # a transposed read would show
    assert d["intrinsic"]["intrinsic_matrix"] == [cam.fx, 0.0, 0.0, 0.0, cam.fy, 0.0, cam.cx, cam.cy, 1.0]
    assert (d["intrinsic"]["width"], d["intrinsic"]["height"]) == (53, 37)
    back = outputs.RenderCamera.from_open3d_json(path, z_near=0.25, point_size=3, background=(1, 2, 3))
    assert back == cam
    # a file as Open3D writes it, by hand: identity rotation, translation (1, 2, 3)
    hand = dict(class_name="PinholeCameraParameters", extrinsic=[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 1, 2, 3, 1],
                intrinsic=dict(height=480, width=640, intrinsic_matrix=[500.0, 0, 0, 0, 510.0, 0, 319.5, 239.5, 1]), version_major=1, version_minor=0)
    json.dump(hand, open(tmp_path / "hand.json", "w"))
    got = outputs.RenderCamera.from_open3d_json(str(tmp_path / "hand.json"))
    assert got.ext == (1, 0, 0, 1, 0, 1, 0, 2, 0, 0, 1, 3) and (got.fx, got.fy, got.cx, got.cy) == (500.0, 510.0, 319.5, 239.5)
    assert (got.width, got.height, got.point_size, got.background) == (640, 480, 5, (255, 255, 255))


def test_top_camera_centres_and_puts_far_at_the_top():
    graft.build()
    for w, h, centre in ((512, 512, (0.0, 0.0, 20.0)), (96, 64, (1.5, 0.5, 12.0)), (53, 37, (0.0, 1.5, 20.0))):
        cam = outputs.top_camera(w, h, centre=centre, point_size=1)
        assert cam.cx == w / 2 - 0.5 and cam.cy == h / 2 - 0.5 and cam.fx == cam.fy == pytest.approx((w / 2) / np.tan(np.pi / 6))
        cx, cy, cz = centre
        pts = np.float32([[cx, cy, cz - 100.0], [cx, cy, cz], [cx, cy, cz + 3.0], [cx + 3.0, cy, cz]])         # row 0 is the minimum and goes
        img = outputs.render_rw(pts, [[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0]], camera=cam)
        where = {int(img[y, x, 2]): (int(y), int(x)) for y, x in np.argwhere((img != 255).any(-1))}
        assert sorted(where) == [1, 2, 3]
        assert where[1] == (int(np.floor(cam.cy)), int(np.floor(cam.cx)))                                   # the centre, on the central pixel
        assert where[2][1] == where[1][1] and where[2][0] < where[1][0]                                     # farther in z: above it
        assert where[3][0] == where[1][0] and where[3][1] > where[1][1]                                     # world x is image x


def _raw_host(cam_struct, n=3, null=None):
    xyz, rgb = np.zeros((3, 3), np.float32), np.zeros((3, 3), np.uint8)
    out = np.full(cam_struct.height * cam_struct.width * 3 if 0 < cam_struct.width <= 64 and 0 < cam_struct.height <= 64 else 64, 0xA5, np.uint8)
    rec, flag = L.sd_rw_result(), C.c_int32(-7)
    args = dict(xyz=xyz.ctypes.data_as(C.c_void_p), rgb=rgb.ctypes.data_as(C.c_void_p), rec=C.byref(rec), cam=C.byref(cam_struct),
                out=out.ctypes.data_as(C.c_void_p), flag=C.byref(flag))
    if null:
        args[null] = None
    st = L.load().sd_render_rw_host(args["xyz"], args["rgb"], n, args["rec"], args["cam"], args["out"], args["flag"])
    return st, out, flag.value


def test_argument_refusals():
    graft.build()
    good = R.top(16, 8)
    assert _raw_host(good.struct())[0] == L.SD_OK
    for null in ("xyz", "rgb", "rec", "cam", "out", "flag"):
        st, out, flag = _raw_host(good.struct(), null=null)
        assert st == L.SD_ERR_INVALID and (out == 0xA5).all() and flag == -7, null
    assert _raw_host(good.struct(), n=0, null="xyz")[0] == L.SD_OK       # an empty cloud needs no arrays
    need = C.c_size_t(7)
    lib = L.load()
    for field, value in (("width", 0), ("width", 16385), ("height", 0), ("height", 16385), ("point_size", 0), ("point_size", 17),
                         ("z_near", 0.0), ("z_near", -1.0), ("z_near", np.nan), ("z_near", np.inf), ("fx", np.nan), ("fy", np.inf),
                         ("cx", -np.inf), ("cy", np.nan)):
        cam = good.struct()
        setattr(cam, field, value)
        st, out, flag = _raw_host(cam)
        assert st == L.SD_ERR_INVALID and (out == 0xA5).all() and flag == -7, (field, value)
        assert lib.sd_render_workspace(2, 100, C.byref(cam), C.byref(need)) == L.SD_ERR_INVALID and need.value == 7, (field, value)
    for i in (0, 5, 11):
        cam = good.struct()
        cam.ext[i] = np.nan
        assert _raw_host(cam)[0] == L.SD_ERR_INVALID
    cam = good.struct()
    for B, cap in ((0, 10), (65536, 10), (1, -1)):
        assert lib.sd_render_workspace(B, cap, C.byref(cam), C.byref(need)) == L.SD_ERR_INVALID and need.value == 7
    assert lib.sd_render_workspace(1, 10, None, C.byref(need)) == L.SD_ERR_INVALID and lib.sd_render_workspace(1, 10, C.byref(cam), None) == L.SD_ERR_INVALID
    assert lib.sd_render_workspace(3, 300, C.byref(cam), C.byref(need)) == L.SD_OK
    assert need.value >= 3 * 16 * 8 * 8 and need.value % 8 == 0          # the keys: eight bytes per pixel per frame
    with pytest.raises(ValueError):
        outputs.render_rw(np.zeros((1, 3)), np.zeros((1, 3)), camera=outputs.top_camera(16, 8, point_size=17))
    with pytest.raises(ValueError):
        outputs.SequenceOutputs(".", [], render="top")


def test_sizeof_sd_render_camera():
    assert C.sizeof(L.sd_render_camera) == 12 * 8 + 5 * 8 + 3 * 4 + 4 == 152
    assert L.sd_render_camera.background.offset == 148 and L.sd_render_camera.width.offset == 136
    assert (L.SD_RENDER_MAX_EXTENT, L.SD_RENDER_MAX_POINT) == (16384, 16)


def _result():
    rng = np.random.default_rng(3)
    rec = np.zeros((), RW_DTYPE)
    rec["found"] = 1
    rec["left_pt"], rec["right_pt"] = (-3.4150002, 1.6, 10.0), (0.995, 1.6, 10.0)
    rec["width"] = 4.41000023
    pts = (rng.random((400, 3)) * [10.0, 0.3, 12.0] + [-5.0, 1.5, 5.0]).astype(np.float32)
    return dict(record=rec, dist_rw=4.41000023, road3D_final=pts, road_colors_final=rng.integers(0, 250, (400, 3), dtype=np.uint8))


def test_save_frame_outputs_writes_the_render(tmp_path):
    graft.build()
    res = _result()
    cam = outputs.top_camera(160, 120, centre=(0.0, 0.0, 10.0), altitude=20.0)
    runs = {}
    for key, kw in (("default", {}), ("none", dict(render=None)), ("render", dict(render=cam))):
        d = tmp_path / key
        d.mkdir()
        files = outputs.save_frame_outputs(str(d / "f"), res, 10.0, **kw)
        runs[key] = {os.path.basename(p): open(p, "rb").read() for p in files}
    assert runs["default"] == runs["none"]
    assert sorted(runs["render"]) == sorted(list(runs["default"]) + ["f_render.png"])
    assert all(runs["render"][k] == v for k, v in runs["default"].items())
    want = outputs.render_rw(res["road3D_final"], res["road_colors_final"], res["record"]["left_pt"], res["record"]["right_pt"], cam)
    assert np.array_equal(frame_io.imread(str(tmp_path / "render" / "f_render.png")), want)
    assert R.line_pixels(want) > 20 and (want != 255).any(-1).sum() > 500
    with pytest.raises(ValueError):
        outputs.save_frame_outputs(str(tmp_path / "x"), res, 10.0, render="top")


def _stub_run(directory, render_kw, renders=None):
    """one batch of three frames through SequenceOutputs from host arrays, as a step would submit them"""
    names = ["a_000", "a_001", "a_002"]
    outs = outputs.SequenceOutputs(str(directory), names, threads=2, **render_kw)
    recs = np.zeros(3, RW_DTYPE)
    recs["found"] = [1, 0, 1]
    recs["left_pt"], recs["right_pt"], recs["width"] = (-2.0, 1.5, 10.0), (2.5, 1.5, 10.0), 4.5
    rng = np.random.default_rng(5)
    import torch
    final = dict(xyz=torch.from_numpy(R.cloud(3, 3 * 40).reshape(3, 40, 3)), rgb=torch.from_numpy(rng.integers(0, 250, (3, 40, 3), dtype=np.uint8)),
                 n=torch.tensor([40, 0, 17], dtype=torch.int32))
    images = torch.from_numpy(rng.integers(0, 256, (3, 24, 32, 3), dtype=np.uint8))
    more = {} if renders is None else dict(renders=torch.from_numpy(renders))
    try:
        outs.submit(0, torch.from_numpy(recs.view(np.uint8).reshape(3, -1).copy()), (24, 32), images=images, final=final, **more)
    finally:
        manifest = outs.close()
    tree = {os.path.relpath(os.path.join(r, f), directory): open(os.path.join(r, f), "rb").read() for r, _, fs in os.walk(directory) for f in fs}
    return manifest, tree, (recs, final)


def test_the_default_run_writes_what_it_wrote(tmp_path):
    """the guard: render=None is a run without the keyword -- the same file set and the same manifest bytes; with a camera the only additions
    are the _render.png files and the manifest's 'render' list"""
    graft.build()
    _, plain, _ = _stub_run(tmp_path / "plain", {})
    _, none, (recs, final) = _stub_run(tmp_path / "none", dict(render=None))
    assert plain == none and "manifest_rank0.json" in plain and len(plain) == 1 + 3 * 3
    assert b"render" not in plain["manifest_rank0.json"]
    cam = R.top(48, 40)
    want = np.stack([outputs.render_rw(final["xyz"][i, :int(final["n"][i])].numpy(), final["rgb"][i, :int(final["n"][i])].numpy(),
                                       recs[i]["left_pt"] if recs[i]["found"] else None, recs[i]["right_pt"] if recs[i]["found"] else None, cam)
                     for i in range(3)])
    with pytest.raises(ValueError):
        _stub_run(tmp_path / "missing", dict(render=cam))                # a camera, but the step handed no renders over
    _, with_render, _ = _stub_run(tmp_path / "render", dict(render=cam), renders=want)
    added = sorted(set(with_render) - set(plain))
    assert added == [os.path.join(outputs.SEQ_RENDER_DIR, f"a_00{i}_render.png") for i in range(3)]
    assert all(with_render[k] == v for k, v in plain.items() if k != "manifest_rank0.json")
    m_plain, m_render = json.loads(plain["manifest_rank0.json"]), json.loads(with_render["manifest_rank0.json"])
    assert m_render["render"] == added and set(m_render["files"]) - set(m_plain["files"]) == set(added)
    assert {k: v for k, v in m_render.items() if k not in ("render", "files")} == {k: v for k, v in m_plain.items() if k != "files"}
    for i, rel in enumerate(added):
        assert np.array_equal(frame_io.imread(str(tmp_path / "render" / rel)), want[i]), rel
    assert (want[0] != 255).any() and (want[1] == 255).all()             # frame 1: no point and no line
