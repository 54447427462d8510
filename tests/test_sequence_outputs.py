"""CPU: the files of the sequence tool written from the batched driver (semantic_depth_cityscapes_sequence.py:303-361): the PIL-exact
overlay the compose kernel restates, the native PNG writer, the ``_rw.ply`` bytes, the output names, and a world-2 gloo run in which
every rank writes only its shard and a manifest."""
import json
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import __graft_entry__ as graft
from semantic_depth_amd import frame_io, outputs, pcl
from semantic_depth_amd.distributed import RECORD_BYTES, run_sequence_files, shard_range
from semantic_depth_amd.point_cloud_2_ply import PointCloud2Ply
from tests import sequence_ref as R


@pytest.fixture(scope="module", autouse=True)
def _built():
    graft.build()


# ------------------------------------------------------------------------------------------------ overlay arithmetic
@pytest.mark.parametrize("fence_color", [R.FENCE_SEQ, R.FENCE_SINGLE])
def test_numpy_paste_is_bit_identical_to_pillow(fence_color):
    pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(11)
    for h, w in ((37, 53), (64, 128)):
        frame = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        frame[0, :8] = [[0, 0, 0], [255, 255, 255], [1, 2, 3], [254, 253, 252], [128, 64, 128], [190, 153, 153], [127, 128, 129], [255, 0, 255]]
        road = rng.random((h, w)) < 0.4
        fence = rng.random((h, w)) < 0.3            # overlaps the road on ~12 % of the pixels: the fence blends over the pasted road
        road[0, :8] = fence[0, :8] = True
        want = R.pillow_paste(frame, road, fence, fence_color=fence_color)
        got = R.pil_paste(frame, road, fence, fence_color=fence_color)
        assert np.array_equal(got, want)
        assert np.array_equal(got[~(road | fence)], frame[~(road | fence)])


# ------------------------------------------------------------------------------------------------ PNG writer
@pytest.mark.parametrize("h,w", [(1, 1), (7, 13), (31, 1), (1, 33), (1024, 2048)])
def test_png_writer_round_trips_through_the_native_reader_and_pillow(tmp_path, h, w):
    PILImage = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(h * 7 + w)
    n = 3 if h * w < 10000 else 2
    frames = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    frames[0] = frames[0] // 32 * 32                 # (a compressible frame too)
    for level in ((0, 1, 9) if h * w < 10000 else (1,)):
        paths = [str(tmp_path / f"f{level}_{i}.png") for i in range(n)]
        assert outputs.write_png_batch(paths, frames, level=level, threads=2) == paths
        for i, p in enumerate(paths):
            assert np.array_equal(frame_io.imread(p), frames[i])
            with PILImage.open(p) as im:
                assert im.mode == "RGB" and im.size == (w, h)
                assert np.array_equal(np.asarray(im)[..., ::-1], frames[i])


def test_png_writer_reports_an_unwritable_path(tmp_path):
    frames = np.zeros((2, 4, 4, 3), np.uint8)
    with pytest.raises(OSError):
        outputs.write_png_batch([str(tmp_path / "ok.png"), str(tmp_path / "missing_dir" / "x.png")], frames)
    assert np.array_equal(frame_io.imread(str(tmp_path / "ok.png")), frames[0])


# ------------------------------------------------------------------------------------------------ _rw.ply
def _cloud(rng, n):
    xyz = np.stack([rng.uniform(-4, 4, n), rng.uniform(-1.5, 0.5, n), rng.uniform(3, 20, n)], 1).astype(np.float32).astype(np.float64)
    return xyz, rng.integers(0, 256, (n, 3), dtype=np.uint8)


@pytest.mark.parametrize("found", [False, True])
def test_rw_ply_bytes_equal_point_cloud_2_ply(tmp_path, found):
    """seq:357-361: PointCloud2Ply(road3D, road_colors, '<dir>/<name>_rw') [+ add_extra_point_cloud(line_rw, colors_line_rw)]"""
    rng = np.random.default_rng(5 + found)
    xyz, rgb = _cloud(rng, 5000)
    left = np.array([[-3.25, -1.0, 9.98]], np.float32).astype(np.float64) if found else None
    right = np.array([[2.5, -1.1, 9.98]], np.float32).astype(np.float64) if found else None
    pc = PointCloud2Ply(xyz, rgb, str(tmp_path / "frame_rw"))
    if found:
        line, colors_line = pcl.create_3Dline_from_3Dpoints(left.copy(), right.copy(), [250, 0, 0])
        pc.add_extra_point_cloud(line, colors_line)
    pc.prepare_and_save_point_cloud()
    want = open(tmp_path / "frame_rw.ply", "rb").read()
    assert outputs.rw_ply_bytes(xyz, rgb, left, right) == want
    assert left is None or left[0, 1] == -1.0            # (the end points of the caller are not mutated)


def test_rw_ply_of_an_empty_cloud_has_no_vertex():
    b = outputs.rw_ply_bytes(np.zeros((0, 3)), np.zeros((0, 3), np.uint8))
    assert b == PointCloud2Ply.ply_header.format(vertex_count=0).encode()


# ------------------------------------------------------------------------------------------------ names
def test_output_names_follow_the_reference():
    """seq:689-699: for input_frame in sorted(glob(...)): output_name = splitext(basename(input_frame))[0]"""
    paths = ["data/seq/stuttgart_02_000000_005200_leftImg8bit.png", "data/seq/stuttgart_02_000000_005176_leftImg8bit.png",
             "data/a/z.frame.jpg", "data/seq/x"]
    assert outputs.sequence_names(paths) == ["z.frame", "stuttgart_02_000000_005176_leftImg8bit", "stuttgart_02_000000_005200_leftImg8bit", "x"]


# ------------------------------------------------------------------------------------------------ the driver with a stub step
def _stub_records(first, n, h, w):
    from semantic_depth_amd.engine import RW_DTYPE
    rec = np.zeros(n, RW_DTYPE)
    rec["found"] = (np.arange(first, first + n) % 2 == 0).astype(np.int32)
    rec["width"] = 5.0 + 0.25 * np.arange(first, first + n)
    rec["left_pt"] = [-2.5, -1.0, 9.98]
    rec["right_pt"][:, 0] = rec["width"] - 2.5
    rec["right_pt"][:, 1:] = [-1.0, 9.98]
    return rec


def _stub_cloud(i):
    return _cloud(np.random.default_rng(100 + i), 50 + 7 * i)


def _stub_image(frame, i):
    return (frame.astype(np.int32) + i).astype(np.uint8)


def make_stub_step(outs):
    """stands in for make_engine_step(..., outputs=): per batch, the records, 'result images' and final road clouds it submits are
    functions of the global frame index (host tensors)"""
    def step(frames, first):
        n, h, w = frames.shape[:3]
        rec = _stub_records(first, n, h, w)
        imgs = torch.from_numpy(np.stack([_stub_image(frames[i].numpy(), first + i) for i in range(n)]))
        cap = max(len(_stub_cloud(first + i)[0]) for i in range(n))
        xyz, rgb, cnt = np.zeros((n, cap, 3), np.float32), np.zeros((n, cap, 3), np.uint8), np.zeros(n, np.int32)
        for i in range(n):
            x, c = _stub_cloud(first + i)
            xyz[i, :len(x)], rgb[i, :len(x)], cnt[i] = x, c, len(x)
        rbuf = torch.from_numpy(rec.view(np.uint8).reshape(-1, RECORD_BYTES).copy())
        outs.submit(first, rbuf, (h, w), images=imgs, final=dict(xyz=torch.from_numpy(xyz), rgb=torch.from_numpy(rgb), n=torch.from_numpy(cnt)))
        return rbuf
    step.outputs = outs
    return step


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _outputs_worker(rank, world, port, paths, out_dir, batch, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["LOCAL_WORLD_SIZE"] = str(world)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        outs = outputs.SequenceOutputs(out_dir, outputs.sequence_names(paths), depth=10.0, threads=2)
        run_sequence_files(paths, make_stub_step(outs), batch=batch, device="cpu", workers=2)
        q.put((rank, outs.manifest))
    finally:
        dist.destroy_process_group()


def _write_frames(tmp_path, n, h, w):
    rng = np.random.default_rng(9)
    frames = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    src = tmp_path / "in"
    src.mkdir()
    paths = [outputs.write_png(str(src / f"seq_{i:03d}_leftImg8bit.png"), frames[i]) for i in range(n)]
    return frames, paths


def _check_frame_files(out_dir, name, i, frame, h, w):
    img = frame_io.imread(os.path.join(out_dir, outputs.SEQ_IMG_DIR, name + ".png"))
    assert np.array_equal(img, _stub_image(frame, i))
    rec = _stub_records(i, 1, h, w)[0]
    left = rec["left_pt"].astype(np.float64)[None, :] if rec["found"] else None
    right = rec["right_pt"].astype(np.float64)[None, :] if rec["found"] else None
    xyz, rgb = _stub_cloud(i)
    ply = open(os.path.join(out_dir, outputs.SEQ_PLY_DIR, name + "_rw.ply"), "rb").read()
    assert ply == outputs.rw_ply_bytes(xyz.astype(np.float32).astype(np.float64), rgb, left, right)
    ov = json.load(open(os.path.join(out_dir, outputs.SEQ_IMG_DIR, name + "_overlay.json")))
    banner, items = outputs.overlay_items_sequence(w, h, 10.0, bool(rec["found"]), left, right, float(rec["width"]))
    assert ov == json.loads(json.dumps(dict(banner=banner, items=items)))
    assert (ov["banner"] is None) == (not rec["found"])


def test_sequence_outputs_world2_gloo_each_rank_writes_its_shard(tmp_path):
    n, h, w = 7, 24, 40
    frames, paths = _write_frames(tmp_path, n, h, w)
    out_dir = str(tmp_path / "out")
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_outputs_worker, args=(r, 2, port, paths[::-1], out_dir, 2, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=180) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    names = outputs.sequence_names(paths)
    union = []
    for rank, manifest in res:
        assert manifest == os.path.join(out_dir, f"manifest_rank{rank}.json")
        m = json.load(open(manifest))
        lo, hi = shard_range(n, rank, 2)
        assert m["status"] == "ok" and m["valid"] and m["frames"] == [lo, hi] and m["world"] == 2
        want = sorted(os.path.join(d, names[i] + sfx) for i in range(lo, hi)
                      for d, sfx in ((outputs.SEQ_IMG_DIR, ".png"), (outputs.SEQ_IMG_DIR, "_overlay.json"), (outputs.SEQ_PLY_DIR, "_rw.ply")))
        assert m["files"] == want
        union += m["files"]
    assert len(union) == len(set(union)) == 3 * n
    on_disk = sorted(os.path.join(d, f) for d in (outputs.SEQ_IMG_DIR, outputs.SEQ_PLY_DIR) for f in os.listdir(os.path.join(out_dir, d)))
    assert on_disk == sorted(union)
    for i in range(n):
        _check_frame_files(out_dir, names[i], i, frames[i], h, w)


def test_a_range_error_from_finish_raises_and_marks_the_manifest_invalid(tmp_path):
    from semantic_depth_amd.engine import RangeError
    n, h, w = 5, 8, 12
    frames, paths = _write_frames(tmp_path, n, h, w)
    out_dir = str(tmp_path / "out")
    outs = outputs.SequenceOutputs(out_dir, outputs.sequence_names(paths), threads=2, ply=False)
    step = make_stub_step(outs)                        # (the stub submits clouds too; the PLY files are not asked for)

    def finish():
        raise RangeError("3 activation values left the fp16 range")
    step.finish = finish
    with pytest.raises(RangeError):
        run_sequence_files(paths, step, batch=2, device="cpu", workers=1)
    m = json.load(open(os.path.join(out_dir, "manifest_rank0.json")))
    assert m["status"] == "range_error" and m["valid"] is False
    assert len(m["files"]) == 2 * n and not os.path.exists(os.path.join(out_dir, outputs.SEQ_PLY_DIR))


def test_outputs_off_leaves_the_driver_unchanged(tmp_path):
    n, h, w = 3, 8, 8
    frames, paths = _write_frames(tmp_path, n, h, w)

    def step(fr, first):
        return torch.from_numpy(_stub_records(first, fr.shape[0], h, w).view(np.uint8).reshape(-1, RECORD_BYTES).copy())
    step.outputs = None
    got = run_sequence_files(paths, step, batch=2, device="cpu", workers=1)
    assert torch.equal(got, torch.from_numpy(_stub_records(0, n, h, w).view(np.uint8).reshape(-1, RECORD_BYTES).copy()))
    assert sorted(os.listdir(tmp_path)) == ["in"]
