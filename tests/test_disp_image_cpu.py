"""CPU: the disparity images of include/semdepth.h on the host -- sd_disp_image_host against what scipy.misc.imresize + plt.imsave leave
(tests/golden/disp_image.npz, recorded by tests/golden/make_disp_image_golden.py), the two colour tables, the integer index rule against
matplotlib's float32 one, the numpy restatement of tests/disp_image_cases.py against the host twin on random maps with non-finite pixels,
the checker against five seeded mistakes, and SequenceOutputs(disp=) on host tensors.  Neither Pillow nor matplotlib is imported."""
import hashlib
import json
import os

import numpy as np
import pytest

import disp_image_cases as D
import png_device_cases as PN
import sequence_all_routes_cases as A
from semantic_depth_amd import frame_io, outputs

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "disp_image.npz")


@pytest.fixture(scope="module")
def golden():
    A.PD.lib()
    return np.load(GOLDEN)


def host(disp, mults, out_h, out_w, cmap):
    return outputs.disparity_image(disp, out_h, out_w, cmap, mults)


def pinned_resize(img8, out_h, out_w):
    """the project's host twin of Pillow's bilinear resample (held to Pillow by tests/test_seg_eval_cpu.py)"""
    import ctypes as C

    from semantic_depth_amd import _lib as L
    src = np.ascontiguousarray(img8, np.uint8)
    dst = np.empty((out_h, out_w), np.uint8)
    st = L.load().sd_resize_pil_bilinear_u8_host(src.ctypes.data_as(C.c_void_p), 1, src.shape[0], src.shape[1], 1, 1, 0, dst.ctypes.data_as(C.c_void_p),
                                                 out_h, out_w)
    assert st == 0
    return dst


def test_host_twin_equals_imsave_pixel_for_pixel(golden):
    names = [str(n) for n in golden["names"]]
    assert len(names) == 12 and {"batch3", "constant", "two_valued", "tiny_3x5_1x1", "mult_1", "mult_3800"} <= set(names)
    assert D.check(host, golden) == []
    # the fixture's inputs are the seeded cases of the case file
    cases = D.make_cases()
    for n in names:
        assert np.array_equal(cases[n]["disp"], golden[n + "/disp"]) and np.array_equal(cases[n]["mults"], golden[n + "/mults"]), n


def test_colour_tables(golden):
    for m in D.MAPS:
        assert np.array_equal(outputs.disp_colormap(m), golden["table/" + m]), m
    gray = outputs.disp_colormap("gray")
    assert (gray[:, 0] == gray[:, 1]).all() and (gray[:, 0] == gray[:, 2]).all()
    off = np.flatnonzero(gray[:, 0] != np.arange(256))
    assert len(off) == 24 and off[0] == 33 and off[1] == 37 and off[2] == 41 and off[-1] == 244
    assert (gray[off, 0] == off - 1).all()
    assert tuple(outputs.disp_colormap("plasma")[0]) == (12, 7, 134)
    with pytest.raises(ValueError):
        outputs.disp_colormap("viridis")


def test_integer_index_rule_is_matplotlibs_float32_rule():
    triples = 0
    for lo8 in range(255):                                 # every lo8 < hi8 and every lo8 <= p <= hi8, one lo8 at a time
        hi8, p = np.meshgrid(np.arange(lo8 + 1, 256), np.arange(lo8, 256), indexing="ij", sparse=True)
        ok = p <= hi8
        fl = D.colour_index_float32(p, lo8, hi8)
        it = np.minimum(255, 256 * (p - lo8) // (hi8 - lo8))
        assert np.array_equal(fl[ok], it[ok]), lo8
        triples += int(ok.sum())
    assert triples == sum((256 - d) * (d + 1) for d in range(1, 256))


@pytest.mark.parametrize("cmap", D.MAPS)
def test_restatement_equals_host_twin_on_random_maps(cmap):
    rng = np.random.default_rng(77)
    table = outputs.disp_colormap(cmap)
    for k, (B, h, w, oh, ow) in enumerate([(2, 8, 16, 20, 40), (3, 7, 13, 9, 11), (1, 16, 32, 5, 7), (2, 9, 5, 9, 5), (4, 3, 5, 1, 1), (1, 1, 1, 4, 6)]):
        disp = (rng.standard_normal((B, h, w)) * 10 ** rng.uniform(-3, 3)).astype(np.float32)
        mults = rng.choice([1.0, 3800.0, 2048.0], B).astype(np.float32)
        want_flags = np.zeros(B, np.int32)
        if k % 2 == 0:                                     # NaN / +-inf pixels in frame 0: byte 0, flag 1
            flat = disp[0].reshape(-1)
            flat[rng.integers(0, flat.size, 3)] = [np.nan, np.inf, -np.inf]
            want_flags[0] = 1
        if k == 1:                                         # an all-NaN frame
            disp[2] = np.nan
            want_flags[2] = 1
        got, flags = host(disp, mults, oh, ow, cmap)
        want, wflags = D.restate(disp, mults, oh, ow, table, pinned_resize)
        assert np.array_equal(flags, want_flags) and np.array_equal(wflags, want_flags), (k, flags)
        assert np.array_equal(got, want), (k, np.argwhere(got != want)[:3])
        if k == 1:
            assert (got[2] == table[0][::-1]).all()
        # a frame alone gives the bytes it has inside the batch; no multipliers means 1.0
        alone, f1 = host(disp[-1:], mults[-1:], oh, ow, cmap)
        assert np.array_equal(alone[0], got[-1]) and f1[0] == flags[-1]
        ones, _ = host(disp, None, oh, ow, cmap)
        assert np.array_equal(ones, host(disp, np.ones(B, np.float32), oh, ow, cmap)[0])


def test_the_checker_catches_the_seeded_mistakes(golden):
    tables = {m: golden["table/" + m] for m in D.MAPS}
    assert D.check(lambda d, mu, oh, ow, m: D.restate(d, mu, oh, ow, tables[m], pinned_resize), golden) == []
    caught = {}
    for mistake in D.MISTAKES:
        caught[mistake] = D.check(lambda d, mu, oh, ow, m: D.restate(d, mu, oh, ow, tables[m], pinned_resize, mistake), golden)
        assert caught[mistake], mistake
    assert len(D.MISTAKES) == 5
    assert set(caught["batch_range"]) == {"batch3/gray", "batch3/plasma"}
    assert all(c.endswith("/gray") for c in caught["identity_gray"]) and all(c.endswith("/plasma") for c in caught["swap_plasma"])
    assert "boundary_same/gray" in caught["float64_scale"]


def test_refusals_of_the_host_functions():
    d = np.zeros((1, 4, 4), np.float32)
    with pytest.raises(ValueError):
        outputs.disparity_image(d, 4, 4, "jet")
    with pytest.raises(ValueError):
        outputs.disparity_image(d, 0, 4)
    with pytest.raises(ValueError):
        outputs.disparity_image(np.zeros((1, 66, 4), np.float32), 2, 4)          # a downscale factor above 32
    with pytest.raises(ValueError):
        outputs.disparity_image(d, 4, 16385)
    with pytest.raises(ValueError):
        outputs.disparity_image(d, 4, 4, mults=[1.0, 2.0])
    import ctypes as C

    from semantic_depth_amd import _lib as L
    need = C.c_size_t()
    lib = L.load()
    assert lib.sd_disp_image_workspace(0, 4, 4, 4, 4, C.byref(need)) == L.SD_ERR_INVALID
    assert lib.sd_disp_image_workspace(1, 4, 4, 4, 0, C.byref(need)) == L.SD_ERR_INVALID
    assert lib.sd_disp_image_workspace(2, 4, 4, 4, 4, C.byref(need)) == L.SD_OK and need.value % 16 == 0 and need.value >= 2 * 16 + 2 * 4 + 32
    same = need.value
    assert lib.sd_disp_image_workspace(2, 4, 4, 8, 8, C.byref(need)) == L.SD_OK and need.value > same + 2 * 64


def test_write_disp_image(tmp_path, golden):
    c = D.make_cases()["mult_3800"]
    path = outputs.write_disp_image(str(tmp_path / "frame"), c["disp"][0], c["out_h"], c["out_w"], "plasma", 3800.0)
    assert path == str(tmp_path / "frame_disp.png")
    assert np.array_equal(frame_io.imread(path)[..., ::-1], golden["mult_3800/plasma"][0])


# ------------------------------------------------------------------------------------------------ SequenceOutputs(disp=)
def disp_maps():
    """one 12 x 16 map per frame of sequence_all_routes_cases; frame 2 holds a NaN"""
    rng = np.random.default_rng(5)
    maps = (rng.random((len(A.NAMES), 12, 16), dtype=np.float32) * np.float32(0.08)).astype(np.float32)
    maps[2, 3, 4] = np.nan
    return maps


def tree_digest(tree):
    h = hashlib.sha256()
    for k in sorted(tree):
        h.update(k.encode() + b"\0" + tree[k] + b"\0")
    return h.hexdigest()


def test_disp_none_leaves_files_and_manifest_as_they_were(tmp_path):
    a = A.run(tmp_path / "a", every=False)                 # (the routes that were there before disp=)
    assert a.disp is None
    a.close()
    b = outputs.SequenceOutputs(str(tmp_path / "b"), A.NAMES, threads=2, png="device", ply="device", render=A.CAMERA,
                                video=outputs.Video(fps=25, quality=A.QUALITY, route="device"), disp=None)
    b.begin(0, 1, 0, len(A.NAMES))
    for lo, kw in A.batches():
        kw = A._tensors(A.base(kw), lambda t: t)
        b.submit(lo, kw.pop("records"), (A.H, A.W), **kw, disp_images=None, disp_streams=None)
    b.close()
    ta, tb = A.tree(tmp_path / "a"), A.tree(tmp_path / "b")
    assert ta == tb and not any(k.startswith(outputs.SEQ_DISP_DIR) for k in ta)
    m = json.loads(ta["manifest_rank0.json"])
    assert sorted(m) == sorted(["rank", "world", "frames", "status", "valid", "files", "recomputed", "ply_fallback", "render", "video", "video_fallback"])
    # the digest of this tree as the parent commit wrote it (recorded from that commit's outputs.py on the same cases)
    assert tree_digest(ta) == PARENT_TREE_DIGEST


PARENT_TREE_DIGEST = "ae976096085e18a2d8e278ee6edfa4b9b523f19ea11b57774e91eb236edc1a22"


@pytest.mark.parametrize("png", ["host", "device"])
@pytest.mark.parametrize("cmap", ["gray", "plasma"])
def test_sequence_outputs_write_the_disparity_images(tmp_path, png, cmap):
    maps = disp_maps()
    mults = np.full(len(A.NAMES), 3800.0, np.float32)
    want, flags = outputs.disparity_image(maps, A.H, A.W, cmap, mults)
    assert flags.tolist() == [0, 0, 1, 0, 0, 0, 0, 0]
    if png == "device":       # beside every other route
        outs = outputs.SequenceOutputs(str(tmp_path), A.NAMES, threads=2, png="device", ply="device", render=A.CAMERA,
                                       video=outputs.Video(fps=25, quality=A.QUALITY, route="device"), text="draw", profile=[8.0, 10.0])
        outs.set_disp(cmap)
    else:                     # alone, without the result images
        outs = outputs.SequenceOutputs(str(tmp_path), A.NAMES, threads=2, images=False, ply=False, items=False, disp=cmap)
    outs.begin(0, 1, 0, len(A.NAMES))
    for lo, kw in A.batches():
        n = len(kw["records"])
        if png == "device":
            kw = dict(A.base(kw), disp_streams=A._rows([PN.encode_host(im) for im in want[lo:lo + n]], PN.bound(A.H, A.W)), disp_flags=flags[lo:lo + n],
                      profile=np.zeros((n, 2, 48), np.uint8))
        else:
            kw = dict(records=kw["records"], disp_images=want[lo:lo + n], disp_flags=flags[lo:lo + n])
        kw = A._tensors(kw, lambda t: t)
        outs.submit(lo, kw.pop("records"), (A.H, A.W), **kw)
    m = json.load(open(outs.close()))
    for i, name in enumerate(A.NAMES):
        assert np.array_equal(frame_io.imread(str(tmp_path / outputs.SEQ_DISP_DIR / f"{name}_disp.png")), want[i]), name
    assert outputs.SEQ_DISP_DIR == "result_sequence_disp"
    assert m["disp"] == [os.path.join(outputs.SEQ_DISP_DIR, f"{name}_disp.png") for name in A.NAMES]
    assert m["disp_nonfinite"] == [A.NAMES[2]] and m["status"] == "ok"
    on_disk = sorted(set(A.tree(tmp_path)) - {"manifest_rank0.json"})
    assert m["files"] == on_disk
    if png == "host":
        assert on_disk == m["disp"]
    else:
        assert len(on_disk) == 6 * len(A.NAMES) + 1 and len(m["render"]) == len(A.NAMES) and m["video"] == ["result_imgs.avi"]


def test_sequence_outputs_refusals(tmp_path):
    with pytest.raises(ValueError):
        outputs.SequenceOutputs(str(tmp_path), A.NAMES, disp="jet")
    outs = outputs.SequenceOutputs(str(tmp_path), A.NAMES, images=False, ply=False, items=False)
    with pytest.raises(ValueError):
        outs.configure(disp="viridis")
    with pytest.raises(ValueError):
        outs.set_disp(True)
    assert outs.disp is None
    outs.configure(disp="plasma")
    outs.configure()                                       # None leaves the choice as it is
    assert outs.disp == "plasma"
    rec = A._tensors(A.batches()[0][1]["records"], lambda t: t)
    img = np.zeros((3, A.H, A.W, 3), np.uint8)
    with pytest.raises(ValueError):                        # the host route needs the images
        outs.submit(0, rec, (A.H, A.W))
    with pytest.raises(ValueError):
        outs.submit(0, rec, (A.H, A.W), disp_streams=(img.reshape(3, -1), np.zeros(3, np.int64)))
    outs.set_png("device")
    with pytest.raises(ValueError):                        # the device route needs the streams
        outs.submit(0, rec, (A.H, A.W), disp_images=img)
    outs.disp = "jet"                                      # a name that went round configure
    with pytest.raises(ValueError):
        outs.submit(0, rec, (A.H, A.W), disp_images=img)
    outs.disp = "plasma"
    outs.set_png("host")
    outs.submit(0, rec, (A.H, A.W), disp_images=img)
    with pytest.raises(RuntimeError):                      # no change after the first batch
        outs.set_disp("gray")
    with pytest.raises(RuntimeError):
        outs.configure(disp="gray")
    outs.close()
