"""CPU: the scene PLY route without a GPU.  The lattice rule of csrc/scene_format.hpp (sd_scene_lattice_host) against pcl.plane_grid, bit
for bit; whole files of sd_scene_format_host against the plain-numpy statement outputs.scene_ply_bytes, byte for byte; the ROAD | RW_LINE
mask against the road PLY writer; the flags.  (The device half is tests/test_gpu_scene.py.)"""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as graft
import ply_device_cases as P
import scene_cases as S
from semantic_depth_amd import _lib as L
from semantic_depth_amd import outputs, pcl
from semantic_depth_amd.engine import BOX_DTYPE, F2F_DTYPE


@pytest.fixture(scope="module")
def lib():
    graft.build()
    return L.load()


def lattice_host(lib, b4, plane, axis):
    box = S.box(*b4)
    pl = np.ascontiguousarray(plane, np.float64)
    na, nb = C.c_uint32(), C.c_uint32()
    assert lib.sd_scene_lattice_host(box.ctypes.data_as(C.c_void_p), pl.ctypes.data_as(C.c_void_p), axis, C.byref(na), C.byref(nb), None, 0) == L.SD_OK
    out = np.empty((na.value * nb.value, 3), np.float64)
    assert lib.sd_scene_lattice_host(box.ctypes.data_as(C.c_void_p), pl.ctypes.data_as(C.c_void_p), axis, C.byref(na), C.byref(nb),
                                     out.ctypes.data_as(C.c_void_p), len(out)) == L.SD_OK
    return out


def plane_grid(b4, plane, axis):
    """pcl.plane_grid on a float32 cloud whose bounding box is the box"""
    ia, ib = [(1, 2), (0, 2), (0, 1)][axis]
    cloud = np.zeros((2, 3), np.float32)
    cloud[:, ia], cloud[:, ib] = (b4[0], b4[1]), (b4[2], b4[3])
    return pcl.plane_grid(cloud, dict(Cx=plane[0], Cy=plane[1], Cz=plane[2], C=plane[3]), axis)[0].reshape(-1, 3)


def same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


PLANES = ((S.ROAD_PLANE_COEF, 1), (S.LEFT_PLANE_COEF, 0), (S.RIGHT_PLANE_COEF, 0))


def test_lattice_equals_plane_grid_on_exact_multiples(lib):
    boxes = S.exact_multiple_boxes()
    assert len(boxes) >= 2000
    for i, b4 in enumerate(boxes):
        plane, axis = PLANES[i % 3]
        got, want = lattice_host(lib, b4, plane, axis), plane_grid(b4, plane, axis)
        assert same_bits(got, want), (b4, got.shape, want.shape)


@pytest.mark.parametrize("plane,axis", PLANES)
def test_lattice_equals_plane_grid_on_special_boxes(lib, plane, axis):
    counts = []
    for b4 in S.special_boxes():
        got, want = lattice_host(lib, b4, plane, axis), plane_grid(b4, plane, axis)
        assert same_bits(got, want), (b4, got.shape, want.shape)
        counts.append(len(got))
    assert counts[1] == 20 and counts[2] == 0 and counts[4] == 0       # one sample along a; a zero extent: no lattice
    rng = np.random.default_rng(5)
    for _ in range(300):                                               # random boxes: all values
        lo = rng.uniform(-20, 20, 2).astype(np.float32)
        b4 = np.array([lo[0], lo[0] + rng.uniform(0, 2), lo[1], lo[1] + rng.uniform(0, 2)], np.float32)
        assert same_bits(lattice_host(lib, b4, plane, axis), plane_grid(b4, plane, axis)), b4


def test_the_model_is_the_rule_and_every_seeded_mistake_is_caught():
    """the cases above are sharp enough: the Python model of the rule equals pcl.plane_grid on all of them, and each seeded mistake (a
    float64 count, b fastest, a fused lift, 0.05 as the step) differs from it on many (the counts are in the assertion message)"""
    cases = [(b4, *PLANES[i % 3]) for i, b4 in enumerate(S.exact_multiple_boxes())] + [(b4, p, a) for b4 in S.special_boxes() for p, a in PLANES]
    want = [plane_grid(b4, p, a) for b4, p, a in cases]
    assert all(same_bits(S.lattice_model(b4, p, a), w) for (b4, p, a), w in zip(cases, want))
    caught = {m: sum(not same_bits(S.lattice_model(b4, p, a, m), w) for (b4, p, a), w in zip(cases, want)) for m in S.MISTAKES}
    # no mistake hinges on a handful of boxes: each is caught on at least 100 of the 2018 cases
    assert all(n >= 100 for n in caught.values()), (caught, len(cases))


def host(f, mask=S.ALL, fence=True, lattice_cap=0):
    return outputs.scene_format_host(mask=mask, lattice_cap=lattice_cap, **S.args(f, fence))


def check_file(f, mask=S.ALL, fence=True):
    got, flag = host(f, mask, fence)
    want = outputs.scene_ply_bytes(mask=mask, **S.args(f, fence))
    assert flag == 0 and P.first_difference(got, want) is None, P.first_difference(got, want)
    return got


def vertex_count(data: bytes) -> int:
    return int(data.split(b"element vertex ")[1].split(b"\n")[0])


def test_whole_file_every_segment_present(lib):
    f = S.frame(1)
    data = check_file(f)
    rows = 300 + 20 * 30 + 1001 + 200 + 180 + 20 * 30 + 21 * 28 + 1001
    assert vertex_count(data) == rows - 1                              # (the one road point at the minimum went)
    for key, mask in S.FILE_MASKS.items():
        check_file(f, mask)
    check_file(f, fence=False)                                         # approach 'rw': the fence segments are absent
    assert vertex_count(check_file(f, S.FILE_MASKS["fence"], fence=False)) == 0


def test_whole_file_absent_segments(lib):
    check_file(S.frame(2, found=False))
    check_file(S.without_left(S.frame(3)))
    check_file(S.without_left(S.frame(4, found=False)))
    empty_road = S.frame(5, n_road=0)
    empty_road["road_box"] = S.box(0, 0, 0, 0, 0)
    check_file(empty_road)
    check_file(empty_road, S.FILE_MASKS["road"])


@pytest.mark.parametrize("where", S.MIN_PLACES)
def test_whole_file_minimum_in_each_kind_of_segment(lib, where):
    base = S.frame(6)
    f = S.with_min_in(base, where)
    data = check_file(f)
    dropped = dict(road=1, road_plane=20, rw_line=2, fence_l=1, fence_r=1, plane_l=20, plane_r=21, f2f_line=2, shared=2)[where]
    total = vertex_count(outputs.scene_ply_bytes(**S.args(f))) + dropped
    rows = 300 + 1001 + 200 + 180 + 1001
    lat = {k: (20, 30) for k in ("road_plane", "plane_l")}
    lat["plane_r"] = (21, 28)
    if where in lat:                                                   # (the moved box is 0.5 / 0.4 m deep: 10 / 8 samples along b)
        lat[where] = (lat[where][0], 10 if where == "road_plane" else 8)
    assert total == rows + sum(a * b for a, b in lat.values()), (where, vertex_count(data))


def test_road_and_line_mask_equals_the_road_ply_writer(lib):
    for c in P.line_cases() + P.filter_cases() + P.edge_cases():
        f = dict(road_xyz=c["xyz"], road_rgb=c["rgb"], record=c["rec"], road_box=None)
        got, flag = host(f, S.ROAD | S.RW_LINE, fence=False)
        st, ref, rflag = P.host(c)
        assert st == L.SD_OK and (flag, got) == (rflag, ref), c["name"]
        assert got == P.want(c), c["name"]


def test_flags(lib):
    f = S.frame(7)
    nan = S.with_min_in(f, "road")
    nan["fence"]["right_xyz"][11, 1] = np.nan
    assert host(nan) == (b"", 1)
    assert host(nan, S.FILE_MASKS["road"])[1] == 0                     # (only the selected segments count)
    nanbox = dict(f, road_box=S.box(np.nan, 1.0, -9.0, -7.5, 5))
    assert host(nanbox) == (b"", 1)
    huge = dict(f, record=f["record"].copy())
    huge["record"]["plane"][3] = 1e300                                 # the lifted coordinate leaves the range
    assert host(huge) == (b"", 1)
    end = dict(f, f2f=f["f2f"].copy())
    end["f2f"]["left_pt"][0] = np.inf
    assert host(end) == (b"", 1)
    assert host(f, lattice_cap=600)[1] == 0 and host(f, lattice_cap=599) == (b"", 3)       # the largest lattice has 600 rows
    assert host(f, S.FILE_MASKS["road"], lattice_cap=1)[1] == 0


def test_capacity_one_byte_short_packs_the_frame_behind(lib):
    """flag 2 on the host call: the size the text needs is reported and nothing is written; a caller that packs frames back to back (as
    the device call does) keeps the frame behind at the offset the flagged one left"""
    frames = [S.frame(8), S.frame(9, n_road=120), S.frame(10, found=False)]
    texts = [host(f)[0] for f in frames]
    cap = len(texts[0]) + len(texts[1]) - 1                            # one byte short for the middle frame; the last one is shorter and fits
    assert len(texts[2]) < len(texts[1])
    out = np.full(cap + 8, 0xA5, np.uint8)
    off, flags, offsets = 0, [], [0]
    for f in frames:
        kw = S.args(f)
        rec = np.ascontiguousarray(kw["record"].reshape(1))
        f2 = np.ascontiguousarray(kw["f2f"].reshape(1))
        rb, fb = np.ascontiguousarray(kw["road_box"].reshape(1)), np.ascontiguousarray(kw["fence_boxes"])
        fence = kw["fence"]
        size, flag = C.c_size_t(), C.c_int32()
        st = lib.sd_scene_format_host(kw["road3D"].ctypes.data_as(C.c_void_p), kw["road_colors"].ctypes.data_as(C.c_void_p), len(kw["road3D"]),
                                      fence["left_xyz"].ctypes.data_as(C.c_void_p), fence["left_rgb"].ctypes.data_as(C.c_void_p),
                                      fence["right_xyz"].ctypes.data_as(C.c_void_p), fence["right_rgb"].ctypes.data_as(C.c_void_p),
                                      rec.ctypes.data_as(C.c_void_p), f2.ctypes.data_as(C.c_void_p), rb.ctypes.data_as(C.c_void_p),
                                      fb.ctypes.data_as(C.c_void_p), S.ALL, 0, out[off:].ctypes.data_as(C.c_void_p), cap - off, C.byref(size), C.byref(flag))
        assert st == L.SD_OK
        flags.append(flag.value)
        off += size.value if flag.value == 0 else 0
        offsets.append(off)
        if flag.value == 2:
            assert size.value == len(texts[len(flags) - 1])            # what it would have needed
    assert flags == [0, 2, 0] and offsets == [0, len(texts[0]), len(texts[0]), len(texts[0]) + len(texts[2])]
    assert out[:offsets[1]].tobytes() == texts[0] and out[offsets[2]:offsets[3]].tobytes() == texts[2] and (out[offsets[3]:] == 0xA5).all()


def test_the_frames_of_the_device_test_are_what_it_needs(lib):
    """tests/test_gpu_scene.py's frames: a 512-row segment, a 1 x n lattice, 4097 lattice rows against a cap of 4096, flags 1 and 3 from
    the host statement, and frame 2 the longest file under every mask (so that the frame behind a capacity flag still fits)"""
    def rows(b, plane=S.ROAD_PLANE_COEF, axis=1):
        b4 = [b["lo_a"], b["hi_a"], b["lo_b"], b["hi_b"]]
        na, nb = C.c_uint32(), C.c_uint32()
        pl = np.ascontiguousarray(plane, np.float64)
        assert lib.sd_scene_lattice_host(S.box(*b4).ctypes.data_as(C.c_void_p), pl.ctypes.data_as(C.c_void_p), axis, C.byref(na), C.byref(nb), None, 0) == 0
        return na.value, nb.value
    f0, f1, f2 = S.gpu_frames("flag3")
    assert rows(f0["road_box"]) == (16, 32) and rows(f1["road_box"])[0] == 1 and rows(f2["fence_boxes"][1], S.RIGHT_PLANE_COEF, 0) == (17, 241)
    assert host(f2, lattice_cap=4096) == (b"", 3) and host(f2, lattice_cap=4097)[1] == 0
    assert host(S.gpu_frames("flag1")[2]) == (b"", 1)
    f0, f1, f2 = S.gpu_frames("flag2")
    for mask in S.FILE_MASKS.values():
        assert len(host(f1, mask)[0]) < len(host(f2, mask)[0]) and host(f0, mask)[1] == 0


def test_scene_dataclass_and_abi():
    assert BOX_DTYPE.itemsize == 24 and F2F_DTYPE.itemsize == 152
    assert outputs.Scene().route == "device" and outputs.Scene().lattice_cap == 1 << 18 and outputs.Scene().capacity_per_frame == 24 << 20
    assert outputs.Scene(files=["road"]).files == ("road",)
    for bad in (dict(route="gpu"), dict(files=()), dict(files=("scene", "scene")), dict(files=("all",)), dict(lattice_cap=-1)):
        with pytest.raises(ValueError):
            outputs.Scene(**bad)
