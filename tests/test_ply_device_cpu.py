"""CPU: the device route of the road PLYs as its host statement, sd_ply_format_rw_host (the function whose bytes the kernels of ply_gpu.hip
must reproduce, tests/test_gpu_ply_device.py), against outputs.rw_ply_bytes byte for byte; the workspace bound; and the writer side of
SequenceOutputs(ply="device") fed with the host statement's text.  The cases are those of tests/ply_device_cases.py."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import ply_device_cases as P
from semantic_depth_amd import _lib as L
from semantic_depth_amd import outputs
from semantic_depth_amd.point_cloud_2_ply import PointCloud2Ply

GOOD = {c["name"]: c for c in P.good_cases()}
FLAGGED = {c["name"]: c for c in P.flagged_cases()}


@pytest.mark.parametrize("name", sorted(GOOD))
def test_host_statement_is_rw_ply_bytes(name):
    c = GOOD[name]
    ref = P.want(c)
    st, got, flag = P.host(c)
    assert st == L.SD_OK and flag == 0
    assert len(got) <= P.bound(len(c["xyz"]))
    diff = P.first_difference(got, ref)
    assert diff is None, f"{name}: {diff}"


def test_the_cases_reach_what_they_are_meant_to():
    """the rounding cases hold ties, carries, signed zeros and the longest row; the filter cases drop what they say"""
    text = b"".join(P.want(c) for c in P.rounding_cases())
    for s in (b"0.007812 ", b"0.023438 ", b"0.039062 ", b"1.000000 ", b"10.000000 ", b"100000.000000 ", b"-0.000000 ", b"0.000000 ",
              b"0.000001 ", b"2147483520.000000 ", b"-2147483520.000000 ", b" 0 ", b" 9 ", b" 10 ", b" 99 ", b" 100 ", b" 255"):
        assert s in text, s
    assert max(len(r) for r in text.split(b"\n")) + 1 <= P.ROW_CAP
    assert len(b"-2147483520.000000 -2147483520.000000 -2147483520.000000 255 255 255\n") == P.ROW_CAP
    head = PointCloud2Ply.ply_header
    assert P.want(GOOD["all_rows_one_z"]) == head.format(vertex_count=0).encode()
    assert P.want(GOOD["flat_cloud_no_line"]) == head.format(vertex_count=0).encode()
    assert P.want(GOOD["flat_cloud_line_above"]).startswith(head.format(vertex_count=P.LINE_ROWS).encode())
    assert P.want(GOOD["flat_cloud_line_below"]).startswith(head.format(vertex_count=30 + P.LINE_ROWS - 2).encode())
    assert P.want(GOOD["minimum_on_a_line_point"]).startswith(head.format(vertex_count=30 + P.LINE_ROWS - 1).encode())
    z = GOOD["shared_minimum"]["xyz"][:, 2]
    at_min = int((z == z.min()).sum())
    assert at_min >= 4 and P.want(GOOD["shared_minimum"]).startswith(head.format(vertex_count=50 - at_min).encode())
    assert P.want(GOOD["minus_zero_minimum"]).startswith(head.format(vertex_count=1).encode())


def test_header_of_a_file_without_a_vertex():
    st, got, flag = P.host(GOOD["empty_no_line"])
    assert (st, flag) == (L.SD_OK, 0)
    assert got == PointCloud2Ply.ply_header.format(vertex_count=0).encode()
    assert got.endswith(b"end_header\n    ") and got.startswith(b"ply\n    format ascii 1.0\n    element vertex 0\n    property float x\n")
    assert len(PointCloud2Ply.ply_header.format(vertex_count=2 ** 31 - 1)) == P.HEADER_CAP == L.SD_PLY_HEADER_CAP
    assert (L.SD_PLY_ROW_CAP, L.SD_PLY_LINE_ROWS) == (P.ROW_CAP, P.LINE_ROWS)


@pytest.mark.parametrize("name", sorted(FLAGGED))
def test_frames_outside_the_range_are_flagged_not_formatted(name):
    st, got, flag = P.host(FLAGGED[name])
    assert (st, flag, got) == (L.SD_OK, 1, b"")


@pytest.mark.parametrize("name", ["rounding_0", "seam_256", "empty_no_line", "empty_line"])
def test_a_capacity_one_byte_short_is_refused(name):
    c = GOOD[name]
    ref = P.want(c)
    st, got, _ = P.host(c, cap=len(ref))
    assert st == L.SD_OK and got == ref
    assert P.host(c, cap=len(ref) - 1)[0] == L.SD_ERR_INVALID


def test_host_statement_refuses_bad_arguments():
    lib = P.lib()
    c = GOOD["one_point"]
    rec = L.sd_rw_result.from_buffer_copy(c["rec"].tobytes())
    out = np.zeros(1024, np.uint8)
    size, flag = C.c_size_t(), C.c_int32()
    args = [c["xyz"].ctypes.data_as(C.c_void_p), c["rgb"].ctypes.data_as(C.c_void_p), 1, C.byref(rec), out.ctypes.data_as(C.c_void_p), out.size,
            C.byref(size), C.byref(flag)]
    assert lib.sd_ply_format_rw_host(*args) == L.SD_OK
    for i, v in ((0, None), (1, None), (2, -1), (3, None), (4, None), (6, None), (7, None)):
        bad = list(args)
        bad[i] = v
        assert lib.sd_ply_format_rw_host(*bad) == L.SD_ERR_INVALID, i


def test_workspace_bounds_every_case():
    lib = P.lib()
    ws, tb = C.c_size_t(), C.c_size_t()
    for B, cap in ((0, 8), (-1, 8), (1, -1), (65536, 8)):
        assert lib.sd_ply_format_workspace(B, cap, C.byref(ws), C.byref(tb)) == L.SD_ERR_INVALID
    for group in P.batches(P.good_cases()):
        B, cap = len(group), len(group[0]["xyz"])
        assert lib.sd_ply_format_workspace(B, cap, C.byref(ws), C.byref(tb)) == L.SD_OK
        assert tb.value == B * (P.HEADER_CAP + (cap + P.LINE_ROWS) * P.ROW_CAP)
        assert sum(len(P.want(c)) for c in group) <= tb.value
        nblk = -(-(cap + P.LINE_ROWS) // P.BLOCK)
        assert ws.value >= B * nblk * 28 + B * 16 and ws.value < B * nblk * 28 + B * 16 + 4096
    assert lib.sd_ply_format_workspace(32, 512 * 1024, C.byref(ws), C.byref(tb)) == L.SD_OK
    assert tb.value > 2 ** 30 and tb.value == 32 * (209 + (512 * 1024 + 1001) * 69)


def test_sequence_outputs_ply_choice_is_checked(tmp_path):
    import torch
    for bad in ("gpu", "", None, 1):
        with pytest.raises(ValueError):
            outputs.SequenceOutputs(str(tmp_path), ["a"], ply=bad)
    for ply, on, route in ((True, True, "host"), (False, False, "host"), ("host", True, "host"), ("device", True, "device")):
        o = outputs.SequenceOutputs(str(tmp_path), ["a"], ply=ply, images=False)
        assert (o.ply, o.ply_route) == (on, route)
        o.close()
    o = outputs.SequenceOutputs(str(tmp_path), ["a", "b"], images=False, items=False)
    with pytest.raises(ValueError):
        o.set_ply("gpu")
    with pytest.raises(ValueError):
        o.set_ply(True)
    o.set_ply("device")
    c = GOOD["one_point"]
    rec = torch.from_numpy(np.frombuffer(c["rec"].tobytes(), np.uint8).copy()[None])
    final = dict(xyz=c["xyz"][None], rgb=c["rgb"][None], n=np.array([1], np.int32))
    with pytest.raises(ValueError):                  # the device route needs the text beside the clouds
        o.submit(0, rec, (4, 4), final=final)
    o.set_ply("host")
    o.submit(0, rec, (4, 4), final=final)
    with pytest.raises(RuntimeError):
        o.set_ply("device")
    o.close()


def _batch(cases):
    """the tensors of one batch as the step hands them to submit(): records, road_final and the text of the host statement"""
    import torch
    n = len(cases)
    cap = max(len(c["xyz"]) for c in cases)
    xyz, rgb = np.full((n, cap, 3), np.nan, np.float32), np.full((n, cap, 3), 0xA5, np.uint8)
    cnt = np.array([len(c["xyz"]) for c in cases], np.int32)
    text, offsets, flags = [], [0], []
    for i, c in enumerate(cases):
        xyz[i, :cnt[i]], rgb[i, :cnt[i]] = c["xyz"], c["rgb"]
        st, got, flag = P.host(c)
        assert st == L.SD_OK
        text.append(got)
        offsets.append(offsets[-1] + len(got))
        flags.append(flag)
    rec = torch.from_numpy(np.stack([np.frombuffer(c["rec"].tobytes(), np.uint8) for c in cases]).copy())
    blob = np.frombuffer(b"".join(text) + b"\xa5" * 64, np.uint8)
    return rec, dict(xyz=xyz, rgb=rgb, n=cnt), (blob, np.array(offsets, np.int64), np.array(flags, np.int32))


def test_sequence_outputs_device_route_from_host_arrays(tmp_path):
    """the writer side alone (no GPU): host arrays in place of Engine.format_rw_ply's tensors give the files and the manifest of the host
    route, plus 'ply_fallback' with the frames that carried a flag"""
    groups = [[GOOD["line_long_fractions"], FLAGGED["nan_in_cloud"], GOOD["empty_no_line"]],
              [FLAGGED["two_to_the_31"], GOOD["seam_256"], GOOD["rounding_1"]]]
    names = [f"f{i}_{c['name']}" for i, c in enumerate(sum(groups, []))]
    man = {}
    for route in ("host", "device"):
        o = outputs.SequenceOutputs(str(tmp_path / route), names, images=False, ply=route, threads=2)
        lo = 0
        for g in groups:
            rec, final, text = _batch(g)
            o.submit(lo, rec, (8, 8), final=final, **(dict(ply_text=text) if route == "device" else {}))
            lo += len(g)
        o.close()
        man[route] = json.load(open(o.manifest))
    assert man["device"].pop("ply_fallback") == [names[1], names[3]] and "ply_fallback" not in man["host"]
    assert man["host"] == man["device"] and len(man["host"]["files"]) == 2 * len(names)
    for nm, c in zip(names, sum(groups, [])):
        a, b = (open(os.path.join(str(tmp_path / r), outputs.SEQ_PLY_DIR, nm + "_rw.ply"), "rb").read() for r in ("host", "device"))
        assert a == b == P.want(c), nm
