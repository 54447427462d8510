"""CPU: the scratch layouts (csrc/arena.hpp and the layout functions written with it).

* every public workspace size query and the handle arena's total answer what the commit named in tests/golden/workspace_sizes.json
  answered, refusals included (tests/workspace_sizes_cases.py); the handle totals also pin the Open3D, compaction and fuse scratches
* scripts/check_layouts.cpp, built with the host compiler alone, finds every layout ordered, aligned as stated, inside its total and
  of the size the queries always reported"""
import os
import shutil
import subprocess

import pytest

import __graft_entry__ as graft
import workspace_sizes_cases as W
from semantic_depth_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    graft.build()
    return L.load()


def test_every_size_query_answers_what_the_recorded_commit_answered(lib):
    doc = W.golden()
    assert "commit" in doc["header"]
    asked, _ = W.grid()
    assert [[fn, args] for fn, args, _ in doc["queries"]] == asked          # (the golden file covers the whole list)
    bad = [(fn, args, want, got) for fn, args, want in doc["queries"] if (got := W.call(lib, fn, args)) != want]
    assert not bad, bad[:5]
    for fn in ("sd_jpeg_reconstruct_workspace", "sd_jpeg_entropy_workspace", "sd_jpeg_sync_workspace", "sd_png_reconstruct_workspace",
               "sd_png_encode_workspace", "sd_jpeg_encode_workspace", "sd_ply_format_workspace", "sd_scene_workspace", "sd_text_workspace_bytes",
               "sd_overlay_workspace_bytes", "sd_render_workspace", "sd_fuse_sweep_workspace", "sd_rw_profile_workspace", "sd_resize_pil_workspace",
               "sd_disp_image_workspace"):
        answers = [r for f, _, r in doc["queries"] if f == fn]
        assert any(r[0] in (0, None) and r[1] > 0 for r in answers) and any(r[0] not in (0, None) or r[1] == 0 for r in answers), fn


def test_every_handle_arena_has_the_recorded_size(lib):
    doc = W.golden()
    assert [cfg for cfg, _ in doc["handles"]] == W.grid()[1]
    bad = [(cfg, want, got) for cfg, want in doc["handles"] if (got := W.handle_total(lib, cfg)) != want]
    assert not bad, bad


def test_check_layouts_program_passes(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler on this machine")
    exe = str(tmp_path / "check_layouts")
    subprocess.run([cxx, "-O1", "-std=c++17", os.path.join(ROOT, "scripts", "check_layouts.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "0 failures" in r.stdout
