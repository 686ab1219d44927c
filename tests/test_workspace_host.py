"""csrc/workspace.hpp on the host: the layout of multi-piece workspace blocks, checked by a stand-alone program under the
address and undefined-behaviour sanitizers (no GPU, nothing loaded into Python)."""
import os
import shutil
import subprocess

from conftest import REPO

SRC = os.path.join(REPO, "python-visual-similarity_amd", "csrc", "bench", "ws_layout_check.cpp")


def test_workspace_layouts_match_their_closed_forms(tmp_path):
    """bench/ws_layout_check.cpp includes only workspace.hpp: generic properties of WsLayout (aligned, disjoint, large enough
    pieces; bytes() covers the last; an empty layout is 0 bytes) and the layouts of four call sites (filtered top-k lists, f32
    kNN lists, the k-means++ block, the SIFT candidate block) against the byte arithmetic those sites used to carry inline."""
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler (g++, c++ or clang++) on PATH"
    exe = str(tmp_path / "ws_layout_check")
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=all", "-o", exe, SRC], capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
