"""csrc/workspace.hpp's Carver -- the one statement of a device workspace's layout, run once to measure it and once
to carve it -- compiled for the host and exercised by tests/workspace_check.cpp.  No GPU, no libmq_hip.so."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "macaque-3d-pose-estimation_amd", "csrc")


def test_carver_measures_and_carves_alike(tmp_path):
    """400 pseudo-random take sequences from a fixed seed (element sizes 1, 2, 4, 8, 16; aligns 1 ... 256; counts
    that include 0), each split into an outer layout function with an inner one called on the same carver, under
    -fsanitize=address,undefined:
    measuring and carving give the same offset for every take and the same used(); every pointer has its alignment,
    the ranges are disjoint, in order, with less padding than the alignment, and end at used(); fits() holds with
    exactly used() bytes and not with one fewer; a byte count, an offset or an alignment step that would wrap size_t
    (and an alignment that is no power of two or below alignof(T), and a base off the 256-byte grid) makes fits()
    false and used() SIZE_MAX in both modes, and stays so."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "the workspace check needs a host C++ compiler"
    exe = str(tmp_path / "workspace_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "workspace_check.cpp"),
                    "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "runtime error" not in out.stderr
    assert out.stdout.strip().endswith("400 sequences, 0 failures")
