"""The cell container's host staging without a GPU: tests/drivers/host_cells_check.cpp includes nothing but
hemocell_amd/csrc/host_cells.h (standard library only) and checks that appending a cell, the stable compaction, sizing for
a download, the id-only edits and the swap of a built temporary keep the struct's invariants, with and without
force_repulsion, on cells of three vertices."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_cells_invariants(tmp_path):
    exe = str(tmp_path / "host_cells_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "hemocell_amd", "csrc"),
                        os.path.join(ROOT, "tests", "drivers", "host_cells_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert r.stdout.strip() == "host_cells ok"
