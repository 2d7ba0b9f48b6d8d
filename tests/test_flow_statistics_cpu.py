"""The running statistics without a GPU: the numpy restatement (tests/flow_statistics_ref.py) on inputs small enough to work out
by hand, the facade header and its example compile and link, and the C ABI declares and binds the hc_stats_* symbols."""
import ctypes
import os
import re
import subprocess

import numpy as np

import flow_statistics_ref as FS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "hemocell_amd", "compat")]

DIMS = (6, 5, 4)
PER = (True, False, True)


def test_cell_density_nearest_node_by_hand():
    pos = np.array([[2.5, 1.5, 0.5],      # exactly on a half node on every axis: floor(p + 0.5) goes up -> (3, 2, 1)
                    [2.49, 1.49, 0.49],   # just below: (2, 1, 0)
                    [-0.6, 2.0, 3.7],     # across the periodic faces of x and z: (-1, 2, 4) -> (5, 2, 0)
                    [6.2, 4.49, -0.5],    # x wraps to 0; y = 4 is the last node; z: floor(0.0) = 0
                    [3.0, -0.51, 1.0],    # outside the closed y face (node -1): dropped
                    [3.0, 4.5, 1.0],      # node 5 of 5 on the closed axis: dropped
                    [1.0, 1.0, 1.0]])     # alive = False: not counted
    alive = np.array([1, 1, 1, 1, 1, 1, 0], bool)
    got = FS.cell_density(pos, alive, DIMS, PER)
    want = np.zeros(DIMS, np.int64)
    for node in ((3, 2, 1), (2, 1, 0), (5, 2, 0), (0, 4, 0)):
        want[node] += 1
    assert np.array_equal(got, want) and got.sum() == 4


def test_cell_density_counts_every_vertex_of_a_node():
    pos = np.tile([[1.2, 2.1, 2.9]], (5, 1))
    got = FS.cell_density(pos, np.ones(5, bool), DIMS, PER)
    assert got[1, 2, 3] == 5 and got.sum() == 5
    assert FS.cell_density(np.zeros((0, 3)), np.zeros(0, bool), DIMS, PER).sum() == 0


TET = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]])


def _tetra(centre, r=0.9):
    """a tetrahedron around `centre` that holds that node and no other"""
    c = np.asarray(centre, dtype=np.float64)
    return c + r * np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]]) + np.array([0.05, 0.03, 0.02])


def test_inside_tetrahedron_around_one_node():
    mask = np.zeros(DIMS, np.uint8)
    got = FS.inside([dict(pos=_tetra((2, 2, 1)), tri=TET)], mask, PER)
    want = np.zeros(DIMS, np.int64); want[2, 2, 1] = 1
    assert np.array_equal(got, want)


def test_inside_wraps_drops_walls_overlaps_and_incomplete_cells():
    mask = np.zeros(DIMS, np.uint8); mask[:, 0, :] = 1; mask[:, -1, :] = 1
    cells = [dict(pos=_tetra((-1, 2, 4)), tri=TET),                  # across the periodic x and z faces: node (5, 2, 0)
             dict(pos=_tetra((3, 0, 1)), tri=TET),                   # around a wall node: no count
             dict(pos=_tetra((3, -1, 1)), tri=TET),                  # around a node beyond the closed face: dropped
             dict(pos=_tetra((1, 2, 2)), tri=TET), dict(pos=_tetra((1, 2, 2), 0.8), tri=TET),   # two cells around one node: 2
             dict(pos=_tetra((4, 3, 2)), tri=TET, complete=False)]   # an incomplete cell has no closed surface
    got = FS.inside(cells, mask, PER)
    want = np.zeros(DIMS, np.int64); want[5, 2, 0] = 1; want[1, 2, 2] = 2
    assert np.array_equal(got, want)
    nv = 4
    packed = np.concatenate([c["pos"] for c in cells[3:]])
    alive = np.ones(len(packed), bool); alive[2 * nv + 1] = False
    split = FS.cells_of(packed, alive, TET, nv)
    assert [c["complete"] for c in split] == [True, True, False]
    assert np.array_equal(FS.inside(split, mask, PER), FS.inside(cells[3:], mask, PER))


def test_inside_skips_a_cell_that_blew_up():
    mask = np.zeros(DIMS, np.uint8)
    big = _tetra((2, 2, 1), r=14.0)   # 28 nodes wide: more than four periods of x (6) and z (4)
    assert FS.inside([dict(pos=big, tri=TET)], mask, PER).sum() == 0


def test_fluid_sums_are_the_host_loop():
    rng = np.random.default_rng(1)
    ref = FS.FluidSums(7)
    acc = np.zeros((7, 16))
    for _ in range(3):
        rho, u, pi = rng.standard_normal(7), rng.standard_normal((7, 3)), rng.standard_normal((7, 6))
        ref.add(rho, u, pi)
        for i in range(7):
            row = [rho[i], *u[i]] + [u[i, a] * u[i, b] for a, b in FS.UU_PAIRS] + list(pi[i])
            for k, v in enumerate(row):
                acc[i, k] += v
    assert ref.samples == 3
    assert np.array_equal(ref.rho_u, acc[:, :4]) and np.array_equal(ref.uu, acc[:, 4:10]) and np.array_equal(ref.pi, acc[:, 10:])


def test_abi_declares_and_binds_the_statistics_symbols():
    from hemocell_amd import capi
    src = open(os.path.join(ROOT, "include", "hemocell_amd.h")).read()
    names = ["hc_stats_create", "hc_stats_destroy", "hc_stats_set_every", "hc_stats_sample", "hc_stats_reset", "hc_stats_samples",
             "hc_stats_download_fluid", "hc_stats_download_cells"]
    lib = ctypes.CDLL(capi.LIB_PATH)
    for n in names:
        assert re.search(r"^int\s+%s\s*\(" % n, src, flags=re.M), n
        assert n in capi.SIGNATURES and hasattr(lib, n), n
    for macro, value in (("HC_STATS_RHO_U", 1), ("HC_STATS_UU", 2), ("HC_STATS_PI", 4), ("HC_STATS_CELL_DENSITY", 8), ("HC_STATS_INSIDE", 16)):
        assert re.search(r"^#define\s+%s\s+%d\s*$" % (macro, value), src, flags=re.M), macro
    from hemocell_amd import host
    assert (host.Statistics.RHO_U, host.Statistics.UU, host.Statistics.PI, host.Statistics.CELL_DENSITY, host.Statistics.INSIDE) == (1, 2, 4, 8, 16)


def test_facade_header_and_example_compile_and_link(tmp_path):
    """compat/helper/flowStatistics.h forwards to compat/flowStatistics.h; the example links against the library, with the HDF5
    writer compiled in where the HDF5 headers are at hand (syntax only: the link recipe with HDF5 is the GPU tests')"""
    from hemocell_amd import capi
    example = os.path.join(ROOT, "examples", "statistics", "pipe_profile.cpp")
    libdir = os.path.dirname(capi.LIB_PATH)
    r = subprocess.run(["g++", "-std=c++14", "-O1", "-Wno-deprecated-declarations"] + INC + [example, "-o", str(tmp_path / "pipe_profile"),
                        "-L" + libdir, "-lhemocell_amd", "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    if os.path.exists("/opt/conda/include/hdf5.h"):
        r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-Wno-deprecated-declarations", "-DHEMOCELL_WITH_HDF5", "-I/opt/conda/include"] + INC + [example],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
    fwd = open(os.path.join(ROOT, "hemocell_amd", "compat", "helper", "flowStatistics.h")).read()
    assert '#include "../flowStatistics.h"' in fwd
