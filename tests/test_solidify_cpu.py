"""Solidify mechanics without a GPU: hand-made cases for the restatement tests/solidify_ref.py, the symbols and host names, the
fixture directory."""
import os
import subprocess

import numpy as np
import pytest

import solidify_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = os.path.join(ROOT, "tests", "golden", "solidify_case")
REF = os.environ.get("HEMOCELL_REFERENCE", "/root/reference")
INC = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "hemocell_amd", "compat")]


def test_site_rule_with_an_enclosed_wall_node():
    """a 5 x 5 x 4 box, not periodic: a two-layer floor with a hole above one node.  Every floor node of the upper layer touches
    fluid; of the lower layer only the nodes around the hole do; nodes outside the box are not visited"""
    m = np.zeros((5, 5, 4), np.uint8)
    m[:, :, :2] = 1
    m[2, 2, 1] = 0
    b = SR.populate(np.zeros_like(m), m, (False, False, False), (0, 4, 0, 4, 0, 3))
    assert b[:, :, 1].sum() == 24 and b[2, 2, 1] == 0
    assert b[1:4, 1:4, 0].all() and b[:, :, 0].sum() == 9      # the lower layer sees fluid only through the hole
    assert not b[:, :, 2:].any()
    part = SR.populate(np.zeros_like(m), m, (False, False, False), (-2, 1, 3, 9, 1, 1))
    assert part.sum() == 4 and part[:2, 3:, 1].all()
    assert np.array_equal(SR.populate(part, m, (False, False, False), (0, 4, 0, 4, 0, 3)), b)   # calls add up


def test_the_27_neighbours_wrap_on_periodic_axes_only():
    """a wall column at x = 0 whose only fluid neighbours lie across the x seam: a site when x is periodic, none when it is not"""
    m = np.ones((4, 3, 3), np.uint8)
    m[3, :, :] = 0
    m[1, :, :] = 1
    box = (0, 0, 0, 2, 0, 2)
    assert SR.populate(np.zeros_like(m), m, (True, False, False), box)[0].all()
    assert not SR.populate(np.zeros_like(m), m, (False, False, False), box).any()
    # the flag pass: the site (0, 1, 0) reaches a vertex at x = 3.8 through the seam, at the distance to the unwrapped site (4, 1, 0)
    m = np.zeros((4, 3, 4), np.uint8)
    m[:, :, 0] = 1
    b = np.zeros_like(m)
    b[0, 1, 0] = 1
    T = np.full(m.size, 1e-4)
    pos = np.array([[3.8, 1.0, 1.0], [3.8, 1.0, 1.0]])
    for per, want in (((True, False, False), True), ((False, False, False), False)):
        fl, cand = SR.flag(np.zeros(2, bool), pos, [True, False], b, m, per, T, 1.1, 10.0)
        assert list(fl) == [want, False] and list(cand) == [want, False]    # the second vertex is a removed particle


def test_a_vertex_exactly_at_the_threshold_distance():
    m = np.zeros((6, 6, 5), np.uint8)
    m[:, :, 0] = 1
    b = (m != 0).astype(np.uint8)
    T = np.full(m.size, 2e-5)                          # |T / 1e-7| = 200
    pos = np.array([[2.0, 3.0, 1.25], [2.0, 3.0, np.nextafter(1.25, 2.0)], [2.5, 3.5, 0.75], [2.0, 3.0, 1.6], [2.0, 3.0, 0.3]])
    live = np.ones(5, bool)
    fl, cand = SR.flag(np.zeros(5, bool), pos, live, b, m, (True, True, False), T, 1.25, 100.0)
    assert list(cand) == [True, False, True, False, True]
    assert list(fl) == [True, False, True, False, False]     # the last one's nearest node is a wall node: Tresca 0
    fl, _ = SR.flag(fl, pos, live, b, m, (True, True, False), T, 1.25, 300.0)
    assert list(fl) == [True, False, True, False, False]     # set flags stay set
    assert not SR.flag(np.zeros(5, bool), pos, live, b, m, (True, True, False), T, 1.25, 300.0)[0].any()


def test_tresca_of_known_tensors():
    pi = np.array([[0, 1e-4, 0, 0, 0, 0], [2e-4, 0, 0, -1e-4, 0, -1e-4], [1e-4, 0, 0, 1e-4, 0, 1e-4], [0, 0, 0, 0, 0, 0]], dtype=np.float64)
    t, norm = SR.tresca(pi, np.ones(4), 1.0, np.zeros(4, np.uint8))
    assert np.allclose(t, [1.5e-4, 2.25e-4, 0.0, 0.0], rtol=1e-12, atol=1e-18) and norm[3] == 0.0
    assert np.all(SR.tresca(pi, np.ones(4), 1.0, np.ones(4, np.uint8))[0] == 0.0)


def test_symbols_and_host_names_exist():
    from hemocell_amd import capi, host
    names = ("hcl_binding_populate", "hcl_binding_clear", "hcl_binding_download", "hcl_binding_upload", "hcl_download_tresca",
             "hcp_type_set_solidify", "hcp_set_solidify_timescale", "hcp_solidify_prepare", "hcp_solidify_flag",
             "hcp_solidify_flags_download", "hcp_solidify_flags_upload", "hcp_solidify_counts")
    header = open(os.path.join(ROOT, "include", "hemocell_amd.h")).read()
    lib = capi.lib()
    for n in names:
        assert n in capi.SIGNATURES and n + "(" in header and hasattr(lib, n), n
    for n in ("populateBindingSites", "bindingSites", "tresca"):
        assert callable(getattr(host.Lattice, n)), n
    for n in ("setSolidifyTimeScaleSeparation", "prepareSolidification", "solidifyCells", "solidifyFlags", "setSolidifyFlags", "solidify_counts"):
        assert callable(getattr(host.Cells, n)), n
    assert "solidify" in host.CellType.__init__.__code__.co_varnames


def test_fixture_directory_and_thresholds():
    from hemocell_amd import host
    assert sorted(os.listdir(CASE)) == ["PLT.pos", "PLT.xml", "README.md", "config.xml"]
    m = host.read_material(os.path.join(CASE, "PLT.xml"))
    assert m["distanceThreshold"] == 1.5 and m["shearThreshold"] == 100.0
    rows = open(os.path.join(CASE, "PLT.pos")).read().split()
    assert int(rows[0]) == 3 and len(rows) == 1 + 3 * 6


def test_the_ray_cast_is_one_copy():
    """interior.hip and solidify.hip include the same ray cast; neither keeps a copy of its own"""
    src = {n: open(os.path.join(ROOT, "hemocell_amd", "csrc", n)).read() for n in ("interior.hip", "solidify.hip", "raycast.h")}
    for n in ("interior.hip", "solidify.hip"):
        assert '#include "raycast.h"' in src[n] and "int moller_trumbore(" not in src[n] and "void stage_cell(" not in src[n]
    assert "int moller_trumbore(" in src["raycast.h"] and "void stage_cell(" in src["raycast.h"]
    assert "solidify.hip" in open(os.path.join(ROOT, "hemocell_amd", "csrc", "Makefile")).read()


# ---- the facade

def test_solidify_example_links(tmp_path):
    from hemocell_amd import capi
    out = str(tmp_path / "solidify_channel")
    libdir = os.path.dirname(capi.LIB_PATH)
    r = subprocess.run(["g++", "-std=c++14", "-O1", "-Wno-deprecated-declarations"] + INC +
                       [os.path.join(ROOT, "examples", "solidify", "solidify_channel.cpp"), "-o", out, "-L" + libdir, "-lhemocell_amd",
                        "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


@pytest.mark.parametrize("driver", ["cases/solidify_example/solidify_example.cpp", "cases/CEPAC/CEPAC.cpp"])
def test_reference_drivers_compile_unchanged(driver):
    src = os.path.join(REF, *driver.split("/"))
    if not os.path.exists(src):
        pytest.skip("reference tree not present (it does not travel to the GPU box)")
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-DSOLIDIFY_MECHANICS", "-DHEMOCELL_COMPAT_MAIN", "-Wno-deprecated-declarations"] + INC + [src],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_no_stale_refusals_in_the_facade():
    txt = open(os.path.join(ROOT, "hemocell_amd", "compat", "hemocell.h")).read()
    for gone in ("enableSolidifyMechanics", "setSolidifyTimeScaleSeperation", "prepareSolidification"):
        assert 'refuse("solidify mechanics (%s)")' % gone not in txt
    # the combinations that stay refused keep these lines
    assert 'refuse("solidify mechanics (solidifyCells)")' in txt and 'refuse("binding sites (populateBindingSites)")' in txt
    assert os.path.exists(os.path.join(ROOT, "hemocell_amd", "compat", "bindingField.h"))
