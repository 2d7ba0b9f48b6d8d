"""Lees-Edwards boundary without a GPU: the reference's leesEdwards driver compiles unchanged against the facade, the
repository's own driver links against libhemocell_amd.so, the C ABI and capi.py name the new entry points, and the numpy
restatement of the pass (tests/lees_edwards_ref.py) behaves as its definition says."""
import math
import os
import re
import subprocess
import xml.etree.ElementTree as ET

import numpy as np
import pytest

import lees_edwards_ref as LE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("HEMOCELL_REFERENCE", "/root/reference")
INC = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "hemocell_amd", "compat")]
CASE = os.path.join(ROOT, "tests", "golden", "lees_edwards_case")
NEW = ["hcl_set_lees_edwards", "hcl_set_lees_edwards_displacement", "hcl_lees_edwards_apply", "hcl_lees_edwards_state"]


def test_reference_lees_edwards_driver_compiles_unchanged():
    src = os.path.join(REF, "cases", "leesEdwards", "leesEdwards.cpp")
    if not os.path.exists(src):
        pytest.skip("reference tree not present (it does not travel to the GPU box)")
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-DHEMOCELL_COMPAT_MAIN", "-Wno-deprecated-declarations"] + INC + [src],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_lees_edwards_example_driver_links(tmp_path):
    from hemocell_amd import capi
    out = str(tmp_path / "lees_edwards")
    libdir = os.path.dirname(capi.LIB_PATH)
    r = subprocess.run(["g++", "-std=c++14", "-O1", "-Wno-deprecated-declarations"] + INC +
                       [os.path.join(ROOT, "examples", "shear", "lees_edwards.cpp"), "-o", out, "-L" + libdir, "-lhemocell_amd",
                        "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_new_symbols_in_header_and_capi():
    src = open(os.path.join(ROOT, "include", "hemocell_amd.h")).read()
    from hemocell_amd import capi
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, src), name
        assert name in capi.SIGNATURES, name
    assert '"lees_edwards"' in src


def _random_state(dims, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-0.02, 0.02, size=(int(np.prod(dims)), 19))


@pytest.mark.parametrize("k", [0, 1, 3, -2, 12])
def test_integer_displacement_copies_node_x_plus_minus_k(k):
    """g = fmod(k, 1) = 0: the copied populations are those of node x+k (top) and x-k (bottom), exactly"""
    dims = (13, 5, 7)
    nx, ny, nz = dims
    f = _random_state(dims, 1)
    out = LE.le_pass(f, dims, 0.7, float(k), -0.01, 0.01).reshape(nx, ny, nz, 19)
    f4 = f.reshape(nx, ny, nz, 19)
    for x in range(nx):
        for tq, sq in LE.TOP_MAP:
            assert np.array_equal(out[x, :, nz - 1, tq], f4[(x + k) % nx, :, nz - 1, sq])
        for tq, sq in LE.BOTTOM_MAP:
            assert np.array_equal(out[x, :, 0, tq], f4[(x - k) % nx, :, 0, sq])
    assert np.array_equal(out[:, :, 1:nz - 1], f4[:, :, 1:nz - 1])   # the other layers are untouched


def test_zero_displacement_is_swaps_and_relaxation():
    """D = 0: the five populations are the node's own pre-pass values (6 <-> 16 and 7 <-> 15 swapped); the other 14 are the
    BGK relaxation towards (rhoBar, j = (v, 0, 0))"""
    dims = (6, 4, 5)
    nx, ny, nz = dims
    f = _random_state(dims, 2)
    omega, vt, vb = 1.0 / 1.82, -1e-3, 1e-3
    out = LE.le_pass(f, dims, omega, 0.0, vt, vb).reshape(nx, ny, nz, 19)
    f4 = f.reshape(nx, ny, nz, 19)
    top, bot = f4[:, :, nz - 1], f4[:, :, 0]
    for tq, sq in LE.TOP_MAP:
        assert np.array_equal(out[:, :, nz - 1, tq], top[:, :, sq])
    for tq, sq in LE.BOTTOM_MAP:
        assert np.array_equal(out[:, :, 0, tq], bot[:, :, sq])
    relaxed = LE.collide_external(top.reshape(-1, 19).copy(), vt, omega).reshape(nx, ny, 19)
    others = [q for q in range(19) if q not in dict(LE.TOP_MAP)]
    assert np.array_equal(out[:, :, nz - 1, others], relaxed[:, :, others])
    # the relaxation conserves rhoBar and moves the momentum towards j = (v, 0, 0)
    rb = top.sum(-1)
    assert np.allclose(relaxed.sum(-1), rb, atol=1e-15)
    jx = (relaxed * LE.C[:, 0]).sum(-1)
    jx0 = (top * LE.C[:, 0]).sum(-1)
    assert np.allclose(jx, (1 - omega) * jx0 + omega * vt, atol=1e-15)


def test_fractional_displacement_interpolates_and_extrapolates():
    dims = (9, 3, 4)
    nx, ny, nz = dims
    f = _random_state(dims, 3)
    f4 = f.reshape(nx, ny, nz, 19)
    for D in (0.37, -0.6):
        out = LE.le_pass(f, dims, 1.0, D, 0.0, 0.0).reshape(nx, ny, nz, 19)
        g = math.fmod(D, 1.0)
        x = 4
        s1, s2 = math.ceil(D + x) % nx, math.floor(D + x) % nx
        assert out[x, 0, nz - 1, 3] == g * f4[s1, 0, nz - 1, 3] + (1 - g) * f4[s2, 0, nz - 1, 3]
        b1, b2 = math.floor(-D + x) % nx, math.ceil(-D + x) % nx
        assert out[x, 0, 0, 7] == g * f4[b1, 0, 0, 15] + (1 - g) * f4[b2, 0, 0, 15]
    assert math.fmod(-0.6, 1.0) < 0   # D < 0: g < 0 and the reference extrapolates; the restatement keeps it


def test_fixture_parameters():
    """cases/leesEdwards: 500 s^-1 at dt 1e-7 and dx 0.5 um: a 50^3 box, v_top = -(nz-1) gamma / 2 = -1.225e-3 lu and
    d = gamma * dt = 5e-12 lu per iteration (the reference multiplies the lattice shear rate by the physical dt)"""
    dom = ET.parse(os.path.join(CASE, "config.xml")).getroot().find("domain")
    rd = lambda k: float(dom.find(k).text)
    dx, dt, shear = rd("dx"), rd("dt"), rd("shearrate")
    n = int(100.0 * (1e6 * dx))
    assert n == 50
    gamma = shear * dt
    vt, vb = LE.velocities(n, gamma)
    assert math.isclose(vt, -1.225e-3, rel_tol=1e-12) and vb == -vt
    assert math.isclose(gamma * dt, 5e-12, rel_tol=1e-12)
    assert LE.displacement(gamma * dt, 1000, n) == math.fmod(gamma * dt * 1000, 50.0)
    assert open(os.path.join(CASE, "RBC_HO.pos")).readline().strip() == "515"
