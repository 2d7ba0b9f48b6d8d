"""The pre-inlet through the C++ facade, without a GPU: the reference's eight pre-inlet drivers and the twenty drivers of
oracle/ref_drivers.py compile unchanged against hemocell_amd/compat, the repository's own driver links, and the facade's
host-side geometry and pulse functions (tests/drivers/preinlet_geometry.cpp calls them) give the boxes that
helper/preInlet.cpp's rules give by hand and the values of a numpy restatement of PreInlet::interpolate."""
import math
import os
import subprocess

import numpy as np
import pytest

from oracle import ref_drivers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("HEMOCELL_REFERENCE", "/root/reference")
INC = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "hemocell_amd", "compat")]
PREINLET_DRIVERS = ["examples/pipeflow_with_preinlet/pipeflow_with_preinlet.cpp",
                    "examples/curvedflow_with_preinlet/curvedflow_with_preinlet.cpp", "cases/AR2/AR2.cpp",
                    "cases/AR2_pulsatile/AR2_pulsatile.cpp", "cases/AR2_stiff/AR2_stiff.cpp",
                    "cases/injured_vessel/injured_vessel.cpp", "cases/preinlet_shear/preinlet_shear.cpp",
                    "cases/stl_preinlet/stl_preinlet.cpp"]


def _syntax_only(driver):
    src = os.path.join(REF, driver)
    if not os.path.exists(src):
        pytest.skip("reference tree not present (it does not travel to the GPU box)")
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-DHEMOCELL_COMPAT_MAIN", "-Wno-deprecated-declarations"] + INC + [src],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


@pytest.mark.parametrize("driver", PREINLET_DRIVERS)
def test_reference_preinlet_driver_compiles_unchanged(driver):
    _syntax_only(driver)


@pytest.mark.parametrize("driver", sorted(ref_drivers.DRIVERS.values()))
def test_reference_driver_still_compiles(driver):
    _syntax_only(driver)


def _link(tmp_path, source, name):
    from hemocell_amd import capi
    out = str(tmp_path / name)
    libdir = os.path.dirname(capi.LIB_PATH)
    r = subprocess.run(["g++", "-std=c++14", "-O1", "-Wno-deprecated-declarations"] + INC + [os.path.join(ROOT, source), "-o", out,
                        "-L" + libdir, "-lhemocell_amd", "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def test_preinlet_example_driver_links(tmp_path):
    _link(tmp_path, "examples/preinlet/pipe_with_preinlet.cpp", "pipe_with_preinlet")


@pytest.fixture(scope="module")
def geom(tmp_path_factory):
    exe = _link(tmp_path_factory.mktemp("geom"), "tests/drivers/preinlet_geometry.cpp", "preinlet_geometry")

    def run(*args, rc=0):
        r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
        assert r.returncode == rc, r.stdout + r.stderr
        return r.stdout + r.stderr
    return run


def _parse(out):
    return {l.split()[0]: [float(v) for v in l.split()[1:]] for l in out.strip().splitlines()}


# The flag matrix is 9 x 7 x 7 with fluid where the two in-plane coordinates (u, v; ascending axis order) lie in [2, 4] x [4, 6],
# lengthN = 5 and particleEnvelope = 3, the slice is the matrix's face on the direction's side.  By helper/preInlet.cpp:
# the slice's fluid box, enlarged by 1 (u: 1..5, v: 3..7, the axis: face - 1 .. face + 1), extended by 5 away from the domain,
# v clipped to the lattice's 6 (:453-559); fluidInlet = that cut with the matrix's box, flattened to its last plane for *neg
# and its first for *pos (:399-422); the send box = fluidInlet moved 5 into the pre-inlet, 3 long (:267-294); offset +-5 (:317-335).
# Boxes are x0 x1 y0 y1 z0 z1.
BY_HAND = {
    "Xneg": dict(location=[-6, 1, 1, 5, 3, 6], fluidInlet=[1, 1, 1, 5, 3, 6], sendBox=[-4, -1, 1, 5, 3, 6], offset=[5, 0, 0], shift=[-1, 1, 3]),
    "Xpos": dict(location=[7, 14, 1, 5, 3, 6], fluidInlet=[7, 7, 1, 5, 3, 6], sendBox=[9, 12, 1, 5, 3, 6], offset=[-5, 0, 0], shift=[2, 1, 3]),
    "Yneg": dict(location=[1, 5, -6, 1, 3, 6], fluidInlet=[1, 5, 1, 1, 3, 6], sendBox=[1, 5, -4, -1, 3, 6], offset=[0, 5, 0], shift=[1, -1, 3]),
    "Ypos": dict(location=[1, 5, 5, 12, 3, 6], fluidInlet=[1, 5, 5, 5, 3, 6], sendBox=[1, 5, 7, 10, 3, 6], offset=[0, -5, 0], shift=[1, 0, 3]),
    "Zneg": dict(location=[1, 5, 3, 6, -6, 1], fluidInlet=[1, 5, 3, 6, 1, 1], sendBox=[1, 5, 3, 6, -4, -1], offset=[0, 0, 5], shift=[1, 3, -1]),
    "Zpos": dict(location=[1, 5, 3, 6, 5, 12], fluidInlet=[1, 5, 3, 6, 5, 5], sendBox=[1, 5, 3, 6, 7, 10], offset=[0, 0, -5], shift=[1, 3, 0]),
}


@pytest.mark.parametrize("direction", sorted(BY_HAND))
def test_geometry_by_hand(geom, direction):
    """location, fluidInlet, the send box and its offset as written out by hand above; the window is the send box in the
    pre-inlet's local coordinates with its faces half a node outside (nodes 2 .. 5 of 8: 1.5 .. 5.5 in every direction), the
    shift takes a local position to the global one and adds the offset"""
    got = _parse(geom("geometry", direction, "slice", 5, 3, 1))
    for key, want in BY_HAND[direction].items():
        assert got[key] == want, (key, got[key], want)
    assert got["window"] == [1.5, 5.5]


@pytest.mark.parametrize("direction", sorted(BY_HAND))
def test_geometry_without_a_lattice_is_not_clipped(geom, direction):
    """preInletFromSlice before initializeLattice (examples/pipeflow_with_preinlet): v keeps the 7 the enlargement gave it;
    fluidInlet is cut with the flag matrix anyway"""
    got = _parse(geom("geometry", direction, "slice", 5, 3, 0))
    want = list(BY_HAND[direction]["location"])
    axis = "XYZ".index(direction[0])
    v = 1 if axis == 2 else 2   # the second in-plane axis
    want[2 * v + 1] = 7
    assert got["location"] == want
    assert got["fluidInlet"] == BY_HAND[direction]["fluidInlet"]


def test_geometry_auto_from_boundary(geom):
    """autoPreinletFromBoundary: the slice is the plane one node inside the face (:596-619), so everything lies one node further in"""
    got = _parse(geom("geometry", "Xneg", "auto", 5, 3, 1))
    assert got["location"] == [-5, 2, 1, 5, 3, 6] and got["fluidInlet"] == [2, 2, 1, 5, 3, 6]
    assert got["sendBox"] == [-3, 0, 1, 5, 3, 6] and got["shift"] == [0, 1, 3] and got["window"] == [1.5, 5.5]
    got = _parse(geom("geometry", "Zpos", "auto", 5, 3, 1))
    assert got["location"] == [1, 5, 3, 6, 4, 11] and got["fluidInlet"] == [1, 5, 3, 6, 4, 4] and got["sendBox"] == [1, 5, 3, 6, 6, 9]


@pytest.mark.parametrize("direction", sorted(BY_HAND))
def test_geometry_refusals(geom, direction):
    assert "Not a flat slice, refusing to create preInlet" in geom("geometry", direction, "thick", 5, 3, 1, rc=1)
    assert "no preinlet found, is it in the correct location?" in geom("geometry", direction, "empty", 5, 3, 1, rc=1)


@pytest.mark.parametrize("what, message", [("twice", "declared twice"), ("outside", "lies outside the lattice"),
                                           ("le-then-open", "do not combine"), ("open-then-le", "do not combine")])
def test_zou_he_names_record_and_refuse(geom, what, message):
    """the facade's description of the open boundaries: consecutive records per (kind, axis, side), setBoundaryVelocity /
    setBoundaryDensity reach the declared nodes only (node (0, 1, 1) is the 7th of the inlet plane) and leave the mask alone;
    a node declared twice, a node outside the lattice and Lees-Edwards beside open boundaries (either order) are refused"""
    out = geom("refuse", what, rc=1)
    if what != "le-then-open":   # (there the first declaration is the refused call)
        assert "declared 2 records, 25 + 25 nodes, u 0.01 rho 1.01 mask 0" in out
    assert message in out and "not refused" not in out


# ---- the pulse: PreInlet::interpolate (helper/preInlet.cpp:841-870) and setDrivingForceTimeDependent (:874-886) restated
TIMES = np.array([0.0, 0.25, 0.5, 0.75, 1.0])
VALUES = np.array([0.6, 1.4, 1.0, 0.7, 0.6])


def interpolate_ref(x, extrapolate):
    n = len(TIMES)
    if x >= TIMES[n - 2]:
        i = n - 2
    else:
        i = 0
        while x > TIMES[i + 1]:
            i += 1
    xL, yL, xR, yR = TIMES[i], VALUES[i], TIMES[i + 1], VALUES[i + 1]
    if not extrapolate:
        if x < xL:
            yR = yL
        if x > xR:
            yL = yR
    return float(yL + (yR - yL) / (xR - xL) * (x - xL))


@pytest.mark.parametrize("extrapolate", [0, 1])
@pytest.mark.parametrize("x", [-0.1, 0.0, 0.1, 0.25, 0.6, 0.75, 1.0, 1.3])
def test_interpolate_matches_restatement(geom, x, extrapolate):
    got = float(geom("interpolate", repr(x), extrapolate))
    assert got == interpolate_ref(x, bool(extrapolate))


def test_interpolate_end_points():
    """the restatement itself: the table's values at its points, clamped beyond the ends unless extrapolating"""
    assert interpolate_ref(0.0, False) == 0.6 and interpolate_ref(1.0, False) == 0.6 and interpolate_ref(0.25, True) == 1.4
    assert interpolate_ref(-0.1, False) == 0.6 and interpolate_ref(1.3, False) == 0.6
    assert math.isclose(interpolate_ref(-0.1, True), 0.6 - 0.1 * (1.4 - 0.6) / 0.25, rel_tol=1e-15)
    assert math.isclose(interpolate_ref(1.3, True), 0.6 + 0.3 * (0.6 - 0.7) / 0.25, rel_tol=1e-15)


@pytest.mark.parametrize("t", [0.0, 3e-6, 1e-5, 2e-5, 2.7e-5, 4.05e-5])
def test_pulse_factor_wraps_by_pfrequency(geom, t):
    """pFrequency = 50000 at a pulse of 1 s: one period is 2e-5 s, so t = 2e-5 is t = 0 again and 2.7e-5 is 0.7e-5"""
    pf, end = 50000.0, float(TIMES[-1])
    phase = math.fmod(t * (pf * end), end)
    want = interpolate_ref(phase, False) / (sum(VALUES.tolist()) / len(VALUES))   # PreInlet::average adds in order
    assert float(geom("pulse", repr(pf), repr(t))) == want
    if t == 2e-5:   # up to the rounding of t * pFrequency
        assert math.isclose(want, float(geom("pulse", repr(pf), "0.0")), rel_tol=1e-12)
