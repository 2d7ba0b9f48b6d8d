"""The CEPAC scalar field without a GPU: properties of the restatement tests/scalar_ref.py that the GPU tests pin the kernel
to (tests/test_gpu_scalar.py) -- conservation, the diffusivity and the advection speed, sources -- and that the Python host
and the C ABI carry the feature."""
import os
import subprocess

import numpy as np
import pytest

import open_boundary_ref as OB
import scalar_ref as SR
from hemocell_amd import host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("HEMOCELL_REFERENCE", "/root/reference")
INC = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "hemocell_amd", "compat")]


def _random_velocity(shape, mask, seed, umax=0.05):
    """a non-uniform velocity field of magnitude <= umax, 0 on nodes that are not fluid"""
    rng = np.random.default_rng(seed)
    u = rng.uniform(-1.0, 1.0, size=tuple(shape) + (3,))
    u *= umax * rng.uniform(0.0, 1.0, size=tuple(shape) + (1,)) / np.linalg.norm(u, axis=-1, keepdims=True)
    u[mask != 0] = 0.0
    assert np.linalg.norm(u, axis=-1).max() <= umax
    return u


def _total(g):
    """sum of C over EVERY node in extended precision: what sits on a wall node is in transit back to the fluid"""
    return float(np.sum(SR.concentration(g).astype(np.longdouble)))


@pytest.mark.parametrize("case", ["periodic box", "walled pipe"])
def test_mass_is_conserved(case):
    """no sources, random non-uniform velocity of magnitude <= 0.05, 200 steps: the relative drift of sum C is <= 1e-12.  The
    relaxation keeps sum_i g_i (sum t_i = 1, sum t_i c_i = 0) and bounce-back and streaming only move populations, so the
    drift is rounding: about 19 roundings of 1e-16 per node and step, which add up like a random walk."""
    if case == "periodic box":
        shape, periodic = (16, 6, 6), (True, True, True)
        mask = np.zeros(shape, np.uint8)
    else:
        shape, periodic = (20, 17, 17), (True, False, False)
        mask, _ = host.pipe_mask(*shape)
    rng = np.random.default_rng(3)
    g = SR.equilibrium(shape, 1.0, mask)
    g[mask == 0] += SR.T * rng.uniform(0.0, 1.0, size=(int((mask == 0).sum()), 1))   # C between 1 and 2, node by node
    u = _random_velocity(shape, mask, 4)
    m0 = _total(g)
    for _ in range(200):
        g = SR.step(g, mask, periodic, 1.0 / 0.8, u)
    drift = abs(_total(g) - m0) / m0
    print("relative drift of sum C after 200 steps (%s): %.3e" % (case, drift))
    assert drift <= 1e-12
    assert np.ptp(SR.concentration(g)[mask == 0]) > 1e-3   # the field has not simply died out


def test_diffusivity_and_advection_speed():
    """32 x 4 x 4 periodic, C0 = 1 + 0.5 sin(2 pi x / 32), tau = 0.8, uniform u = (0.02, 0.01, -0.03), 200 steps: the mode's
    amplitude within 1 % of exp(-D k^2 t), D = (tau - 0.5) / 3, and its phase within 1e-3 rad of -k u_x t.  The populations
    start at the equilibrium of the moving fluid, t_i (Cbar + 3 C c_i.u): started at the rest equilibrium t_i Cbar the flux
    needs about tau steps to reach u C and the mode lags by k u_x (1 - tau) for good (7.9e-4 rad here, measured; none at
    tau = 1), which is an error of the initial state, not of the step"""
    shape, tau, t = (32, 4, 4), 0.8, 200
    k = 2.0 * np.pi / 32
    x = np.arange(32)
    mask = np.zeros(shape, np.uint8)
    C0 = 1.0 + 0.5 * np.sin(k * x)
    u = np.empty(shape + (3,)); u[...] = (0.02, 0.01, -0.03)
    c_u = OB.C @ u[0, 0, 0]
    g = SR.T * ((C0 - 1.0)[:, None, None, None] + 3.0 * C0[:, None, None, None] * c_u) * np.ones(shape + (1,))
    for _ in range(t):
        g = SR.step(g, mask, (True, True, True), 1.0 / tau, u)
    Cx = SR.concentration(g)
    assert np.abs(Cx - Cx[:, :1, :1]).max() < 1e-14   # still a function of x alone
    mode = np.sum((Cx[:, 0, 0] - 1.0) * np.exp(-1j * k * x)) * 2.0 / 32   # A exp(i phi) of A sin(k x + phi) is i times this
    amp, phase = abs(mode), np.angle(1j * mode)
    D = (tau - 0.5) / 3.0
    want_amp, want_phase = 0.5 * np.exp(-D * k * k * t), -k * 0.02 * t
    print("amplitude %.6f (theory %.6f, off by %.3f %%), phase %.6e rad (theory %.6e, off by %.2e)" %
          (amp, want_amp, 100 * abs(amp / want_amp - 1), phase, want_phase, abs(phase - want_phase)))
    assert abs(amp / want_amp - 1.0) <= 0.01
    assert abs(phase - want_phase) <= 1e-3


def test_source_nodes_report_their_value_and_feed_the_field():
    shape, periodic = (12, 7, 7), (True, False, False)
    mask = np.zeros(shape, np.uint8)
    mask[:, 0, :] = mask[:, -1, :] = mask[:, :, 0] = mask[:, :, -1] = 1
    src = SR.Sources(shape)
    src.add((3, 5, 0, 2, 2, 4), 1.75)   # touches the wall y = 0: the wall nodes of the box stay wall
    g = SR.equilibrium(shape, 1.0, mask)
    u = np.zeros(shape + (3,))
    for _ in range(20):
        g = SR.step(g, mask, periodic, 1.0 / 0.9, u, src)
    Cx = SR.concentration(g, mask, src)
    assert np.all(Cx[3:6, 1:3, 2:5] == 1.75)
    plain = SR.concentration(g)   # without the observer's substitution
    assert 1.0 < Cx[7, 2, 3] < 1.75 and Cx[7, 2, 3] > Cx[9, 2, 3]   # it spreads, and decays with distance
    src.clear()
    assert np.array_equal(SR.concentration(g, mask, src), plain)


def test_ninth_source_value_is_refused():
    src = SR.Sources((4, 4, 4))
    for k in range(SR.MAX_SOURCES):
        src.add((k % 4, k % 4, k // 4, k // 4, 0, 0), 1.0 + k)
    src.add((1, 1, 1, 1, 1, 1), 3.0)   # a value already in the table takes no new entry
    with pytest.raises(ValueError, match="more than 8 distinct source values"):
        src.add((2, 2, 2, 2, 2, 2), 99.0)
    assert src.cls[2, 2, 2] == 0 and len(src.values) == 8
    src.add((9, 9, 0, 0, 0, 0), 50.0)   # wholly outside: nothing registered, nothing refused
    assert len(src.values) == 8
    src.add((0, 0, 0, 0, 0, 0), 99.0)   # painting over the only node of value 1.0 gives its slot back
    assert len(src.values) == 8 and 1.0 not in src.values and src.value_field()[0, 0, 0] == 99.0 and src.value_field()[1, 0, 0] == 2.0


def test_host_and_abi_carry_the_field():
    """the names the issue's users call: they do not exist before this feature"""
    from hemocell_amd import capi
    for name in ("hcl_scalar_create", "hcl_scalar_destroy", "hcl_scalar_init_equilibrium", "hcl_scalar_set_source_box",
                 "hcl_scalar_clear_sources", "hcl_scalar_step", "hcl_scalar_download", "hcl_scalar_download_populations",
                 "hcl_scalar_upload_populations", "hcl_scalar_download_velocity", "hcl_scalar_stats", "hcp_sample_scalar"):
        assert name in capi.SIGNATURES
        assert hasattr(capi.lib(), name)
    for name in ("initializeAtEquilibrium", "addSource", "clearSources", "collideAndStream", "concentration", "velocity",
                 "populations", "set_populations", "stats", "destroy"):
        assert callable(getattr(host.Scalar, name))
    assert callable(host.Lattice.createCEPACfield) and callable(host.Cells.sampleScalar)


# ---- the facade
CASE = os.path.join(ROOT, "tests", "golden", "cepac_case")


def test_cepac_example_links_and_the_fixture_is_data(tmp_path):
    from hemocell_amd import capi
    out = str(tmp_path / "cepac_channel")
    libdir = os.path.dirname(capi.LIB_PATH)
    r = subprocess.run(["g++", "-std=c++14", "-O1", "-Wno-deprecated-declarations"] + INC +
                       [os.path.join(ROOT, "examples", "cepac", "cepac_channel.cpp"), "-o", out, "-L" + libdir, "-lhemocell_amd",
                        "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert sorted(os.listdir(CASE)) == ["PLT.pos", "PLT.xml", "RBC.pos", "RBC.xml", "README.md", "config.xml"]
    txt = open(os.path.join(ROOT, "hemocell_amd", "compat", "hemocell.h")).read()
    assert 'refuse("the CEPAC field (createCEPACfield)")' in txt       # the run configurations the library refuses
    assert 'refuse("the CEPAC field (setCEPACOutputs)")' not in txt   # the outputs are stored now


def test_reference_cepac_driver_compiles_unchanged():
    src = os.path.join(REF, "cases", "CEPAC", "CEPAC.cpp")
    if not os.path.exists(src):
        pytest.skip("reference tree not present (it does not travel to the GPU box)")
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-DHEMOCELL_COMPAT_MAIN", "-Wno-deprecated-declarations"] + INC + [src],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
