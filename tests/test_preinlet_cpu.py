"""Zou-He open boundaries and the pre-inlet coupling without a GPU: the C ABI and its binding name the new entry points, the
numpy restatement's completion reproduces the prescribed moments, and the pre-inlet's driving-force arithmetic."""
import os
import re

import numpy as np
import pytest

import open_boundary_ref as OB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["hcl_open_boundary_add", "hcl_open_boundary_add_box", "hcl_open_boundary_clear", "hcl_open_boundary_slots",
               "hcl_open_boundary_set_velocity", "hcl_open_boundary_set_density", "hcl_open_boundary_values",
               "hcl_plane_velocity"]


def test_header_and_binding_name_the_open_boundary_abi():
    src = open(os.path.join(ROOT, "include", "hemocell_amd.h")).read()
    for n in NEW_SYMBOLS:
        assert re.search(r"^int\s+" + n + r"\s*\(", src, flags=re.M), n
    assert "#define HC_OB_VELOCITY 0" in src and "#define HC_OB_PRESSURE 1" in src
    from hemocell_amd import capi
    for n in NEW_SYMBOLS:
        assert n in capi.SIGNATURES, n


def test_host_layer_has_the_palabos_names():
    from hemocell_amd import host
    for n in ("addVelocityBoundary0N", "addVelocityBoundary0P", "addPressureBoundary0N", "addPressureBoundary0P",
              "setBoundaryVelocity", "setBoundaryDensity", "planeVelocity"):
        assert callable(getattr(host.Lattice, n)), n
    assert callable(host.PreInlet.applyPreInlet)


def _random(m, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-0.01, 0.01, size=(m, 19))


@pytest.mark.parametrize("kind", [OB.VEL_0N, OB.VEL_0P])
def test_velocity_completion_gives_the_prescribed_moments(kind):
    m = 2000
    f = _random(m, 3 + kind)
    rng = np.random.default_rng(7)
    val = np.zeros((m, 4))
    val[:, 0] = rng.uniform(-0.05, 0.05, m); val[:, 1] = rng.uniform(-0.02, 0.02, m); val[:, 2] = rng.uniform(-0.02, 0.02, m)
    before = f.copy()
    OB.complete(f, kind, val)
    unknown = [10, 13, 14, 15, 16] if kind == OB.VEL_0N else [1, 4, 5, 6, 7]
    known = [q for q in range(19) if q not in unknown]
    assert np.array_equal(f[:, known], before[:, known])
    rho, u = OB.real_moments(f)
    # rho is what the known populations imply: (S_0 + 2 S_out) / (1 -+ u_x)
    g = before.astype(np.longdouble) + OB.T
    s0 = g[:, [0, 2, 3, 8, 9, 11, 12, 17, 18]].sum(axis=1)
    s_out = g[:, [1, 4, 5, 6, 7] if kind == OB.VEL_0N else [10, 13, 14, 15, 16]].sum(axis=1)
    rho_want = (s0 + 2 * s_out) / (1 - val[:, 0] if kind == OB.VEL_0N else 1 + val[:, 0])
    assert float(np.abs(rho - rho_want).max()) <= 1e-15
    assert float(np.abs(u - val[:, :3]).max()) <= 1e-15


@pytest.mark.parametrize("kind", [OB.PRES_0N, OB.PRES_0P])
def test_pressure_completion_gives_the_prescribed_density(kind):
    m = 2000
    f = _random(m, 11 + kind)
    val = np.zeros((m, 4))
    val[:, 3] = np.random.default_rng(5).uniform(0.98, 1.02, m)
    OB.complete(f, kind, val)
    rho, u = OB.real_moments(f)
    assert float(np.abs(rho - val[:, 3]).max()) <= 1e-15
    assert float(np.abs(u[:, 1:]).max()) <= 1e-15


def test_restated_step_conserves_mass_in_a_periodic_box():
    """the bulk step itself: a periodic box without forces keeps its mass (sum of the stored populations) to round-off"""
    dims = (6, 5, 4)
    S = _random(int(np.prod(dims)), 2).reshape(dims + (19,)) * 0.1
    out = OB.step(S, np.zeros(dims, np.uint8), (True, True, True), 1.0 / 0.8, (0.0, 0.0, 0.0))
    assert abs(float(out.sum()) - float(S.sum())) < 1e-15


def test_driving_force_of_the_fixture_case():
    """host.preinlet_driving_force (what the pre-inlet coupling drives with) against the restatement of
    PreInlet::calculateDrivingForce, for examples/pipeflow_with_preinlet: Re = 0.5 (<preInlet><parameters><Re>), nu_lbm from
    the nuP, dx, dt of its config"""
    from hemocell_amd import host
    Re, nuP, dx, dt = 0.5, 1.1e-6, 5e-7, 1e-7
    nu = nuP * dt / (dx * dx)
    for area in (1257, 317, 52):   # a few gathered plane areas (fluid nodes)
        R, u_max, F = host.preinlet_driving_force(Re, nu, area, "Xpos")
        R_ref = OB.pipe_radius(area)
        assert R == R_ref
        assert (u_max, F) == OB.driving_force(Re, nu, R_ref, "Xpos")
        assert F < 0 and host.preinlet_driving_force(Re, nu, area, "Xneg")[2] == -F
        # Poiseuille in a pipe of radius R: the force that gives the centre-line velocity u_max is 4 nu u_max / R^2
        assert -F == pytest.approx(4 * nu * u_max / R ** 2, rel=1e-15)
    with pytest.raises(host.HcError, match="Xpos and Xneg"):
        host.preinlet_driving_force(Re, nu, 100, "Zpos")
