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


def _walled_channel(dims):
    m = np.zeros(dims, np.uint8)
    m[:, 0, :] = m[:, -1, :] = 1
    m[:, :, 0] = m[:, :, -1] = 1
    return m


def _four_kinds(dims, seed):
    """velocity 0N and pressure 0N patches on x = 0, velocity 0P and pressure 0P patches on x = nx - 1, split in y"""
    nx, ny, nz = dims
    h = ny // 2
    rng = np.random.default_rng(seed)
    code = -np.ones(dims, np.int64)
    val = []
    for kind, x, ys in ((OB.VEL_0N, 0, slice(0, h)), (OB.PRES_0N, 0, slice(h, ny)), (OB.VEL_0P, nx - 1, slice(0, h)),
                        (OB.PRES_0P, nx - 1, slice(h, ny))):
        n = code[x, ys].size
        code[x, ys] = ((len(val) + np.arange(n)) << 2 | kind).reshape(code[x, ys].shape)
        for _ in range(n):
            if kind in (OB.VEL_0N, OB.VEL_0P):
                val.append([rng.uniform(-0.02, 0.02), rng.uniform(-0.01, 0.01), rng.uniform(-0.01, 0.01), 1.0])
            else:
                val.append([0.0, 0.0, 0.0, 1.0 + rng.uniform(-0.01, 0.01)])
    return code, np.array(val)


@pytest.mark.parametrize("with_force", [False, True])
def test_observe_gives_the_prescribed_values_on_open_nodes(with_force):
    """observe() on a stepped channel: velocity nodes show u_bc + F / 2 (j = rho u_bc), pressure nodes the
    prescribed density and u_y = u_z = F / 2; with F = 0 that is u_bc and u_y = u_z = 0.  Bound: 1e-14 against the prescribed
    values in np.longdouble, as test_completed_moments_equal_the_prescribed_values.  Nodes without a code, and open-boundary
    codes on bounce-back nodes, keep their plain moments."""
    dims = (10, 9, 8)
    mask = _walled_channel(dims)
    code, val = _four_kinds(dims, 3)
    rng = np.random.default_rng(12)
    body = (2e-6, 3e-7, -1e-7) if with_force else (0.0, 0.0, 0.0)
    F = 1e-5 * rng.standard_normal(dims + (3,)) * (mask == 0)[..., None] if with_force else None
    S = rng.uniform(-0.005, 0.005, size=dims + (19,))
    for _ in range(4):
        S = OB.step(S, mask, (False, False, False), 1.0 / 0.9, body, code, val, F=F)
    rho, u, pi = OB.observe(S, mask, (False, False, False), body, F, code, val)
    rho_plain, u_plain, pi_plain = OB.observe(S, mask, (False, False, False), body, F)
    half = (np.asarray(body, np.longdouble) + (F if F is not None else 0.0)) / 2
    half = np.broadcast_to(half, dims + (3,))
    fluid = mask == 0
    for kind in range(4):
        sel = fluid & (code >= 0) & ((code & 3) == kind)
        assert sel.any()
        v = val[code[sel] >> 2].astype(np.longdouble)
        if kind in (OB.VEL_0N, OB.VEL_0P):
            assert float(np.abs(u[sel] - (v[:, :3] + half[sel])).max()) <= 1e-14
        else:
            assert float(np.abs(rho[sel] - v[:, 3]).max()) <= 1e-14
            assert float(np.abs(u[sel][:, 1:] - half[sel][:, 1:]).max()) <= 1e-14
        assert float(np.abs(rho[sel] - rho_plain[sel]).max()) > 1e-3   # the unknown populations came from outside as zeros
    untouched = ~(fluid & (code >= 0))
    assert np.array_equal(rho[untouched], rho_plain[untouched]) and np.array_equal(u[untouched], u_plain[untouched])
    assert np.array_equal(pi[untouched], pi_plain[untouched])
    # Pi_neq of the completed populations, independently in extended precision
    P = S.reshape(-1, 19).copy()
    OB._complete_open(P, fluid.reshape(-1), code, val)
    g = P.astype(np.longdouble)
    c = OB.C.astype(np.longdouble)
    r = g.sum(axis=1); j = g @ c
    want = np.stack([(g * c[:, a] * c[:, b]).sum(axis=1) - j[:, a] * j[:, b] / (1 + r) - (r / 3 if a == b else 0)
                     for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))], axis=1)
    assert float(np.abs(pi.reshape(-1, 6) - want).max()) <= 1e-15


def test_restated_step_with_boxes_walls_and_a_force_field():
    """the additions to step(): a zero force field and an all-covering box change nothing but what they say; the last box wins;
    a moving wall at rest is a bounce-back wall, and a moving one adds 6 t_i (c_i . u_w) of momentum per reflected population"""
    dims = (7, 6, 5)
    per = (True, False, False)
    mask = _walled_channel(dims)
    rng = np.random.default_rng(2)
    S = rng.uniform(-0.005, 0.005, size=dims + (19,))
    body, omega = (1e-6, -2e-6, 3e-6), 1.0 / 0.8
    base = OB.step(S, mask, per, omega, body)
    assert np.array_equal(OB.step(S, mask, per, omega, body, F=np.zeros(dims + (3,))), base)
    everywhere = (0, 6, 0, 5, 0, 4)
    assert np.array_equal(OB.step(S, mask, per, omega, (9.0, 9.0, 9.0), boxes=[(1, 2, 1, 2, 1, 2), everywhere],
                                  box_forces=[(5.0, 5.0, 5.0), body]), base)
    F = 1e-5 * rng.standard_normal(dims + (3,))
    one = OB.step(S, mask, per, omega, (0.0, 0.0, 0.0), boxes=[(2, 3, 0, 5, 0, 4)], box_forces=[body], F=F)
    Fb = F.copy(); Fb[2:4] += np.asarray(body)
    assert np.array_equal(one, OB.step(S, mask, per, omega, (0.0, 0.0, 0.0), F=Fb))
    m3 = mask.copy(); m3[:, 0, :] = 3
    assert np.array_equal(OB.step(S, m3, per, omega, body, wall_u={3: (0.0, 0.0, 0.0)}), base)
    w = np.array([0.01, 0.0, -0.003])
    moved = OB.step(S, m3, per, omega, body, wall_u={3: w})
    # what the wall nodes hand to the fluid in one step: sum over the wall nodes and i of c_i * (-6 t_i c_i . u_w) reflected into
    # opp(i), i.e. + 6 t_i (c_i . u_w) c_i per direction -> 2 u_w per wall node over all 18 directions (sum t_i c_ia c_ib = 1/3)
    n_wall = int((m3 == 3).sum())
    dP = (moved - base).reshape(-1, 19) @ OB.C
    assert np.abs(dP.sum(axis=0) - 2.0 * n_wall * w).max() <= 1e-12 + np.abs(_lost_through_the_faces(m3, w)).max()


def _lost_through_the_faces(mask, w):
    """momentum the moving-wall nodes send out of the non-periodic y and z faces (it leaves the domain): per wall node and
    direction i pointing outside, 6 t_i (c_i . u_w) c_i"""
    lost = np.zeros(3)
    nx, ny, nz = mask.shape
    for x, y, z in zip(*np.nonzero(mask == 3)):
        for q in range(1, 19):
            c = OB.C[q]
            ty, tz = y + c[1], z + c[2]
            if ty < 0 or ty >= ny or tz < 0 or tz >= nz:
                lost += 6.0 * OB.T[q] * float(c @ w) * c
    return lost


def _two_kinds(dims, inlet, outlet, seed):
    """one kind over the plane x = 0 and one over x = nx - 1"""
    nx, ny, nz = dims
    rng = np.random.default_rng(seed)
    code = -np.ones(dims, np.int64)
    val = []
    for kind, x in ((inlet, 0), (outlet, nx - 1)):
        code[x] = ((len(val) + np.arange(ny * nz)) << 2 | kind).reshape(ny, nz)
        for _ in range(ny * nz):
            if kind in (OB.VEL_0N, OB.VEL_0P):
                sign = 1.0 if kind == OB.VEL_0N else -1.0   # inflow on either side
                val.append([sign * rng.uniform(0.0, 0.02), rng.uniform(-0.01, 0.01), rng.uniform(-0.01, 0.01), 1.0])
            else:
                val.append([0.0, 0.0, 0.0, 1.0 + rng.uniform(-0.01, 0.01)])
    return code, np.array(val)


@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("layout", ["0N velocity, 0P pressure", "0P velocity, 0N pressure", "four kinds"])
def test_c_oracle_equals_the_restatement_bit_for_bit(orc, layout, fused):
    """orc_lattice_set_open_boundary: 50 steps of a walled channel with a body force from random populations, in both
    collide forms, every node compared with step() after every step; orc_node_rho_u against observe().  All four kinds run
    (two per lattice, and the four at once).  The states compared stay finite with |rho - 1| < 0.1 on fluid nodes."""
    from oracle import oracle as O
    dims = (12, 9, 8)
    per = (False, False, False)
    omega, body = 1.0 / 0.9, (2e-6, 3e-7, -1e-7)
    mask = _walled_channel(dims)
    if layout == "four kinds":
        code, val = _four_kinds(dims, 5)
    else:
        code, val = _two_kinds(dims, *((OB.VEL_0N, OB.PRES_0P) if layout.startswith("0N") else (OB.PRES_0N, OB.VEL_0P)), seed=6)
    assert set(int(k) for k in code[code >= 0] & 3) == ({0, 1, 2, 3} if layout == "four kinds" else
                                                        ({0, 3} if layout.startswith("0N") else {1, 2}))
    L = O.OracleLattice(orc, *dims, (0, 0, 0), omega)
    try:
        L.set_mask(mask); L.set_force_uniform(body)
        L.set_open_boundary(code, val)
        L.ptr.contents.fused = fused
        S = np.random.default_rng(8).uniform(-0.005, 0.005, size=dims + (19,))
        L.f[:] = S.reshape(-1, 19)
        for it in range(50):
            S = OB.step(S, mask, per, omega, body, code, val)
            L.collide_stream()
            assert np.array_equal(L.f.reshape(dims + (19,)), S), it
            rho, u, _ = OB.observe(S, mask, per, body, None, code, val)
            assert np.isfinite(S).all() and float(np.abs(rho[mask == 0] - 1.0).max()) < 0.1
        rho_o, u_o = np.empty(L.n), np.empty((L.n, 3))
        r = np.zeros(1)
        for k in range(L.n):
            orc.orc_node_rho_u(L.ptr, k, O.dptr(r), O.dptr(u_o[k]))
            rho_o[k] = r[0]
        assert np.array_equal(rho_o.reshape(dims), rho) and np.array_equal(u_o.reshape(dims + (3,)), u)
        # without the table the step is the plain one again
        L.set_open_boundary(None, None)
        L.collide_stream()
        assert np.array_equal(L.f.reshape(dims + (19,)), OB.step(S, mask, per, omega, body))
    finally:
        L.destroy()
