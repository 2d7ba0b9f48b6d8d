"""Zou-He open boundaries on the GPU against the numpy restatement in tests/open_boundary_ref.py, their invariants, a channel
run to steady state, and the one-process pre-inlet coupling (host.PreInlet)."""
import numpy as np
import pytest

import open_boundary_ref as OB

pytestmark = pytest.mark.gpu


def _channel_mask(nx, ny, nz):
    m = np.zeros((nx, ny, nz), np.uint8)
    m[:, 0, :] = m[:, -1, :] = 1
    m[:, :, 0] = m[:, :, -1] = 1
    return m


def _parabola(ny, nz, u_max):
    """a Poiseuille-like profile on the fluid nodes 1..n-2 of a walled cross-section, [ny][nz]"""
    y = (np.arange(ny) - (ny - 1) / 2.0) / ((ny - 2) / 2.0)
    z = (np.arange(nz) - (nz - 1) / 2.0) / ((nz - 2) / 2.0)
    p = u_max * np.clip(1 - y[:, None] ** 2, 0, None) * np.clip(1 - z[None, :] ** 2, 0, None)
    return p


def _open_channel(gpu, dims, omega, body, u_max, n_pressure=3):
    """walled x channel: velocity 0N nodes on the plane x = 0 with a parabolic profile, a pressure 0P box (rho = 1) over the
    last n_pressure planes.  Returns the lattice, the mask, ob_code and ob_val as the restatement wants them."""
    nx, ny, nz = dims
    L = gpu.Lattice(nx, ny, nz, (False, False, False), omega)
    mask = _channel_mask(nx, ny, nz)
    L.defineBounceBack(mask)
    L.setExternalVector(body)
    first_v, nv = L.addVelocityBoundary0N((0, 0, 0, ny - 1, 0, nz - 1))
    prof = _parabola(ny, nz, u_max)
    u = np.zeros((ny * nz, 3)); u[:, 0] = prof.reshape(-1); u[:, 1] = 0.1 * prof.reshape(-1); u[:, 2] = -0.05 * prof.reshape(-1)
    L.setBoundaryVelocity((0, 0, 0, ny - 1, 0, nz - 1), u)
    first_p, npres = L.addPressureBoundary0P((nx - n_pressure, nx - 1, 0, ny - 1, 0, nz - 1))
    L.setBoundaryDensity((nx - n_pressure, nx - 1, 0, ny - 1, 0, nz - 1), 1.0)
    code = -np.ones((nx, ny, nz), np.int64)
    code[0] = ((first_v + np.arange(nv)) << 2 | OB.VEL_0N).reshape(ny, nz)
    code[nx - n_pressure:] = ((first_p + np.arange(npres)) << 2 | OB.PRES_0P).reshape(n_pressure, ny, nz)
    val = L.openBoundaryValues(0, nv + npres)
    assert np.array_equal(val[:nv, :3], u) and np.all(val[:nv, 3] == 1.0) and np.all(val[nv:, 3] == 1.0)
    return L, mask, code, val


def test_open_channel_matches_restatement_bit_for_bit(gpu):
    dims = (24, 16, 16)
    omega, body = 1.0 / 0.9, (2e-6, 3e-7, -1e-7)
    L, mask, code, val = _open_channel(gpu, dims, omega, body, 0.02)
    try:
        rng = np.random.default_rng(4)
        L.set_populations(rng.uniform(-0.005, 0.005, size=(L.n, 19)))
        S = L.populations().reshape(dims + (19,))
        fluid = mask == 0
        for target in (1, 50):
            done = 0 if target == 1 else 1
            for _ in range(target - done):
                S = OB.step(S, mask, (False, False, False), omega, body, code, val)
            L.collideAndStream(target - done)
            got = L.populations().reshape(dims + (19,))
            assert np.array_equal(got[fluid], S[fluid]), (target, np.abs(got[fluid] - S[fluid]).max())
        # the completion does something: the same run without open boundaries differs
        S_plain = OB.step(L.populations().reshape(dims + (19,)), mask, (False, False, False), omega, body)
        S_open = OB.step(L.populations().reshape(dims + (19,)), mask, (False, False, False), omega, body, code, val)
        assert not np.array_equal(S_plain[fluid], S_open[fluid])
    finally:
        L.destroy()


def test_completed_moments_equal_the_prescribed_values(gpu):
    """velocity nodes on x = 4, pressure nodes on x = 8 of a periodic box without forces: after one step the post-collision
    populations P(x, q) = S(x + c_q, q) of those nodes carry u_bc (velocity) and rho = 1, u_y = u_z = 0 (pressure)"""
    dims = (12, 8, 8)
    nx, ny, nz = dims
    L = gpu.Lattice(nx, ny, nz, (True, True, True), 1.0 / 0.7)
    try:
        rng = np.random.default_rng(9)
        L.set_populations(rng.uniform(-0.005, 0.005, size=(L.n, 19)))
        fv, nv = L.addVelocityBoundary0N((4, 4, 0, ny - 1, 0, nz - 1))
        u_bc = np.stack([rng.uniform(-0.03, 0.03, nv), rng.uniform(-0.01, 0.01, nv), rng.uniform(-0.01, 0.01, nv)], axis=1)
        L.setOpenBoundaryVelocitySlots(fv, u_bc)
        fp, npres = L.addPressureBoundary0P((8, 8, 0, ny - 1, 0, nz - 1))
        L.setOpenBoundaryDensitySlots(fp, np.ones(npres))
        L.collideAndStream(1)
        S = L.populations().reshape(dims + (19,))
        for x, kind in ((4, "v"), (8, "p")):
            P = np.empty((ny * nz, 19))
            for q in range(19):
                c = OB.C[q]
                P[:, q] = np.roll(S[:, :, :, q], (-c[0], -c[1], -c[2]), axis=(0, 1, 2))[x].reshape(-1)
            rho, u = OB.real_moments(P)
            if kind == "v":
                assert float(np.abs(u - u_bc).max()) <= 1e-14
            else:
                assert float(np.abs(rho - 1.0).max()) <= 1e-14
                assert float(np.abs(u[:, 1:]).max()) <= 1e-14
    finally:
        L.destroy()


def test_channel_steady_state_has_one_mass_flux(gpu):
    dims = (48, 18, 18)
    nx, ny, nz = dims
    L, mask, code, val = _open_channel(gpu, dims, 1.0, (0.0, 0.0, 0.0), 0.01, n_pressure=1)
    try:
        prof = _parabola(ny, nz, 0.01)
        u = np.zeros((ny * nz, 3)); u[:, 0] = prof.reshape(-1)
        L.setBoundaryVelocity((0, 0, 0, ny - 1, 0, nz - 1), u)   # axial inlet profile
        L.latticeEquilibrium(1.0, (0.0, 0.0, 0.0))
        L.collideAndStream(20000)
        # the discrete mass flux through the face between the planes x and x+1: what streams across it, sum over c_x = +1 of
        # S(x+1) minus sum over c_x = -1 of S(x) (the t_i of both sets cancel), every node of the planes included
        S = L.populations().reshape(dims + (19,))
        plus, minus = [10, 13, 14, 15, 16], [1, 4, 5, 6, 7]
        flux = S[1:, :, :, plus].sum(axis=(1, 2, 3)) - S[:-1, :, :, minus].sum(axis=(1, 2, 3))
        assert flux.mean() > 0
        assert float(np.abs(flux - flux.mean()).max() / flux.mean()) <= 1e-4, flux
    finally:
        L.destroy()


def _plane_velocity_ref(S, yz, x, body):
    f = S[x].reshape(-1, 19)[yz]
    r = np.zeros(len(yz)); j = [np.zeros(len(yz)) for _ in range(3)]
    for q in range(19):
        r = r + f[:, q]
        for d in range(3):
            if OB.C[q][d] == 1: j[d] = j[d] + f[:, q]
            elif OB.C[q][d] == -1: j[d] = j[d] + (-f[:, q])
    invRho = 1.0 / (1.0 + r)
    return np.stack([j[d] * invRho + body[d] / 2.0 for d in range(3)], axis=1)


@pytest.mark.parametrize("pre_n, pre_origin, dom_n", [(12, (0, 0), 12), (12, (2, 2), 16)])
def test_preinlet_coupling_in_one_process(gpu, pre_n, pre_origin, dom_n):
    """pre-inlet (periodic in x, driven along +x: Xneg) and domain (0N velocity inlet, 0P pressure outlet), nodes matched by
    global (y, z) -- the second case has a smaller pre-inlet cross-section that starts at global (2, 2): after every iteration
    the domain's inlet velocities are the pre-inlet's plane velocities of that iteration, which the domain's next step then
    uses -- the domain lags by one iteration"""
    pre_dims, dom_dims = (10, pre_n, pre_n), (20, dom_n, dom_n)
    omega, F = 1.0, (1e-5, 0.0, 0.0)
    pre = gpu.Lattice(*pre_dims, (True, False, False), omega)
    dom = gpu.Lattice(*dom_dims, (False, False, False), omega)
    try:
        pmask = _channel_mask(*pre_dims)
        pre.defineBounceBack(pmask); pre.setExternalVector(F); pre.latticeEquilibrium()
        dmask = _channel_mask(*dom_dims)
        dom.defineBounceBack(dmask); dom.latticeEquilibrium()
        ly, lz = np.nonzero(pmask[0] == 0)
        gyz = np.stack([ly + pre_origin[0], lz + pre_origin[1]], axis=1)   # global (y, z) of the pre-inlet's fluid nodes
        coupling = gpu.PreInlet(pre, dom, gyz, pre_dims[0] - 1, 0, direction="Xneg", pre_origin=pre_origin)
        n = len(gyz)
        dom_nodes = np.stack([np.zeros(n, int), gyz[:, 0], gyz[:, 1]], axis=1)
        assert np.array_equal(dom.openBoundarySlots(dom_nodes), coupling.first + np.arange(n))
        assert np.all(dom.openBoundaryValues(coupling.first, n)[:, :3] == 0.0)   # starts at u = 0
        nx, ny, nz = dom_dims
        fp, npres = dom.addPressureBoundary0P((nx - 1, nx - 1, 0, ny - 1, 0, nz - 1))
        code = -np.ones(dom_dims, np.int64)
        code[0, gyz[:, 0], gyz[:, 1]] = (coupling.first + np.arange(n)) << 2 | OB.VEL_0N
        code[nx - 1] = ((fp + np.arange(npres)) << 2 | OB.PRES_0P).reshape(ny, nz)
        pre_yz = ly * pre_n + lz
        for it in range(30):
            S_dom = dom.populations().reshape(dom_dims + (19,))
            val = dom.openBoundaryValues(0, coupling.first + n + npres)
            sent = coupling.iterate(1)
            assert np.array_equal(sent, _plane_velocity_ref(pre.populations().reshape(pre_dims + (19,)), pre_yz, pre_dims[0] - 1, F))
            assert np.array_equal(dom.openBoundaryValues(coupling.first, n)[:, :3], sent)
            want = OB.step(S_dom, dmask, (False, False, False), omega, (0.0, 0.0, 0.0), code, val)
            got = dom.populations().reshape(dom_dims + (19,))
            assert np.array_equal(got[dmask == 0], want[dmask == 0]), it
        assert sent[:, 0].mean() > 0
        _, u = dom.rho_u()
        assert u.reshape(dom_dims + (3,))[2][dmask[2] == 0][:, 0].mean() > 0   # the flow has entered the domain
        with pytest.raises(gpu.HcError, match="outside the pre-inlet"):
            gpu.PreInlet(pre, dom, gyz + 3, pre_dims[0] - 1, 1, direction="Xneg", pre_origin=pre_origin)
    finally:
        pre.destroy(); dom.destroy()


def test_clear_then_add_starts_from_rest(gpu):
    """slots declared after hcl_open_boundary_clear start at u = 0, rho = 1, whatever the cleared slots held"""
    L = gpu.Lattice(8, 6, 6, (False, False, False), 1.0)
    try:
        first, n = L.addVelocityBoundary0N((0, 0, 0, 5, 0, 5))
        L.setBoundaryVelocity((0, 0, 0, 5, 0, 5), (0.01, 0.02, 0.03))
        L.setBoundaryDensity((0, 0, 0, 5, 0, 5), 1.1)
        assert np.all(L.openBoundaryValues(first, n) == np.array([0.01, 0.02, 0.03, 1.1]))
        L.clearOpenBoundaries()
        assert (L.openBoundarySlots([[0, 2, 2]]) == -1).all()
        first, n = L.addPressureBoundary0P((7, 7, 0, 5, 0, 5))
        assert first == 0
        assert np.all(L.openBoundaryValues(first, n) == np.array([0.0, 0.0, 0.0, 1.0]))
    finally:
        L.destroy()


def test_refusals(gpu):
    L = gpu.Lattice(8, 6, 6, (False, False, False), 1.0)
    try:
        with pytest.raises(gpu.HcError, match="orientation"):
            L.addOpenBoundaryNodes(0, 0, [[0, 1, 1]])
        with pytest.raises(gpu.HcError, match="outside"):
            L.addVelocityBoundary0N((8, 8, 0, 5, 0, 5))
        with pytest.raises(gpu.HcError, match="not an open-boundary node"):
            L.setBoundaryDensity((0, 0, 0, 5, 0, 5), 1.0)
    finally:
        L.destroy()
    S = gpu.Lattice(8, 6, 6, (True, True, True), 1.0, x0=0, nx_global=16, n_slabs=2)
    try:
        with pytest.raises(gpu.HcError, match="n_slabs = 1"):
            S.addVelocityBoundary0N((0, 0, 0, 5, 0, 5))
    finally:
        S.destroy()
