"""Zou-He open boundaries on the GPU in every kind, kernel variant and observer, against tests/open_boundary_ref.py.

Fluid-only comparisons are bit for bit on fluid nodes after 1 and after 50 steps from random populations in +-0.005 (both sides
are plain IEEE double without contraction).  Every such run also asserts that the restatement's own state stays finite with
|rho - 1| < 0.1 on fluid nodes, so that two blown-up states cannot agree.  Observers (rho_u, pi_neq, planeVelocity, fluid_stats,
the IBM interpolation) must report the moments of the COMPLETED populations on open-boundary nodes: OB.observe()."""
import ctypes as C

import numpy as np
import pytest

import open_boundary_ref as OB

pytestmark = pytest.mark.gpu

DIMS = (24, 17, 19)   # odd cross-section: the plane stride is padded to a multiple of 16 and differs from ny * nz
OMEGA, BODY = 1.0 / 0.9, (2e-6, 3e-7, -1e-7)
NONPER = (False, False, False)
FACADE = {OB.VEL_0N: "addVelocityBoundary0N", OB.VEL_0P: "addVelocityBoundary0P", OB.PRES_0N: "addPressureBoundary0N",
          OB.PRES_0P: "addPressureBoundary0P"}


def _channel_mask(nx, ny, nz, moving_class=None):
    m = np.zeros((nx, ny, nz), np.uint8)
    m[:, 0, :] = m[:, -1, :] = 1
    m[:, :, 0] = m[:, :, -1] = 1
    if moving_class is not None:
        m[:, 0, :] = moving_class
    return m


def _parabola(ny, nz, u_max):
    y = (np.arange(ny) - (ny - 1) / 2.0) / ((ny - 2) / 2.0)
    z = (np.arange(nz) - (nz - 1) / 2.0) / ((nz - 2) / 2.0)
    return u_max * np.clip(1 - y[:, None] ** 2, 0, None) * np.clip(1 - z[None, :] ** 2, 0, None)


def _box_shape(box):
    return (box[1] - box[0] + 1, box[3] - box[2] + 1, box[5] - box[4] + 1)


def _velocity_values(box, dims, sign, u_max=0.02):
    """per-node profile on a box: u_x = sign * parabola, u_y = 0.1 parabola, u_z = -0.05 parabola (all non-zero off the walls)"""
    p = _parabola(dims[1], dims[2], u_max)[box[2]:box[3] + 1, box[4]:box[5] + 1]
    p = np.broadcast_to(p, _box_shape(box)).reshape(-1)
    return np.stack([sign * p, 0.1 * p, -0.05 * p], axis=1)


def _density_values(box, seed):
    return 1.0 + np.random.default_rng(seed).uniform(-0.01, 0.01, int(np.prod(_box_shape(box))))


def _layout(name, dims):
    """[(kind, box, values)]"""
    nx, ny, nz = dims
    h = ny // 2
    if name == "original":    # velocity 0N on x = 0, pressure 0P over the last three planes
        bv, bp = (0, 0, 0, ny - 1, 0, nz - 1), (nx - 3, nx - 1, 0, ny - 1, 0, nz - 1)
        return [(OB.VEL_0N, bv, _velocity_values(bv, dims, 1.0)), (OB.PRES_0P, bp, _density_values(bp, 21))]
    if name == "mirrored":    # velocity 0P on x = nx - 1 with u_x < 0, pressure 0N over the first three planes
        bv, bp = (nx - 1, nx - 1, 0, ny - 1, 0, nz - 1), (0, 2, 0, ny - 1, 0, nz - 1)
        return [(OB.VEL_0P, bv, _velocity_values(bv, dims, -1.0)), (OB.PRES_0N, bp, _density_values(bp, 22))]
    if name == "four":        # all four kinds at once, split in y
        a, b = (0, 0, 0, h - 1, 0, nz - 1), (0, 0, h, ny - 1, 0, nz - 1)
        c, d = (nx - 1, nx - 1, 0, h - 1, 0, nz - 1), (nx - 1, nx - 1, h, ny - 1, 0, nz - 1)
        return [(OB.VEL_0N, a, _velocity_values(a, dims, 1.0)), (OB.PRES_0N, b, _density_values(b, 23)),
                (OB.VEL_0P, c, _velocity_values(c, dims, 1.0)), (OB.PRES_0P, d, _density_values(d, 24))]
    raise ValueError(name)


def _declare(L, dims, patches):
    """declares the patches through the facade; returns ob_code [nx][ny][nz] and ob_val as the restatement wants them"""
    code = -np.ones(dims, np.int64)
    total = 0
    for kind, box, values in patches:
        first, n = getattr(L, FACADE[kind])(box)
        assert first == total and n == len(values)
        if kind in (OB.VEL_0N, OB.VEL_0P):
            L.setOpenBoundaryVelocitySlots(first, values)
        else:
            L.setOpenBoundaryDensitySlots(first, values)
        code[box[0]:box[1] + 1, box[2]:box[3] + 1, box[4]:box[5] + 1] = ((first + np.arange(n)) << 2 | kind).reshape(_box_shape(box))
        total += n
    val = L.openBoundaryValues(0, total)
    for kind, box, values in patches:
        slots = code[box[0]:box[1] + 1, box[2]:box[3] + 1, box[4]:box[5] + 1].reshape(-1) >> 2
        if kind in (OB.VEL_0N, OB.VEL_0P):
            assert np.array_equal(val[slots, :3], values) and np.all(val[slots, 3] == 1.0)
        else:
            assert np.array_equal(val[slots, 3], values) and np.all(val[slots, :3] == 0.0)
    return code, val


def _open_channel(gpu, layout, dims=DIMS, mask=None, seed=4):
    L = gpu.Lattice(*dims, NONPER, OMEGA)
    try:
        mask = _channel_mask(*dims) if mask is None else mask
        L.defineBounceBack(mask)
        L.setExternalVector(BODY)
        code, val = _declare(L, dims, _layout(layout, dims))
        L.set_populations(np.random.default_rng(seed).uniform(-0.005, 0.005, size=(L.n, 19)))
    except Exception:
        L.destroy()
        raise
    return L, mask, code, val


def _guard(S, mask, code, val, **kw):
    """the comparison is between two meaningful states: finite, and |rho - 1| < 0.1 on fluid nodes (completed moments)"""
    assert np.isfinite(S).all()
    rho, _, _ = OB.observe(S, mask, NONPER, BODY, None, code, val, **kw)
    dev = float(np.abs(rho[mask == 0] - 1.0).max())
    assert dev < 0.1, dev
    return dev


def _compare_1_and_50(L, mask, code, val, dims=DIMS, advance=None, **kw):
    """steps the lattice and the restatement to 1 and to 50 steps and compares fluid nodes bit for bit; kw goes to OB.step
    (boxes, box_forces, wall_u).  Returns the last restated state."""
    fluid = mask == 0
    S = L.populations().reshape(dims + (19,))
    obs = {k: v for k, v in kw.items() if k in ("boxes", "box_forces")}
    done = 0
    for target in (1, 50):
        for _ in range(target - done):
            S = OB.step(S, mask, NONPER, OMEGA, BODY, code, val, **kw)
            _guard(S, mask, code, val, **obs)
        if advance is None:
            L.collideAndStream(target - done)
        else:
            advance(target - done)
        done = target
        got = L.populations().reshape(dims + (19,))
        assert np.array_equal(got[fluid], S[fluid]), (target, float(np.abs(got[fluid] - S[fluid]).max()))
    return S


# ---- gap 1: all four kinds run on the GPU

@pytest.mark.parametrize("layout", ["mirrored", "four"])
def test_every_kind_matches_restatement_bit_for_bit(gpu, layout):
    """velocity 0P (u_x < 0, u_y, u_z != 0: the signs of the uy / ny terms of f[4..7]) and pressure 0N with a density that varies
    per node; and one lattice holding all four kinds"""
    L, mask, code, val = _open_channel(gpu, layout)
    try:
        kinds = set(int(k) for k in (code[code >= 0] & 3))
        assert kinds == ({OB.VEL_0P, OB.PRES_0N} if layout == "mirrored" else {0, 1, 2, 3})
        S = _compare_1_and_50(L, mask, code, val)
        plain = OB.step(S, mask, NONPER, OMEGA, BODY)
        assert not np.array_equal(plain[mask == 0], OB.step(S, mask, NONPER, OMEGA, BODY, code, val)[mask == 0])
    finally:
        L.destroy()


def test_completed_moments_of_0p_velocity_and_0n_pressure_nodes(gpu):
    """velocity 0P nodes on x = 4 and pressure 0N nodes on x = 8 of a periodic box without forces: after one step the
    post-collision populations P(x, q) = S(x + c_q, q) of those nodes carry u_bc and the prescribed density with u_y = u_z = 0,
    to the bound of test_completed_moments_equal_the_prescribed_values"""
    dims = (12, 8, 8)
    nx, ny, nz = dims
    L = gpu.Lattice(nx, ny, nz, (True, True, True), 1.0 / 0.7)
    try:
        rng = np.random.default_rng(19)
        L.set_populations(rng.uniform(-0.005, 0.005, size=(L.n, 19)))
        fv, nv = L.addVelocityBoundary0P((4, 4, 0, ny - 1, 0, nz - 1))
        u_bc = np.stack([rng.uniform(-0.03, 0.03, nv), rng.uniform(-0.01, 0.01, nv), rng.uniform(-0.01, 0.01, nv)], axis=1)
        L.setOpenBoundaryVelocitySlots(fv, u_bc)
        fp, npres = L.addPressureBoundary0N((8, 8, 0, ny - 1, 0, nz - 1))
        rho_bc = 1.0 + rng.uniform(-0.01, 0.01, npres)
        L.setOpenBoundaryDensitySlots(fp, rho_bc)
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
                assert float(np.abs(rho - rho_bc).max()) <= 1e-14
                assert float(np.abs(u[:, 1:]).max()) <= 1e-14
    finally:
        L.destroy()


def test_preinlet_xpos_coupling(gpu):
    """test_preinlet_coupling_in_one_process mirrored: the pre-inlet lies above the domain and is driven along -x, the domain's
    inlet is a 0P velocity plane on its last plane and its outlet a 0N pressure plane on plane 0"""
    pre_dims, dom_dims = (10, 12, 12), (20, 12, 12)
    omega, F = 1.0, (-1e-5, 0.0, 0.0)
    pre = gpu.Lattice(*pre_dims, (True, False, False), omega)
    dom = gpu.Lattice(*dom_dims, NONPER, omega)
    try:
        pmask = _channel_mask(*pre_dims)
        pre.defineBounceBack(pmask); pre.setExternalVector(F); pre.latticeEquilibrium()
        dmask = _channel_mask(*dom_dims)
        dom.defineBounceBack(dmask); dom.latticeEquilibrium()
        ly, lz = np.nonzero(pmask[0] == 0)
        gyz = np.stack([ly, lz], axis=1)
        nx, ny, nz = dom_dims
        coupling = gpu.PreInlet(pre, dom, gyz, 0, nx - 1, direction="Xpos")
        n = len(gyz)
        fp, npres = dom.addPressureBoundary0N((0, 0, 0, ny - 1, 0, nz - 1))
        code = -np.ones(dom_dims, np.int64)
        code[nx - 1, gyz[:, 0], gyz[:, 1]] = (coupling.first + np.arange(n)) << 2 | OB.VEL_0P
        code[0] = ((fp + np.arange(npres)) << 2 | OB.PRES_0N).reshape(ny, nz)
        pre_yz = ly * pre_dims[2] + lz
        for it in range(30):
            S_dom = dom.populations().reshape(dom_dims + (19,))
            val = dom.openBoundaryValues(0, coupling.first + n + npres)
            sent = coupling.iterate(1)
            _, u_pre, _ = OB.observe(pre.populations().reshape(pre_dims + (19,)), pmask, None, F)
            assert np.array_equal(sent, u_pre[0].reshape(-1, 3)[pre_yz])
            assert np.array_equal(dom.openBoundaryValues(coupling.first, n)[:, :3], sent)
            want = OB.step(S_dom, dmask, NONPER, omega, (0.0, 0.0, 0.0), code, val)
            got = dom.populations().reshape(dom_dims + (19,))
            assert np.array_equal(got[dmask == 0], want[dmask == 0]), it
        assert sent[:, 0].mean() < 0
        _, u = dom.rho_u()
        assert u.reshape(dom_dims + (3,))[nx - 3][dmask[nx - 3] == 0][:, 0].mean() < 0   # the flow has entered the domain, along -x
    finally:
        pre.destroy(); dom.destroy()


# ---- gap 2: collide_stream_kernel<true, true>

def test_open_channel_with_body_force_boxes(gpu):
    """two body-force boxes, the second covering the inlet plane and overlapping the first (the last box wins)"""
    L, mask, code, val = _open_channel(gpu, "original")
    try:
        nx, ny, nz = DIMS
        boxes = [(5, 14, 2, 10, 3, 15), (0, 6, 0, ny - 1, 0, nz - 1)]
        forces = [(-3e-6, 1e-6, 2e-6), (5e-6, -2e-6, 1e-6)]
        L.setExternalVectorBoxes(boxes, forces)
        _compare_1_and_50(L, mask, code, val, boxes=boxes, box_forces=forces)
        # the observers take the force of the box that holds the node
        S = L.populations().reshape(DIMS + (19,))
        _, u_ref, _ = OB.observe(S, mask, NONPER, BODY, None, code, val, boxes=boxes, box_forces=forces)
        _, u = L.rho_u()
        assert np.array_equal(u.reshape(DIMS + (3,)), u_ref)
    finally:
        L.destroy()


# ---- gap 3: IBM force and split launches on an open lattice

def _lattice_with_cells(gpu, layout, n_cells=2):
    """an open channel of DIMS whose omega is the cell parameters', with RBCs bound to it (mid-channel, clear of the walls)"""
    P = gpu.base_parameters()
    L, mask, code, val = _open_channel(gpu, layout)
    try:
        h = gpu.HemoCell(L, P)
        h.cellfields.addCellType(gpu.CellType.rbc(P), 1)
        for k in range(n_cells):
            assert h.cellfields.addCell(0, (7.0 + 10.0 * k, 8.0, 9.0), (0.0, 0.0, 0.0))
    except Exception:
        L.destroy()
        raise
    return L, mask, code, val, h


def _vertices_next_to_the_open_planes(n_per_cell, seed):
    """positions of two cells' vertices: the first cell's within one node of the plane x = 0, the second's within one node of
    x = nx - 1; y and z anywhere between the walls, so that some stencils also meet bounce-back nodes"""
    nx, ny, nz = DIMS
    rng = np.random.default_rng(seed)
    p = np.empty((2 * n_per_cell, 3))
    p[:n_per_cell, 0] = rng.uniform(0.02, 0.98, n_per_cell)
    p[n_per_cell:, 0] = rng.uniform(nx - 1.98, nx - 1.02, n_per_cell)
    p[:, 1] = rng.uniform(1.0, ny - 2.0, 2 * n_per_cell)
    p[:, 2] = rng.uniform(1.0, nz - 2.0, 2 * n_per_cell)
    return p


def test_open_channel_with_ibm_force(gpu):
    """the fdirty branch with ob_n > 0: vertex forces spread (reproducible spread) onto nodes of the inlet and outlet planes, the
    field read back and handed to the restatement, one step compared bit for bit; three steps later the buffer comes round
    again and the collide has zeroed it"""
    lib = gpu.capi.lib()
    L, mask, code, val, h = _lattice_with_cells(gpu, "four")
    gpu.check(lib.hc_set_reproducible_spread(1))
    try:
        cf = h.cellfields
        nv = len(cf.positions) // 2
        cf.positions = _vertices_next_to_the_open_planes(nv, 5)
        cf.forces = 1e-4 * np.random.default_rng(6).standard_normal((2 * nv, 3))
        cf.spreadParticleForce(True)
        F = L.ibm_force().reshape(DIMS + (3,))
        assert np.abs(F[0]).max() > 0 and np.abs(F[-1]).max() > 0 and np.all(F[mask != 0] == 0.0)
        S = L.populations().reshape(DIMS + (19,))
        want = OB.step(S, mask, NONPER, OMEGA, BODY, code, val, F=F)
        _guard(want, mask, code, val)
        assert not np.array_equal(want[mask == 0], OB.step(S, mask, NONPER, OMEGA, BODY, code, val)[mask == 0])
        L.collideAndStream(1)
        got = L.populations().reshape(DIMS + (19,))
        assert np.array_equal(got[mask == 0], want[mask == 0]), float(np.abs(got - want)[mask == 0].max())
        L.collideAndStream(2)   # the third step after the spread reads the same buffer again: the collide has zeroed it
        assert np.all(L.ibm_force() == 0.0)
    finally:
        gpu.check(lib.hc_set_reproducible_spread(0))
        L.destroy()


@pytest.mark.parametrize("parts", [(1, 2), (3, 4)])
def test_split_launches_give_the_bits_of_one_launch(gpu, parts):
    """interior first, then both face planes in one launch (x_split / x_jump): the inlet and outlet planes are those face planes"""
    L, mask, code, val = _open_channel(gpu, "four")
    try:
        def advance(n):
            for _ in range(n):
                for p in parts:
                    L.collide_part(p)
                L.step_end()
        _compare_1_and_50(L, mask, code, val, advance=advance)
    finally:
        L.destroy()


# ---- gap 4: the padded plane stride

@pytest.mark.parametrize("padding", [1, -1])
def test_open_channel_with_forced_plane_padding(gpu, padding):
    """ob_code is indexed by the padded node number, which hcl_open_boundary_add forms on the host: 1 pads every plane by eight
    rows more, -1 removes the padding (the plane stride is then the odd 17 x 19)"""
    lib = gpu.capi.lib()
    gpu.check(lib.hc_debug_force_plane_padding(padding))
    L = None
    try:
        L, mask, code, val = _open_channel(gpu, "four")
        _compare_1_and_50(L, mask, code, val)
        S = L.populations().reshape(DIMS + (19,))
        rho_ref, u_ref, _ = OB.observe(S, mask, NONPER, BODY, None, code, val)
        rho, u = L.rho_u()
        assert np.array_equal(rho.reshape(DIMS), rho_ref) and np.array_equal(u.reshape(DIMS + (3,)), u_ref)
    finally:
        gpu.check(lib.hc_debug_force_plane_padding(0))
        if L is not None:
            L.destroy()


# ---- gap 5: moving walls, Lees-Edwards

def test_open_channel_next_to_a_moving_wall(gpu):
    """the y = 0 face is a moving wall (class 3); the boundary boxes include those wall nodes, which stay walls"""
    mask = _channel_mask(*DIMS, moving_class=3)
    L, mask, code, val = _open_channel(gpu, "four", mask=mask)
    try:
        w = (0.01, 0.0, -0.004)
        L.setBoundaryVelocity(3, w)
        assert (code[0, 0, :] >= 0).all() and (mask[0, 0, :] == 3).all()
        S = _compare_1_and_50(L, mask, code, val, wall_u={3: w})
        still = OB.step(S, mask, NONPER, OMEGA, BODY, code, val)
        assert not np.array_equal(still[mask == 0], OB.step(S, mask, NONPER, OMEGA, BODY, code, val, wall_u={3: w})[mask == 0])
    finally:
        L.destroy()


def test_lees_edwards_and_open_boundaries_refuse_each_other(gpu):
    """the Lees-Edwards pass takes plain moments of gathered populations on its z layers; what it should read or leave on a node
    the collide completes is undefined, so both entry points refuse the combination"""
    A = gpu.Lattice(12, 8, 8, (True, True, True), 1.0)
    B = gpu.Lattice(12, 8, 8, (True, True, True), 1.0)
    try:
        A.addVelocityBoundary0N((4, 4, 0, 7, 0, 7))
        with pytest.raises(gpu.HcError, match="open boundaries and Lees-Edwards do not combine"):
            A.setLeesEdwards(0.01, -0.01)
        A.clearOpenBoundaries()
        A.setLeesEdwards(0.01, -0.01)   # composes again once the nodes are gone
        B.setLeesEdwards(0.01, -0.01)
        with pytest.raises(gpu.HcError, match="open boundaries and Lees-Edwards do not combine"):
            B.addPressureBoundary0P((8, 8, 0, 7, 0, 7))
        assert (B.openBoundarySlots([[8, 3, 3]]) == -1).all()
    finally:
        A.destroy(); B.destroy()


# ---- gap 6: what observers report on open-boundary nodes

@pytest.mark.parametrize("layout", ["original", "mirrored", "four"])
def test_observers_report_the_completed_moments(gpu, layout):
    """rho_u, pi_neq, planeVelocity and fluid_stats on a stepped channel: bit for bit OB.observe() (same completion, same order of
    the moments), and against the prescribed values themselves in extended precision: u_bc + F / 2 on velocity nodes, the
    prescribed density and u_y = u_z = F / 2 on pressure nodes, to 1e-14"""
    L, mask, code, val = _open_channel(gpu, layout)
    try:
        nx, ny, nz = DIMS
        L.collideAndStream(7)
        S = L.populations().reshape(DIMS + (19,))
        _guard(S, mask, code, val)
        rho_ref, u_ref, pi_ref = OB.observe(S, mask, NONPER, BODY, None, code, val)
        rho, u = L.rho_u()
        rho, u, pi = rho.reshape(DIMS), u.reshape(DIMS + (3,)), L.pi_neq().reshape(DIMS + (6,))
        # the prescribed values, independently of observe()
        fluid = mask == 0
        half = np.asarray(BODY, np.longdouble) / 2
        for kind in sorted(set(int(k) for k in code[code >= 0] & 3)):
            sel = fluid & (code >= 0) & ((code & 3) == kind)
            v = val[code[sel] >> 2]
            if kind in (OB.VEL_0N, OB.VEL_0P):
                err = np.abs(u[sel].astype(np.longdouble) - (v[:, :3].astype(np.longdouble) + half))
            else:
                err = np.abs(np.concatenate([(rho[sel].astype(np.longdouble) - v[:, 3])[:, None],
                                             u[sel][:, 1:].astype(np.longdouble) - half[1:]], axis=1))
            assert float(err.max()) <= 1e-14, (kind, float(err.max()))
        assert np.array_equal(rho, rho_ref)
        assert np.array_equal(u, u_ref)
        assert np.array_equal(pi, pi_ref)
        # plain moments would differ: the unknown populations of a face plane are the zeros that came from outside
        rho_plain, _, _ = OB.observe(S, mask, NONPER, BODY)
        assert not np.array_equal(rho_plain[fluid], rho_ref[fluid])
        for x in (0, nx - 1, 5):
            yz = np.flatnonzero(mask[x].reshape(-1) == 0)
            assert np.array_equal(L.planeVelocity(x, yz), u_ref[x].reshape(-1, 3)[yz]), x
            walls = np.flatnonzero(mask[x].reshape(-1) != 0)[:7]
            assert np.all(L.planeVelocity(x, walls) == 0.0)
        speed = np.sqrt((u_ref[fluid].astype(np.longdouble) ** 2).sum(axis=1))
        mn, mx, mean, n = L.fluid_stats(0)
        assert n == int(fluid.sum())
        assert abs(mn - float(speed.min())) <= 1e-14 and abs(mx - float(speed.max())) <= 1e-14
        assert abs(mean - float(speed.mean())) <= 1e-14
    finally:
        L.destroy()


def _interpolate_ref(pos, u, mask):
    """interpolationCoefficientsPhi2 on a lattice that is not periodic: the 2 x 2 x 2 nodes around the vertex, tent weights,
    bounce-back nodes and nodes outside left out, the rest normalised; v = sum_k (u_k w_k) in ascending (i, j, k) order"""
    dims = np.array(mask.shape)
    out = np.zeros_like(pos)
    for n, p in enumerate(pos):
        c = np.floor(p + 0.5).astype(int)
        d0 = np.where(p < c, -1, 0)
        nodes, w = [], []
        for i in range(2):
            for j in range(2):
                for k in range(2):
                    g = c + d0 + (i, j, k)
                    if (g < 0).any() or (g >= dims).any():
                        continue
                    t = np.clip(1.0 - np.abs(p - g), 0.0, None)
                    wt = t[0] * t[1] * t[2]
                    if wt != 0.0 and mask[tuple(g)] == 0:
                        nodes.append(tuple(g)); w.append(wt)
        assert w, "every stencil node of the vertex is masked"
        total = 0.0
        for wt in w:   # the kernel's sum: ascending (i, j, k) over the admitted nodes
            total = total + wt
        coeff = 1.0 / total
        a = np.zeros(3)
        for g, wt in zip(nodes, w):
            a = a + u[g] * (wt * coeff)
        out[n] = a
    return out


@pytest.mark.parametrize("per_vertex", [0, 1])
def test_interpolation_next_to_the_open_planes(gpu, per_vertex):
    """vertices within one node of the inlet and of the outlet plane: every stencil takes half of its nodes from an open plane.
    The LDS-tiled kernel (one cell per plane, so each bounding box is small) and the per-vertex kernel against the completed
    node velocities of OB.observe(); the bound is test_ibm_phases_vs_oracle's"""
    lib = gpu.capi.lib()
    L, mask, code, val, h = _lattice_with_cells(gpu, "four")
    gpu.check(lib.hc_debug_ibm_per_vertex(per_vertex))
    try:
        cf = h.cellfields
        nv = len(cf.positions) // 2
        pos = _vertices_next_to_the_open_planes(nv, 8)
        cf.positions = pos
        L.collideAndStream(5)
        S = L.populations().reshape(DIMS + (19,))
        _, u_ref, _ = OB.observe(S, mask, NONPER, BODY, None, code, val)
        _, u_plain, _ = OB.observe(S, mask, NONPER, BODY)
        cf.interpolateFluidVelocity()
        want = _interpolate_ref(pos, u_ref, mask)
        got = cf.velocities
        assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max(), float(np.abs(got - want).max())
        # plain moments of the face planes would be far off
        assert np.abs(_interpolate_ref(pos[::40], u_plain, mask) - want[::40]).max() > 1e-4
    finally:
        gpu.check(lib.hc_debug_ibm_per_vertex(0))
        L.destroy()


# ---- gap 7: slot bookkeeping

def test_slots_keep_their_values_when_the_table_grows(gpu):
    """10 nodes with values, then 5000 more (the slot table is reallocated): the first 10 read back unchanged and the step uses
    them"""
    dims = (20, 18, 18)
    nx, ny, nz = dims
    L = gpu.Lattice(*dims, NONPER, OMEGA)
    try:
        mask = _channel_mask(*dims)
        L.defineBounceBack(mask); L.setExternalVector(BODY)
        rng = np.random.default_rng(31)
        first_nodes = np.stack([np.zeros(10, int), 4 + np.arange(10), np.full(10, 7)], axis=1)
        f0 = L.addOpenBoundaryNodes(0, -1, first_nodes)
        u10 = rng.uniform(-0.02, 0.02, (10, 3))
        L.setOpenBoundaryVelocitySlots(f0, u10)
        g = np.mgrid[2:nx - 1, 0:ny, 0:nz].reshape(3, -1).T[:5000]
        f1 = L.addOpenBoundaryNodes(1, 1, g)
        assert (f0, f1) == (0, 10)
        rho = 1.0 + rng.uniform(-0.01, 0.01, 5000)
        L.setOpenBoundaryDensitySlots(f1, rho)
        val = L.openBoundaryValues(0, 5010)
        assert np.array_equal(val[:10, :3], u10) and np.all(val[:10, 3] == 1.0)
        assert np.array_equal(val[10:, 3], rho) and np.all(val[10:, :3] == 0.0)
        assert np.array_equal(L.openBoundarySlots(first_nodes), np.arange(10))
        code = -np.ones(dims, np.int64)
        code[tuple(first_nodes.T)] = np.arange(10) << 2 | OB.VEL_0N
        code[tuple(g.T)] = (10 + np.arange(5000)) << 2 | OB.PRES_0P
        L.set_populations(rng.uniform(-0.005, 0.005, size=(L.n, 19)))
        S = L.populations().reshape(dims + (19,))
        for _ in range(3):
            S = OB.step(S, mask, NONPER, OMEGA, BODY, code, val)
        L.collideAndStream(3)
        assert np.isfinite(S).all()
        assert np.array_equal(L.populations().reshape(dims + (19,))[mask == 0], S[mask == 0])
    finally:
        L.destroy()


def test_a_node_declared_twice_is_refused(gpu):
    """a node holds one slot: a second declaration is refused, in a later call or within one list, and changes nothing"""
    L = gpu.Lattice(8, 6, 6, NONPER, 1.0)
    try:
        first, n = L.addVelocityBoundary0N((0, 0, 0, 5, 0, 5))
        L.setBoundaryVelocity((0, 0, 0, 5, 0, 5), (0.01, 0.0, 0.0))
        with pytest.raises(gpu.HcError, match="declared twice"):
            L.addPressureBoundary0N((0, 1, 2, 3, 2, 3))
        with pytest.raises(gpu.HcError, match="declared twice"):
            L.addOpenBoundaryNodes(1, 1, [[7, 1, 1], [7, 2, 2], [7, 1, 1]])
        assert (L.openBoundarySlots([[1, 2, 2], [7, 1, 1], [7, 2, 2]]) == -1).all()
        assert np.array_equal(L.openBoundarySlots([[0, 2, 2]]), [2 * 6 + 2])
        assert np.all(L.openBoundaryValues(first, n) == np.array([0.01, 0.0, 0.0, 1.0]))
        assert L.addPressureBoundary0P((7, 7, 0, 5, 0, 5)) == (n, 36)
    finally:
        L.destroy()


def _hip_runtime():
    """the HIP runtime the product library has loaded, for a device buffer of the test's own"""
    with open("/proc/self/maps") as f:
        paths = sorted({line.split()[-1] for line in f if "libamdhip64" in line})
    assert len(paths) == 1, paths
    hip = C.CDLL(paths[0])
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    return hip


def test_values_set_from_device_memory_equal_the_host_path(gpu):
    """on_device = 1 of both setters: the values come from a device buffer (hipMalloc + a blocking hipMemcpy of the runtime the
    library itself uses) and land where the host path puts them"""
    A = gpu.Lattice(8, 6, 6, NONPER, 1.0)
    B = gpu.Lattice(8, 6, 6, NONPER, 1.0)
    hip = _hip_runtime()
    dev = C.c_void_p()
    try:
        rng = np.random.default_rng(41)
        u, rho = rng.uniform(-0.02, 0.02, (36, 3)), 1.0 + rng.uniform(-0.01, 0.01, 36)
        for L in (A, B):
            assert L.addVelocityBoundary0N((0, 0, 0, 5, 0, 5)) == (0, 36)
            assert L.addPressureBoundary0P((7, 7, 0, 5, 0, 5)) == (36, 36)
        A.setOpenBoundaryVelocitySlots(3, u[3:20]); A.setOpenBoundaryDensitySlots(36, rho)
        src = np.ascontiguousarray(np.concatenate([u[3:20].reshape(-1), rho]))
        assert hip.hipMalloc(C.byref(dev), src.nbytes) == 0
        assert hip.hipMemcpy(dev, src.ctypes.data, src.nbytes, 1) == 0   # hipMemcpyHostToDevice, blocking
        gpu.check(B.lib.hcl_open_boundary_set_velocity(B.ptr, 3, 17, dev, 1))
        gpu.check(B.lib.hcl_open_boundary_set_density(B.ptr, 36, 36, C.c_void_p(dev.value + 17 * 3 * 8), 1))
        got = B.openBoundaryValues(0, 72)   # synchronises the stream the setters ran on
        assert np.array_equal(got, A.openBoundaryValues(0, 72))
        assert np.array_equal(got[3:20, :3], u[3:20]) and np.all(got[:3, :3] == 0.0) and np.array_equal(got[36:, 3], rho)
    finally:
        A.destroy(); B.destroy()
        if dev.value:
            hip.hipFree(dev)


def test_cleared_boundaries_step_and_observe_as_a_plain_lattice(gpu, orc):
    """after clearOpenBoundaries() the collide and the observers are the plain ones again: the oracle's bits"""
    from oracle import oracle as O
    L, mask, code, val = _open_channel(gpu, "four")
    Lo = O.OracleLattice(orc, *DIMS, (0, 0, 0), OMEGA)
    try:
        L.collideAndStream(3)
        L.clearOpenBoundaries()
        Lo.set_mask(mask); Lo.set_force_uniform(BODY)
        Lo.f[:] = L.populations()
        for _ in range(5):
            orc.orc_collide_stream(Lo.ptr)
        L.collideAndStream(5)
        fluid = mask.reshape(-1) == 0
        got = L.populations()
        assert np.array_equal(got[fluid], Lo.f[fluid])
        rho_ref, u_ref, _ = OB.observe(got.reshape(DIMS + (19,)), mask, NONPER, BODY)
        rho, u = L.rho_u()
        assert np.array_equal(rho.reshape(DIMS), rho_ref) and np.array_equal(u.reshape(DIMS + (3,)), u_ref)
    finally:
        Lo.destroy(); L.destroy()


# ---- gap 3 again: hc_iterate on an open lattice, against the oracle with open boundaries

@pytest.mark.parametrize("case", ["atomic", "reproducible", "beside"])
def test_coupled_channel_against_the_oracle(orc, gpu, case):
    """a walled 48 x 34 x 34 channel, not periodic in x: 0N velocity inlet with a parabolic profile, 0P pressure outlet, one
    RBC whose lowest vertex starts 2.5 nodes downstream of the inlet plane, one PLT mid-channel, velocity updates every 2nd
    (beside: 3rd) iteration; 60 iterations of hc_iterate against orc_sim_iterate with the bounds of
    test_iterate_trajectories_vs_oracle: positions <= 1e-9 lu, populations and forces <= 1e-6 relative.  beside: no deletion
    checks inside the call, so the side-stream schedule runs (collide_stream_beside is counted).  Every vertex is alive on
    both sides at the end, so a deletion cannot hide a divergence."""
    from oracle import oracle as O
    lib = gpu.capi.lib()
    dims = (48, 34, 34)
    nx, ny, nz = dims
    k_m, k_p = (6, 3) if case == "beside" else (4, 2)
    mask = _channel_mask(*dims)
    Po = O.make_params(orc); Pg = gpu.base_parameters()
    omega = 1.0 / Po.tau
    Lo = O.OracleLattice(orc, *dims, (0, 0, 0), omega)
    Lg = gpu.Lattice(*dims, NONPER, omega)
    gpu.check(lib.hc_set_reproducible_spread(1 if case == "reproducible" else 0))
    try:
        Lo.set_mask(mask); Lg.defineBounceBack(mask)
        Lo.init_equilibrium(); Lg.latticeEquilibrium()
        inlet, outlet = (0, 0, 0, ny - 1, 0, nz - 1), (nx - 1, nx - 1, 0, ny - 1, 0, nz - 1)
        u_in = np.zeros((ny * nz, 3)); u_in[:, 0] = _parabola(ny, nz, 0.01).reshape(-1)
        code, val = _declare(Lg, dims, [(OB.VEL_0N, inlet, u_in), (OB.PRES_0P, outlet, np.ones(ny * nz))])
        Lo.set_open_boundary(code, val)
        So = orc.orc_sim_create(Lo.ptr, C.byref(Po))
        hg = gpu.HemoCell(Lg, Pg)
        for make_o, make_g in ((O.make_rbc, gpu.CellType.rbc), (O.make_plt, gpu.CellType.plt)):
            To = make_o(orc, Po); To.contents.timescale = k_m
            orc.orc_sim_add_type(So, To); hg.cellfields.addCellType(make_g(Pg), k_m)
        So.contents.particle_velocity_timescale = k_p
        hg.setParticleVelocityUpdateTimeScaleSeparation(k_p)
        for t, centre, ang in ((0, (14.0, 16.5, 16.5), (90.0, 0.0, 0.0)), (1, (24.0, 12.0, 20.0), (10.0, 20.0, 30.0))):
            c = np.array(centre); a_ref = np.array(ang) * (3.14159265358979323846 / 180.0) * -1.0
            assert orc.orc_sim_add_cell(So, t, O.dptr(c), O.dptr(a_ref), 0.0) == 1
            assert hg.cellfields.addCell(t, centre, ang)
        cf = hg.cellfields
        n_rbc = cf.types[0].nv
        pos = cf.positions.copy()
        pos[:n_rbc, 0] -= pos[:n_rbc, 0].min() - 2.5   # the RBC's lowest vertex 2.5 nodes downstream of the inlet plane
        orc.orc_sim_set(So, 0, O.dptr(pos)); cf.positions = pos
        F = (0.0, 0.0, 0.0)
        Lo.set_force_uniform(F); Lg.setExternalVector(F)
        Lo.set_threads(8)
        orc.orc_sim_mechanics(So, 1); cf.applyConstitutiveModel(0, True)
        nsteps = 60
        for _ in range(nsteps):
            orc.orc_sim_iterate(So)
        if case == "beside":
            hg.deletion_check_every = 10 ** 6
            gpu.check(lib.hc_profile_reset()); gpu.check(lib.hc_profile_enable(1))
        hg.iterate(nsteps)
        if case == "beside":
            ms, n = C.c_double(), C.c_long()
            gpu.check(lib.hc_profile_enable(0))
            gpu.check(lib.hc_profile_read(b"collide_stream_beside", C.byref(ms), C.byref(n)))
            assert n.value == nsteps - nsteps // k_p - 1
        out = [np.zeros((So.contents.np, 3)) for _ in range(3)]
        for w in range(3):
            orc.orc_sim_get(So, w, O.dptr(out[w]))
        p_o, _, f_o = out
        alive_o = np.zeros(So.contents.np, np.uint8); orc.orc_sim_get_alive(So, alive_o.ctypes.data)
        assert alive_o.all() and cf.alive().all() and len(cf.positions) == len(p_o)
        assert hg.iter == So.contents.iter == nsteps
        fluid = mask.reshape(-1) == 0
        fo, fg = Lo.f[fluid], Lg.populations()[fluid]
        assert np.isfinite(fo).all() and p_o[:n_rbc, 0].mean() > pos[:n_rbc, 0].mean()   # the inlet carries the RBC downstream
        d_p = float(np.abs(cf.positions - p_o).max())
        d_f = float(np.abs(fg - fo).max() / np.abs(fo).max())
        d_F = float(np.abs(cf.forces - f_o).max() / np.abs(f_o).max())
        print("coupled open channel [%s]: max |dx| = %.3e lu, populations %.3e rel, forces %.3e rel" % (case, d_p, d_f, d_F))
        assert d_p <= 1e-9, d_p
        assert d_f <= 1e-6, d_f
        assert d_F <= 1e-6, d_F
    finally:
        gpu.check(lib.hc_set_reproducible_spread(0))
        if case == "beside":
            gpu.check(lib.hc_profile_enable(0))
        Lo.destroy(); Lg.destroy()
