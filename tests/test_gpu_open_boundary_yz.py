"""Zou-He open boundaries on the y and z faces on the GPU, against tests/open_boundary_axis_ref.py.

Walled channels of 17 x 24 x 19 (open along y) and 19 x 17 x 24 (open along z), L-shaped ducts with the inlet and the outlet on
different axes, and a box whose y inlet and z outlet meet at an edge, so that one wavefront holds open nodes of two axes.  Collide comparisons are bit for bit on fluid nodes after 1 and after 50 steps from random populations in
+-0.005; the restated run of every scene is computed once, asserted finite with |rho - 1| < 0.1 on fluid nodes at every step, and
shared by the kernel variants that must reproduce it (forced plane padding, split launches)."""
import ctypes as C
import functools

import numpy as np
import pytest

import open_boundary_axis_ref as AX
import open_boundary_ref as OB

pytestmark = pytest.mark.gpu

OMEGA, BODY, NONPER = AX.OMEGA, AX.BODY, AX.NONPER
VELOCITY = (OB.VEL_0N, OB.VEL_0P)
FACADE = {(k, a): "add%sBoundary%d%s" % ("Velocity" if k in VELOCITY else "Pressure", a, "N" if k in (OB.VEL_0N, OB.PRES_0N) else "P")
          for k in range(4) for a in range(3)}
SCENES = ["y-original", "y-mirrored", "z-original", "z-mirrored", "bent-xy", "bent-yz", "corner-yz"]


@functools.lru_cache(maxsize=None)
def _scene(name):
    """(dims, mask, patches, code, axes, val, S0), all read-only"""
    kind, what = name.split("-")
    if kind == "bent":   # x inlet and y outlet; y inlet and z outlet: two axes on one lattice, in different wavefronts
        dims, mask, patches = AX.bent_duct("xyz".index(what[0]), "xyz".index(what[1]))
    elif kind == "corner":   # y inlet and z outlet in adjacent rows of every x plane: two axes in one wavefront
        dims, mask, patches = AX.corner_box()
    else:
        axis = "xyz".index(kind)
        dims = AX.CHANNEL_DIMS[axis]
        mask, patches = AX.channel_mask(dims, axis), AX.channel_patches(what, axis, dims)
    code, axes, val = AX.declaration(dims, patches)
    S0 = AX.initial_state(dims)
    for a in (mask, code, axes, val, S0):
        a.setflags(write=False)
    return dims, mask, patches, code, axes, val, S0


def _force_boxes(dims, patches):
    """two body-force boxes, the second covering the inlet planes and overlapping the first (the last box wins)"""
    first = [2, dims[0] - 3, 2, dims[1] - 4, 3, dims[2] - 3]
    second = [0, dims[0] - 1, 0, dims[1] - 1, 0, dims[2] - 1]
    a = patches[0][1]
    second[2 * a], second[2 * a + 1] = 0, 6
    return [tuple(first), tuple(second)], [(-3e-6, 1e-6, 2e-6), (5e-6, -2e-6, 1e-6)]


@functools.lru_cache(maxsize=None)
def _restated(name, with_boxes):
    """{1: state, 50: state} of the restatement"""
    dims, mask, patches, code, axes, val, S0 = _scene(name)
    kw = {}
    if with_boxes:
        kw["boxes"], kw["box_forces"] = _force_boxes(dims, patches)
    S, out = S0, {}
    for n in range(1, 51):
        S = AX.step(S, mask, NONPER, OMEGA, BODY, code, axes, val, **kw)
        assert np.isfinite(S).all()
        rho, _, _ = AX.observe(S, mask, NONPER, BODY, None, code, axes, val, **kw)
        dev = float(np.abs(rho[mask == 0] - 1.0).max())
        assert dev < 0.1, (n, dev)
        if n in (1, 50):
            S.setflags(write=False)
            out[n] = S
    plain = OB.step(out[1], mask, NONPER, OMEGA, BODY, **kw)
    assert not np.array_equal(plain[mask == 0], AX.step(out[1], mask, NONPER, OMEGA, BODY, code, axes, val, **kw)[mask == 0])
    return out


def _declare(L, patches, code, axes, val):
    """declares the patches through the facade and checks slots, axes and values against the restatement's declaration"""
    total = 0
    for kind, axis, box, values in patches:
        first, n = getattr(L, FACADE[(kind, axis)])(box)
        assert first == total and n == len(values)
        if kind in VELOCITY:
            L.setOpenBoundaryVelocitySlots(first, values)
        else:
            L.setOpenBoundaryDensitySlots(first, values)
        total += n
    assert np.array_equal(L.openBoundaryValues(0, total), val)
    nodes = np.argwhere(code >= 0)
    assert np.array_equal(L.openBoundarySlots(nodes), code[code >= 0] >> 2)
    assert np.array_equal(L.openBoundaryAxes(nodes), axes[code >= 0])
    assert (L.openBoundaryAxes(np.argwhere(code < 0)[::7]) == -1).all()


def _lattice(gpu, name):
    dims, mask, patches, code, axes, val, S0 = _scene(name)
    L = gpu.Lattice(*dims, NONPER, OMEGA)
    try:
        L.defineBounceBack(mask)
        L.setExternalVector(BODY)
        _declare(L, patches, code, axes, val)
        L.set_populations(S0.reshape(-1, 19))
        assert np.array_equal(L.populations().reshape(dims + (19,)), S0)
    except Exception:
        L.destroy()
        raise
    return L


def _compare_1_and_50(L, name, with_boxes=False, advance=None):
    dims, mask = _scene(name)[:2]
    want = _restated(name, with_boxes)
    fluid = mask == 0
    done = 0
    for target in (1, 50):
        if advance is None:
            L.collideAndStream(target - done)
        else:
            advance(target - done)
        done = target
        got = L.populations().reshape(dims + (19,))
        assert np.array_equal(got[fluid], want[target][fluid]), (target, float(np.abs(got[fluid] - want[target][fluid]).max()))


# ---- 1, 2: every kind on the y and z faces; two axes on one lattice

@pytest.mark.parametrize("name", SCENES)
def test_matches_restatement_bit_for_bit(gpu, name):
    """velocity N with a parabola and non-zero tangential components + pressure P with per-node densities; velocity P with an
    inward (negative) normal velocity + pressure N; the L-shaped ducts with an x inlet and a y outlet, and a y inlet and a z
    outlet (edge nodes are walls), whose two axes lie in different wavefronts; and the corner box, where the first wavefront
    of every interior x plane holds fluid open nodes of both axes, so the per-node switch diverges within a wave"""
    dims, mask, patches, code, axes = _scene(name)[:5]
    if name.startswith("bent"):
        assert len(set(int(a) for a in axes[code >= 0])) == 2
    elif name.startswith("corner"):
        for x in range(1, dims[0] - 1):
            assert AX.axes_per_wave(mask, code, axes, x, 5)[0] == {1, 2}, x
    else:
        assert set(int(k) for k in code[code >= 0] & 3) == ({OB.VEL_0N, OB.PRES_0P} if name.endswith("original") else {OB.VEL_0P, OB.PRES_0N})
    L = _lattice(gpu, name)
    try:
        _compare_1_and_50(L, name)
    finally:
        L.destroy()


# ---- 3: the other collide variants

@pytest.mark.parametrize("name", SCENES)
def test_with_body_force_boxes(gpu, name):
    """collide_stream_kernel<true, true>"""
    dims, mask, patches, code, axes, val, _ = _scene(name)
    L = _lattice(gpu, name)
    try:
        boxes, forces = _force_boxes(dims, patches)
        L.setExternalVectorBoxes(boxes, forces)
        _compare_1_and_50(L, name, with_boxes=True)
        _, u_ref, _ = AX.observe(_restated(name, True)[50], mask, NONPER, BODY, None, code, axes, val, boxes=boxes, box_forces=forces)
        _, u = L.rho_u()
        live = AX.exchanging(mask)   # the solid block of the L-shaped ducts holds nodes that the collide skips
        assert np.array_equal(u.reshape(dims + (3,))[live], u_ref[live])
    finally:
        L.destroy()


@pytest.mark.parametrize("padding", [1, -1])
@pytest.mark.parametrize("name", SCENES)
def test_with_forced_plane_padding(gpu, name, padding):
    """ob_code is indexed by the padded node number: 1 pads every plane by eight rows more, -1 removes the padding"""
    lib = gpu.capi.lib()
    gpu.check(lib.hc_debug_force_plane_padding(padding))
    L = None
    try:
        L = _lattice(gpu, name)
        _compare_1_and_50(L, name)
    finally:
        gpu.check(lib.hc_debug_force_plane_padding(0))
        if L is not None:
            L.destroy()


@pytest.mark.parametrize("parts", [(1, 2), (3, 4)])
@pytest.mark.parametrize("name", SCENES)
def test_split_launches_give_the_bits_of_one_launch(gpu, name, parts):
    L = _lattice(gpu, name)
    try:
        def advance(n):
            for _ in range(n):
                for p in parts:
                    L.collide_part(p)
                L.step_end()
        _compare_1_and_50(L, name, advance=advance)
    finally:
        L.destroy()


# ---- 4: observers

@pytest.mark.parametrize("name", ["y-original", "y-mirrored", "z-original", "z-mirrored", "corner-yz"])
def test_observers_report_the_completed_moments(gpu, name):
    """rho_u, pi_neq and planeVelocity (on x planes, the only ones it has) on a stepped lattice: bit for bit AX.observe(), and
    against the prescribed values in extended precision: u_bc + F / 2 on velocity nodes, the prescribed density and tangential
    velocity F / 2 on pressure nodes, to 1e-14 (the bound of the x tests).  fluid_stats (what 0) reduces on the device in an
    order numpy does not have, so its minimum, maximum and mean are checked to 1e-14 against the speeds of AX.observe(), as
    the x test checks them, not to the bit.  The corner box puts nodes of two axes into one wavefront of these kernels."""
    dims, mask, patches, code, axes, val, _ = _scene(name)
    L = _lattice(gpu, name)
    try:
        L.collideAndStream(7)
        S = L.populations().reshape(dims + (19,))
        assert np.isfinite(S).all()
        rho_ref, u_ref, pi_ref = AX.observe(S, mask, NONPER, BODY, None, code, axes, val)
        fluid = mask == 0
        assert float(np.abs(rho_ref[fluid] - 1.0).max()) < 0.1
        rho, u = L.rho_u()
        rho, u, pi = rho.reshape(dims), u.reshape(dims + (3,)), L.pi_neq().reshape(dims + (6,))
        half = np.asarray(BODY, np.longdouble) / 2
        for kind, axis in sorted(set((int(k) & 3, int(a)) for k, a in zip(code[code >= 0], axes[code >= 0]))):
            sel = fluid & (code >= 0) & ((code & 3) == kind) & (axes == axis)
            assert sel.any()
            tangential = [a for a in range(3) if a != axis]
            v = val[code[sel] >> 2]
            if kind in VELOCITY:
                err = np.abs(u[sel].astype(np.longdouble) - (v[:, :3].astype(np.longdouble) + half))
            else:
                err = np.abs(np.concatenate([(rho[sel].astype(np.longdouble) - v[:, 3])[:, None],
                                             u[sel][:, tangential].astype(np.longdouble) - half[tangential]], axis=1))
            print("%s kind %d: largest error against the prescribed values %.3e" % (name, kind, float(err.max())))
            assert float(err.max()) <= 1e-14, (kind, float(err.max()))
        assert np.array_equal(rho, rho_ref)
        assert np.array_equal(u, u_ref)
        assert np.array_equal(pi, pi_ref)
        rho_plain, _, _ = OB.observe(S, mask, NONPER, BODY)
        assert not np.array_equal(rho_plain[fluid], rho_ref[fluid])
        for x in (1, dims[0] // 2, dims[0] - 2):   # plane_velocity_kernel<true> on planes that cross the open faces
            yz = np.flatnonzero(mask[x].reshape(-1) == 0)
            assert (code[x].reshape(-1)[yz] >= 0).any()
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


# ---- 5: interpolation next to the open planes

def _vertices_next_to_the_open_planes(dims, axis, n_per_cell, seed):
    """the first cell's vertices within one node of the first plane of `axis`, the second's within one node of the last; the
    other coordinates anywhere between the walls, so that some stencils also meet bounce-back nodes"""
    rng = np.random.default_rng(seed)
    p = np.empty((2 * n_per_cell, 3))
    for a in range(3):
        p[:, a] = rng.uniform(1.0, dims[a] - 2.0, 2 * n_per_cell)
    p[:n_per_cell, axis] = rng.uniform(0.02, 0.98, n_per_cell)
    p[n_per_cell:, axis] = rng.uniform(dims[axis] - 1.98, dims[axis] - 1.02, n_per_cell)
    return p


@pytest.mark.parametrize("per_vertex", [0, 1])
@pytest.mark.parametrize("name", ["y-original", "z-original"])
def test_interpolation_next_to_the_open_planes(gpu, name, per_vertex):
    """the LDS-tiled and the per-vertex kernel against a phi2 interpolation of the completed node velocities of AX.observe();
    the bound is that of the x test"""
    lib = gpu.capi.lib()
    dims, mask, patches, code, axes, val, _ = _scene(name)
    axis = "xyz".index(name[0])
    P = gpu.base_parameters()
    L = _lattice(gpu, name)
    gpu.check(lib.hc_debug_ibm_per_vertex(per_vertex))
    try:
        h = gpu.HemoCell(L, P)
        h.cellfields.addCellType(gpu.CellType.rbc(P), 1)
        # the RBC disc (radius 7.82 nodes) lies in the x-z plane as it comes; turned about z it lies in the y-z plane.  Either
        # way it spans the open axis and the 19-node axis, and its thin side the 17-node axis, clear of the walls
        for k in range(2):
            centre, angles = ([8.0, 7.0 + 10.0 * k, 9.0], (0.0, 0.0, 90.0)) if axis == 1 else ([9.0, 8.0, 7.0 + 10.0 * k], (0.0, 0.0, 0.0))
            assert h.cellfields.addCell(0, tuple(centre), angles)
        cf = h.cellfields
        nv = len(cf.positions) // 2
        pos = _vertices_next_to_the_open_planes(dims, axis, nv, 8)
        cf.positions = pos
        L.collideAndStream(5)
        S = L.populations().reshape(dims + (19,))
        _, u_ref, _ = AX.observe(S, mask, NONPER, BODY, None, code, axes, val)
        _, u_plain, _ = OB.observe(S, mask, NONPER, BODY)
        cf.interpolateFluidVelocity()
        want = AX.interpolate_phi2(pos, u_ref, mask)
        got = cf.velocities
        assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max(), float(np.abs(got - want).max())
        assert np.abs(AX.interpolate_phi2(pos[::40], u_plain, mask) - want[::40]).max() > 1e-4
    finally:
        gpu.check(lib.hc_debug_ibm_per_vertex(0))
        L.destroy()


# ---- 6: refusals and bookkeeping

def test_refusals_and_read_back(gpu):
    L = gpu.Lattice(8, 6, 6, NONPER, 1.0)
    try:
        with pytest.raises(gpu.HcError, match="axis must be 0, 1 or 2"):
            L.addOpenBoundaryNodes(0, -1, [[1, 0, 1]], axis=3)
        with pytest.raises(gpu.HcError, match="axis must be 0, 1 or 2"):
            L._add_open_box(1, 1, (0, 7, 0, 0, 0, 5), axis=-1)
        assert (L.openBoundaryAxes([[1, 0, 1], [0, 0, 0]]) == -1).all()
        first, n = L.addVelocityBoundary1N((1, 6, 0, 0, 0, 5))
        assert (first, n) == (0, 36)
        L.setBoundaryVelocity((1, 6, 0, 0, 0, 5), (0.0, 0.01, 0.0))
        # a node that is open on y already is refused on x and on z, and nothing changes
        with pytest.raises(gpu.HcError, match="declared twice"):
            L.addPressureBoundary0N((0, 1, 0, 5, 0, 5))
        with pytest.raises(gpu.HcError, match="declared twice"):
            L.addOpenBoundaryNodes(1, 1, [[3, 3, 5], [2, 0, 5]], axis=2)
        assert np.array_equal(L.openBoundaryAxes([[0, 3, 3], [3, 3, 5], [2, 0, 5], [6, 0, 0]]), [-1, -1, 1, 1])
        assert np.array_equal(L.openBoundarySlots([[0, 3, 3], [3, 3, 5], [2, 0, 5]]), [-1, -1, 6 + 5])
        assert np.all(L.openBoundaryValues(first, n) == np.array([0.0, 0.01, 0.0, 1.0]))
        assert L.addPressureBoundary2P((1, 6, 1, 4, 5, 5)) == (36, 24)
        assert L.addPressureBoundary0P((7, 7, 1, 4, 1, 4)) == (60, 16)
        assert np.array_equal(L.openBoundaryAxes([[2, 0, 5], [2, 1, 5], [7, 2, 2], [7, 0, 0], [9, 0, 0]]), [1, 2, 0, -1, -1])
        L.clearOpenBoundaries()
        assert (L.openBoundaryAxes([[2, 0, 5], [2, 1, 5], [7, 2, 2]]) == -1).all()
    finally:
        L.destroy()


def test_cleared_boundaries_step_as_a_plain_lattice(gpu):
    dims, mask, _, _, _, _, S0 = _scene("bent-yz")
    A = _lattice(gpu, "bent-yz")
    B = gpu.Lattice(*dims, NONPER, OMEGA)
    try:
        B.defineBounceBack(mask); B.setExternalVector(BODY); B.set_populations(S0.reshape(-1, 19))
        A.collideAndStream(1)
        assert not np.array_equal(A.populations(), OB.step(S0, mask, NONPER, OMEGA, BODY).reshape(-1, 19))
        A.set_populations(S0.reshape(-1, 19))
        A.clearOpenBoundaries()
        A.collideAndStream(3); B.collideAndStream(3)
        live = AX.exchanging(mask).reshape(-1)   # the collide skips solid nodes that no fluid node touches
        assert np.array_equal(A.populations()[live], B.populations()[live])
        ra, ua = A.rho_u(); rb, ub = B.rho_u()
        assert np.array_equal(ra[live], rb[live]) and np.array_equal(ua[live], ub[live])
    finally:
        A.destroy(); B.destroy()


def test_lees_edwards_is_refused_with_y_open_nodes(gpu):
    A = gpu.Lattice(12, 8, 8, (True, True, True), 1.0)
    B = gpu.Lattice(12, 8, 8, (True, True, True), 1.0)
    try:
        A.addVelocityBoundary1N((0, 11, 3, 3, 0, 7))
        with pytest.raises(gpu.HcError, match="open boundaries and Lees-Edwards do not combine"):
            A.setLeesEdwards(0.01, -0.01)
        B.setLeesEdwards(0.01, -0.01)
        with pytest.raises(gpu.HcError, match="open boundaries and Lees-Edwards do not combine"):
            B.addPressureBoundary2P((0, 11, 0, 7, 5, 5))
        assert (B.openBoundaryAxes([[3, 3, 5]]) == -1).all()
    finally:
        A.destroy(); B.destroy()


# ---- 7: axis 0 through the new entry point

def test_axis_0_through_the_new_entry_point_gives_the_old_bits(gpu):
    dims = AX.CHANNEL_DIMS[0]
    mask = AX.channel_mask(dims, 0)
    patches = AX.channel_patches("four", 0, dims)
    S0 = AX.initial_state(dims)
    A = gpu.Lattice(*dims, NONPER, OMEGA)
    B = gpu.Lattice(*dims, NONPER, OMEGA)
    try:
        for L in (A, B):
            L.defineBounceBack(mask); L.setExternalVector(BODY); L.set_populations(S0.reshape(-1, 19))
        for kind, axis, box, values in patches:
            k, o = (0 if kind in VELOCITY else 1), (-1 if kind in (OB.VEL_0N, OB.PRES_0N) else 1)
            bb = (C.c_int * 6)(*box)
            fa, na, fb, nb = C.c_int(), C.c_int(), C.c_int(), C.c_int()
            gpu.check(A.lib.hcl_open_boundary_add_box_axis(A.ptr, k, 0, o, bb, C.byref(fa), C.byref(na)))
            gpu.check(B.lib.hcl_open_boundary_add_box(B.ptr, k, o, bb, C.byref(fb), C.byref(nb)))
            assert (fa.value, na.value) == (fb.value, nb.value) and na.value == len(values)
            for L in (A, B):
                (L.setOpenBoundaryDensitySlots if k else L.setOpenBoundaryVelocitySlots)(fa.value, values)
        nodes = np.argwhere(mask >= 0)
        assert np.array_equal(A.openBoundarySlots(nodes), B.openBoundarySlots(nodes))
        assert np.array_equal(A.openBoundaryAxes(nodes), B.openBoundaryAxes(nodes))
        A.collideAndStream(50); B.collideAndStream(50)
        got = A.populations()
        assert np.isfinite(got).all() and np.array_equal(got, B.populations())
        assert not np.array_equal(got[mask.reshape(-1) == 0][:, 10], S0.reshape(-1, 19)[mask.reshape(-1) == 0][:, 10])
    finally:
        A.destroy(); B.destroy()
