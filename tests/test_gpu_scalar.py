"""The CEPAC scalar field on the GPU (hemocell_amd/csrc/scalar.hip) against its numpy restatement tests/scalar_ref.py, bit for
bit: the step under every kind of wall and body force, the advecting velocity with and without an IBM force, hc_iterate's
schedule, sources, the device reduction, the vertex sampler against tests/ibm_ref.py, and the refusals.

Comparisons run over the fluid nodes: the kernel skips solid nodes that have no fluid neighbour and the restatement bounces
them, and nothing such a node holds ever reaches a fluid node (tests/scalar_ref.py)."""
import ctypes as C

import numpy as np
import pytest

import open_boundary_ref as OB
import scalar_ref as SR
from tests import ibm_ref as IR

pytestmark = pytest.mark.gpu

OMEGA_FLOW = 1.0 / 1.1
TAU = 0.8


def _walls(shape, cls_top=1):
    m = np.zeros(shape, np.uint8)
    m[:, 0, :] = m[:, :, 0] = m[:, :, -1] = 1
    m[:, -1, :] = cls_top
    return m


def _config(gpu, name):
    """(dims, periodic, mask, body, boxes, box_forces, wall_u)"""
    dims, per = (37, 9, 11), (True, False, False)   # odd, not a multiple of 64
    body, boxes, forces, wall_u = (0.0, 0.0, 0.0), None, None, None
    if name == "periodic":
        return dims, (True, True, True), np.zeros(dims, np.uint8), body, boxes, forces, wall_u
    if name == "pipe":
        dims = (20, 17, 17)
        mask = gpu.pipe_mask(*dims)[0]
        return dims, per, mask, body, boxes, forces, wall_u
    mask = _walls(dims, 3 if name == "moving wall" else 1)
    if name == "moving wall":
        wall_u = {3: (0.03, 0.0, -0.01)}
    if name == "body force":
        body = (2e-4, -1e-4, 5e-5)
    if name == "force regions":
        body = (1e-4, 0.0, 0.0)
        boxes, forces = [(0, 17, 0, 8, 0, 10), (10, 30, 2, 5, 3, 7)], [(-2e-4, 1e-4, 0.0), (0.0, 3e-4, -1e-4)]
    return dims, per, mask, body, boxes, forces, wall_u


def _lattice(gpu, dims, per, mask, body=(0.0, 0.0, 0.0), boxes=None, forces=None, wall_u=None, omega=OMEGA_FLOW):
    L = gpu.Lattice(*dims, per, omega)
    if mask.any():
        L.defineBounceBack(mask)
    L.setExternalVector(body)
    if boxes is not None:
        L.setExternalVectorBoxes(boxes, forces)
    for cls, w in (wall_u or {}).items():
        L.setBoundaryVelocity(cls, w)
    return L


def _same_on_fluid(got, want, mask):
    fl = mask.reshape(-1) == 0
    g, w = got.reshape(len(fl), -1)[fl], want.reshape(len(fl), -1)[fl]
    assert np.array_equal(g, w), "max |diff| on fluid nodes %.3e" % np.abs(g - w).max()


@pytest.mark.parametrize("padding", [1, -1])
@pytest.mark.parametrize("name", ["periodic", "walls", "pipe", "moving wall", "body force", "force regions"])
def test_step_bit_for_bit(gpu, name, padding):
    """random flow and scalar populations of magnitude 0.01, 3 rounds of hcl_collide_stream followed by hcl_scalar_step"""
    dims, per, mask, body, boxes, forces, wall_u = _config(gpu, name)
    gpu.check(gpu.capi.lib().hc_debug_force_plane_padding(padding))
    L = None
    try:
        L = _lattice(gpu, dims, per, mask, body, boxes, forces, wall_u)
        S = L.createCEPACfield(TAU)
        rng = np.random.default_rng(17)
        f = rng.uniform(-0.01, 0.01, size=dims + (19,))
        g = rng.uniform(-0.01, 0.01, size=dims + (19,))
        L.set_populations(f.reshape(-1, 19)); S.set_populations(g.reshape(-1, 19))
        _same_on_fluid(S.populations(), g, mask)
        for _ in range(3):
            L.collideAndStream(1)
            f = OB.step(f, mask, per, OMEGA_FLOW, body, boxes=boxes, box_forces=forces, wall_u=wall_u)
            u = SR.velocity(f, mask, body, boxes=boxes, box_forces=forces)
            ug = S.velocity()
            _same_on_fluid(ug, u, mask)
            _same_on_fluid(ug, L.rho_u()[1], mask)   # without cells the observer's velocity, bit for bit
            assert not ug.reshape(dims + (3,))[mask != 0].any()
            S.collideAndStream()
            g = SR.step(g, mask, per, 1.0 / TAU, u)
            _same_on_fluid(S.populations(), g, mask)
            _same_on_fluid(S.concentration(), SR.concentration(g), mask)
        _same_on_fluid(L.populations(), f, mask)   # the flow is what it was going to be
    finally:
        gpu.check(gpu.capi.lib().hc_debug_force_plane_padding(0))
        if L is not None:
            L.destroy()


def test_collide_stream_alone_leaves_the_scalar(gpu):
    dims = (12, 6, 6)
    L = gpu.Lattice(*dims, (True, True, True), OMEGA_FLOW)
    try:
        S = L.createCEPACfield(TAU)
        g = np.random.default_rng(1).uniform(-0.01, 0.01, size=(L.n, 19))
        S.set_populations(g)
        L.collideAndStream(3)
        assert np.array_equal(S.populations(), g)
        S.initializeAtEquilibrium(1.5, box=(2, 4, 0, 5, 0, 5))   # the box's nodes see the equilibrium of 1.5, the others what they saw
        want = g.reshape(dims + (19,)).copy()
        want[2:5] = SR.T * 0.5
        assert np.array_equal(S.populations().reshape(dims + (19,)), want)
        S.initializeAtEquilibrium(2.0)
        assert np.array_equal(S.concentration(), SR.concentration(SR.equilibrium(dims, 2.0)).reshape(-1))
    finally:
        L.destroy()


# ---- with membrane cells: the IBM force enters the advecting velocity
IBM_DIMS, IBM_PER, IBM_BODY = (24, 16, 16), (True, True, True), (3e-5, 0.0, -1e-5)


def _rbc_scene(gpu, seed=5):
    L = gpu.Lattice(*IBM_DIMS, IBM_PER, OMEGA_FLOW)
    P = gpu.base_parameters()
    h = gpu.HemoCell(L, P)
    h.cellfields.addCellType(gpu.CellType.rbc(P), 1)
    assert h.cellfields.addCell(0, (11.3, 8.2, 7.9), (30.0, 10.0, 0.0))
    L.latticeEquilibrium()
    L.setExternalVector(IBM_BODY)
    S = L.createCEPACfield(TAU)
    rng = np.random.default_rng(seed)
    S.set_populations(rng.uniform(-0.01, 0.01, size=(L.n, 19)))
    return L, h, S, rng


def test_ibm_force_enters_the_velocity(gpu):
    """phase by phase: spread, ibm_force(), collide, step_end, scalar step"""
    mask = np.zeros(IBM_DIMS, np.uint8)
    L, h, S, rng = _rbc_scene(gpu)
    try:
        cells = h.cellfields
        g = S.populations().reshape(IBM_DIMS + (19,))
        for _ in range(2):
            cells.forces = rng.uniform(-1e-3, 1e-3, size=(cells.counts()[0], 3))
            cells.spreadParticleForce(False)
            F = L.ibm_force()
            assert np.count_nonzero(F) > 100 and not F.reshape(IBM_DIMS + (3,))[0].any()   # touched and untouched nodes
            L.collide_part(0); L.step_end()
            f = L.populations().reshape(IBM_DIMS + (19,))
            u = SR.velocity(f, mask, IBM_BODY, F=F)
            assert np.array_equal(S.velocity(), u.reshape(-1, 3))
            assert not np.array_equal(u, SR.velocity(f, mask, IBM_BODY))   # the force is in it
            S.collideAndStream()
            g = SR.step(g, mask, IBM_PER, 1.0 / TAU, u)
            assert np.array_equal(S.populations().reshape(g.shape), g)
    finally:
        h.cellfields.destroy(); L.destroy()


@pytest.mark.parametrize("overlap", [0, 1])
def test_iterate_steps_the_scalar_whatever_the_call_pattern(gpu, overlap):
    """with the reproducible spread, twelve calls of hc_iterate(.., 1) and one call of hc_iterate(.., 12) give the same bits"""
    lib = gpu.capi.lib()
    got = []
    try:
        gpu.check(lib.hc_set_reproducible_spread(1)); gpu.check(lib.hc_set_overlap(overlap))
        for calls, n in ((12, 1), (1, 12)):
            L, h, S, _ = _rbc_scene(gpu)
            try:
                h.setParticleVelocityUpdateTimeScaleSeparation(3)
                g0 = S.populations()
                h.cellfields.applyConstitutiveModel(0, True)
                for _ in range(calls):
                    h.iterate(n)
                assert h.iter == 12
                got.append((S.populations(), L.populations(), h.cellfields.positions))
                assert not np.array_equal(got[-1][0], g0)
            finally:
                h.cellfields.destroy(); L.destroy()
    finally:
        gpu.check(lib.hc_set_reproducible_spread(0)); gpu.check(lib.hc_set_overlap(1))
    for a, b in zip(*got):
        assert np.array_equal(a, b)


def test_sources_bit_for_bit(gpu):
    """two boxes with different values, one touching a wall, 20 steps beside a driven flow"""
    dims, per, body = (21, 9, 10), (True, False, False), (2e-4, 0.0, 0.0)
    mask = _walls(dims)
    L = _lattice(gpu, dims, per, mask, body)
    try:
        L.latticeEquilibrium()
        S = L.createCEPACfield(TAU)
        src = SR.Sources(dims)
        for box, val in (((3, 5, 0, 2, 2, 4), 1.75), ((12, 12, 4, 6, 5, 5), 0.25)):   # the first reaches into the wall y = 0
            S.addSource(box, val); src.add(box, val)
        f = L.populations().reshape(dims + (19,))
        g = SR.equilibrium(dims, 1.0, mask)
        _same_on_fluid(S.populations(), g, mask)

        def advance(n):
            nonlocal f, g
            for _ in range(n):
                L.collideAndStream(1); S.collideAndStream()
                f = OB.step(f, mask, per, OMEGA_FLOW, body)
                g = SR.step(g, mask, per, 1.0 / TAU, SR.velocity(f, mask, body), src)
            _same_on_fluid(S.populations(), g, mask)
            _same_on_fluid(S.concentration(), SR.concentration(g, mask, src), mask)

        advance(20)
        Cg = S.concentration().reshape(dims)
        assert np.all(Cg[3:6, 1:3, 2:5] == 1.75) and np.all(Cg[12, 4:7, 5] == 0.25)
        assert 1.0 < Cg[8, 2, 3] < 1.75   # and it has spread
        S.clearSources(); src.clear()
        advance(2)   # the boxes are back to the plain collide
        assert not np.any(S.concentration().reshape(dims)[3:6, 1:3, 2:5] == 1.75)
        for k in range(8):   # the table is empty again: eight values fit, a ninth is refused and changes nothing
            S.addSource((1 + k, 1 + k, 1, 1, 1, 1), 2.0 + k)
        S.addSource((2, 2, 2, 2, 2, 2), 2.0)   # a value that is in the table already
        before = S.concentration()
        with pytest.raises(gpu.HcError, match="more than HC_MAX_SCALAR_SOURCES distinct source values"):
            S.addSource((4, 4, 4, 4, 4, 4), 77.0)
        assert np.array_equal(S.concentration(), before)
        with pytest.raises(gpu.HcError, match="the value is not a number"):
            S.addSource((4, 4, 4, 4, 4, 4), float("nan"))
        S.addSource((50, 60, 1, 1, 1, 1), 88.0)   # wholly outside: nothing registered, nothing refused
        assert np.array_equal(S.concentration(), before)
        S.addSource((2, 2, 1, 1, 1, 1), 77.0)   # painting over the only node of value 3.0 gives its slot back
        after = S.concentration().reshape(dims)
        assert after[2, 1, 1] == 77.0 and after[1, 1, 1] == 2.0 and after[2, 2, 2] == 2.0 and after[8, 1, 1] == 9.0
    finally:
        L.destroy()


def test_stats_against_the_download(gpu):
    dims = (20, 17, 17)
    mask = gpu.pipe_mask(*dims)[0]
    L = _lattice(gpu, dims, (True, False, False), mask)
    try:
        S = L.createCEPACfield(TAU)
        S.set_populations(np.random.default_rng(2).uniform(-0.01, 0.01, size=(L.n, 19)))
        S.addSource((4, 6, 7, 9, 7, 9), 3.5)   # the observers' C_s counts
        Cf = S.concentration()[mask.reshape(-1) == 0]
        total, lo, hi = S.stats()
        want = float(np.sum(Cf.astype(np.longdouble)))
        assert abs(total - want) <= 1e-12 * abs(want)
        assert lo == Cf.min() and hi == Cf.max() == 3.5
    finally:
        L.destroy()


def test_sample_scalar_against_the_interpolation(gpu):
    """an RBC next to the pipe wall (part of its stencils is wall: fewer nodes, renormalised weights) and one across the
    periodic seam in x: <= 1e-13, the bound the interpolation tests hold against the same restatement"""
    dims, per = (32, 26, 26), (True, False, False)
    mask = gpu.pipe_mask(*dims)[0]
    L = _lattice(gpu, dims, per, mask)
    P = gpu.base_parameters()
    cells = gpu.Cells(L, P)
    try:
        cells.addCellType(gpu.CellType.rbc(P), 1)
        assert cells.addCell(0, (9.0, 12.5, 12.5), (90.0, 0.0, 0.0)) and cells.addCell(0, (23.0, 12.5, 12.5), (90.0, 0.0, 0.0))
        pos = cells.positions
        nv = len(pos) // 2
        a = pos[:nv]   # towards the wall along y until the outermost vertex is 0.4 lu inside the radius
        R = (dims[1] - 2) / 2.0
        for _ in range(400):
            if np.hypot(a[:, 1] - 12.5, a[:, 2] - 12.5).max() >= R - 0.4:
                break
            a[:, 1] += 0.05
        pos[nv:, 0] -= 23.3   # the second one sits on the seam, at negative and positive x
        cells.positions = pos
        S = L.createCEPACfield(TAU)
        S.set_populations(np.random.default_rng(9).uniform(-0.02, 0.02, size=(L.n, 19)))
        Cn = S.concentration()
        adm = IR.stencil(pos, dims, per, mask)[2]
        adm_walls = IR.stencil(pos, dims, per, mask, wrong="admit_walls")[2]
        assert (adm_walls & ~adm)[:nv].any() and not (adm_walls & ~adm)[nv:].any()   # wall nodes in stencils of the first cell
        assert (pos[nv:, 0] < 0).any() and (pos[nv:, 0] > 0).any()
        want = IR.interpolate(pos, np.ones(len(pos), bool), np.repeat(Cn[:, None], 3, axis=1), dims, per, mask)["v"][:, 0]
        got = cells.sampleScalar(S)
        err = np.abs(got - want).max()
        print("sampleScalar: max |difference| %.3e over %d vertices, C between %.3f and %.3f" % (err, len(pos), got.min(), got.max()))
        assert err <= 1e-13
        assert np.ptp(got) > 0.01
    finally:
        cells.destroy(); L.destroy()


# ---- refusals: each with its message, hc_last_error set, the lattice usable afterwards
def _refused(gpu, call, message):
    with pytest.raises(gpu.HcError) as e:
        call()
    assert message in str(e.value), str(e.value)
    assert message.encode() in gpu.capi.lib().hc_last_error()


def _usable(L):
    before = L.populations()
    L.collideAndStream(1)
    assert np.isfinite(L.populations()).all() and before.shape == (L.n, 19)


def _small(gpu, per=(True, True, True), **kw):
    L = gpu.Lattice(8, 6, 6, per, OMEGA_FLOW, **kw)
    L.latticeEquilibrium()
    return L


def test_refused_omega(gpu):
    L = _small(gpu)
    try:
        lib = gpu.capi.lib()
        for omega in (0.0, 2.0, -0.5, 2.5, float("nan")):
            out = C.c_void_p()
            assert lib.hcl_scalar_create(L.ptr, omega, C.byref(out)) != 0 and not out
            assert b"hcl_scalar_create: omega must be in (0,2)" in lib.hc_last_error()
        _refused(gpu, lambda: L.createCEPACfield(0.5), "omega must be in (0,2)")
        _usable(L)
        S = L.createCEPACfield(0.500001)   # and one just inside is taken
        _refused(gpu, lambda: L.createCEPACfield(TAU), "hcl_scalar_create: the lattice has a scalar field already")
        S.destroy()
        L.createCEPACfield(TAU)   # after the first one is gone there is room again
        _usable(L)
    finally:
        L.destroy()


def test_refused_slab(gpu):
    L = gpu.Lattice(8, 6, 6, (True, True, True), OMEGA_FLOW, x0=0, nx_global=16, n_slabs=2)
    try:
        _refused(gpu, lambda: L.createCEPACfield(TAU), "hcl_scalar_create: the scalar field needs the whole domain on one GPU (n_slabs = 1)")
    finally:
        L.destroy()


@pytest.mark.parametrize("other", ["open boundaries", "Lees-Edwards", "interior viscosity"])
def test_refused_with_another_feature_in_either_order(gpu, other):
    enable = {"open boundaries": lambda L: L.addVelocityBoundary0N((0, 0, 1, 4, 1, 4)),
              "Lees-Edwards": lambda L: L.setLeesEdwards(0.01, -0.01),
              "interior viscosity": lambda L: L.enableInteriorViscosity([0.9])}[other]
    per = (False, True, True) if other == "open boundaries" else (True, True, True)
    has = {"open boundaries": "the lattice has open-boundary nodes; the scalar field and open boundaries do not combine",
           "Lees-Edwards": "the lattice has a Lees-Edwards boundary; the scalar field and Lees-Edwards do not combine",
           "interior viscosity": "the lattice has interior viscosity enabled; the scalar field and interior viscosity do not combine"}[other]
    back = {"open boundaries": "the lattice has a scalar field; the scalar field and open boundaries do not combine",
            "Lees-Edwards": "hcl_set_lees_edwards: the lattice has a scalar field; the scalar field and Lees-Edwards do not combine",
            "interior viscosity": "hcl_interior_enable: the lattice has a scalar field; the scalar field and interior viscosity do not combine"}[other]
    L = _small(gpu, per)
    try:
        enable(L)
        _refused(gpu, lambda: L.createCEPACfield(TAU), "hcl_scalar_create: " + has)
        _usable(L)
    finally:
        L.destroy()
    L = _small(gpu, per)
    try:
        S = L.createCEPACfield(TAU)
        _refused(gpu, lambda: enable(L), back)
        _usable(L)
        S.collideAndStream()
        assert np.array_equal(S.concentration(), np.ones(L.n))
    finally:
        L.destroy()


def test_refused_with_a_preinlet(gpu):
    lib = gpu.capi.lib()
    pre, dom = _small(gpu), _small(gpu, (False, True, True))
    try:
        P = C.c_void_p()
        gpu.check(lib.hcl_preinlet_create(C.byref(P), pre.ptr, dom.ptr, 0, 0, None, 0, 0))   # a pair that couples no node yet
        for L in (pre, dom):
            _refused(gpu, lambda: L.createCEPACfield(TAU), "hcl_scalar_create: the lattice is part of a pre-inlet pair; the scalar field and a pre-inlet do not combine")
            _usable(L)
        gpu.check(lib.hcl_preinlet_destroy(P))
        S = pre.createCEPACfield(TAU)   # the pair is gone
        P = C.c_void_p()
        assert lib.hcl_preinlet_create(C.byref(P), pre.ptr, dom.ptr, 0, 0, None, 0, 0) != 0 and not P
        assert b"hcl_preinlet_create: a lattice has a scalar field; the scalar field and a pre-inlet do not combine" in lib.hc_last_error()
        prm = gpu.base_parameters()
        cp, cd = gpu.Cells(pre, prm), gpu.Cells(dom, prm)
        try:
            X, shift = C.c_void_p(), np.zeros(3)
            assert lib.hcp_preinlet_create(C.byref(X), cp.ptr, cd.ptr, 0, -1, 0.0, 4.0, gpu.dptr(shift), 1000) != 0 and not X
            assert b"hcp_preinlet_create: a lattice has a scalar field; the scalar field and a pre-inlet do not combine" in lib.hc_last_error()
        finally:
            cp.destroy(); cd.destroy()
        S.collideAndStream(); _usable(pre); _usable(dom)
    finally:
        pre.destroy(); dom.destroy()
