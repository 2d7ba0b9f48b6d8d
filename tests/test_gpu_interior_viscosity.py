"""Interior viscosity on the GPU against tests/interior_viscosity_ref.py: the collide with a per-node omega (populations bit for
bit), the ray-cast and the membrane pass (class fields equal), their cadence inside hc_iterate, neutrality at viscosity ratio 1
and the refusals."""
import ctypes as C

import numpy as np
import pytest

import interior_viscosity_ref as IV
import interior_viscosity_scene as SC

pytestmark = pytest.mark.gpu


def _profile(lib, name):
    ms, n = C.c_double(), C.c_long()
    assert lib.hc_profile_read(name.encode(), C.byref(ms), C.byref(n)) == 0
    return n.value


def _add_unchecked(gpu, cf, t, cell_id):
    c, a = np.array([8.0, 8.0, 8.0]), np.zeros(3)
    gpu.check(gpu.capi.lib().hcp_add_cell_unchecked(cf.ptr, int(t), int(cell_id), gpu.dptr(c), gpu.dptr(a)))


# ---- collide

CDIMS, CPER = (12, 10, 8), (True, False, True)
COMEGA, COMEGAS, CBODY = 1.0 / 0.9, [1.0 / 2.1, 1.0 / 0.62], (2e-6, 3e-7, -1e-7)
CWALL_U = {3: (0.01, 0.0, -0.004)}
CBOXES = ([(2, 7, 1, 5, 0, 7), (6, 11, 3, 8, 2, 5)], [(-3e-6, 1e-6, 2e-6), (5e-6, -2e-6, 1e-6)])


def _collide_mask():
    m = np.zeros(CDIMS, np.uint8)
    m[:, 0, :] = 1
    m[:, -1, :] = 3
    return m


@pytest.mark.parametrize("parts", [(0,), (1, 2), (3, 4)])
@pytest.mark.parametrize("regions", [False, True])
def test_collide_matches_restatement_bit_for_bit(gpu, regions, parts):
    """12 x 10 x 8, periodic along x and z, a bounce-back layer and a moving-wall layer on the y faces, random populations,
    random classes 0..2 with two omegas, a random per-node force (random vertex forces spread reproducibly and read back), body-
    force boxes on and off; three steps in one launch per step and through the split launches.  Fluid nodes, bit for bit."""
    lib = gpu.capi.lib()
    P = gpu.base_parameters()
    L = gpu.Lattice(*CDIMS, CPER, COMEGA)
    gpu.check(lib.hc_set_reproducible_spread(1))
    gpu.check(lib.hc_profile_enable(1))
    try:
        rng = np.random.default_rng(11)
        mask = _collide_mask()
        L.defineBounceBack(mask)
        L.setBoundaryVelocity(3, CWALL_U[3])
        L.setExternalVector(CBODY)
        kw = dict(wall_u=CWALL_U)
        if regions:
            L.setExternalVectorBoxes(*CBOXES)
            kw.update(boxes=CBOXES[0], box_forces=CBOXES[1])
        L.enableInteriorViscosity(COMEGAS)
        cls = rng.integers(0, 3, CDIMS).astype(np.uint8)
        L.setInteriorClasses(cls)
        assert np.array_equal(L.interiorClasses(), cls) and np.array_equal(L.interiorViscosityOmegas(), COMEGAS)
        assert L.bytes_per_node() == 306.0   # no cells yet: 304 B of populations, the mask byte and the class byte
        cf = gpu.Cells(L, P)
        cf.addCellType(gpu.CellType.rbc(P), 1)
        _add_unchecked(gpu, cf, 0, 0)
        nv = len(cf.positions)
        cf.positions = np.stack([rng.uniform(0.0, 12.0, nv), rng.uniform(1.2, 7.8, nv), rng.uniform(0.0, 8.0, nv)], axis=1)
        S = rng.uniform(-0.005, 0.005, CDIMS + (19,))
        L.set_populations(S.reshape(-1, 19))
        fluid = mask == 0
        gpu.check(lib.hc_profile_reset())
        for step in range(3):
            cf.forces = 1e-4 * rng.standard_normal((nv, 3))
            cf.spreadParticleForce(True)
            F = L.ibm_force().reshape(CDIMS + (3,))
            assert np.abs(F).max() > 0
            S = IV.step(S, mask, CPER, COMEGA, COMEGAS, cls, CBODY, F=F, **kw)
            for p in parts:
                L.collide_part(p)
            L.step_end()
            got = L.populations().reshape(CDIMS + (19,))
            assert np.array_equal(got[fluid], S[fluid]), (step, float(np.abs(got - S)[fluid].max()))
        assert np.isfinite(S).all()
        assert _profile(lib, "collide_stream_interior") == 3 * len(parts) == _profile(lib, "collide_stream")
        other = IV.step(S, mask, CPER, COMEGA, COMEGAS, np.zeros(CDIMS, np.uint8), CBODY, **kw)
        assert not np.array_equal(other[fluid], IV.step(S, mask, CPER, COMEGA, COMEGAS, cls, CBODY, **kw)[fluid])
    finally:
        gpu.check(lib.hc_set_reproducible_spread(0))
        gpu.check(lib.hc_profile_enable(0))
        L.destroy()


@pytest.mark.parametrize("regions", [False, True])
def test_uniform_class_equals_a_plain_lattice(gpu, regions):
    """every node in class 1 (omega 0.8) on a lattice created with omega 1.3 = a plain lattice created with omega 0.8, every
    population of every node, after 3 steps; the plain lattice launches the kernel it always launched"""
    lib = gpu.capi.lib()
    A = gpu.Lattice(*CDIMS, CPER, 1.3)
    B = gpu.Lattice(*CDIMS, CPER, 0.8)
    gpu.check(lib.hc_profile_enable(1))
    try:
        S = np.random.default_rng(12).uniform(-0.005, 0.005, (A.n, 19))
        for L in (A, B):
            L.defineBounceBack(_collide_mask())
            L.setBoundaryVelocity(3, CWALL_U[3])
            L.setExternalVector(CBODY)
            if regions:
                L.setExternalVectorBoxes(*CBOXES)
            L.set_populations(S)
        A.enableInteriorViscosity([0.8])
        A.setInteriorClasses(np.ones(CDIMS, np.uint8))
        gpu.check(lib.hc_profile_reset())
        B.collideAndStream(3)
        assert (_profile(lib, "collide_stream"), _profile(lib, "collide_stream_interior")) == (3, 0)
        A.collideAndStream(3)
        assert (_profile(lib, "collide_stream"), _profile(lib, "collide_stream_interior")) == (6, 3)
        assert np.array_equal(A.populations(), B.populations())
        assert not np.array_equal(A.populations(), S)
    finally:
        gpu.check(lib.hc_profile_enable(0))
        A.destroy(); B.destroy()


# ---- the passes

class Scene:
    """the lattice, cells and restatement inputs of interior_viscosity_scene; order: a permutation of the cell list"""

    def __init__(self, gpu, wall_overlap, order=(0, 1, 2, 3), velocity=(0.0, 0.0, 0.0)):
        self.gpu = gpu
        self.P = gpu.base_parameters()
        self.L = gpu.Lattice(*SC.DIMS, SC.PERIODIC, 1.0 / self.P.tau)
        try:
            self.mask = SC.scene_mask()
            self.L.defineBounceBack(self.mask)
            for c, u in SC.WALL_U.items():
                self.L.setBoundaryVelocity(c, u)
            self.L.latticeEquilibrium(1.0, velocity)
            self.h = gpu.HemoCell(self.L, self.P)
            self.cf = self.h.cellfields
            self.types = [gpu.CellType.rbc(self.P, interior_viscosity=True, viscosity_ratio=r) for r in SC.RATIOS]
            for t in self.types:
                self.cf.addCellType(t, 1)
            self.tables = self.types[0].tables()
            cells = SC.scene_cells(self.tables["vertices"], wall_overlap)
            self.cells = sorted([cells[k] for k in order], key=lambda c: c[1])   # storage order: by type, then as appended
            for cid, t, _ in self.cells:
                _add_unchecked(gpu, self.cf, t, cid)
            self.cf.positions = np.concatenate([p for _, _, p in self.cells])
            self.omegas = [1.0 / IV.tau_interior(r, self.P.tau) for r in SC.RATIOS]
        except Exception:
            self.L.destroy()
            raise

    def restatement_cells(self):
        nv = self.types[0].nv
        pos = self.cf.positions
        now = [(cid, t, pos[k * nv:(k + 1) * nv]) for k, (cid, t, _) in enumerate(self.cells)]
        return SC.restatement_cells(now, self.tables, {0: 1, 1: 2})

    def destroy(self):
        self.L.destroy()


@pytest.fixture(scope="module")
def ray_cast_reference(gpu):
    s = Scene(gpu, True)
    try:
        assert np.array_equal(s.L.interiorViscosityOmegas(), s.omegas)
        cells = s.restatement_cells()
        for c, (_, _, p) in zip(cells, s.cells):
            assert np.array_equal(c["pos"], p)
        want = IV.find(cells, s.mask, SC.PERIODIC)
        # the scene does what it is for: both classes, nodes over both periodic faces, a cell reaching through the wall layer,
        # and nodes where the two types overlap
        assert set(np.unique(want)) == {0, 1, 2}
        assert want[0].any() and want[-1].any() and want[:, :, 0].any() and want[:, :, -1].any()
        assert not want[s.mask != 0].any()
        wall_cell = [c for c in cells if c["id"] == 5][0]
        inside = IV.interior_nodes(wall_cell["pos"], wall_cell["tri"])
        assert (inside[:, 1] == 0).any() and (inside[:, 1] < 0).any()
        a, d = (IV.find([c], s.mask, SC.PERIODIC) for c in cells if c["id"] in (7, 3))
        both = (a != 0) & (d != 0)
        assert both.sum() > 50 and np.all(want[both] == 1)   # id 7 (class 1) comes after id 3 (class 2)
        return want
    finally:
        s.destroy()


@pytest.mark.parametrize("order, block", [((0, 1, 2, 3), 256), ((2, 0, 3, 1), 64), ((1, 2, 0, 3), 512)])
def test_ray_cast_equals_restatement(gpu, ray_cast_reference, order, block):
    """the class field of hcp_interior_find is the restatement's, whatever the order in which the cells were appended and
    whatever the workgroup size; a second pass over a field full of stale tags gives the same field"""
    lib = gpu.capi.lib()
    s = Scene(gpu, True, order)
    try:
        gpu.check(lib.hc_debug_interior_block(block))
        s.cf.findInternalParticleGridPoints()
        got = s.L.interiorClasses()
        assert np.array_equal(got, ray_cast_reference), int((got != ray_cast_reference).sum())
        s.L.setInteriorClasses(np.where(s.mask == 0, 2, 0).astype(np.uint8))
        s.cf.findInternalParticleGridPoints()
        assert np.array_equal(s.L.interiorClasses(), ray_cast_reference)
        tau = s.cf.interiorPoints()
        assert np.array_equal(tau[got == 1], np.full(int((got == 1).sum()), 1.0 / s.omegas[0])) and np.all(tau[got == 0] == 0.0)
    finally:
        gpu.check(lib.hc_debug_interior_block(256))
        s.destroy()


@pytest.mark.parametrize("block", [256, 64])
def test_membrane_pass_equals_restatement(gpu, block):
    """six iterations in a moving fluid between sheared walls, then the membrane pass on the stale field of the initial
    positions.  The normals keep the reference's sum order (the triangles of a vertex in ascending order, from 0), so
    hcp_interior_normals equals the restatement's scatter loop bit for bit; the field equals the restatement applied to the
    downloaded positions.  The restatement's log shows nodes that vertices of two cells decide differently."""
    lib = gpu.capi.lib()
    s = Scene(gpu, False, velocity=(0.05, 0.0, -0.03))
    try:
        gpu.check(lib.hc_debug_interior_block(block))
        gpu.check(lib.hc_set_reproducible_spread(1))
        s.cf.findInternalParticleGridPoints()
        stale = s.L.interiorClasses()
        first = s.cf.positions
        s.cf.setInteriorViscosityTimeScaleSeparation(1000, 1000)
        s.h.iter = 1   # iterations 1 .. 6: no pass is due
        s.h.iterate(6)
        assert np.array_equal(s.L.interiorClasses(), stale)
        assert s.cf.deletion_counts()[2:] == (0, 0)
        cells = s.restatement_cells()
        moved = np.concatenate([c["pos"] for c in cells]) - first
        assert 0.05 < np.abs(moved).max() < 2.0
        nv = s.types[0].nv
        n0 = s.cf.interiorNormals(0)
        n1 = s.cf.interiorNormals(1)
        for k, c in enumerate(cells):
            want_n = IV.normals(c["pos"], c["tri"], c["area_mean_eq"])
            got_n = (n0[k * nv:(k + 1) * nv] if c["type"] == 0 else n1)
            assert np.array_equal(got_n, want_n), (c["id"], float(np.abs(got_n - want_n).max()))
        log = []
        want = IV.membrane(stale.copy(), sorted(cells, key=lambda c: -c["id"]), s.mask, SC.PERIODIC, log)
        verdicts = {}
        for node, cid, _, inside in log:
            verdicts.setdefault(node, set()).add((cid, inside))
        contested = [n for n, v in verdicts.items() if len({c for c, _ in v}) > 1 and len({i for _, i in v}) > 1]
        assert len(contested) > 10
        assert not np.array_equal(want, stale)
        s.cf.internalGridPointsMembrane()
        got = s.L.interiorClasses()
        assert np.array_equal(got, want), int((got != want).sum())
        s.cf.internalGridPointsMembrane()   # the vote words were reset: a second pass gives the same field
        assert np.array_equal(s.L.interiorClasses(), want)
    finally:
        gpu.check(lib.hc_debug_interior_block(256))
        gpu.check(lib.hc_set_reproducible_spread(0))
        s.destroy()


# ---- cadence inside hc_iterate

def _state(s):
    return s.L.populations(), s.cf.positions, s.L.interiorClasses()


@pytest.fixture(scope="module")
def phase_by_phase(gpu):
    """24 iterations driven one call at a time: velocity update every 2, membrane pass every 4, entire grid every 12"""
    lib = gpu.capi.lib()
    s = Scene(gpu, False, velocity=(0.05, 0.0, -0.03))
    gpu.check(lib.hc_set_reproducible_spread(1))
    try:
        cf, n_find, n_membrane = s.cf, 0, 0
        for it in range(24):
            cf.spreadParticleForce(True)
            s.L.collideAndStream(1)
            if it % 2 == 0:
                cf.interpolateFluidVelocity()
            cf.advanceParticles(False)
            cf.applyConstitutiveModel(it)
            if it % 12 == 0:
                cf.deleteIncompleteCells()
                cf.findInternalParticleGridPoints()
                n_find += 1
            if it % 4 == 0:
                cf.internalGridPointsMembrane()
                n_membrane += 1
        state = _state(s)
        assert (n_find, n_membrane) == (2, 6) and set(np.unique(state[2])) == {0, 1, 2}
        return state
    finally:
        gpu.check(lib.hc_set_reproducible_spread(0))
        s.destroy()


@pytest.mark.parametrize("overlap", [0, 1])
def test_iterate_runs_the_passes_at_their_cadence(gpu, phase_by_phase, overlap):
    lib = gpu.capi.lib()
    s = Scene(gpu, False, velocity=(0.05, 0.0, -0.03))
    gpu.check(lib.hc_set_reproducible_spread(1))
    gpu.check(lib.hc_set_overlap(overlap))
    gpu.check(lib.hc_profile_enable(1))
    try:
        s.h.setParticleVelocityUpdateTimeScaleSeparation(2)
        s.cf.setInteriorViscosityTimeScaleSeparation(4, 12)
        gpu.check(lib.hc_profile_reset())
        s.h.iterate(24)
        assert s.h.iter == 24
        assert (_profile(lib, "interior_find"), _profile(lib, "interior_membrane")) == (2, 6)
        assert _profile(lib, "collide_stream_interior") == 24
        assert _profile(lib, "collide_stream_beside") == (11 if overlap else 0)   # odd iterations but the last
        for got, want, name in zip(_state(s), phase_by_phase, ("populations", "positions", "classes")):
            assert np.array_equal(got, want), name
    finally:
        gpu.check(lib.hc_set_overlap(1))
        gpu.check(lib.hc_set_reproducible_spread(0))
        gpu.check(lib.hc_profile_enable(0))
        s.destroy()


def test_timescales_must_be_multiples_of_the_velocity_update(gpu):
    s = Scene(gpu, False)
    try:
        s.h.setParticleVelocityUpdateTimeScaleSeparation(2)
        for bad in ((3, 12), (4, 9)):
            s.cf.setInteriorViscosityTimeScaleSeparation(*bad)
            with pytest.raises(gpu.HcError, match="must divide both interior-viscosity timescales"):
                s.h.iterate(1)
        assert s.h.iter == 0
        s.cf.setInteriorViscosityTimeScaleSeparation(4, 12)
        s.h.iterate(1)
    finally:
        s.destroy()


# ---- neutrality

def _one_cell_run(gpu, ratio):
    lib = gpu.capi.lib()
    P = gpu.base_parameters()
    L = gpu.Lattice(40, 40, 20, (True, False, True), 1.0 / P.tau)
    try:
        m = np.zeros((40, 40, 20), np.uint8)
        m[:, 0, :], m[:, -1, :] = 3, 4
        L.defineBounceBack(m)
        L.setBoundaryVelocity(3, (0.02, 0.0, 0.0)); L.setBoundaryVelocity(4, (-0.02, 0.0, 0.0))
        L.latticeEquilibrium(1.0, (0.01, 0.0, 0.0))
        h = gpu.HemoCell(L, P)
        kw = {} if ratio is None else dict(interior_viscosity=True, viscosity_ratio=ratio)
        h.cellfields.addCellType(gpu.CellType.rbc(P, **kw), 1)
        assert h.cellfields.addCell(0, (20.0, 20.0, 10.0), (20.0, 40.0, 0.0))
        if ratio is not None:
            h.cellfields.setInteriorViscosityTimeScaleSeparation(5, 20)
        gpu.check(lib.hc_profile_reset())
        h.iterate(40)
        out = (L.populations(), h.cellfields.positions, _profile(lib, "collide_stream"), _profile(lib, "collide_stream_interior"))
        tagged = int((L.interiorClasses() != 0).sum()) if ratio is not None else 0
        return out + (tagged,)
    finally:
        L.destroy()


def test_viscosity_ratio_one_is_neutral(gpu):
    """40 x 40 x 20, one RBC in shear, 40 iterations: with viscosity ratio 1 (tau_int = tau, the tagged nodes relax with the
    lattice's own omega) populations and vertices equal those of a run without the feature, which launches the collide
    it always launched; ratio 5 differs"""
    lib = gpu.capi.lib()
    gpu.check(lib.hc_set_reproducible_spread(1))
    gpu.check(lib.hc_profile_enable(1))
    try:
        plain = _one_cell_run(gpu, None)
        one = _one_cell_run(gpu, 1.0)
        five = _one_cell_run(gpu, 5.0)
        assert plain[2:4] == (40, 0) and one[2:4] == (40, 40) and one[4] > 300
        assert np.array_equal(one[0], plain[0]) and np.array_equal(one[1], plain[1])
        assert not np.array_equal(five[0], plain[0]) and not np.array_equal(five[1], plain[1])
    finally:
        gpu.check(lib.hc_set_reproducible_spread(0))
        gpu.check(lib.hc_profile_enable(0))


# ---- the restatement on the library's own sphere

def test_restatement_on_the_wbc_sphere_mesh(gpu):
    """the property of tests/test_interior_viscosity_cpu.py::test_ray_cast_parity_on_a_sphere on the WBC_SPHERE mesh of
    hcp_celltype_tables (building a cell type needs the device)"""
    t = gpu.CellType.wbc(gpu.base_parameters())
    try:
        tab = t.tables()
        v = tab["vertices"] - 0.5 * (tab["vertices"].max(axis=0) + tab["vertices"].min(axis=0))
        counts = SC.check_sphere(v, tab["triangles"], SC.SPHERE_CENTRES)
        assert min(counts) > 1500
    finally:
        t.destroy()


# ---- refusals

def test_refusals(gpu):
    """slabs, open boundaries and Lees-Edwards in both orders, a pre-inlet, another model than RBC_HO, classes out of range:
    each returns its message and none aborts"""
    P = gpu.base_parameters()
    lib = gpu.capi.lib()
    made = []

    def lattice(*a, **k):
        made.append(gpu.Lattice(*a, **k))
        return made[-1]
    try:
        L = lattice(8, 8, 8, (False, True, True), 1.0, x0=0, nx_global=16, n_slabs=2)
        with pytest.raises(gpu.HcError, match="n_slabs = 1"):
            L.enableInteriorViscosity([0.5])
        L = lattice(8, 8, 8, (False, True, True), 1.0)
        L.addVelocityBoundary0N((0, 0, 0, 7, 0, 7))
        with pytest.raises(gpu.HcError, match="interior viscosity and open boundaries do not combine"):
            L.enableInteriorViscosity([0.5])
        L = lattice(8, 8, 8, (False, True, True), 1.0)
        L.enableInteriorViscosity([0.5])
        with pytest.raises(gpu.HcError, match="interior viscosity and open boundaries do not combine"):
            L.addVelocityBoundary0N((0, 0, 0, 7, 0, 7))
        with pytest.raises(gpu.HcError, match="exceeds the number of enabled classes"):
            L.setInteriorClasses(np.full((8, 8, 8), 2, np.uint8))
        for bad in ([], [0.5] * 8, [2.0], [0.0]):
            with pytest.raises(gpu.HcError):
                L.enableInteriorViscosity(bad)
        L.collideAndStream(1)   # still a working lattice
        L = lattice(8, 8, 8, (True, True, True), 1.0)
        L.setLeesEdwards(0.01, -0.01)
        with pytest.raises(gpu.HcError, match="interior viscosity and Lees-Edwards do not combine"):
            L.enableInteriorViscosity([0.5])
        L = lattice(8, 8, 8, (True, True, True), 1.0)
        L.enableInteriorViscosity([0.5])
        with pytest.raises(gpu.HcError, match="interior viscosity and Lees-Edwards do not combine"):
            L.setLeesEdwards(0.01, -0.01)
        with pytest.raises(gpu.HcError):
            lattice(4, 4, 4).interiorClasses()   # not enabled
        # a pre-inlet beside interior viscosity
        pre, dom = lattice(8, 8, 8, (True, False, False), 1.0), lattice(8, 8, 8, (False, False, False), 1.0)
        pre.enableInteriorViscosity([0.5])
        with pytest.raises(gpu.HcError, match="interior viscosity and a pre-inlet do not combine"):
            gpu.PreInlet(pre, dom, [(3, 3)], 2, 0, direction="Xneg", device=True)
        # ... and enabled after the handles exist: hc_preinlet_iterate refuses on its own and steps nothing
        pre, dom = lattice(12, 10, 10, (True, False, False), 1.0 / P.tau), lattice(16, 10, 10, (False, False, False), 1.0 / P.tau)
        wall = lambda d: np.pad(np.zeros((d[0], d[1] - 2, d[2] - 2), np.uint8), ((0, 0), (1, 1), (1, 1)), constant_values=1)
        pre.defineBounceBack(wall((12, 10, 10))); dom.defineBounceBack(wall((16, 10, 10)))
        pre.latticeEquilibrium(); dom.latticeEquilibrium()
        pc, dc = gpu.Cells(pre, P), gpu.Cells(dom, P)
        rbc = gpu.CellType.rbc(P)
        pc.addCellType(rbc, 1); dc.addCellType(rbc, 1)
        g = np.stack(np.nonzero(wall((12, 10, 10))[0] == 0), axis=1)
        coupling = gpu.PreInlet(pre, dom, g, 11, 0, direction="Xneg", device=True, cells=(pc, dc), window=(2.0, 10.0),
                                id_stride=1000)
        try:
            coupling.iterate(1)
            before = dom.populations()
            pre.enableInteriorViscosity([0.5])
            with pytest.raises(gpu.HcError, match="hc_preinlet_iterate: a lattice has interior viscosity enabled"):
                coupling.iterate(1)
            assert coupling.iter == 1 and np.array_equal(dom.populations(), before)
        finally:
            coupling.destroy()
        # a type is marked once
        L = lattice(24, 24, 24, (True, True, True), 1.0 / P.tau)
        cf = gpu.Cells(L, P)
        cf.addCellType(gpu.CellType.rbc(P, interior_viscosity=True, viscosity_ratio=5.0), 1)
        tau5 = 5.0 * (P.tau - 0.5) + 0.5
        gpu.check(lib.hcp_type_set_interior_viscosity(cf.ptr, 0, tau5))   # the same again: nothing changes
        assert lib.hcp_type_set_interior_viscosity(cf.ptr, 0, tau5 + 1.0) != 0
        assert b"marked already with another tau_int" in lib.hc_last_error()
        assert len(L.interiorViscosityOmegas()) == 1
        # models without a normal
        L = lattice(24, 24, 24, (True, True, True), 1.0 / P.tau)
        cf = gpu.Cells(L, P)
        plt = gpu.CellType.plt(P, interior_viscosity=True, viscosity_ratio=5.0)
        with pytest.raises(gpu.HcError, match="HC_MODEL_RBC_HO"):
            cf.addCellType(plt, 1)
        with pytest.raises(gpu.HcError, match="no cell type has interior viscosity"):
            cf.findInternalParticleGridPoints()
        with pytest.raises(gpu.HcError, match="no cell type has interior viscosity"):
            cf.internalGridPointsMembrane()
    finally:
        for L in made:
            L.destroy()
