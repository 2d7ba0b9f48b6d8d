"""Running statistics on the device (csrc/stats.hip, stats_fluid_kernel in csrc/lattice.hip; host.Statistics) against the
existing observers and the numpy restatement tests/flow_statistics_ref.py.

Every comparison is exact (array_equal on fp64 sums and on integer counts): a fluid sum is the same additions of the same
observer values in the same order, and the counts are integers.  The reference of a sampled run is the same system stepped in
calls that end where the samples fall, with rho_u() / pi_neq() / positions / alive() downloaded there."""
import numpy as np
import pytest

import flow_statistics_ref as FS
import open_boundary_axis_ref as AX

pytestmark = pytest.mark.gpu

ALL_FLUID = 1 | 2 | 4
ALL = ALL_FLUID | 8 | 16
T19 = np.array([1 / 3] + [1 / 18] * 3 + [1 / 36] * 6 + [1 / 18] * 3 + [1 / 36] * 6)


def _random_populations(seed, n, amp=0.02):
    return amp * np.random.default_rng(seed).standard_normal((n, 19)) * T19[None, :]


def _check_fluid(st, ref, what):
    assert st.samples == ref.samples
    for bit, want in ((1, ref.rho_u), (2, ref.uu), (4, ref.pi)):
        if what & bit:
            got = st.sums(bit)
            assert np.array_equal(got, want), (bit, np.abs(got - want).max())
    assert np.abs(ref.rho_u).max() > 0


# ---- 1: fluid only

DIMS1 = (12, 10, 8)


def _fluid_system(gpu):
    nx, ny, nz = DIMS1
    P = gpu.base_parameters()
    L = gpu.Lattice(nx, ny, nz, (True, False, True), 1.0 / 0.9)
    mask = np.zeros(DIMS1, np.uint8); mask[:, 0, :] = 1; mask[:, -1, :] = 1
    L.defineBounceBack(mask)
    L.set_populations(_random_populations(11, L.n))
    L.setExternalVector((1e-5, -2e-6, 3e-6))
    L.setExternalVectorBoxes([(2, 6, 1, 7, 0, 5)], [(-3e-5, 1e-6, 2e-6)])
    return L, gpu.HemoCell(L, P)


@pytest.mark.parametrize("what", [ALL_FLUID, 1, 2, 4])
@pytest.mark.parametrize("padded", [False, True])
def test_fluid_sums_equal_summed_observers(gpu, padded, what):
    """12 x 10 x 8, plates on the y faces, a body force and a force region, random populations, an empty container: every = 3
    over one call of 10 iterations against calls of 3, 3, 3, 1 with the observers summed on the host; all sets and each alone,
    with and without the padded plane stride"""
    lib = gpu.capi.lib()
    gpu.check(lib.hc_debug_force_plane_padding(1 if padded else 0))
    try:
        L, h = _fluid_system(gpu)
        st = gpu.Statistics(L, h.cellfields, what=what, every=3)
        Lr, hr = _fluid_system(gpu)
        try:
            h.iterate(10)
            ref = FS.FluidSums(Lr.n)
            for n in (3, 3, 3, 1):
                hr.iterate(n)
                if n == 3:
                    ref.add_lattice(Lr)
            _check_fluid(st, ref, what)
            assert st.samples == 3
            assert np.array_equal(L.populations(), Lr.populations())
            for bit in (1, 2, 4):   # only the selected sets exist
                if not what & bit:
                    with pytest.raises(gpu.HcError, match="not selected"):
                        st.sums(bit)
        finally:
            st.destroy()
            for x in (h, hr):
                x.cellfields.destroy()
            L.destroy(); Lr.destroy()
    finally:
        gpu.check(lib.hc_debug_force_plane_padding(0))


# ---- 2: with cells

PIPE = (48, 34, 34)


def _cell_system(gpu):
    """one RBC and one PLT in the pipe of the parity tests, velocity update every 2, material model every 4"""
    nx, ny, nz = PIPE
    P = gpu.base_parameters()
    mask, _ = gpu.pipe_mask(nx, ny, nz)
    L = gpu.Lattice(nx, ny, nz, (True, False, False), 1.0 / P.tau)
    L.defineBounceBack(mask); L.latticeEquilibrium(); L.setExternalVector((3e-5, 0.0, 0.0))
    h = gpu.HemoCell(L, P)
    types = [gpu.CellType.rbc(P), gpu.CellType.plt(P)]
    for t in types:
        h.cellfields.addCellType(t, 4)
    h.setParticleVelocityUpdateTimeScaleSeparation(2)
    assert h.cellfields.addCell(0, (10.0, 16.5, 16.5), (90, 0, 0))
    assert h.cellfields.addCell(1, (45.5, 20.0, 13.0), (10, 20, 30))   # across the periodic seam
    h.cellfields.applyConstitutiveModel(0, True)
    return L, h, types, mask


def _cell_reference(cf, types, mask, periodic, dens, ins):
    """adds the restatement's counts of the container's state now to dens / ins (per type)"""
    pos, alive = cf.positions, cf.alive()
    for t, ct in enumerate(types):
        first, n = cf.type_range(t)
        rows = slice(first, first + n * ct.nv)
        dens[t] += FS.cell_density(pos[rows], alive[rows], mask.shape, periodic)
        ins[t] += FS.inside(FS.cells_of(pos[rows], alive[rows], ct.tables()["triangles"], ct.nv), mask, periodic)


def _destroy(*things):
    for x in things:
        if x is not None:
            x.destroy()


def test_cells_sums_counts_and_no_perturbation(gpu):
    """every = 3 over ONE call of 12 iterations with the velocity update every 2: samples fall on velocity-update steps (after
    iterations 2 and 8), between them (5, which would have overlapped) and at the end of the call.  Fluid sums equal the
    observers summed over calls of 3; the counts equal the restatement on the positions downloaded there; and the stepped state
    equals a run without statistics bit for bit"""
    lib = gpu.capi.lib()
    gpu.check(lib.hc_set_reproducible_spread(1))
    made = []
    try:
        L, h, types, mask = _cell_system(gpu); made += [h.cellfields, L]
        st = gpu.Statistics(L, h.cellfields, what=ALL, every=3); made.insert(0, st)
        Lr, hr, types_r, _ = _cell_system(gpu); made += [hr.cellfields, Lr]
        Lp, hp, types_p, _ = _cell_system(gpu); made += [hp.cellfields, Lp]
        made += types + types_r + types_p
        periodic = (True, False, False)
        h.iterate(12)
        hp.iterate(12)
        ref = FS.FluidSums(Lr.n)
        dens = [np.zeros(PIPE, np.int64) for _ in types]; ins = [np.zeros(PIPE, np.int64) for _ in types]
        for _ in range(4):
            hr.iterate(3)
            ref.add_lattice(Lr)
            _cell_reference(hr.cellfields, types_r, mask, periodic, dens, ins)
        assert st.samples == 4
        _check_fluid(st, ref, ALL_FLUID)
        for t in range(2):
            got_d, got_i = st.counts(8, t).reshape(PIPE), st.counts(16, t).reshape(PIPE)
            assert dens[t].sum() == 4 * types[t].nv and ins[t].sum() > 0
            assert np.array_equal(got_d, dens[t]) and np.array_equal(got_i, ins[t]), t
            assert np.array_equal(st.cell_density(t), dens[t].reshape(-1) / 4.0)
            assert np.array_equal(st.hematocrit(t), ins[t].reshape(-1) / 4.0)
        assert ins[0].max() == 4 and (ins[0][mask != 0] == 0).all()
        # the means are the sums over the samples
        assert np.array_equal(st.mean_density(), ref.rho_u[:, 0] / 4.0) and np.array_equal(st.mean_velocity(), ref.rho_u[:, 1:] / 4.0)
        assert np.array_equal(st.mean_pi_neq(), ref.pi / 4.0)
        u = ref.rho_u[:, 1:] / 4.0
        cov = ref.uu / 4.0 - np.stack([u[:, a] * u[:, b] for a, b in FS.UU_PAIRS], axis=1)
        assert np.array_equal(st.velocity_covariance(), cov)
        # the observer perturbs nothing, not even through the overlap a sampled iteration gives up
        for other in (hr, hp):
            assert np.array_equal(L.populations(), other.lattice.populations())
            assert np.array_equal(h.cellfields.positions, other.cellfields.positions)
            assert np.array_equal(h.cellfields.forces, other.cellfields.forces)
    finally:
        _destroy(*made)
        gpu.check(lib.hc_set_reproducible_spread(0))


# ---- 3: the cell sets at their edges, explicit samples on placed cells

BOX3 = (16, 14, 12)
PER3 = (True, False, True)


def _place(gpu, cf, t, centre, cell_id):
    """a cell of type t (the last type that holds cells) with the centre of its bounding box at `centre`, wherever that is:
    no wall test"""
    c = np.array(centre, dtype=np.float64); a = np.zeros(3)
    gpu.check(gpu.capi.lib().hcp_add_cell_unchecked(cf.ptr, t, cell_id, gpu.dptr(c), gpu.dptr(a)))
    pos = cf.positions
    mine = pos[-cf.types[t].nv:]
    mine += c - 0.5 * (mine.min(axis=0) + mine.max(axis=0))
    cf.positions = pos


def _edge_system(gpu, wall_block=False):
    P = gpu.base_parameters()
    mask = np.zeros(BOX3, np.uint8); mask[:, 0, :] = 1; mask[:, -1, :] = 1
    if wall_block:
        mask[7:9, 6:8, 5:7] = 1
    L = gpu.Lattice(*BOX3, PER3, 1.0 / P.tau)
    L.defineBounceBack(mask); L.latticeEquilibrium()
    cf = gpu.Cells(L, P)
    types = [gpu.CellType.plt(P), gpu.CellType.rbc(P)]   # no RBC is ever placed: a type without cells
    for t in types:
        cf.addCellType(t, 1)
    return L, cf, types, mask


@pytest.mark.parametrize("case", ["periodic_face", "closed_face", "wall_nodes", "two_overlapping", "removed_vertices", "gone_cell"])
def test_cell_sets_at_their_edges(gpu, case):
    L, cf, types, mask = _edge_system(gpu, wall_block=case in ("wall_nodes", "gone_cell"))
    st = None
    try:
        if case == "periodic_face":      # across x = 0 and z = 0, both periodic
            _place(gpu, cf, 0, (0.3, 7.0, 0.2), 1)
        elif case == "closed_face":      # cut by the y = 0 face: vertices outside are dropped, the wall plane gets no inside count
            _place(gpu, cf, 0, (8.0, 0.3, 6.0), 1)
        elif case == "wall_nodes":       # around the wall block inside the box
            _place(gpu, cf, 0, (8.0, 7.0, 6.0), 1)
        elif case == "two_overlapping":
            _place(gpu, cf, 0, (8.0, 7.0, 6.0), 1); _place(gpu, cf, 0, (8.6, 7.3, 6.2), 2)
        elif case == "removed_vertices":  # what removeParticles leaves behind: an incomplete cell next to a complete one
            _place(gpu, cf, 0, (4.0, 7.0, 6.0), 1); _place(gpu, cf, 0, (11.0, 7.0, 6.0), 2)
            rec = cf.records()
            drop = (rec["cellId"] == 2) & (rec["vertexId"] % 5 == 0)
            cf.set_records(rec[~drop])
            assert cf.deletion_counts()[2:] == (1, int(drop.sum()))
        else:                             # gone_cell: the cell deletion mode takes the cell that sits on the wall block
            cf.setDeletionMode("cell")
            _place(gpu, cf, 0, (3.0, 7.0, 6.0), 1); _place(gpu, cf, 0, (8.0, 7.0, 6.0), 2)
            cf.advanceParticles(check_deletions=False)   # velocities are zero: nothing moves, the tag is set on the device
        st = gpu.Statistics(L, cf, what=8 | 16)
        st.sample(); st.sample()
        assert st.samples == 2
        got = [[st.counts(s, t).reshape(BOX3) for t in range(2)] for s in (8, 16)]
        pos, alive = cf.positions, cf.alive()            # settles: a gone cell is no longer listed
        dens = [np.zeros(BOX3, np.int64) for _ in types]; ins = [np.zeros(BOX3, np.int64) for _ in types]
        _cell_reference(cf, types, mask, PER3, dens, ins)
        for t in range(2):
            assert np.array_equal(got[0][t], 2 * dens[t]) and np.array_equal(got[1][t], 2 * ins[t]), t
        assert got[0][1].sum() == 0 and got[1][1].sum() == 0      # the type without cells
        assert (ins[0][mask != 0] == 0).all() and ins[0].sum() > 0
        nv = types[0].nv
        if case == "periodic_face":
            assert pos[:, 0].min() < -0.5 and pos[:, 2].min() < -0.5 and dens[0].sum() == nv
            assert dens[0][-1].sum() > 0 and dens[0][:, :, -1].sum() > 0
        elif case == "closed_face":
            assert pos[:, 1].min() < -0.5 and 0 < dens[0].sum() < nv and dens[0][:, 0, :].sum() > 0
        elif case == "wall_nodes":
            free = FS.inside(FS.cells_of(pos, alive, types[0].tables()["triangles"], nv), np.zeros_like(mask), PER3)
            assert (free[mask != 0] > 0).any()
        elif case == "two_overlapping":
            assert ins[0].max() == 2
        elif case == "removed_vertices":
            assert dens[0].sum() == alive.sum() < 2 * nv and ins[0][8:].sum() == 0 and ins[0][:8].sum() > 0
        else:
            assert cf.counts()[1] == 1 and dens[0].sum() == nv and ins[0][6:].sum() == 0
    finally:
        _destroy(st, cf, L, *types)


def test_cell_sets_on_a_wide_valence_stl_mesh(gpu):
    """the malaria fixture's STL mesh (vertices of valence other than six) in a periodic box, across a corner"""
    P = gpu.base_parameters()
    dims, per = (24, 22, 20), (True, True, True)
    L = gpu.Lattice(*dims, per, 1.0 / P.tau)
    L.latticeEquilibrium()
    cf = gpu.Cells(L, P)
    T = gpu.CellType.malaria(P)
    st = None
    try:
        cf.addCellType(T, 1)
        _place(gpu, cf, 0, (1.5, 20.5, 10.0), 3)
        st = gpu.Statistics(L, cf, what=8 | 16)
        st.sample()
        mask = np.zeros(dims, np.uint8)
        dens = [np.zeros(dims, np.int64)]; ins = [np.zeros(dims, np.int64)]
        _cell_reference(cf, [T], mask, per, dens, ins)
        assert dens[0].sum() == T.nv and ins[0].sum() > 0
        assert np.array_equal(st.counts(8, 0).reshape(dims), dens[0]) and np.array_equal(st.counts(16, 0).reshape(dims), ins[0])
    finally:
        _destroy(st, cf, L, T)


# ---- 4: the other kinds of lattice

def _sum_chunks(h, L, ref, chunks, sample_after):
    for n, s in zip(chunks, sample_after):
        h.iterate(n)
        if s:
            ref.add_lattice(L)


def _open_lattice(gpu):
    """walled x channel, Zou-He velocity inlet on x = 0, pressure outlet over the last two planes"""
    nx, ny, nz = 14, 9, 8
    L = gpu.Lattice(nx, ny, nz, (False, False, False), 1.0 / 0.9)
    L.defineBounceBack(AX.channel_mask((nx, ny, nz), 0))
    L.setExternalVector((2e-6, 3e-7, -1e-7))
    L.addVelocityBoundary0N((0, 0, 0, ny - 1, 0, nz - 1))
    y = 1 - ((np.arange(ny) - (ny - 1) / 2.0) / ((ny - 2) / 2.0)) ** 2
    z = 1 - ((np.arange(nz) - (nz - 1) / 2.0) / ((nz - 2) / 2.0)) ** 2
    prof = 0.02 * np.clip(y[:, None], 0, None) * np.clip(z[None, :], 0, None)
    u = np.zeros((ny * nz, 3)); u[:, 0] = prof.reshape(-1); u[:, 1] = 0.1 * prof.reshape(-1)
    L.setBoundaryVelocity((0, 0, 0, ny - 1, 0, nz - 1), u)
    L.addPressureBoundary0P((nx - 2, nx - 1, 0, ny - 1, 0, nz - 1))
    L.setBoundaryDensity((nx - 2, nx - 1, 0, ny - 1, 0, nz - 1), 1.0)
    L.set_populations(np.random.default_rng(4).uniform(-0.005, 0.005, size=(L.n, 19)))
    return L


def _lees_edwards_lattice(gpu):
    L = gpu.Lattice(13, 7, 9, (True, True, True), 1.0 / 1.82)
    L.set_populations(_random_populations(6, L.n, 0.01))
    L.setExternalVector((1e-6, -2e-7, 3e-7))
    L.setLeesEdwards(-0.004, 0.004)
    L.setLeesEdwardsDisplacement(0.0, 0.37)
    return L


@pytest.mark.parametrize("kind", ["open", "lees_edwards"])
def test_other_lattice_kinds(gpu, kind):
    """an open-boundary lattice (the completed moments on its Zou-He nodes) and a Lees-Edwards lattice: every = 2 over one call
    of 7 iterations against calls of 2, 2, 2, 1"""
    make = _open_lattice if kind == "open" else _lees_edwards_lattice
    P = gpu.base_parameters()
    L, Lr = make(gpu), make(gpu)
    h, hr = gpu.HemoCell(L, P), gpu.HemoCell(Lr, P)
    st = gpu.Statistics(L, what=ALL_FLUID, every=2)
    try:
        h.iterate(7)
        ref = FS.FluidSums(Lr.n)
        _sum_chunks(hr, Lr, ref, (2, 2, 2, 1), (1, 1, 1, 0))
        _check_fluid(st, ref, ALL_FLUID)
        assert np.array_equal(L.populations(), Lr.populations())
    finally:
        _destroy(st, h.cellfields, hr.cellfields, L, Lr)


class _Coupled:
    """a periodic pre-inlet and a domain with a pressure outlet, one platelet each, coupled on the device along +x"""
    PRE, DOM, WINDOW, SHIFT, U0 = (13, 11, 12), (16, 11, 12), (2.0, 11.5), (0.5, 0.0, 0.0), (0.04, 0.0, 0.0)

    def __init__(self, gpu):
        self.P = P = gpu.base_parameters()
        omega = 1.0 / P.tau
        self.parts = []
        self.dmask = AX.channel_mask(self.DOM, 0)
        self.pre = gpu.Lattice(*self.PRE, (True, False, False), omega); self.parts.append(self.pre)
        self.dom = gpu.Lattice(*self.DOM, (False, False, False), omega); self.parts.append(self.dom)
        self.pre.defineBounceBack(AX.channel_mask(self.PRE, 0)); self.pre.latticeEquilibrium(1.0, self.U0)
        self.dom.defineBounceBack(self.dmask); self.dom.latticeEquilibrium(1.0, self.U0)
        self.pre.setExternalVector((2e-5, 0.0, 0.0))
        self.type = gpu.CellType.plt(P); self.parts.append(self.type)
        self.pc, self.dc = gpu.Cells(self.pre, P), gpu.Cells(self.dom, P)
        self.parts[:0] = [self.pc, self.dc]
        self.pc.addCellType(self.type, 1); self.dc.addCellType(self.type, 1)
        g = np.stack(np.nonzero(self.dmask[0] == 0), axis=1)
        self.coupling = gpu.PreInlet(self.pre, self.dom, g, self.PRE[0] - 1, 0, direction="Xneg", device=True, cells=(self.pc, self.dc),
                                     window=self.WINDOW, shift=self.SHIFT, id_stride=1000, cells_every=1)
        self.parts.insert(0, self.coupling)
        self.dom.setOpenBoundaryVelocitySlots(self.coupling.first, np.tile(np.asarray(self.U0), (len(g), 1)))
        self.dom._add_open_box(1, 1, [self.DOM[0] - 1, self.DOM[0] - 1, 0, self.DOM[1] - 1, 0, self.DOM[2] - 1], 0)
        assert self.pc.addCell(0, (5.0, 5.0, 5.5), (10.0, 20.0, 30.0), cell_id=40)
        pos = self.pc.positions
        pos[:, 0] -= pos[:, 0].min() - (self.WINDOW[0] - 0.2)   # enters the window after a few iterations
        self.pc.positions = pos
        assert self.dc.addCell(0, (11.0, 5.0, 5.5), (10.0, 20.0, 30.0), cell_id=1)
        self.pc.applyConstitutiveModel(0, True); self.dc.applyConstitutiveModel(0, True)

    def destroy(self):
        _destroy(*self.parts)


def test_preinlet_iterate_samples_the_domain(gpu):
    """hc_preinlet_iterate with the handle on the domain: every = 3 over one call of 12 coupled iterations against calls of 3.
    The sample falls after the hand-over and the cell check of its iteration, so the inlet nodes report the velocities just
    handed over and an injected cell counts from the check that brought it"""
    lib = gpu.capi.lib()
    gpu.check(lib.hc_set_reproducible_spread(1))
    a = b = st = None
    try:
        a, b = _Coupled(gpu), _Coupled(gpu)
        st = gpu.Statistics(a.dom, a.dc, what=ALL, every=3)
        a.coupling.iterate(12)
        ref = FS.FluidSums(b.dom.n)
        dens = [np.zeros(_Coupled.DOM, np.int64)]; ins = [np.zeros(_Coupled.DOM, np.int64)]
        for _ in range(4):
            b.coupling.iterate(3)
            ref.add_lattice(b.dom)
            _cell_reference(b.dc, [b.type], b.dmask, (False, False, False), dens, ins)
        _check_fluid(st, ref, ALL_FLUID)
        assert np.array_equal(st.counts(8, 0).reshape(_Coupled.DOM), dens[0])
        assert np.array_equal(st.counts(16, 0).reshape(_Coupled.DOM), ins[0])
        assert dens[0].sum() >= 4 * a.type.nv and ins[0].sum() > 0
        assert np.array_equal(a.dom.populations(), b.dom.populations()) and np.array_equal(a.dc.positions, b.dc.positions)
    finally:
        _destroy(st, a, b)
        gpu.check(lib.hc_set_reproducible_spread(0))


# ---- 5: the handle

def test_handle_behaviour_and_refusals(gpu):
    L, h = _fluid_system(gpu)
    Lr, hr = _fluid_system(gpu)
    P = gpu.base_parameters()
    made = [h.cellfields, hr.cellfields, L, Lr]
    try:
        st = gpu.Statistics(L, what=ALL_FLUID); made.insert(0, st)   # every = 0: explicit samples only
        h.iterate(4); hr.iterate(4)
        assert st.samples == 0 and not st.sums(1).any()
        with pytest.raises(gpu.HcError, match="no samples"):
            st.mean_velocity()
        ref = FS.FluidSums(L.n)
        st.sample(); ref.add_lattice(Lr)
        _check_fluid(st, ref, ALL_FLUID)
        st.setEvery(2)
        h.iterate(6)                                      # a download while the call's work is still queued
        first = st.sums(1)
        for _ in range(3):
            hr.iterate(2); ref.add_lattice(Lr)
        assert st.samples == 4 and np.array_equal(first, ref.rho_u)
        _check_fluid(st, ref, ALL_FLUID)
        st.reset()
        assert st.samples == 0 and not st.sums(1).any() and not st.sums(2).any() and not st.sums(4).any()
        st.setEvery(0)
        h.iterate(3)
        assert st.samples == 0
        # refusals, each with its message
        with pytest.raises(gpu.HcError, match="has an hc_stats already"):
            gpu.Statistics(L, what=1)
        with pytest.raises(gpu.HcError, match="cadence must be >= 0"):
            st.setEvery(-1)
        with pytest.raises(gpu.HcError, match="not selected"):
            st.counts(8, 0)
        with pytest.raises(gpu.HcError, match="must be one of"):
            st.sums(3)
        with pytest.raises(gpu.HcError, match="hc_stats refers to the lattice"):
            L.destroy()
        with pytest.raises(gpu.HcError, match="different lattice"):
            gpu.Statistics(Lr, h.cellfields, what=8)
        for what in (0, 32, 1 | 64):
            with pytest.raises(gpu.HcError, match="non-empty mask"):
                gpu.Statistics(Lr, what=what)
        with pytest.raises(gpu.HcError, match="need a cell container"):
            gpu.Statistics(Lr, what=1 | 8)
        slab = gpu.Lattice(8, 8, 8, (True, False, False), 1.0, x0=0, nx_global=16, n_slabs=2); made.append(slab)
        with pytest.raises(gpu.HcError, match="n_slabs = 1"):
            gpu.Statistics(slab, what=1)
        T = gpu.CellType.plt(P); made.append(T)
        cf = gpu.Cells(Lr, P); made.insert(0, cf)
        cf.addCellType(T, 1)
        sc = gpu.Statistics(Lr, cf, what=8 | 16); made.insert(0, sc)
        for t in (-1, 1):
            with pytest.raises(gpu.HcError, match="type index out of range"):
                sc.counts(8, t)
        with pytest.raises(gpu.HcError, match="not selected"):
            sc.sums(1)
        with pytest.raises(gpu.HcError, match="hc_stats refers to the container"):
            cf.destroy()
        sc.sample()
        assert sc.samples == 1 and sc.counts(8, 0).sum() == 0
        cf.addCellType(T, 1)
        with pytest.raises(gpu.HcError, match="added to the container after"):
            sc.sample()
    finally:
        _destroy(*made)
