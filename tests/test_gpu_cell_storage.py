"""The storage paths of the cell container (csrc/cells.hip and the scratch blocks of ibm.hip, mechanics.hip, exchange.hip):
regrowth of the device regions, compaction after a deletion, hole filling on the device, the staged slot lists, the information and extents scratch, and create / destroy.  Other
suites reach them only through slab or pre-inlet runs.  32 x 32 x 32 all-fluid periodic lattice, the RBC and PLT types of
host.CellType; every comparison is bit for bit."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 32
PER = (True, True, True)
RBC, PLT = 0, 1
FIELDS = ("position", "v", "force", "force_repulsion", "cellId", "vertexId", "restime", "celltype")
# two RBCs whose membranes are ~0.7 lu apart and a platelet at the first one's rim (the placement of
# test_gpu_parity.py::test_repulsion_vs_oracle), a second platelet away from all of them
RBCS = [((14.0, 16.5, 15.2), (90, 0, 0)), ((15.0, 16.5, 18.4), (90, 0, 0))]
PLTS = [((21.5, 16.5, 14.0), (0, 0, 0)), ((27.0, 27.0, 27.0), (0, 0, 0))]
K_REP, CUTOFF_UM = 2e-6, 0.7


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype.kind == "f" else a


def _same(a, b):
    """equal bit for bit (floats compared as bits, so -0.0 and NaN count); record arrays field by field"""
    if a.dtype.names:
        return len(a) == len(b) and all(np.array_equal(_bits(a[f]), _bits(b[f])) for f in FIELDS)
    return np.array_equal(_bits(a), _bits(b))


class _Box:
    """lattice, the two cell types and one container; destroy() in the order a driver uses"""

    def __init__(self, gpu, facade=False, u=(0.0, 0.0, 0.0), periodic=PER, mask=None):
        self.P = gpu.base_parameters()
        self.L = gpu.Lattice(N, N, N, periodic, 1.0 / self.P.tau)
        if mask is not None:
            self.L.defineBounceBack(mask)
        self.L.latticeEquilibrium(1.0, u)
        self.types = [gpu.CellType.rbc(self.P), gpu.CellType.plt(self.P)]
        self.h = gpu.HemoCell(self.L, self.P) if facade else None
        self.cells = self.h.cellfields if facade else gpu.Cells(self.L, self.P)
        for t in self.types:
            self.cells.addCellType(t, 1)

    def destroy(self):
        self.cells.destroy()
        for t in self.types:
            t.destroy()
        self.L.destroy()


@pytest.fixture
def box(gpu):
    made = []

    def make(facade=False, **kw):
        made.append(_Box(gpu, facade, **kw))
        return made[-1]
    yield make
    for b in made:
        b.destroy()


def _grid(n, spacing=6.0, first=3.0):
    """n platelet centres on a regular grid of the periodic box"""
    k = int(round(N / spacing))
    pts = [(first + spacing * a, first + spacing * b, first + spacing * c) for c in range(k) for b in range(k) for a in range(k)]
    assert len(pts) >= n
    return pts[:n]


def _free_grid(cells, n):
    """n grid points with no vertex within 4.2 lu (Chebyshev; a platelet's radius of 2.5 lu plus the repulsion cut-off of
    1.4 lu is 3.9) in the periodic box"""
    pos = cells.positions
    out = []
    for c in _grid(216, spacing=N / 6.0, first=N / 12.0):
        d = np.abs(pos - np.array(c))
        d = np.minimum(d, N - d)
        if not (d.max(axis=1) < 4.2).any():
            out.append(c)
    assert len(out) >= n, len(out)
    return out[:n]


def test_region_growth_carries_every_state(gpu, box):
    """70 platelets join 2 RBCs and 2 platelets: more than the region's 2 + 2 / 4 + 64 slots, so every device array is
    reallocated through the host staging.  Positions, velocities, forces, force_repulsion, the incomplete cell's tag and its
    dead particle all come back as they were."""
    b = box(facade=True)
    cells, h = b.cells, b.h
    for c, a in RBCS:
        assert cells.addCell(RBC, c, a)
    for c, a in PLTS:
        assert cells.addCell(PLT, c, a)
    cells.setRepulsion(K_REP, CUTOFF_UM, 1)
    cells.enableBoundaryParticles(K_REP, CUTOFF_UM, 1)
    h.iterate(3)
    assert np.abs(cells.repulsion_forces).max() > 0.0
    rec = cells.records()
    victim = cells.cell_ids()[-1]   # the second platelet
    keep = ~((rec["celltype"] == PLT) & (rec["cellId"] == victim) & (rec["vertexId"] == 5))
    assert keep.sum() == len(rec) - 1
    cells.set_records(rec[keep])

    rec0, rep0, alive0, del0 = cells.records(), cells.repulsion_forces, cells.alive(), cells.deletion_counts()
    n0 = len(alive0)
    assert n0 == len(rec) and len(rec0) == n0 - 1
    assert del0[2:] == (1, 1) and (~alive0).sum() == 1
    assert np.abs(rep0).max() > 0.0 and np.abs(rec0["force"]).max() > 0.0 and np.abs(rec0["v"]).max() > 0.0

    for c in _free_grid(cells, 70):
        assert cells.addCell(PLT, c)
    rec1, rep1, alive1, del1 = cells.records(), cells.repulsion_forces, cells.alive(), cells.deletion_counts()
    nv = b.types[PLT].nv
    assert len(alive1) == n0 + 70 * nv and len(rec1) == len(rec0) + 70 * nv
    assert _same(rec1[:len(rec0)], rec0)
    assert _same(rep1[:n0], rep0)
    assert np.array_equal(alive1[:n0], alive0)
    assert del1 == del0                                   # still one incomplete cell with one dead particle
    new = rec1[len(rec0):]
    assert alive1[n0:].all()
    assert np.array_equal(new["vertexId"].reshape(70, nv), np.tile(np.arange(nv), (70, 1)))   # complete
    assert (new["celltype"] == PLT).all() and len(np.unique(new["cellId"])) == 70
    for f in ("v", "force", "force_repulsion"):
        assert _same(new[f], np.zeros((70 * nv, 3)))
    assert _same(rep1[n0:], np.zeros((70 * nv, 3)))
    h.iterate(2)
    assert np.isfinite(cells.positions).all()


def _five_cells(b):
    """One RBC and four platelets (P0..P3, at z = 12: lowest vertex at z = 9.5) whose records carry seeded force and
    force_repulsion; v is zero except (0, 0, -8) on P1, and vertex 5 of P3 is left out, so P3 is incomplete.  Returns the five
    cell ids, RBC first."""
    cells = b.cells
    assert cells.addCell(RBC, (16.0, 16.0, 18.0))
    for x, y, _ in _grid(4):
        assert cells.addCell(PLT, (x, y, 12.0))
    cells.setRepulsion(K_REP, CUTOFF_UM, 1)   # the repulsion arrays exist from here on
    ids = cells.cell_ids()
    rec = cells.records()
    assert rec["position"][rec["celltype"] == PLT][:, 2].min() > 9.0   # clear of a wall at z <= 5; P1's step of -8 puts it there
    rng = np.random.default_rng(23)
    rec["force"] = 1e-3 * rng.standard_normal((len(rec), 3))
    rec["force_repulsion"] = 1e-3 * rng.standard_normal((len(rec), 3))
    rec["v"] = 0.0
    plt = rec["celltype"] == PLT
    rec["v"][plt & (rec["cellId"] == ids[2])] = (0.0, 0.0, -8.0)
    cells.set_records(rec[~(plt & (rec["cellId"] == ids[4]) & (rec["vertexId"] == 5))])
    assert np.array_equal(cells.cell_ids(), ids)
    assert cells.deletion_counts() == (0, 0, 1, 1)
    return ids


def test_compaction_carries_every_state(gpu, box):
    """P1 moves into the wall below it in one advance and, in deletion mode "cell", is gone at once; the compaction that
    follows closes the gap: every record field, the repulsion forces, the incomplete tag of P3 and its dead particle move one
    slot down together, and the cells in front stay where they were.  The other cells have v = 0, and p + 0.0 keeps p's bits."""
    mask = np.zeros((N, N, N), np.uint8)
    mask[:, :, :6] = 1
    mask[:, :, N - 1] = 1
    b = box(periodic=(True, True, False), mask=mask)
    cells = b.cells
    ids = _five_cells(b)
    nr, nv = b.types[RBC].nv, b.types[PLT].nv
    rec0, rep0, alive0 = cells.records(), cells.repulsion_forces, cells.alive()
    assert np.abs(rep0).max() > 0.0 and (~alive0).sum() == 1 and not alive0[nr + 3 * nv + 5]

    cells.setDeletionMode("cell")
    cells.advanceParticles(True)

    stay = ~((rec0["celltype"] == PLT) & (rec0["cellId"] == ids[2]))
    assert stay.sum() == len(rec0) - nv
    assert _same(cells.records(), rec0[stay])
    assert np.array_equal(cells.cell_ids(), ids[[0, 1, 3, 4]])
    alive1 = cells.alive()
    assert len(alive1) == nr + 3 * nv and np.array_equal(np.flatnonzero(~alive1), [nr + 2 * nv + 5])
    assert cells.deletion_counts() == (1, 0, 1, 1)
    stay_v = np.ones(len(alive0), bool)
    stay_v[nr + nv:nr + 2 * nv] = False
    assert _same(cells.repulsion_forces, rep0[stay_v])


def test_remove_cells_fills_holes_from_the_tail(gpu, box):
    """hcp_remove_cells takes P1 out on the device: the last cell, P3, moves into its slot with its whole state, only the
    host's id list follows.  A platelet added afterwards arrives with zero v, force and force_repulsion."""
    b = box()
    cells = b.cells
    ids = _five_cells(b)
    nr, nv = b.types[RBC].nv, b.types[PLT].nv
    rec0 = cells.records()
    slots = np.array([1], dtype=np.int32)
    gpu.check(gpu.capi.lib().hcp_remove_cells(cells.ptr, PLT, slots.ctypes.data_as(C.POINTER(C.c_int)), len(slots)))
    assert np.array_equal(cells.cell_ids(), ids[[0, 1, 4, 3]])
    rec1 = cells.records()
    assert len(rec1) == len(rec0) - nv
    assert _same(rec1[rec1["celltype"] == RBC], rec0[rec0["celltype"] == RBC])
    for cid in ids[[1, 4, 3]]:
        now, then = rec1[(rec1["celltype"] == PLT) & (rec1["cellId"] == cid)], rec0[(rec0["celltype"] == PLT) & (rec0["cellId"] == cid)]
        assert len(then) == (nv - 1 if cid == ids[4] else nv) and _same(now, then)
    assert rec1["cellId"][nr] == ids[1] and rec1["cellId"][nr + nv] == ids[4]   # P0, then P3 in the slot P1 left
    assert np.array_equal(np.flatnonzero(~cells.alive()), [nr + nv + 5])        # with its dead particle

    assert cells.addCell(PLT, (27.0, 3.0, 12.0))
    rec2 = cells.records()
    assert _same(rec2[:len(rec1)], rec1)
    new = rec2[len(rec1):]
    assert len(new) == nv and (new["celltype"] == PLT).all() and np.array_equal(new["vertexId"], np.arange(nv))
    for f in ("v", "force", "force_repulsion"):
        assert _same(new[f], np.zeros((nv, 3)))


def test_slot_list_outgrows_its_staging_block(gpu, box):
    """hcp_interpolate_cells with lists of 1, 600 and 5 slots: the first staging block holds 2 * 1 + 256 ints, the second
    list outgrows it and the third reuses the larger block."""
    b = box()
    cells, L = b.cells, b.L
    rng = np.random.default_rng(5)
    L.set_populations(L.populations() + 1e-3 * rng.standard_normal((L.n, 19)))   # a velocity that differs from node to node
    for c in _grid(6):
        assert cells.addCell(PLT, c)
    nv = b.types[PLT].nv
    cells.interpolateFluidVelocity()
    ref = cells.velocities
    assert len(np.unique(ref[:, 0])) > 6
    sentinel = 7.0 + np.arange(ref.size, dtype=np.float64).reshape(ref.shape)
    lib = gpu.capi.lib()
    for slots in ([4], list(rng.permutation(np.tile(np.arange(6), 100))), [5, 0, 3, 1, 4]):
        cells.velocities = sentinel
        s = np.ascontiguousarray(slots, dtype=np.int32)
        gpu.check(lib.hcp_interpolate_cells(cells.ptr, PLT, s.ctypes.data_as(C.POINTER(C.c_int)), len(s)))
        v = cells.velocities
        listed = np.zeros(6, bool)
        listed[s] = True
        rows = np.repeat(listed, nv)
        assert _same(v[rows], ref[rows])
        assert _same(v[~rows], sentinel[~rows])


def _deformed(b, n_plt):
    """1 RBC and n_plt platelets, every vertex moved a little (the same way in every container built so)"""
    cells = b.cells
    assert cells.addCell(RBC, (16.0, 16.0, 16.0), (10.0, 20.0, 30.0))
    for c in _grid(n_plt):
        assert cells.addCell(PLT, c)
    pos = cells.positions
    cells.positions = pos + 0.05 * np.random.default_rng(11).standard_normal(pos.shape)
    return cells


def test_information_scratch_grows_and_is_reused(gpu, box):
    """cell_info and force_components share one scratch block that grows with the request; the results do not depend on
    the order of the requests, that is on which of them grew the block"""
    a, b = _deformed(box(), 80), _deformed(box(), 80)
    ra = [a.cell_info(PLT), a.cell_info(RBC), a.cell_info(PLT), a.force_components(RBC), a.force_components(PLT)]
    rb = [b.force_components(PLT), b.force_components(RBC), b.cell_info(PLT), b.cell_info(RBC), b.cell_info(PLT)][::-1]
    for x, y in zip(ra, rb):
        if isinstance(x, dict):
            assert sorted(x) == sorted(y) and all(_same(x[k], y[k]) for k in x)
        else:
            assert np.abs(x).max() > 0.0 and _same(x, y)
    assert all(_same(ra[0][k], ra[2][k]) for k in ra[0])


def test_extents_block_grows(gpu, box):
    """hcp_cell_extents with 1 platelet, then with 81: past the block's 1 + 1 / 4 + 64 = 65 cells"""
    b = box()
    cells = b.cells
    nv = b.types[PLT].nv
    lib = gpu.capi.lib()
    pts = _grid(81)
    for first, last in ((0, 1), (1, 81)):
        for c in pts[first:last]:
            assert cells.addCell(PLT, c, (10.0, 20.0, 30.0))
        ext = np.full((last, 3), np.nan)
        gpu.check(lib.hcp_cell_extents(cells.ptr, PLT, gpu.dptr(ext)))
        x = cells.positions[:, 0].reshape(last, nv)
        assert _same(ext[:, 0], x.min(axis=1)) and _same(ext[:, 1], x.max(axis=1))
        assert np.array_equal(ext[:, 2], np.full(last, float(nv)))


def _round(gpu, prepare=None):
    b = _Box(gpu, facade=True, u=(0.02, 0.01, -0.01))   # the cells move with the fluid and deform against each other's wake
    try:
        for c, a in RBCS:
            assert b.cells.addCell(RBC, c, a)
        for c, a in PLTS:
            assert b.cells.addCell(PLT, c, a)
        if prepare:
            prepare(b.cells)
        b.h.iterate(4)
        return b.cells.positions
    finally:
        b.destroy()   # cells, cell types, lattice


def test_create_and_destroy_are_repeatable(gpu):
    """Three rounds of build, iterate(4), download, destroy give the same positions bit for bit; a fourth, with both
    repulsions on, is destroyed while the sort buffers of the spread and of the repulsion exist.  All four run the
    reproducible spread: the default spread sums a node's force with atomic adds in whatever order the threads arrive
    (csrc/ibm.hip), so only the reproducible one can repeat a run bit for bit."""
    def prepare(cells):
        cells.setRepulsion(K_REP, CUTOFF_UM, 1)
        cells.enableBoundaryParticles(K_REP, CUTOFF_UM, 1)
    lib = gpu.capi.lib()
    gpu.check(lib.hc_set_reproducible_spread(1))
    try:
        first = _round(gpu)
        assert np.isfinite(first).all()
        for _ in range(2):
            assert _same(_round(gpu), first)
        with_rep = _round(gpu, prepare)
        assert np.isfinite(with_rep).all() and not _same(with_rep, first)
    finally:
        gpu.check(lib.hc_set_reproducible_spread(0))
