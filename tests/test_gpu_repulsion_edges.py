"""Vertex-vertex repulsion, wall-node repulsion and wall tagging on the device at every periodic and open edge.

csrc/repulsion.hip (rep_keys_kernel, rep_force_kernel, boundary_rep_kernel) and csrc/cells.hip (advance_kernel) each
bin a vertex at its nearest node and wrap that node per axis.  Here they meet all eight periodicity triples of a
12 x 10 x 11 lattice, vertices outside the open faces, cells stored on other laps, ties of floor(x + 0.5), a pair exactly
one cut-off apart, removed particles, a gone cell before its compaction, an empty first type, regions with slack and
the regrowth of the sort buffers -- against the CPU oracle and against tests/repulsion_ref.py, on the inputs that
tests/test_repulsion_edges_cpu.py shows to be sufficient.  The bound is that of repulsion_ref.bound(): the terms are the
same doubles everywhere, so only the order of the sum differs."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from tests import repulsion_ref as R
from tests.test_repulsion_edges_cpu import CASES, IDS, K_REP, K_WALL, OracleCase, built, ratio, wrong_by

pytestmark = pytest.mark.gpu
RBC, PLT = 0, 1


class GpuCase:
    """a device lattice and container that hold the cells of a built case at the case's positions"""

    def __init__(self, gpu, case, dims, periodic, mask=None, mode="particle"):
        self.gpu, self.lib = gpu, gpu.capi.lib()
        self.P = gpu.base_parameters()
        self.L = gpu.Lattice(dims[0], dims[1], dims[2], periodic, 1.0 / self.P.tau)
        self.L.latticeEquilibrium()
        self.types = [gpu.CellType.rbc(self.P), gpu.CellType.plt(self.P)]
        self.cf = gpu.Cells(self.L, self.P)
        for T in self.types:
            self.cf.addCellType(T, 1)
        for nv in case["sizes"]:                     # placed before the mask is set: nothing is refused
            assert self.cf.addCell({R.NV_RBC: RBC, R.NV_PLT: PLT}[nv], (5.0, 5.0, 5.0))
        if mask is not None:
            self.L.defineBounceBack(mask)
        self.cf.setDeletionMode(mode)
        self.cf.positions = case["pos"]

    def set_repulsion(self, k=K_REP):                # the cut-off in lattice units, exactly
        self.gpu.check(self.lib.hcp_set_repulsion(self.cf.ptr, k, R.CUTOFF, 1))

    def set_boundary_repulsion(self, k=K_WALL):
        self.gpu.check(self.lib.hcp_set_boundary_repulsion(self.cf.ptr, k, R.CUTOFF, 1))

    def advance(self, vel=None, settle=True):
        self.cf.velocities = np.zeros((self.cf.counts()[0], 3)) if vel is None else vel
        self.cf.advanceParticles(settle)

    def destroy(self):
        self.cf.destroy()
        for T in self.types:
            T.destroy()
        self.L.destroy()


def _compare(r_g, ref, r_o=None, what=""):
    """device against the restatement (and the oracle) within the bound; -> the largest ratio to it"""
    q = ratio(r_g, ref)
    print("%s device / bound %.3f" % (what, q))
    assert q <= 1.0
    if r_o is not None:
        assert (np.abs(r_g - r_o) <= R.bound(ref)).all()
    return q


@pytest.mark.parametrize("periodic,dims", CASES, ids=IDS)
def test_periodicity_sweep(orc, gpu, periodic, dims):
    """particle mode: the advance removes what tagged() says, then hcp_repulsion against oracle and restatement"""
    b = built(periodic, dims)
    case, ref, alive = b["case"], b["ref"], b["alive"]
    R.check_conditions(b["cond"], periodic)
    oc, gc = OracleCase(orc, case, dims, periodic, b["mask"]), GpuCase(gpu, case, dims, periodic, b["mask"])
    try:
        oc.advance(); gc.advance()
        assert np.array_equal(gc.cf.alive(), alive) and np.array_equal(oc.alive(), alive)
        gc.set_repulsion()
        orc.orc_sim_repulsion(oc.S, K_REP, R.CUTOFF); gc.cf.applyRepulsionForce()
        r_o, r_g = oc.get(3), gc.cf.repulsion_forces
    finally:
        oc.destroy(); gc.destroy()
    _compare(r_g, ref, r_o, "sweep %s" % (periodic,))
    assert np.abs(r_g.sum(0)).max() <= 4 * ref["k"].sum() * R.U * ref["abs"].sum(0).max()   # action = reaction
    outside = ~R.in_grid(R.nearest_node(case["pos"]), dims, periodic)
    assert (~alive).sum() >= 20 and (all(periodic) or outside.sum() >= 20)
    assert not r_g[~alive].any() and not r_g[outside].any()
    for w, res in b["wrong"].items():
        if not np.array_equal(res["sum"], ref["sum"]):
            assert wrong_by(r_g, res) >= 100.0, w


def test_ties_and_cutoff(gpu):
    """vertices on half-integer coordinates are binned, pushed and tagged as floor(x + 0.5) says; the pair exactly one
    cut-off apart reads 0 and its twin, one ulp closer, holds its single term bit for bit"""
    periodic, dims = (1, 0, 1), R.DIMS
    b = built(periodic, dims)
    case, ref, pos = b["case"], b["ref"], b["case"]["pos"]
    tie = (np.mod(pos, 1.0) == 0.5).any(axis=1)
    assert tie.sum() >= 40 and (ref["k"][tie] > 0).sum() >= 10 and (~b["alive"][tie]).sum() >= 1
    on_face = tie & ((pos[:, 1] == -0.5) | (pos[:, 1] == dims[1] - 0.5))
    assert on_face.sum() >= 2
    gc = GpuCase(gpu, case, dims, periodic, b["mask"])
    try:
        gc.advance()
        assert np.array_equal(gc.cf.alive()[tie], b["alive"][tie])
        gc.set_repulsion(); gc.cf.applyRepulsionForce()
        r_g = gc.cf.repulsion_forces
    finally:
        gc.destroy()
    sub = dict(sum=ref["sum"][tie], abs=ref["abs"][tie], k=ref["k"][tie])
    _compare(r_g[tie], sub, None, "ties")
    for i in case["cut"]:
        assert ref["k"][i] == 0 and not r_g[i].any()
    for i in case["twin"]:
        assert ref["k"][i] == 1 and r_g[i, 2] != 0.0 and np.array_equal(r_g[i], ref["sum"][i])


@pytest.mark.parametrize("mode", ["particle", "cell"])
def test_gone_and_incomplete_cells(orc, gpu, mode):
    """One advance puts the low vertices of cell 0 on the wall.  Particle mode: the removed vertices neither push nor
    are pushed and the survivors still do.  Cell mode: the whole cell is silent while it still sits in storage (the
    repulsions run before anything asks for the compaction), so the neighbours read what the oracle computes with the
    cell deleted.  Both repulsions."""
    g = R.build_gone_case()
    periodic, dims = (1, 1, 0), R.DIMS
    end = g["pos"] + g["vel"]
    lost = R.tagged(end, g["mask"], periodic)
    assert 10 <= lost.sum() < R.NV_PLT and not lost[R.NV_PLT:].any()
    alive = ~lost if mode == "particle" else g["cell_of"] != 0
    keep = np.ones(len(end), dtype=bool) if mode == "particle" else g["cell_of"] != 0
    ref = R.repulsion(end, g["cell_of"], alive, dims, periodic, K_REP, R.CUTOFF)
    push = R.repulsion(end, g["cell_of"], alive, dims, periodic, K_REP, R.CUTOFF, wrong="dead_push")
    assert (ref["k"][R.NV_PLT:2 * R.NV_PLT] > 0).sum() >= 10 and (ref["k"][:R.NV_PLT] > 0).sum() >= (10 if mode == "particle" else 0)
    oc, gc = OracleCase(orc, g, dims, periodic, g["mask"], mode), GpuCase(gpu, g, dims, periodic, g["mask"], mode)
    try:
        gc.set_repulsion(); gc.set_boundary_repulsion()
        oc.advance(g["vel"]); gc.advance(g["vel"], settle=False)          # nothing compacts yet
        orc.orc_sim_repulsion(oc.S, K_REP, R.CUTOFF); gc.cf.applyRepulsionForce()
        r_o, r_g = oc.get(3), gc.cf.repulsion_forces                      # the download settles: the gone cell leaves here
        assert gc.cf.counts()[0] == keep.sum() == oc.S.contents.np
        assert np.array_equal(gc.cf.positions, end[keep]) and np.array_equal(gc.cf.alive(), alive[keep])
        sub = dict(sum=ref["sum"][keep], abs=ref["abs"][keep], k=ref["k"][keep])
        _compare(r_g, sub, r_o, "gone, %s mode" % mode)
        assert not r_g[~alive[keep]].any()
        assert wrong_by(r_g, dict(sum=push["sum"][keep], abs=push["abs"][keep], k=push["k"][keep])) >= 100.0
    finally:
        oc.destroy(); gc.destroy()
    # wall-node repulsion in the same state, on a fresh pair so that in cell mode it too runs before the compaction;
    # force_repulsion starts from zero on both sides, so all three agree bit for bit
    rb, _ = R.boundary_repulsion(end, alive, g["mask"], periodic, K_WALL, R.CUTOFF, np.zeros(end.shape))
    oc, gc = OracleCase(orc, g, dims, periodic, g["mask"], mode), GpuCase(gpu, g, dims, periodic, g["mask"], mode)
    try:
        gc.set_boundary_repulsion()
        oc.advance(g["vel"]); gc.advance(g["vel"], settle=False)
        orc.orc_sim_boundary_repulsion(oc.S, K_WALL, R.CUTOFF); gc.cf.applyBoundaryRepulsionForce()
        b_o, b_g = oc.get(3), gc.cf.repulsion_forces
    finally:
        oc.destroy(); gc.destroy()
    assert np.array_equal(b_g, rb[keep]) and np.array_equal(b_g, b_o)
    assert (np.abs(b_g).sum(1) > 0).sum() >= 10 and not b_g[~alive[keep]].any()


def test_type_bookkeeping(gpu):
    """Keys are packed densely over the types while the sorted values are region indices.  First an empty RBC type
    before the platelets (their region starts 64 cells in); then 66 RBCs, past the region's first 1 + 64 cells, so that
    the platelet region starts well behind the packed count."""
    periodic, dims = (1, 0, 1), R.DIMS
    g = R.build_gone_case()
    end = g["pos"] + g["vel"]
    alive = np.ones(len(end), dtype=bool)
    ref = R.repulsion(end, g["cell_of"], alive, dims, periodic, K_REP, R.CUTOFF)
    assert len(ref["pairs"]) >= 50
    gc = GpuCase(gpu, dict(sizes=g["sizes"], pos=end), dims, periodic)
    try:
        gc.set_repulsion(); gc.cf.applyRepulsionForce()
        _compare(gc.cf.repulsion_forces, ref, None, "empty first type")
    finally:
        gc.destroy()

    b = built(periodic, dims)
    case = b["case"]
    alive = np.ones(len(case["pos"]), dtype=bool)
    n_parked = 65
    parked = np.zeros((n_parked, R.NV_RBC, 3))                             # outside the open y faces: in no bin
    parked[:, :, 0] = 5.0 + 0.001 * np.arange(R.NV_RBC)
    parked[:, :, 1] = -20.0 - np.arange(n_parked)[:, None]
    parked[:, :, 2] = 5.0
    pos = np.concatenate([case["pos"][:R.NV_RBC], parked.reshape(-1, 3), case["pos"][R.NV_RBC:]])   # new RBCs join their type
    cell_of = np.concatenate([case["cell_of"][:R.NV_RBC], 100 + np.repeat(np.arange(n_parked), R.NV_RBC), case["cell_of"][R.NV_RBC:]])
    is_parked = cell_of >= 100
    ref = R.repulsion(pos, cell_of, np.ones(len(pos), dtype=bool), dims, periodic, K_REP, R.CUTOFF)
    assert len(ref["pairs"]) >= 50 and (ref["k"][:R.NV_RBC] > 0).sum() >= 50 and (ref["k"][~is_parked][R.NV_RBC:] > 0).sum() >= 50
    gc = GpuCase(gpu, case, dims, periodic)
    try:
        gc.set_repulsion(); gc.cf.applyRepulsionForce()                    # the regions exist: 1 + 1 / 4 + 64 RBC cells
        first = gc.cf.repulsion_forces
        for _ in range(n_parked):
            assert gc.cf.addCell(RBC, (5.0, 5.0, 5.0))
        assert gc.cf.counts()[:2] == (len(pos), n_parked + len(case["sizes"]))
        gc.cf.positions = pos
        gc.cf.applyRepulsionForce()
        r_g = gc.cf.repulsion_forces
    finally:
        gc.destroy()
    one = R.repulsion(case["pos"], case["cell_of"], alive, dims, periodic, K_REP, R.CUTOFF)
    _compare(first, one, None, "region without growth")
    _compare(r_g, ref, None, "grown RBC region")
    assert not r_g[is_parked].any()


def test_sort_regrowth(gpu):
    """hcp_repulsion sizes its sort buffers at the first call (n + n / 4 + 1024 = 1106 for one platelet), regrows them
    when 18 platelets exceed that, and reuses the block when most cells are gone again"""
    periodic, dims = (0, 1, 1), R.DIMS
    case = R.build_case(periodic, dims, seed=2, n_plt=18, big=False)
    assert len(case["pos"]) > R.NV_PLT + R.NV_PLT // 4 + 1024
    alive = np.ones(len(case["pos"]), dtype=bool)
    gc = GpuCase(gpu, dict(sizes=case["sizes"][:1], pos=case["pos"][:R.NV_PLT]), dims, periodic)
    try:
        gc.set_repulsion(); gc.cf.applyRepulsionForce()
        assert not gc.cf.repulsion_forces.any()                            # one cell: nobody to push
        for _ in range(17):
            assert gc.cf.addCell(PLT, (5.0, 5.0, 5.0))
        gc.cf.positions = case["pos"]
        gc.cf.applyRepulsionForce()
        ref = R.repulsion(case["pos"], case["cell_of"], alive, dims, periodic, K_REP, R.CUTOFF)
        assert len(ref["pairs"]) >= 50
        _compare(gc.cf.repulsion_forces, ref, None, "regrown sort buffers")
        rec = gc.cf.records()
        ids = gc.cf.cell_ids()
        stay = [1, 3, 4, 8, 17]                                            # a lapped cell, the cut-off pair and two more
        gc.cf.set_records(rec[np.isin(rec["cellId"], ids[stay])])
        keep = np.isin(case["cell_of"], stay)
        assert np.array_equal(gc.cf.positions, case["pos"][keep])
        gc.cf.applyRepulsionForce()
        ref = R.repulsion(case["pos"][keep], case["cell_of"][keep], alive[keep], dims, periodic, K_REP, R.CUTOFF)
        assert len(ref["pairs"]) >= 10
        _compare(gc.cf.repulsion_forces, ref, None, "reused sort buffers")
    finally:
        gc.destroy()


@pytest.mark.parametrize("periodic,dims", CASES, ids=IDS)
def test_boundary_repulsion_sweep(orc, gpu, periodic, dims):
    """solid blocks that touch the faces, vertices on other laps and outside the open faces, removed particles: the
    first and the accumulating second call equal the oracle and the float64 restatement bit for bit"""
    b = built(periodic, dims)
    case, mask, alive = b["case"], b["mask"], b["alive"]
    flag = R.boundary_flags(mask, periodic)
    assert flag[0, 2, 5] if periodic[0] else not flag[0, 2, 5]             # its only fluid neighbours lie across the x seam
    oc, gc = OracleCase(orc, case, dims, periodic, mask), GpuCase(gpu, case, dims, periodic, mask)
    try:
        oc.advance(); gc.advance()
        gc.set_boundary_repulsion()
        r0 = np.zeros(case["pos"].shape)
        for call in (1, 2):
            orc.orc_sim_boundary_repulsion(oc.S, K_WALL, R.CUTOFF); gc.cf.applyBoundaryRepulsionForce()
            r_g = gc.cf.repulsion_forces
            r0, _ = R.boundary_repulsion(case["pos"], alive, mask, periodic, K_WALL, R.CUTOFF, r0)
            assert np.array_equal(r_g, oc.get(3)) and np.array_equal(r_g, r0), call
    finally:
        oc.destroy(); gc.destroy()
    touched = np.abs(r_g).sum(1) > 0
    outside = ~R.in_grid(R.nearest_node(case["pos"]), dims, periodic)
    assert touched.sum() >= 20 and not touched[~alive].any() and not touched[outside].any()


@pytest.mark.parametrize("mode", ["particle", "cell"])
@pytest.mark.parametrize("periodic,dims", CASES, ids=IDS)
def test_tagging_sweep(orc, gpu, periodic, dims, mode):
    """advanceParticles with targets on solid and on fluid nodes through the seams, on other laps, on ties and outside
    the open faces: positions, alive() and deletion_counts() equal the oracle and tagged()"""
    b = built(periodic, dims)
    case, mask = b["case"], b["mask"]
    rng = np.random.default_rng(7)
    vel = rng.uniform(-0.4, 0.4, case["pos"].shape)
    vel[(np.mod(case["pos"], 1.0) == 0.5).any(axis=1)] = 0.0               # the ties stay ties
    start = case["pos"] - vel
    end = start + vel
    hit = R.tagged(end, mask, periodic)
    tie = (np.mod(end, 1.0) == 0.5).any(axis=1)
    assert hit.sum() >= 20 and tie.sum() >= 40 and hit[tie].any() and (~hit[tie]).any()
    lapped = np.isin(case["cell_of"], (1, 2))
    assert not any(periodic) or (hit[lapped].any() and (~hit[lapped]).any())
    gone = np.array([hit[case["cell_of"] == c].any() for c in range(len(case["sizes"]))])
    keep = np.ones(len(end), dtype=bool) if mode == "particle" else ~gone[case["cell_of"]]
    inputs = dict(sizes=case["sizes"], pos=start)
    oc, gc = OracleCase(orc, inputs, dims, periodic, mask, mode), GpuCase(gpu, inputs, dims, periodic, mask, mode)
    try:
        oc.advance(vel); gc.advance(vel)
        p_g, a_g, counts = gc.cf.positions, gc.cf.alive(), gc.cf.deletion_counts()
        p_o, a_o = oc.get(0), oc.alive()
        deleted = (oc.S.contents.cells_deleted, oc.S.contents.particles_deleted)
    finally:
        oc.destroy(); gc.destroy()
    assert np.array_equal(p_g, end[keep]) and np.array_equal(p_o, end[keep])
    if mode == "particle":
        assert np.array_equal(a_g, ~hit) and np.array_equal(a_o, ~hit)
        assert counts == (0, hit.sum(), gone.sum(), hit.sum()) and deleted == (0, hit.sum())
    else:
        assert a_g.all() and a_o.all()
        assert counts == (gone.sum(), 0, 0, 0) and deleted[0] == gone.sum() and 0 < gone.sum()


def test_coupled_run_across_the_y_and_z_seams(orc, gpu):
    """16 x 14 x 15, periodic (0, 1, 1), a solid slab at the low x face, both repulsions every 2nd iteration: two RBCs,
    one across the y seam and one across the z seam, 30 iterations against the oracle"""
    dims, periodic = (16, 14, 15), (0, 1, 1)
    mask = np.zeros(dims, dtype=np.uint8)
    mask[0:2] = 1
    Po, Pg = O.make_params(orc), gpu.base_parameters()
    Lo = O.OracleLattice(orc, dims[0], dims[1], dims[2], periodic, 1.0 / Po.tau)
    Lg = gpu.Lattice(dims[0], dims[1], dims[2], periodic, 1.0 / Po.tau)
    Lo.set_mask(mask); Lg.defineBounceBack(mask)
    Lo.init_equilibrium(); Lg.latticeEquilibrium()
    So = orc.orc_sim_create(Lo.ptr, C.byref(Po))
    hg = gpu.HemoCell(Lg, Pg)
    To, Tg = O.make_rbc(orc, Po), gpu.CellType.rbc(Pg)
    lib = gpu.capi.lib()
    try:
        orc.orc_sim_add_type(So, To); hg.cellfields.addCellType(Tg, 1)
        for centre, ang in (((4.3, 13.0, 4.0), (0.0, 0.0, 90.0)), ((9.0, 6.0, 14.0), (0.0, 0.0, 90.0))):
            c = np.array(centre)
            a = np.array(ang) * (3.14159265358979323846 / 180.0) * -1.0
            assert orc.orc_sim_add_cell(So, 0, O.dptr(c), O.dptr(a), 0.0) and hg.cellfields.addCell(0, centre, ang)
        cf = hg.cellfields
        pos = cf.positions
        assert pos[:642, 1].max() > 13.5 and pos[642:, 2].max() > 14.5 and (pos[:642, 0] < 2.25).sum() >= 20   # the seams and the wall are reached
        gpu.check(lib.hcp_set_repulsion(cf.ptr, K_REP, R.CUTOFF, 2)); cf.rep_timescale = 2
        gpu.check(lib.hcp_set_boundary_repulsion(cf.ptr, K_WALL, R.CUTOFF, 2)); cf.brep_timescale = 2
        s = So.contents
        s.rep_enabled = s.brep_enabled = 1; s.rep_timescale = s.brep_timescale = 2
        s.rep_const, s.rep_cutoff, s.brep_const, s.brep_cutoff = K_REP, R.CUTOFF, K_WALL, R.CUTOFF
        orc.orc_sim_mechanics(So, 1); cf.applyConstitutiveModel(0, True)
        for _ in range(30):
            orc.orc_sim_iterate(So)
        hg.iterate(30)
        p_o, r_o = np.zeros((So.contents.np, 3)), np.zeros((So.contents.np, 3))
        orc.orc_sim_get(So, 0, O.dptr(p_o)); orc.orc_sim_get(So, 3, O.dptr(r_o))
        a_o = np.ones(So.contents.np, dtype=np.uint8); orc.orc_sim_get_alive(So, a_o.ctypes.data)
        assert np.array_equal(cf.alive(), a_o.astype(bool))
        assert np.abs(cf.positions - p_o).max() <= 1e-9
        r_g = cf.repulsion_forces
        assert (np.abs(r_o[:642]).sum(1) > 0).sum() >= 20 and (np.abs(r_o[642:]).sum(1) > 0).sum() >= 20
        assert np.abs(r_g - r_o).max() <= 1e-9 * np.abs(r_o).max()
    finally:
        hg.cellfields.destroy(); Tg.destroy(); Lg.destroy()
        orc.orc_sim_destroy(So); orc.orc_celltype_destroy(To); Lo.destroy()
