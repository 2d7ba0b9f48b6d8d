"""The pre-inlet's cells into a domain cut into x-slabs (csrc/preinlet.hip: hcp_preinlet_create_slab, the collective
hcp_preinlet_apply and hc_preinlet_iterate; host.PreInlet(cells=(pre_cells, slab_cells)) on the inlet rank, host.PreInletPeer on
the others) against the same calls on one domain, bit for bit with hc_set_reproducible_spread(1): the records of the vertices
every rank owns, gathered over the ranks, and the populations on fluid nodes.  Pre-inlet 40 x 34 x 34, RBC (type 0) and PLT
(type 1); domain 96 x 34 x 34 as 2 slabs, 120 x 34 x 34 as 3.  The inputs are tests/preinlet_cells_slabs_scene.py, which
tests/test_preinlet_cells_slabs_cpu.py checks without a GPU; the ranks are tests/slab_ranks.py.  The same function runs a scene on
a rank of the world and, as rank 0 of a world of one, on the single domain."""
import ctypes as C
import os
import types

import numpy as np
import pytest

import open_boundary_axis_ref as AX
import preinlet_cells_ref as PC
import preinlet_cells_slabs_scene as SC
import slab_ranks

pytestmark = pytest.mark.gpu

SV = SC.REC
FIELDS = ("position", "v", "force", "force_repulsion", "cellId", "vertexId", "restime", "celltype")
HC_ERR_ARG = 2
ZERO = (0.0, 0.0, 0.0)


@pytest.fixture
def reproducible(gpu):
    """hc_set_reproducible_spread(1) for this process and, through the environment, for the ranks it starts"""
    os.environ["HEMOCELL_REPRODUCIBLE_SPREAD"] = "1"
    gpu.check(gpu.capi.lib().hc_set_reproducible_spread(1))
    yield
    os.environ.pop("HEMOCELL_REPRODUCIBLE_SPREAD", None)
    gpu.check(gpu.capi.lib().hc_set_reproducible_spread(0))


def _scene(direction, slabs, window, shift, pre_cells, residents, laps=None, sink=None, cells_every=1, k_p=1, u0=ZERO,
           randomise=False, coupling=True):
    """slabs: the number of slabs the GLOBAL domain is made for (the single domain is the same box on one rank)"""
    return dict(direction=direction, slabs=slabs, window=tuple(window), shift=tuple(shift), pre_cells=list(pre_cells),
                residents=list(residents), laps=dict(laps or {}), sink=sink, cells_every=cells_every, k_p=k_p, u0=tuple(u0),
                randomise=randomise, coupling=coupling)


def _randomise(cells):
    """non-zero velocities and forces on every vertex, a function of the cell's type and id alone: the same on every holder"""
    ids = cells.cell_ids()
    n = cells.counts()[0]
    vel, frc = np.zeros((n, 3)), np.zeros((n, 3))
    first_cell = 0
    for t in range(len(cells.types)):
        f, nc = cells.type_range(t)
        nv = cells.types[t].nv
        for c in range(nc):
            rng = np.random.default_rng([t, int(ids[first_cell + c])])
            rows = slice(f + c * nv, f + (c + 1) * nv)
            vel[rows] = rng.uniform(-1e-3, 1e-3, size=(nv, 3)); frc[rows] = rng.uniform(-1e-4, 1e-4, size=(nv, 3))
        first_cell += nc
    if n:
        cells.velocities = vel; cells.forces = frc


def _add_pre_cells(b, cells, laps):
    for t, cid, centre, ang in cells:
        assert b.pc.addCell(t, centre, ang, cell_id=cid)
    if laps:
        ids, pos, first_cell = b.pc.cell_ids(), b.pc.positions, 0
        for t in range(2):
            f, nc = b.pc.type_range(t)
            nv = b.pc.types[t].nv
            for c in range(nc):
                pos[f + c * nv:f + (c + 1) * nv, 0] += laps.get(int(ids[first_cell + c]), 0) * SC.PRE[0]
            first_cell += nc
        b.pc.positions = pos


def _build(rank, world, sc):
    """this rank's slab of the scene with its cells; on the rank that holds the inlet plane the pre-inlet with its cells and
    host.PreInlet, elsewhere host.PreInletPeer"""
    from hemocell_amd import host
    from hemocell_amd.slab import SlabRunner
    sign = SC.SIGN[sc["direction"]]
    nxg = SC.domain(sc["slabs"])[0]
    nx = nxg // world
    P = host.base_parameters()
    b = types.SimpleNamespace(host=host, P=P, pre=None, pc=None, coupling=None, nxg=nxg)
    b.r = r = SlabRunner(nx, SC.CROSS[0], SC.CROSS[1], rank, world, P, periodic=AX.NONPER, particle_timescale=sc["k_p"], material_timescale=1)
    b.mask = AX.channel_mask((nxg,) + SC.CROSS, 0)
    r.define_bounce_back(b.mask)
    r.lattice.latticeEquilibrium(1.0, sc["u0"])
    b.types = [host.CellType.rbc(P), host.CellType.plt(P)]
    for ct in b.types:
        r.add_cell_type(ct)
    for t, cid, centre, ang in sc["residents"]:
        r.cells.addCell(t, centre, ang, cell_id=cid)
    placed = r.sync_placement()
    assert tuple(placed) == tuple(sum(1 for c in sc["residents"] if c[0] == t) for t in range(2)), placed
    b.inlet = rank == (0 if sign < 0 else world - 1)
    kw = dict(window=sc["window"], shift=sc["shift"], id_stride=SC.STRIDE, sink=sc["sink"], cells_every=sc["cells_every"],
              particle_timescale=sc["k_p"])
    if b.inlet:
        pmask = AX.channel_mask(SC.PRE, 0)
        b.pre = host.Lattice(*SC.PRE, (True, False, False), 1.0 / P.tau)
        b.pre.defineBounceBack(pmask); b.pre.latticeEquilibrium(1.0, sc["u0"])
        b.pc = host.Cells(b.pre, P)
        for ct in b.types:
            b.pc.addCellType(ct, 1)
        _add_pre_cells(b, sc["pre_cells"], sc["laps"])
    if sc["randomise"]:
        _randomise(r.cells)
        if b.pc is not None:
            _randomise(b.pc)
    else:
        r.prepare()
        if b.pc is not None:
            b.pc.applyConstitutiveModel(0, True)
    if not sc["coupling"]:
        return b
    if b.inlet:
        ly, lz = np.nonzero(pmask[0] == 0)
        g = np.stack([ly, lz], axis=1)
        b.coupling = host.PreInlet(b.pre, r.lattice, g, SC.PRE[0] - 1 if sign < 0 else 0, 0 if sign < 0 else nx - 1,
                                   direction=sc["direction"], device=True, cells=(b.pc, r.cells), **kw)
        r.lattice.setOpenBoundaryVelocitySlots(b.coupling.first, np.tile(np.asarray(sc["u0"], float), (len(g), 1)))
    else:
        b.coupling = host.PreInletPeer(r.cells, direction=sc["direction"], **kw)
    out_plane = nxg - 1 if sign < 0 else 0
    r.add_open_boundary(1, 0, -sign, (out_plane, out_plane, 0, SC.CROSS[0] - 1, 0, SC.CROSS[1] - 1))
    return b


def _destroy(b):
    if b.coupling is not None:
        b.coupling.destroy()
    if b.pc is not None:
        b.pc.destroy()
    b.r.cells.destroy()
    if b.pre is not None:
        b.pre.destroy()
    b.r.lattice.destroy()
    for ct in b.types:
        ct.destroy()


def _state(b, out, key):
    """what this rank contributes to a comparison: the records of the vertices it owns (as bytes), its populations, the ids it
    holds and the coupling's counts"""
    rec = b.r.cells.records()
    g = np.floor(rec["position"][:, 0] + 0.5).astype(np.int64) - b.r.x0
    own = (g >= 0) & (g < b.r.nx)
    out[key + "_rec"] = np.ascontiguousarray(rec[own]).view(np.uint8).reshape(-1, SV.itemsize)
    out[key + "_f"] = b.r.populations()
    out[key + "_held"] = b.r.cells.cell_ids()
    out[key + "_counts"] = np.array(b.coupling.cell_counts())


def _records(blocks):
    rec = np.concatenate([np.ascontiguousarray(x).reshape(-1, SV.itemsize) for x in blocks]).reshape(-1).view(SV)
    return rec[np.lexsort((rec["vertexId"], rec["cellId"], rec["celltype"]))]


def _compare(res, ref, key, exact=True):
    """the ranks' state `key` against the single domain's: owned records gathered over the ranks, populations on fluid nodes, the
    counts on every rank"""
    got, want = _records([r[key + "_rec"] for r in res]), _records([ref[key + "_rec"]])
    assert len(got) == len(want), (key, len(got), len(want))              # every vertex owned by exactly one rank
    for f in ("cellId", "vertexId", "celltype", "restime"):
        assert np.array_equal(got[f], want[f]), (key, f)
    nxg = sum(len(r[key + "_f"]) for r in res) // (SC.CROSS[0] * SC.CROSS[1])
    dims = (nxg,) + SC.CROSS
    fluid = AX.channel_mask(dims, 0) == 0
    f_got = np.concatenate([r[key + "_f"].reshape((-1,) + SC.CROSS + (19,)) for r in res], axis=0)
    f_want = ref[key + "_f"].reshape(dims + (19,))
    assert np.isfinite(f_want).all() and np.isfinite(want["position"]).all()
    err_x = float(np.abs(got["position"] - want["position"]).max()) if len(got) else 0.0
    err_f = float(np.abs(f_got - f_want)[fluid].max())
    print("%s: %d vertices, max |dx| = %.3e, max |df| = %.3e" % (key, len(got), err_x, err_f))
    if exact:
        for f in ("position", "v", "force", "force_repulsion"):
            assert np.array_equal(np.ascontiguousarray(got[f]).view(np.uint64), np.ascontiguousarray(want[f]).view(np.uint64)), (key, f, float(np.abs(got[f] - want[f]).max()))
        assert np.array_equal(f_got[fluid], f_want[fluid]), (key, err_f)
    else:
        assert err_x <= 1e-9, (key, err_x)                                 # the slab tests' bound for the atomic spread
    for r in res:                                                          # 5: global totals, equal on every rank
        assert tuple(r[key + "_counts"]) == tuple(ref[key + "_counts"]), (key, r[key + "_counts"], ref[key + "_counts"])
    return got


def _ids(rec):
    return sorted(set((int(t), int(i)) for t, i in zip(rec["celltype"], rec["cellId"])))


def _check_extents(gpu):
    """the half extents the scene file assumes are those of the placed meshes"""
    P = gpu.base_parameters()
    for (t, ang), half in SC.HALF.items():
        L = gpu.Lattice(32, 32, 32, (True, True, True), 1.0 / P.tau)
        cells = gpu.Cells(L, P)
        ct = (gpu.CellType.rbc if t == 0 else gpu.CellType.plt)(P)
        cells.addCellType(ct, 1)
        assert cells.addCell(0, (16.0, 16.0, 16.0), ang)
        p = cells.positions
        assert np.abs(p.max(axis=0) - 16.0 - half).max() < 1e-6 and np.abs(16.0 - p.min(axis=0) - half).max() < 1e-6
        cells.destroy(); L.destroy(); ct.destroy()


# ---- 1: one static check

def _static_run(rank, world, sc):
    b = _build(rank, world, sc)
    out = {}
    out["check1"] = np.array(b.coupling.applyPreInletCells())
    _state(b, out, "a")
    out["check2"] = np.array(b.coupling.applyPreInletCells())
    if b.pc is not None:   # the slow path: 70 PLTs at once into a region of 65 slots
        _add_pre_cells(b, SC.static_more_cells(), None)
        _randomise(b.pc)
    out["check3"] = np.array(b.coupling.applyPreInletCells())
    _state(b, out, "b")
    out["check4"] = np.array(b.coupling.applyPreInletCells())
    out["plt"] = np.array(b.r.cells.type_range(1)[1])
    out["alive"] = np.array(bool(b.r.cells.alive().all()))
    _destroy(b)
    return out


@pytest.mark.parametrize("direction, world", [("Xneg", 2), ("Xpos", 2), ("Xneg", 3), ("Xpos", 3)])
def test_one_static_check(gpu, tmp_path, reproducible, direction, world):
    """the five cases of test_static_selection_and_copy, a candidate whose new id only the far rank holds, then 70 PLTs that
    grow the inlet rank's region; every check returns the global numbers on every rank"""
    _check_extents(gpu)
    sign = SC.SIGN[direction]
    sc = _scene(direction, world, SC.STATIC_WINDOW, SC.static_shift(direction, world), SC.static_pre_cells(),
                SC.static_residents(direction, world), laps=SC.STATIC_LAPS, randomise=True)
    ref = _static_run(0, 1, sc)
    assert tuple(ref["check1"]) == (2, 0) and tuple(ref["a_counts"]) == (2, 1, 0, 1) and tuple(ref["check2"]) == (0, 0)
    assert tuple(ref["check3"]) == (70, 0) and tuple(ref["b_counts"]) == (72, 1, 0, 3) and tuple(ref["check4"]) == (0, 0)
    new = [(0, PC.new_id(5007, 0, sign, SC.STRIDE)), (1, PC.new_id(5011, 2, sign, SC.STRIDE))]
    collide = (1, PC.new_id(5015, 0, sign, SC.STRIDE))
    assert _ids(_records([ref["a_rec"]])) == sorted([(0, 1), (1, 2), collide] + new)
    res = slab_ranks.run(_static_run, world, tmp_path, sc, salt=40 + 2 * world + (sign > 0))
    for r in res:
        for k in ("check1", "check2", "check3", "check4"):
            assert tuple(r[k]) == tuple(ref[k]), (k, r[k])
        assert bool(r["alive"])
    got = _compare(res, ref, "a")
    assert np.all(got["v"] != 0.0) and np.all(got["force"] != 0.0)
    _compare(res, ref, "b")
    inlet, far = res[SC.inlet_rank(direction, world)], res[SC.far_rank(direction, world)]
    assert collide[1] in far["a_held"] and collide[1] not in inlet["b_held"]      # the far rank's resident kept the candidate out
    assert int(inlet["plt"]) == 72 and int(far["plt"]) == 1                        # the arrivals are the inlet rank's alone


# ---- 2: the coupled run through hc_preinlet_iterate

def _coupled_scene(world):
    return _scene("Xneg", world, SC.COUPLED_WINDOW, SC.coupled_shift(world), SC.coupled_pre_cells(), SC.coupled_residents(world),
                  cells_every=2, u0=SC.U0)


ARRIVAL = (1, 5040 + SC.STRIDE)


def _coupled_single(sc):
    """the one-domain run, two iterations at a time; states are taken when the PLT has arrived (a), when its leading vertex is
    within 0.75 planes of the face between the inlet slab and its neighbour (b), and when it has passed that face by a plane (c).
    Returns (iterations of a, b, c; states; leading vertex at b and c)"""
    b = _build(0, 1, sc)
    face = SC.slab_of(0, sc["slabs"])[1]
    out, at, lead = {}, {}, {}
    for _ in range(150):
        b.coupling.iterate(2)
        cells = PC.by_id(b.r.cells.records())
        if ARRIVAL not in cells:
            continue
        x = float(cells[ARRIVAL]["position"][:, 0].max())
        key = "a" if "a" not in at else "b" if "b" not in at and x >= face - 0.75 else "c" if "b" in at and x >= face + 1.0 else None
        if key:
            at[key], lead[key] = b.coupling.iter, x
            _state(b, out, key)
        if key == "c":
            break
    _destroy(b)
    return at, out, lead


def _coupled_run(rank, world, sc, stops):
    b = _build(rank, world, sc)
    out, done = {}, 0
    for key, it in stops:
        b.coupling.iterate(it - done); done = it
        assert b.coupling.iter == it
        _state(b, out, key)
    out["cells_new"] = np.array(b.r.slab_stats()["cells_new"])
    out["late"] = np.array(b.r.envelope()[1])
    _destroy(b)
    return out


@pytest.mark.parametrize("world", [2, 3])
def test_coupled_run_crosses_the_inner_face(gpu, tmp_path, reproducible, world):
    """cells every 2nd iteration, inflow 0.06: a PLT arrives as close to the inlet slab's inner face as create allows, is
    replicated by the ordinary envelope synchronisation and crosses onto the neighbour"""
    sc = _coupled_scene(world)
    at, ref, lead = _coupled_single(sc)
    face = SC.slab_of(0, world)[1]
    assert sorted(at) == ["a", "b", "c"] and at["a"] < at["b"] < at["c"], at
    assert lead["b"] < face and lead["c"] >= face + 1.0, lead                      # checkpoints before and after the crossing
    print("arrival at iteration %d, before the face at %d (%.3f), past it at %d (%.3f)" % (at["a"], at["b"], lead["b"], at["c"], lead["c"]))
    assert tuple(ref["c_counts"]) == (1, 0, 0, at["c"] // 2)
    res = slab_ranks.run(_coupled_run, world, tmp_path, sc, [(k, at[k]) for k in "abc"], salt=50 + world)
    for key in "abc":
        got = _compare(res, ref, key)
        assert _ids(got) == [(0, 1), ARRIVAL]
    assert ARRIVAL[1] in res[0]["a_held"] and ARRIVAL[1] in res[1]["c_held"]
    assert float(res[1]["cells_new"]) > 0 and all(int(r["late"]) == 0 for r in res)


def test_coupled_run_with_the_atomic_spread(gpu, tmp_path):
    """the same run on 2 slabs with the default spread (atomic adds, whose order is not fixed): owned vertices to the slab tests'
    bound of 1e-9 lu against one domain"""
    gpu.check(gpu.capi.lib().hc_set_reproducible_spread(0))
    sc = _coupled_scene(2)
    at, ref, lead = _coupled_single(sc)
    assert sorted(at) == ["a", "b", "c"] and lead["c"] >= SC.slab_of(0, 2)[1] + 1.0
    res = slab_ranks.run(_coupled_run, 2, tmp_path, sc, [("c", at["c"])], salt=59)
    got = _compare(res, ref, "c", exact=False)
    assert _ids(got) == [(0, 1), ARRIVAL] and float(res[1]["cells_new"]) > 0


# ---- 3: the sink across a face

def _sink_scene(residents, pre_cells):
    return _scene("Xneg", 2, SC.STALE_WINDOW, SC.STALE_SHIFT, pre_cells, residents, sink=SC.SINK_PLANE, u0=SC.U0)


def _sink_run(rank, world, sc, k):
    """k None (the single domain): iteration by iteration until the sink takes PLT 5, the extent of PLT 5 before it went;
    on the ranks: k - 1 iterations, who holds what, the removal iteration, 5 more"""
    b = _build(rank, world, sc)
    out = {}
    if k is None:
        for _ in range(150):
            x = PC.by_id(b.r.cells.records())[(1, 5)]["position"][:, 0]
            b.coupling.iterate(1)
            if b.coupling.cell_counts()[2]:
                break
        k = b.coupling.iter
        out["k"], out["x_before"] = np.array(k), x
    else:
        b.coupling.iterate(k - 1)
        out["held_before"] = b.r.cells.cell_ids()
        b.coupling.iterate(1)
    _state(b, out, "k")
    b.coupling.iterate(5)
    _state(b, out, "k5")
    _destroy(b)
    return out


def test_sink_takes_a_cell_from_both_holders(gpu, tmp_path, reproducible):
    """2 slabs, the sink plane two nodes inside the last: a PLT drifts across it while both ranks own vertices of it and goes from
    both in the same check; the whole state is the single domain's at that iteration and 5 iterations later"""
    sc = _sink_scene(SC.sink_residents(), SC.sink_pre_cells())
    ref = _sink_run(0, 1, sc, None)
    k, x = int(ref["k"]), ref["x_before"]
    face = SC.slab_of(0, 2)[1]
    assert 10 < k < 150 and x.min() < face - 0.5 < x.max() and x.max() <= SC.SINK_PLANE, (k, x.min(), x.max())
    assert tuple(ref["k_counts"]) == (0, 0, 1, k) and tuple(ref["k5_counts"]) == (0, 0, 1, k + 5)
    print("the PLT crosses the sink plane at iteration %d" % k)
    res = slab_ranks.run(_sink_run, 2, tmp_path, sc, k, salt=61)
    for r in res:
        assert 5 in r["held_before"] and 5 not in r["k_held"]                     # both held it; neither does after the check
    for key in ("k", "k5"):
        assert _ids(_compare(res, ref, key)) == [(1, 6)]


# ---- 4: the stale plan

def _stale_run(rank, world, sc):
    """the iteration counter starts at 1, so that iteration 1 -- not a velocity update -- takes the extents for the envelope
    synchronisation of iteration 2 before the check in between changes the cell set"""
    b = _build(rank, world, sc)
    out = {}
    b.coupling.iter = 1
    out["held0"] = b.r.cells.cell_ids()
    b.coupling.iterate(1)
    _state(b, out, "a")
    out["plt"] = np.array(b.r.cells.type_range(1)[1])
    b.coupling.iterate(1)
    _state(b, out, "b")
    b.coupling.iterate(6)
    _state(b, out, "c")
    out["late"] = np.array(b.r.envelope()[1])
    _destroy(b)
    return out


def test_stale_envelope_plan(gpu, tmp_path, reproducible):
    """particle_timescale 2, a check after every iteration: the first check takes PLT 5, of which rank 0 holds a pure copy, and
    brings one from the pre-inlet, so rank 0 holds two PLTs before and after; PLT 6, across the face, has moved into the slot of 5,
    and with the extents taken before the check rank 0 would not forward it at the next synchronisation"""
    sc = _sink_scene(SC.stale_residents(), SC.stale_pre_cells())
    sc["k_p"] = 2
    ref = _stale_run(0, 1, sc)
    assert tuple(ref["a_counts"]) == (1, 0, 1, 1) and tuple(ref["c_counts"]) == (1, 0, 1, 8)
    res = slab_ranks.run(_stale_run, 2, tmp_path, sc, salt=62)
    assert list(res[0]["held0"]) == [5, 6] and sorted(res[1]["held0"]) == [5, 6]                             # 5 in rank 0's first PLT slot
    assert int(res[0]["plt"]) == 2 and list(res[0]["a_held"]) == [6, 6040] and list(res[1]["a_held"]) == [6]   # the count is unchanged
    for key in "abc":
        assert _ids(_compare(res, ref, key)) == [(1, 6), (1, 6040)]
    assert all(int(r["late"]) == 0 for r in res)


# ---- a rank that fails inside a check fails every rank

HC_ERR_STATE = 3


def _failing_run(rank, world, sc):
    b = _build(rank, world, sc)
    lib = b.host.capi.lib()
    out = {}

    def check():
        a, c = C.c_long(-1), C.c_long(-1)
        rc = lib.hcp_preinlet_apply(b.coupling.cells_ptr, C.byref(a), C.byref(c))
        return rc, lib.hc_last_error().decode(), (a.value, c.value)

    held = sorted(b.r.cells.cell_ids())
    # a: the ranks were told different sink planes -- every rank reads that out of the first round
    if rank == 1:
        b.host.check(lib.hcp_preinlet_set_sink(b.coupling.cells_ptr, 1, sc["sink"] + 1.0))
    rc, msg, _ = check()
    out["a"] = np.array(int(rc == HC_ERR_STATE and "disagree about the sink" in msg))
    if rank == 1:
        b.host.check(lib.hcp_preinlet_set_sink(b.coupling.cells_ptr, 1, sc["sink"]))
    # b: rank 1's copy of PLT 5 lies 5 planes further on, past the plane: rank 1, an owner, names it; rank 0, an owner too, keeps
    # it by its own select and fails in the second round, which fails rank 1 as well
    pos0 = b.r.cells.positions
    if rank == 1:
        b.r.cells.positions = pos0 + (5.0, 0.0, 0.0)
    rc, msg, _ = check()
    out["b"] = np.array(int(rc == HC_ERR_STATE and "disagree on whether" in msg and ("rank 0 failed" in msg) == (rank == 1)))
    out["kept"] = np.array(int(sorted(b.r.cells.cell_ids()) == held and b.coupling.cell_counts() == (0, 0, 0, 0)))
    if rank == 1:
        b.r.cells.positions = pos0
    # c: put right, the check runs, and the candidate of the failed checks has not been used up
    rc, msg, got = check()
    out["c"] = np.array(int(rc == 0 and got == (1, 0) and b.coupling.cell_counts() == (1, 0, 0, 1)))
    out["held"] = b.r.cells.cell_ids()
    _destroy(b)
    return out


def test_a_failing_rank_fails_every_rank(gpu, tmp_path, reproducible):
    """the sink scene at rest with the sink plane at 52, beyond the PLT across the face: sink planes that differ between the
    ranks, then a copy that disagrees with its other owner (no orphan), are HC_ERR_STATE on both ranks with nothing changed;
    afterwards the check runs"""
    sc = _scene("Xneg", 2, SC.STALE_WINDOW, SC.STALE_SHIFT, SC.stale_pre_cells(), SC.sink_residents(), sink=SC.SINK_PLANE + 2.0)
    res = slab_ranks.run(_failing_run, 2, tmp_path, sc, salt=63)
    for r in res:
        assert (int(r["a"]), int(r["b"]), int(r["kept"]), int(r["c"])) == (1, 1, 1, 1), {k: r[k] for k in "abc"}
    assert sorted(res[0]["held"]) == [5, 6, 6040] and list(res[1]["held"]) == [5]


# ---- 6: refusals, with nothing changed

def _create_slab(host, pre_cells, dom_cells, axis, sign, window, shift):
    ptr = C.c_void_p()
    sh = np.array(shift, dtype=np.float64)
    lib = host.capi.lib()
    rc = lib.hcp_preinlet_create_slab(C.byref(ptr), pre_cells.ptr if pre_cells is not None else None, dom_cells.ptr, int(axis), int(sign),
                                      float(window[0]), float(window[1]), host.dptr(sh), SC.STRIDE)
    assert (rc == 0) == bool(ptr.value)   # a refused call hands out nothing
    return rc, ptr, lib.hc_last_error().decode()


def _refusal_run(rank, world, sc):
    b = _build(rank, world, sc)
    host, sign = b.host, SC.SIGN[sc["direction"]]
    before = (b.r.cells.counts(), b.r.cells.records().tobytes(), b.r.populations().tobytes())
    own = b.pc                                                           # the pre-inlet's container on the inlet rank, None elsewhere
    spare = spare_cells = None
    if rank == SC.far_rank(sc["direction"], world):                      # a pre-inlet where none belongs
        spare = host.Lattice(*SC.PRE, (True, False, False), 1.0 / b.P.tau)
        spare_cells = host.Cells(spare, b.P)
        for ct in b.types:
            spare_cells.addCellType(ct, 1)
    x0, x1 = SC.slab_of(SC.inlet_rank(sc["direction"], world), world)
    near = list(sc["shift"])
    near[0] = (x1 - SC.E_SHARE + 1.0 - sc["window"][1]) if sign < 0 else (x0 + SC.E_SHARE - 1.0 - sc["window"][0])
    cases = (("particle envelope", own, 0, near), ("only axis 0", own, 1, sc["shift"]),
             ("pre must be null", own if own is not None else spare_cells, 0, sc["shift"]),
             ("needs the pre-inlet", None, 0, sc["shift"]))
    seen = []
    for words, pre_cells, axis, shift in cases:
        rc, ptr, msg = _create_slab(host, pre_cells, b.r.cells, axis, sign, sc["window"], shift)
        seen.append(int(rc == HC_ERR_ARG and not ptr.value and words in msg))
    after = (b.r.cells.counts(), b.r.cells.records().tobytes(), b.r.populations().tobytes())
    rc, ptr, msg = _create_slab(host, own, b.r.cells, 0, sign, sc["window"], sc["shift"])   # the same arguments, put right, are taken
    assert rc == 0, msg
    counts = np.zeros(4, np.int64)
    host.check(host.capi.lib().hcp_preinlet_counts(ptr, host.lptr(counts)))
    host.check(host.capi.lib().hcp_preinlet_destroy(ptr))
    if spare is not None:
        spare_cells.destroy(); spare.destroy()
    _destroy(b)
    return {"seen": np.array(seen), "unchanged": np.array(before == after), "counts": counts}


@pytest.mark.parametrize("direction, world", [("Xneg", 2), ("Xpos", 3)])
def test_refusals_change_nothing(gpu, tmp_path, reproducible, direction, world):
    """a window image within the envelope of the inner face, an axis other than 0, a pre-inlet on a rank without the inlet plane and
    none on the rank with it: HC_ERR_ARG on EVERY rank, with the refusing rank's words; a null fluid handle with a one-domain
    handle likewise"""
    sc = _scene(direction, world, SC.STATIC_WINDOW, SC.static_shift(direction, world), SC.static_pre_cells(),
                SC.static_residents(direction, world), laps=SC.STATIC_LAPS, randomise=True, coupling=False)
    res = slab_ranks.run(_refusal_run, world, tmp_path, sc, salt=70 + world)
    for r in res:
        assert list(r["seen"]) == [1, 1, 1, 1] and bool(r["unchanged"]) and list(r["counts"]) == [0, 0, 0, 0]
    # one domain: hc_preinlet_iterate without a fluid handle steps nothing
    sc["coupling"] = True
    b = _build(0, 1, sc)
    try:
        S, n = b.r.populations(), b.r.cells.counts()
        it = C.c_long(0)
        rc = gpu.capi.lib().hc_preinlet_iterate(None, b.coupling.cells_ptr, C.byref(it), 3, 1, 1, 1, 1)
        assert rc == HC_ERR_ARG and it.value == 0
        with pytest.raises(gpu.HcError, match="fluid handle"):
            gpu.check(rc)
        assert np.array_equal(b.r.populations(), S) and b.r.cells.counts() == n and b.coupling.cell_counts() == (0, 0, 0, 0)
    finally:
        _destroy(b)
