"""two and three ranks (processes sharing the one GPU of the test box) vs one rank: the slab decomposition with the
native schedule of csrc/slab.hip -- halo exchange beside the interior collide, particle envelopes, wall deletions agreed
between the holders of a cell -- must reproduce the single-domain run.  RCCL refuses two ranks on one device, so the
ranks talk through the library's TCP data plane here (HC_TRANSPORT_TCP: same messages, same routing, same schedule);
the RCCL data plane itself is exercised by the rank that is its own periodic neighbour (test below)."""
import multiprocessing as mp
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

NXG, NY, NZ = 144, 34, 34
CELLS = [((10.0, 16.5, 16.5), (90, 0, 0)), ((46.5, 16.0, 17.0), (80, 20, 10)), ((141.0, 17.0, 16.0), (90, 0, 30)),
         ((70.0, 12.0, 20.0), (10, 20, 30)), ((96.5, 17.5, 16.0), (90, 10, 0)), ((57.5, 21.0, 14.0), (90, 0, 0))]
PLTS = [((47.0, 12.0, 21.0), (20, 40, 10)), ((120.0, 20.0, 13.0), (0, 0, 0)), ((143.5, 15.0, 21.5), (70, 0, 30))]   # platelets, two at faces
# fast flow: the cells travel ~6 lu in 250 iterations, so envelope copies are created and dropped at the faces.
# (Beyond ~300 iterations this strongly driven case amplifies a 1e-13 perturbation to 1e-5 even on a single
# domain, so longer runs cannot be compared position by position.)
STEPS, K_P, K_M = 250, 2, 4
FORCE = (3e-4, 0.0, 0.0)


# a cell that is pushed into the pipe wall next to the slab face at x = 72 (both ranks hold a copy): every holder must drop it
# at the next envelope synchronisation (slab runs never deleted such cells); cell 0 stays in the lumen
WALL_CELLS = [((30.0, 16.5, 16.5), (90, 0, 0)), ((69.0, 16.5, 25.0), (90, 0, 0))]

REPULSION = dict(k=2e-6, cutoff_um=0.7, k_b=3e-6, b_cutoff_um=1.0)   # examples/pipeflow/config.xml:36-38 magnitudes


def _build(rank, world, rep=False, padded=False, cells=CELLS, plts=PLTS, force=FORCE, nxg=NXG, del_mode=None, k_p=K_P, push=None, regions=None, envelope=None):
    from hemocell_amd import host
    from hemocell_amd.slab import SlabRunner
    host.check(host.capi.lib().hc_debug_force_plane_padding(1 if padded else 0))   # padded x-plane stride (hc_lattice::xs)
    P = host.base_parameters()
    r = SlabRunner(nxg // world, NY, NZ, rank, world, P, periodic=(True, False, False), particle_timescale=k_p,
                   material_timescale=K_M, deletion_check_every=1)
    mask, _ = host.pipe_mask(nxg, NY, NZ)
    r.define_bounce_back(mask)
    r.lattice.latticeEquilibrium(1.0, (0, 0, 0))
    r.lattice.setExternalVector(force)
    if regions:   # setExternalVector on sub-domains, in GLOBAL node coordinates on every rank
        r.lattice.setExternalVectorBoxes([b for b, _ in regions], [f for _, f in regions])
    r.add_cell_type(host.CellType.rbc(P))
    r.add_cell_type(host.CellType.plt(P))
    if del_mode:
        r.cells.setDeletionMode(del_mode)
    if envelope is not None:
        r.share = r.set_envelope(envelope)
    r.load_cells(0, [np.array(c) for c, _ in cells], [np.array(a) for _, a in cells])
    r.load_cells(1, [np.array(c) for c, _ in plts], [np.array(a) for _, a in plts])
    placed = r.sync_placement()
    assert tuple(placed) == (len(cells), len(plts)), placed     # distinct cells over all slabs
    if rep:
        r.cells.setRepulsion(REPULSION["k"], REPULSION["cutoff_um"], K_P)
        r.cells.enableBoundaryParticles(REPULSION["k_b"], REPULSION["b_cutoff_um"], K_P)
    r.prepare()
    return r, mask


def _run(r, steps, push, query_at=None):
    """push = (cell id, velocity): after iteration 0 has interpolated, that cell gets a held velocity (velocities are only
    refreshed every stepParticleEvery iterations) -- the IBM itself never lets a membrane reach a no-slip wall.
    query_at: after that many iterations the host looks at the cells the way HemoCell::writeOutput does
    (deleteIncompleteCells + counts: this rank compacts its gone cells away on its own, between two synchronisations)"""
    if push is None:
        r.run(steps)
        return
    r.run(1)
    ids = r.cells.cell_ids()
    if len(ids):                                          # a slab may hold no cell at all
        vel = r.cells.velocities.reshape(len(ids), -1, 3)     # RBC only in these cases
        vel[ids == push[0]] = np.array(push[1])
        r.cells.velocities = vel.reshape(-1, 3)
    done = 1
    if query_at is not None:
        r.run(query_at - done); done = query_at
        r.cells.deleteIncompleteCells(); r.cells.counts()
    r.run(steps - done)


def _worker(rank, world, port, out, kw, steps, q):
    try:
        sys.path.insert(0, ROOT)
        from hemocell_amd import host, slab
        slab.comm_init(rank, world, local_rank=0, port=port, transport="tcp")   # every rank on GPU 0
        push = kw.pop("push", None); query_at = kw.pop("query_at", None)
        if rank != 0:
            query_at = None          # only rank 0 looks: the asymmetric case (the other holder still has its copy)
        expect_error = kw.pop("expect_error", False)
        r, _ = _build(rank, world, **kw)
        error = ""
        try:
            _run(r, steps, push, query_at)
        except host.HcError as e:          # host.check raises it with hc_last_error()
            if not expect_error:
                raise
            error = str(e)
        cid, vid, pos = r.owned_vertex_table(0)
        pcid, pvid, ppos = r.owned_vertex_table(1)
        gstats = (r.fluid_stats(0), r.vertex_stats(1), r.vertex_stats(2))    # reduced: every rank gets the global numbers
        rho, u = r.lattice.rho_u()                                            # the face planes pull across the rank faces
        np.savez(os.path.join(out, "r%d.npz" % rank), f=r.populations(), rho=rho, u=u, pi=r.lattice.pi_neq(), cid=cid, vid=vid, pos=pos, pcid=pcid, pvid=pvid, ppos=ppos,
                 held=r.cells.counts()[1], gstats=np.array(gstats), stats=np.array(list(r.slab_stats().values())),
                 deleted=r.cells.counts()[2], error=np.array(error), envelope=np.array(r.envelope()))
        slab.barrier()
        slab.comm_finalize()
        q.put((rank, "ok"))
    except BaseException as e:   # noqa: BLE001 -- the parent reports it; the peers time out on their sockets
        import traceback
        q.put((rank, "FAILED: %r\n%s" % (e, traceback.format_exc())))


def _spawn(world, tmp_path, kw, steps=STEPS, salt=0):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 32000 + (os.getpid() * 5 + world * 97 + salt * 389) % 20000
    os.environ["HEMOCELL_COMM_TIMEOUT"] = "90"
    ps = [ctx.Process(target=_worker, args=(r, world, port, str(tmp_path), kw, steps, q)) for r in range(world)]
    for p in ps:
        p.start()
    res = [q.get(timeout=600) for _ in ps]
    for p in ps:
        p.join(60)
    assert sorted(r[0] for r in res) == list(range(world)) and all(r[1] == "ok" for r in res), res
    names = ("cells_sent", "cells_new", "cells_dropped", "cells_deleted", "iterations", "host_s", "header_wait_s", "particle_steps")
    out = []
    for k in range(world):
        z = dict(np.load(os.path.join(tmp_path, "r%d.npz" % k)))
        z["stats"] = dict(zip(names, z["stats"]))
        out.append(z)
    return out


def _observables_error(ref, res, nxg, fluid):
    """rho, u and Pi_neq of the slabs put side by side against the single domain's, on the fluid nodes: the face planes evaluate
    them from populations pulled across the rank face (hi_ok / lo_ok)"""
    rho_r, u_r = ref.lattice.rho_u()
    pi_r = ref.lattice.pi_neq()
    out = []
    for key, want, c in (("rho", rho_r, 1), ("u", u_r, 3), ("pi", pi_r, 6)):
        got = np.concatenate([r[key].reshape(nxg // len(res), NY * NZ, c) for r in res], axis=0)
        out.append(float(np.abs(got - want.reshape(nxg, NY * NZ, c))[fluid].max()))
    return out


def _initial_x():
    r0, _ = _build(0, 1)
    x = r0.cells.positions[:, 0].copy()
    r0.lattice.destroy()
    return x


@pytest.fixture
def reproducible_spread(gpu):
    """hc_set_reproducible_spread for this process and, through the environment, for the ranks it spawns"""
    os.environ["HEMOCELL_REPRODUCIBLE_SPREAD"] = "1"
    gpu.check(gpu.capi.lib().hc_set_reproducible_spread(1))
    yield
    del os.environ["HEMOCELL_REPRODUCIBLE_SPREAD"]
    gpu.check(gpu.capi.lib().hc_set_reproducible_spread(0))


# the cells of CELLS / PLTS that stay clear of the periodic seam during the run: a cell across the seam lives on one slab as
# its periodic image, 144 lu away, where x + v rounds in other bits than at the unshifted position (the reference shifts
# its envelope copies the same way, core/hemoCellParticleDataTransfer.cpp:33-65); those cases keep a tolerance (below)
INNER_CELLS, INNER_PLTS = [CELLS[k] for k in (0, 1, 3, 4, 5)], [PLTS[k] for k in (0, 1)]


@pytest.mark.parametrize("world,padded,seam", [(2, False, False), (3, False, False), (4, False, False), (2, True, False), (2, False, True), (3, False, True)])
def test_slabs_equal_single_domain_bit_for_bit(tmp_path, gpu, reproducible_spread, world, padded, seam):
    """with the reproducible spread (sums in cell-id order, whatever slot a cell sits in) N slabs give the BITS of the single
    domain: populations and vertex positions after 250 iterations, copies created and dropped at the interior faces on the way --
    what the reference's CI asks of its rank counts (scripts/ci/pipeflow_sanity.sh:25-33), here without any tolerance.
    seam: with the two cells that cross the periodic seam as well; their images round differently (above), the rest of the
    difference the atomic spread showed is gone: 1e-12 where test_slabs_match_single_domain needs 5e-12"""
    nxg = 192 if world == 4 else NXG
    kw = dict(nxg=nxg) if seam else dict(nxg=nxg, cells=INNER_CELLS, plts=INNER_PLTS)
    cells, plts = (CELLS, PLTS) if seam else (INNER_CELLS, INNER_PLTS)
    res = _spawn(world, tmp_path, dict(kw, padded=padded), salt=60 + padded + 2 * seam)
    ref, mask = _build(0, 1, **kw)
    ref.run(STEPS)
    f_ref = ref.lattice.populations().reshape(nxg, NY * NZ, 19)
    f_all = np.concatenate([r["f"].reshape(nxg // world, NY * NZ, 19) for r in res], axis=0)
    fluid = (mask.reshape(nxg, NY * NZ) == 0)
    allpos = ref.cells.positions
    nrbc = len(cells) * 642
    worst = 0.0
    for key, p_ref in ((("cid", "vid", "pos"), allpos[:nrbc].reshape(len(cells), -1, 3)), (("pcid", "pvid", "ppos"), allpos[nrbc:].reshape(len(plts), -1, 3))):
        for r in res:
            d = r[key[2]] - p_ref[r[key[0]], r[key[1]]]
            if seam:
                d[:, 0] = (d[:, 0] + nxg / 2) % nxg - nxg / 2
            worst = max(worst, np.abs(d).max() if len(d) else 0.0)
    err_f = np.abs(f_all - f_ref)[fluid].max()
    print("slabs vs single domain, reproducible spread: max |df| = %.3e, max |dx| = %.3e" % (err_f, worst))
    if seam:
        assert err_f <= 1e-12 and worst <= 1e-11, (err_f, worst)
    else:
        assert err_f == 0.0 and worst == 0.0, (err_f, worst)
    if world in (2, 3):
        err_o = _observables_error(ref, res, nxg, fluid)
        assert max(err_o) <= (1e-12 if seam else 0.0), err_o
    assert sum(r["stats"]["cells_new"] + r["stats"]["cells_dropped"] for r in res) > 0


@pytest.mark.parametrize("world,rep,padded", [(2, False, False), (3, False, False), (4, False, False), (2, True, False), (2, True, True)])
def test_slabs_match_single_domain(tmp_path, gpu, world, rep, padded):
    """the default (atomic) spread.  rep: vertex-vertex and boundary-particle repulsion on (cell records then carry
    force_repulsion); padded: the slabs (not the single-domain reference run) use the padded x-plane stride"""
    nxg = 192 if world == 4 else NXG          # a slab that carries cells is at least 40 planes wide
    res = _spawn(world, tmp_path, dict(rep=rep, padded=padded, nxg=nxg), salt=2 * rep + padded)
    ref, mask = _build(0, 1, rep, nxg=nxg)
    ref.run(STEPS)
    if rep:
        assert np.abs(ref.cells.repulsion_forces).max() > 0   # the repulsions do act in this case
    f_ref = ref.lattice.populations().reshape(nxg, NY * NZ, 19)
    f_two = np.concatenate([r["f"].reshape(nxg // world, NY * NZ, 19) for r in res], axis=0)
    fluid = (mask.reshape(nxg, NY * NZ) == 0)
    err_f = np.abs(f_two - f_ref)[fluid].max()
    if world in (2, 3):
        err_o = _observables_error(ref, res, nxg, fluid)
        assert max(err_o) <= 5e-12, err_o
    # both runs add the spread forces with fp64 atomics in whatever order the hardware takes them, so two runs of the SAME
    # configuration already differ in the last bits and drift apart over the 250 steps: seen 0.3e-12 ... 1.2e-12 from run to run
    # (populations are O(0.1); north_star asks for 1e-6).  The comparison without that noise is
    # test_slabs_equal_single_domain_bit_for_bit above (reproducible spread: exact)
    assert err_f <= 5e-12, err_f
    allpos = ref.cells.positions
    nrbc = len(CELLS) * 642
    worst = 0.0
    for key, p_ref in ((("cid", "vid", "pos"), allpos[:nrbc].reshape(len(CELLS), -1, 3)), (("pcid", "pvid", "ppos"), allpos[nrbc:].reshape(len(PLTS), -1, 3))):
        seen = np.zeros(p_ref.shape[:2], dtype=int)
        for r in res:
            d = r[key[2]] - p_ref[r[key[0]], r[key[1]]]
            d[:, 0] = (d[:, 0] + nxg / 2) % nxg - nxg / 2
            worst = max(worst, np.abs(d).max() if len(d) else 0.0)     # a rank may own no vertex of a type
            np.add.at(seen, (r[key[0]], r[key[1]]), 1)
        assert (seen == 1).all()          # every vertex owned by exactly one rank
    assert worst <= 1e-10, worst          # weights are formed in global coordinates: only the order of the force sums differs
    assert sum(int(r["held"]) for r in res) > len(CELLS) + len(PLTS)   # cells near the faces are replicated
    n_new, n_drop = sum(r["stats"]["cells_new"] for r in res), sum(r["stats"]["cells_dropped"] for r in res)
    assert n_new + n_drop > 0                      # envelope copies changed hands during the run
    if world == 2:
        assert n_new > 0 and n_drop > 0            # both a fresh copy and a dropped copy (faces at x = 72 and the seam)
    assert all(r["stats"]["iterations"] == STEPS and r["stats"]["particle_steps"] == STEPS // K_P for r in res)
    # diagnostics reduced over the slabs equal those of the single domain (same values on every rank)
    ref_stats = (ref.fluid_stats(0), ref.vertex_stats(1), ref.vertex_stats(2))
    for r in res:
        for got, want in zip(r["gstats"], ref_stats):
            assert got[3] == want[3]                                          # same number of nodes / owned vertices
            assert np.allclose(got[:3], want[:3], rtol=1e-6, atol=1e-18), (got, want)
    travelled = np.abs(allpos[:, 0] - _initial_x()).max()
    assert travelled > 5.0, travelled


def _oracle_run(orc, nxg, steps, cells=CELLS, plts=PLTS, force=FORCE, k_p=K_P, k_m=K_M, push=None, delete_at_updates=False):
    """the reference's answer for ANY rank count is the one global block: the oracle on the whole pipe (orc_sim_iterate,
    core/hemoCell.cpp:299-376).  delete_at_updates: the reference run with verbose.cellsDeletedInfo
    (core/hemoCell.cpp:360-363: deleteIncompleteCells at the end of every velocity-update iteration), which is what the
    slab runs do.  -> (populations [n][19], positions, alive flags, lattice, sim)"""
    import ctypes as C

    from hemocell_amd import host
    from oracle import oracle as O
    Po = O.make_params(orc)
    mask, _ = host.pipe_mask(nxg, NY, NZ)
    Lo = O.OracleLattice(orc, nxg, NY, NZ, (1, 0, 0), 1.0 / Po.tau)
    Lo.set_mask(mask); Lo.init_equilibrium(); Lo.set_threads(8)
    So = orc.orc_sim_create(Lo.ptr, C.byref(Po))
    for mk in (O.make_rbc, O.make_plt):
        T = mk(orc, Po); T.contents.timescale = k_m
        orc.orc_sim_add_type(So, T)
    So.contents.particle_velocity_timescale = k_p
    for t, group in ((0, cells), (1, plts)):
        for c, a in group:
            a_ref = np.array(a, dtype=np.float64) * (3.14159265358979323846 / 180.0) * -1.0
            assert orc.orc_sim_add_cell(So, t, O.dptr(np.array(c, dtype=np.float64)), O.dptr(a_ref), 0.0) == 1
    Lo.set_force_uniform(force)
    for d in range(3):
        So.contents.body_force[d] = force[d]
    orc.orc_sim_mechanics(So, 1)
    for it in range(steps):
        orc.orc_sim_iterate(So)
        if delete_at_updates and it % k_p == 0:
            orc.orc_sim_delete_incomplete_cells(So)
        if it == 0 and push is not None:           # _run(): after iteration 0 has interpolated, that cell gets a held velocity
            vel = np.zeros((So.contents.np, 3)); orc.orc_sim_get(So, 1, O.dptr(vel))
            nv = 642
            vel[push[0] * nv:(push[0] + 1) * nv] = np.array(push[1])
            orc.orc_sim_set(So, 1, O.dptr(vel))
    pos = np.zeros((So.contents.np, 3)); orc.orc_sim_get(So, 0, O.dptr(pos))
    alive = np.zeros(So.contents.np, dtype=np.uint8); orc.orc_sim_get_alive(So, alive.ctypes.data)
    return Lo.f.copy(), pos, alive.astype(bool), mask


def test_slabs_with_the_reproducible_spread_match_the_oracle(tmp_path, gpu, orc, reproducible_spread):
    """the same comparison with the gather-form spread: what is left is the oracle adding each contribution to the body force
    where the kernels add their sum to it, and the platelet law's atan2"""
    steps = 120
    res = _spawn(3, tmp_path, dict(), steps=steps, salt=27)
    f_o, p_o, alive, mask = _oracle_run(orc, NXG, steps)
    f_s = np.concatenate([r["f"].reshape(NXG // 3, NY * NZ, 19) for r in res], axis=0)
    fluid = (mask.reshape(NXG, NY * NZ) == 0)
    err_f = np.abs(f_s - f_o.reshape(NXG, NY * NZ, 19))[fluid].max()
    nrbc = len(CELLS) * 642
    worst = 0.0
    for key, p_ref in ((("cid", "vid", "pos"), p_o[:nrbc].reshape(len(CELLS), -1, 3)), (("pcid", "pvid", "ppos"), p_o[nrbc:].reshape(len(PLTS), -1, 3))):
        for r in res:
            d = r[key[2]] - p_ref[r[key[0]], r[key[1]]]
            d[:, 0] = (d[:, 0] + NXG / 2) % NXG - NXG / 2
            worst = max(worst, np.abs(d).max() if len(d) else 0.0)
    print("3 slabs, reproducible spread, vs the oracle: max |df| = %.3e, max |dx| = %.3e" % (err_f, worst))
    assert err_f <= 1e-11 and worst <= 1e-9, (err_f, worst)


@pytest.mark.parametrize("world", [2, 3])
def test_slabs_match_the_oracle(tmp_path, gpu, orc, world):
    """row a12 against the ORACLE, not against the HIP single domain: the reference's result does not depend on the number
    of ranks (scripts/ci/pipeflow_sanity.sh:25-33), so N slabs must give what the oracle gives on the one global block --
    RBC + PLT, cadence (4, 2), a cell across the periodic seam and cells across the interior faces (x = 72; x = 48 and 96),
    envelope copies created and dropped on the way (core/hemoCellFields.cpp:377-499, periodic shift
    core/hemoCellParticleDataTransfer.cpp:33-65, merge core/hemoCellParticleField.cpp:173-235).  Same tolerance as the single
    domain meets in test_iterate_trajectories_vs_oracle: 1e-9 on positions (north_star asks for 1e-6 relative)."""
    steps = 120
    res = _spawn(world, tmp_path, dict(), steps=steps, salt=20 + world)
    f_o, p_o, alive, mask = _oracle_run(orc, NXG, steps)
    assert alive.all()
    f_s = np.concatenate([r["f"].reshape(NXG // world, NY * NZ, 19) for r in res], axis=0)
    fluid = (mask.reshape(NXG, NY * NZ) == 0)
    f_o = f_o.reshape(NXG, NY * NZ, 19)
    err_f = np.abs(f_s - f_o)[fluid].max()
    assert err_f <= 1e-6 * np.abs(f_o[fluid]).max()
    assert err_f <= 1e-11, err_f
    nrbc = len(CELLS) * 642
    worst, moved = 0.0, 0.0
    for key, p_ref in ((("cid", "vid", "pos"), p_o[:nrbc].reshape(len(CELLS), -1, 3)), (("pcid", "pvid", "ppos"), p_o[nrbc:].reshape(len(PLTS), -1, 3))):
        seen = np.zeros(p_ref.shape[:2], dtype=int)
        for r in res:
            d = r[key[2]] - p_ref[r[key[0]], r[key[1]]]
            d[:, 0] = (d[:, 0] + NXG / 2) % NXG - NXG / 2       # the oracle keeps global unwrapped positions too; a slab may hold the image
            worst = max(worst, np.abs(d).max() if len(d) else 0.0)
            np.add.at(seen, (r[key[0]], r[key[1]]), 1)
        assert (seen == 1).all()
    assert worst <= 1e-9, worst
    assert sum(int(r["held"]) for r in res) > len(CELLS) + len(PLTS)
    assert sum(r["stats"]["cells_new"] + r["stats"]["cells_dropped"] for r in res) > 0      # copies changed hands
    assert np.abs(p_o[:, 0] - _initial_x()).max() > 1.5                                       # and the cells did travel


def test_wall_deletion_on_slabs_matches_the_oracle(tmp_path, gpu, orc):
    """a cell pushed into the pipe wall next to the slab face (both ranks hold a copy), reference deletion semantics
    (single particles leave, core/hemoCellParticleField.cpp:566-588; the remnant goes at the next velocity update,
    core/hemoCell.cpp:360-363): the two slabs against the oracle on the global block"""
    kw = dict(cells=WALL_CELLS, plts=[], force=(1e-5, 0.0, 0.0), del_mode="particle", k_p=60)
    push = (1, (0.0, 0.0, 0.1))
    steps = 100
    res = _spawn(2, tmp_path, dict(kw, push=push), steps=steps, salt=31)
    f_o, p_o, alive, mask = _oracle_run(orc, NXG, steps, cells=WALL_CELLS, plts=[], force=kw["force"], k_p=60, push=push, delete_at_updates=True)
    assert len(p_o) == 642                                              # the oracle lost the wall cell as well
    got = np.concatenate([r["pos"] for r in res]); cid = np.concatenate([r["cid"] for r in res]); vid = np.concatenate([r["vid"] for r in res])
    assert (cid == 0).all() and sorted(vid.tolist()) == list(range(642))
    assert np.abs(got - p_o[vid]).max() <= 1e-9
    f_s = np.concatenate([r["f"].reshape(NXG // 2, NY * NZ, 19) for r in res], axis=0)
    fluid = (mask.reshape(NXG, NY * NZ) == 0)
    err_f = np.abs(f_s - f_o.reshape(NXG, NY * NZ, 19))[fluid].max()
    assert err_f <= 1e-11, err_f


# sub-domain forces (cases/kolmogorovFlow/kolmogorovFlow.cpp:136-140): one box across the slab face at x = 72, one across the seam
# (two boxes, since a box does not wrap), one inside a slab that overrides part of the first
REGIONS = [((40, 100, 0, NY - 1, 0, NZ - 1), (1e-4, 0.0, 2e-5)), ((130, NXG - 1, 0, NY - 1, 0, NZ // 2), (-2e-4, 1e-5, 0.0)),
           ((0, 12, 0, NY - 1, 0, NZ // 2), (-2e-4, 1e-5, 0.0)), ((60, 80, 10, 20, 0, NZ - 1), (0.0, 0.0, -3e-5))]


def test_slabs_with_subdomain_forces_match_single_domain(tmp_path, gpu):
    res = _spawn(2, tmp_path, dict(regions=REGIONS), steps=120, salt=7)
    ref, mask = _build(0, 1, regions=REGIONS)
    ref.run(120)
    f_ref = ref.lattice.populations().reshape(NXG, NY * NZ, 19)
    f_two = np.concatenate([r["f"].reshape(NXG // 2, NY * NZ, 19) for r in res], axis=0)
    fluid = (mask.reshape(NXG, NY * NZ) == 0)
    assert np.abs(f_two - f_ref)[fluid].max() <= 5e-12
    plain, _ = _build(0, 1)
    plain.run(120)
    assert np.abs(plain.lattice.populations().reshape(NXG, NY * NZ, 19) - f_ref)[fluid].max() > 1e-6     # the boxes do act
    allpos = ref.cells.positions
    nrbc = len(CELLS) * 642
    for r in res:
        d = r["pos"] - allpos[:nrbc].reshape(len(CELLS), -1, 3)[r["cid"], r["vid"]]
        d[:, 0] = (d[:, 0] + NXG / 2) % NXG - NXG / 2
        assert np.abs(d).max() <= 1e-10




@pytest.mark.parametrize("mode", ["cell", "particle"])
def test_cell_reaching_the_wall_is_deleted_on_every_holder(tmp_path, gpu, mode):
    kw = dict(cells=WALL_CELLS, plts=[], force=(1e-5, 0.0, 0.0), del_mode=mode, k_p=60)
    push = (1, (0.0, 0.0, 0.1))
    steps = 100
    res = _spawn(2, tmp_path, dict(kw, push=push), steps=steps, salt=11 + (mode == "cell"))
    ref, mask = _build(0, 1, **kw)
    _run(ref, steps, push)
    nv, nc, nd = ref.cells.counts()
    if mode == "particle":
        assert nc == 2 and ref.cells.deletion_counts()[2:] [0] == 1          # the reference keeps the remnants until deleteIncompleteCells
        nd += ref.cells.deleteIncompleteCells(); nc = ref.cells.counts()[1]
    assert nc == 1 and nd == 1, (nc, nd)                                   # the single domain lost exactly the wall cell
    assert sum(int(r["held"]) for r in res) == 1                           # ... and so did the slabs: no copy lingers on either rank
    assert sum(r["stats"]["cells_deleted"] for r in res) == 2              # one copy on each side of the face
    # the surviving cell is where the single domain has it (the other one is 39 lu away)
    p_ref = ref.cells.positions.reshape(1, -1, 3)
    got = np.concatenate([r["pos"] for r in res]); cid = np.concatenate([r["cid"] for r in res]); vid = np.concatenate([r["vid"] for r in res])
    assert (cid == 0).all() and sorted(vid.tolist()) == list(range(642))
    assert np.abs(got - p_ref[0, vid]).max() <= 1e-9


def test_cell_compacted_between_synchronisations_stays_deleted(tmp_path, gpu):
    """the wall contact happens after the last velocity update (iteration 0; the next one is iteration 60) and
    the host then looks at the cells (writeOutput: deleteIncompleteCells + counts, iteration 58), which compacts the gone cell
    away on the rank that saw the wall -- the other holder's copy must not come back as a fresh complete cell at iteration 60"""
    kw = dict(cells=WALL_CELLS, plts=[], force=(1e-5, 0.0, 0.0), del_mode="particle", k_p=60)
    res = _spawn(2, tmp_path, dict(kw, push=(1, (0.0, 0.0, 0.1)), query_at=58), steps=100, salt=41)
    assert sum(int(r["held"]) for r in res) == 1                           # no copy lingers or returns
    assert 1 <= sum(int(r["deleted"]) for r in res) <= 2                   # each holder counts its own copy once
    cid = np.concatenate([r["cid"] for r in res]); vid = np.concatenate([r["vid"] for r in res])
    assert (cid == 0).all() and sorted(vid.tolist()) == list(range(642))


# <particleEnvelope> (core/hemoCell.cpp:139): cell 1 is given a held velocity of 0.25 lu per iteration along the pipe; velocities
# are refreshed (and envelopes synchronised) every 60 iterations, so it travels 15 lu between two synchronisations and crosses the face
# at x = 72 from 12 lu away
FAST_CELLS = [((20.0, 16.5, 16.5), (90, 0, 0)), ((52.0, 16.5, 16.5), (90, 0, 0))]


@pytest.mark.parametrize("envelope,ok", [(None, False), (25, False), (36, True)])
def test_particle_envelope_knob_and_device_check(tmp_path, gpu, envelope, ok):
    """the default (4 lu) and <particleEnvelope> 25 (25 - 15.6 = 9.4 lu for an RBC) are too small for 15 lu per velocity update:
    the copy reaches the neighbour with particles already on its side, the merge kernel counts them and hc_iterate fails with
    the envelope named; <particleEnvelope> 36 (20.4 lu, clamped to what a 72-plane slab supports) carries the same run, and
    the result is the single domain's"""
    kw = dict(cells=FAST_CELLS, plts=[], force=(1e-5, 0.0, 0.0), k_p=60, envelope=envelope)
    push = (1, (0.25, 0.0, 0.0))
    steps = 70
    res = _spawn(2, tmp_path, dict(kw, push=push, expect_error=not ok), steps=steps, salt=51 + (envelope or 0))
    share = [float(r["envelope"][0]) for r in res]
    assert share[0] == share[1] and abs(share[0] - {None: 4.0, 25: 25 - 15.64, 36: 36 - 15.64}[envelope]) < 0.1, share
    if not ok:
        errs = [str(r["error"]) for r in res]
        assert any("particle envelope too small" in e for e in errs), errs
        assert sum(int(r["envelope"][1]) for r in res) > 0
        return
    assert all(str(r["error"]) == "" and int(r["envelope"][1]) == 0 for r in res)
    ref, mask = _build(0, 1, **kw)
    _run(ref, steps, push)
    p_ref = ref.cells.positions.reshape(2, -1, 3)
    seen = np.zeros((2, 642), dtype=int)
    for r in res:
        d = r["pos"] - p_ref[r["cid"], r["vid"]]
        assert np.abs(d).max() <= 1e-10
        np.add.at(seen, (r["cid"], r["vid"]), 1)
    assert (seen == 1).all()
    assert p_ref[1, :, 0].max() > 73.0                                                  # it did cross the face at x = 72


def test_envelope_argument_checks(gpu):
    """hcp_set_envelope: before the first cell, after the cell types, positive; on one GPU the value is kept as it is"""
    P = gpu.base_parameters()
    L = gpu.Lattice(48, NY, NZ, (1, 0, 0), 1.0 / P.tau)
    mask, _ = gpu.pipe_mask(48, NY, NZ)
    L.defineBounceBack(mask); L.latticeEquilibrium()
    h = gpu.HemoCell(L, P); cf = h.cellfields
    lib = gpu.capi.lib()
    import ctypes as C
    used = C.c_double()
    with pytest.raises(gpu.capi.HcError, match="cell types first"):
        gpu.check(lib.hcp_set_envelope(cf.ptr, 25.0, C.byref(used)))
    cf.addCellType(gpu.CellType.rbc(P), 1)
    with pytest.raises(gpu.capi.HcError, match="positive"):
        gpu.check(lib.hcp_set_envelope(cf.ptr, -1.0, C.byref(used)))
    gpu.check(lib.hcp_set_envelope(cf.ptr, 25.0, C.byref(used)))
    assert abs(used.value - (25.0 - 15.64)) < 0.1                    # envelope minus the RBC's diameter at dx = 0.5 um
    gpu.check(lib.hcp_set_envelope(cf.ptr, 10.0, C.byref(used)))
    assert used.value == 2.0                                          # never below what the IBM stencil needs
    late = C.c_long(-1)
    gpu.check(lib.hcp_envelope(cf.ptr, C.byref(used), C.byref(late)))
    assert used.value == 2.0 and late.value == 0
    assert cf.addCell(0, (24.0, 16.5, 16.5), (90, 0, 0))
    with pytest.raises(gpu.capi.HcError, match="before the first cell"):
        gpu.check(lib.hcp_set_envelope(cf.ptr, 25.0, C.byref(used)))
    L.destroy()


def test_slab_schedule_over_rccl_matches_hc_iterate(gpu):
    """the real data plane of N > 1 runs (ncclSend / ncclRecv over librccl) on the one GPU of the test box: a single rank that
    is its own periodic neighbour sends to and receives from itself; examples/rccl_selfloop.py asserts that the native slab
    schedule then reproduces hc_iterate (own process: one world per process)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "rccl_selfloop.py"), "128", "30"], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "max |df|" in r.stdout and "slab schedule over RCCL" in r.stdout
