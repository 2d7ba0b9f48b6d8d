"""The output-path kernels against tests/observables_ref.py (extended precision): rho_u / pi_neq (HDF5 Velocity, Density,
ShearStress, StrainRate), fluid_stats (FluidInfo), cell_info (CellInfo CSV, stretch and volume prints), vertex_stats
(ParticleInfo) and the facade's CellInformationFunctionals.

Tolerance: every component |gpu - ref| <= 16 * 2^-53 * sum|terms| (observables_ref returns the sum of the magnitudes of the
terms of each value); min, max, counts and bounding boxes exactly.  Every comparison also runs a mutation control: the same
comparison against a deliberately wrong restatement must miss by orders of magnitude, or the bound could not see a wrong
kernel."""
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest

from tests import observables_ref as R
from oracle import oracle as O
from tests.test_gpu_parity import _add_both, _both_lattices, _oracle_state, _random_populations, _sim_pair

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

MUTATION = 1e3      # a wrong restatement must miss the bound by at least this factor

SHAPES = [(7, 5, 9), (16, 16, 16), (11, 19, 23)]          # plane < one 256-thread block, a power of two, a plane of 437 nodes
PERIODIC = [(1, 1, 1), (1, 0, 0), (0, 0, 0), (0, 1, 1)]
FLUID_CASES = ["box-%dx%dx%d-%d%d%d" % (s + p) for s in SHAPES for p in PERIODIC] + ["pipe_moving_wall", "force_boxes", "cells"]


def _walls(shape, periodic):
    nx, ny, nz = shape
    mask = np.zeros(shape, np.uint8)
    for d, per in enumerate(periodic):
        if not per:
            sl = [slice(None)] * 3
            sl[d] = 0; mask[tuple(sl)] = 1
            sl[d] = -1; mask[tuple(sl)] = 1
    mask[nx // 2, ny // 2 - 1:ny // 2 + 1, nz // 2 - 1:nz // 2 + 2] = 1    # an obstacle inside
    return mask


def _fluid_case(orc, gpu, case):
    """-> (Lg, f, F, mask, periodic, cleanup): the GPU lattice after a few steps and the inputs of the restatement"""
    rng = np.random.default_rng(zlib.crc32(case.encode()))
    if case == "cells":
        # coupled: the force field read right after a spread (the collide consumes it).  The spread sums in hardware order, so
        # the oracle's field agrees only to ~1e-14; the inputs are the GPU's own populations and Fin, checked against the oracle
        # at that level
        nx, ny, nz = 40, 30, 30
        mask, _ = gpu.pipe_mask(nx, ny, nz)
        Po, Lo, Lg, So, hg = _sim_pair(orc, gpu, nx, ny, nz, (1, 0, 0), mask, k_m=2, k_p=1)
        assert _add_both(orc, So, hg, 0, (38.5, 14.2, 15.1), (90, 0, 0)) and _add_both(orc, So, hg, 0, (18.0, 14.5, 12.0), (90, 20, 0))
        F = (2e-5, 0.0, 0.0)
        Lo.set_force_uniform(F); Lg.setExternalVector(F)
        So.contents.body_force[0], So.contents.body_force[1], So.contents.body_force[2] = F
        pos = _oracle_state(orc, So)[0]
        pos = pos + 0.03 * rng.standard_normal(pos.shape)                  # deformed membranes: spread forces well above rounding
        orc.orc_sim_set(So, 0, O.dptr(pos)); hg.cellfields.positions = pos
        orc.orc_sim_mechanics(So, 1); hg.cellfields.applyConstitutiveModel(0, True)
        for _ in range(5):
            orc.orc_sim_iterate(So)
        hg.iterate(5)
        orc.orc_sim_spread(So); hg.cellfields.spreadParticleForce(True)
        f = Lg.populations()
        Fin = Lg.ibm_force()
        fluid = mask.reshape(-1) == 0
        assert np.abs(Fin[fluid]).max() > 0                                  # the spread force is there when read
        assert np.abs(f[fluid] - Lo.f[fluid]).max() <= 1e-13
        Ftot = np.array(F)[None, :] + Fin
        assert np.abs(Ftot[fluid] - Lo.force[fluid]).max() <= 1e-13 * np.abs(Lo.force).max()
        Lg.body_only = np.broadcast_to(np.array(F), Ftot.shape)          # for the mutation control that drops Fin
        return Lg, f, Ftot, mask, (1, 0, 0), lambda: (Lo.destroy(), Lg.destroy())
    if case == "pipe_moving_wall":
        shape, periodic = (12, 14, 14), (1, 0, 0)
        mask, _ = gpu.pipe_mask(*shape)
        mask[:, :2, :][mask[:, :2, :] == 1] = 3                              # one moving-wall class (Ladd bounce-back)
        Lo, Lg = _both_lattices(orc, gpu, *shape, periodic, 1.0 / 0.8, mask)
        Lo.set_wall_velocity(0, (0.01, 0.0, -0.003)); Lg.setBoundaryVelocity(3, (0.01, 0.0, -0.003))
        F = (2e-6, 1e-7, 0.0)
        Lo.set_force_uniform(F); Lg.setExternalVector(F)
    elif case == "force_boxes":
        shape, periodic = (16, 12, 10), (1, 1, 1)
        mask = _walls(shape, periodic)
        Lo, Lg = _both_lattices(orc, gpu, *shape, periodic, 1.0 / 0.9, mask)
        F = (1e-6, 0.0, 0.0)
        boxes = [((0, 7, 0, 11, 0, 9), (3e-5, -1e-5, 2e-6)), ((4, 11, 2, 5, 3, 8), (-2e-5, 4e-6, 1e-5))]
        Lo.set_force_uniform(F); Lg.setExternalVector(F)
        Lg.setExternalVectorBoxes([b for b, _ in boxes], [f for _, f in boxes])
        for b, f in boxes:
            Lo.set_force_box(b, f)
    else:
        dims = case.split("-")
        shape = tuple(int(v) for v in dims[1].split("x"))
        periodic = tuple(int(c) for c in dims[2])
        mask = _walls(shape, periodic)
        Lo, Lg = _both_lattices(orc, gpu, *shape, periodic, 1.0 / 0.9, mask)
        F = (1e-5, -2e-6, 3e-6)
        Lo.set_force_uniform(F); Lg.setExternalVector(F)
    n = int(np.prod(shape))
    f0 = _random_populations(rng, n)
    Lo.f[:] = f0
    Lg.set_populations(f0)
    Lo.collide_stream(3); Lg.collideAndStream(3)
    fg = Lg.populations()
    fluid = mask.reshape(-1) == 0
    assert np.array_equal(fg[fluid], Lo.f[fluid])                            # the step path is pinned bit for bit elsewhere
    # the oracle's state on the fluid nodes; on wall nodes its rows are not the GPU's storage (the parity suite pins fluid rows
    # only), so there the GPU's own post-stream rows are the input -- what rho_u / pi_neq pull there is what they hold
    f = Lo.f.copy()
    f[~fluid] = fg[~fluid]
    return Lg, f, Lo.force.copy(), mask, periodic, lambda: (Lo.destroy(), Lg.destroy())


def _magnitude(v):
    return np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])    # the kernels' order of operations


@pytest.fixture(params=[False, True], ids=["plain", "padded"])
def padded(request, gpu):
    """the padded x-plane stride (hc_lattice::xs), forced the way test_padded_plane_stride does it"""
    lib = gpu.capi.lib()
    gpu.check(lib.hc_debug_force_plane_padding(1 if request.param else 0))
    yield request.param
    gpu.check(lib.hc_debug_force_plane_padding(0))


@pytest.mark.parametrize("case", FLUID_CASES)
def test_fluid_fields_and_statistics_vs_restatement(orc, gpu, padded, case):
    """Lattice.rho_u / pi_neq on every node, fluid and wall, and fluid_stats(0/1/2) over their node sets"""
    Lg, f, F, mask, periodic, cleanup = _fluid_case(orc, gpu, case)
    try:
        rho, u = Lg.rho_u()
        pi = Lg.pi_neq()
        ru, pn = R.rho_u(f, F), R.pi_neq(f)
        err = dict(rho=R.excess(rho, ru["rho"], ru["rho_abs"]), u=R.excess(u, ru["u"], ru["u_abs"]), pi=R.excess(pi, pn["pi"], pn["pi_abs"]))
        assert max(err.values()) <= 1, err
        mut = dict(no_half_force=R.excess(u, R.rho_u(f, F, wrong="no_half_force")["u"], ru["u_abs"]),
                   swap_xy_xz=R.excess(pi, R.pi_neq(f, wrong="swap_xy_xz")["pi"], pn["pi_abs"]),
                   no_cs2=R.excess(pi, R.pi_neq(f, wrong="no_cs2")["pi"], pn["pi_abs"]))
        if case == "cells":
            mut["no_spread_force"] = R.excess(u, R.rho_u(f, Lg.body_only)["u"], ru["u_abs"])
        assert min(mut.values()) > MUTATION, mut
        print("%s: excess %s, mutations %s" % (case, {k: "%.3g" % v for k, v in err.items()}, {k: "%.3g" % v for k, v in mut.items()}))
        # FluidInfo: |u| and |F| over the non-boundary nodes
        fluid = mask.reshape(-1) == 0
        for what, vec, vabs in ((0, ru["u"], ru["u_abs"]), (1, F, np.abs(F))):
            mn, mx, avg, n = Lg.fluid_stats(what)
            m_ref = _magnitude(vec[fluid])
            bound = 16 * 2.0 ** -53 * _magnitude(vabs[fluid]) + 2.0 ** -52 * m_ref
            assert n == fluid.sum()
            if what == 1:           # the force field is data, not a sum: exact
                assert mn == m_ref.min() and mx == m_ref.max()
            else:
                own = _magnitude(u[fluid])      # the same expression on the downloaded field: bit for bit
                assert mn == own.min() and mx == own.max()
                assert abs(mn - m_ref.min()) <= bound.max() and abs(mx - m_ref.max()) <= bound.max()
            assert abs(avg - m_ref.mean()) <= bound.max() + 1e-14 * m_ref.mean()
        if periodic == (1, 1, 1):
            # mass: the stored populations of every bulk node, P(x, i) = S(x + c_i, i) -- on a fully periodic lattice every stored
            # value is some node's post-stream value
            f4 = R.hp(f).reshape(Lg.nx, Lg.ny, Lg.nz, 19)
            mass = sum(np.roll(f4[..., q], tuple(-R.C[q]), axis=(0, 1, 2)) for q in range(19)).reshape(-1)
            mass_abs = sum(np.roll(np.abs(f4[..., q]), tuple(-R.C[q]), axis=(0, 1, 2)) for q in range(19)).reshape(-1)
            mn, mx, avg, n = Lg.fluid_stats(2)
            assert n == Lg.n
            ref = R.to_double(mass)
            b = 16 * 2.0 ** -53 * R.to_double(mass_abs).max()
            assert abs(mn - ref.min()) <= b and abs(mx - ref.max()) <= b and abs(avg - ref.mean()) <= b
    finally:
        cleanup()


# ---------------------------------------------------------------------------------------------------------- cell information
MALARIA_CASE = os.path.join(ROOT, "tests", "golden", "malaria_case")
STLS = {"stretch": os.path.join(MALARIA_CASE, "vRBC_uniform.stl"), "pipeflow": os.path.join(MALARIA_CASE, "vRBC_uniform_pipeflowMalaria.stl")}
MESHES = {"RBC": lambda gpu, P: gpu.CellType.rbc(P),
          "PLT_ELL": lambda gpu, P: gpu.CellType.plt(P),                       # ELLIPSOID_FROM_SPHERE, the octasphere
          "WBC_SPHERE": lambda gpu, P: gpu.CellType.wbc(P),
          "MALARIA_STRETCH": lambda gpu, P: gpu.CellType.malaria(P, stl=STLS["stretch"]),     # wide per-vertex tables
          "MALARIA_PIPEFLOW": lambda gpu, P: gpu.CellType.malaria(P, stl=STLS["pipeflow"]),
          "RBC_FROM_STL": lambda gpu, P: gpu.CellType.rbc(P, stl=STLS["stretch"])}


def _cell_field(gpu, names, per_type, seed):
    P = gpu.base_parameters()
    L = gpu.Lattice(48, 48, 48, (1, 1, 1), 1.0 / P.tau)
    L.latticeEquilibrium()
    cf = gpu.Cells(L, P)
    rng = np.random.default_rng(seed)
    types = []
    for name in names:
        T = MESHES[name](gpu, P)
        t = cf.addCellType(T, 1)
        types.append((t, T))
        for k in range(per_type):
            assert cf.addCell(t, tuple(rng.uniform(14, 34, 3)), tuple(rng.uniform(0, 180, 3)))
    return L, cf, types


def _apply_state(cf, types, state, rng):
    pos = cf.positions
    if state == "perturbed":
        pos = pos + 0.05 * rng.standard_normal(pos.shape)
    elif state in ("stretched", "far"):
        for t, T in types:
            f, n = cf.type_range(t)
            p = pos[f:f + n * T.nv].reshape(n, T.nv, 3)
            if state == "stretched":   # 1.6 x along x about each centroid: the extremes of the bbox move to other vertices
                c = p.mean(axis=1, keepdims=True)
                p[..., 0] = c[..., 0] + 1.6 * (p[..., 0] - c[..., 0])
            else:                      # centred near x = 900 lu: the triple products cancel by five orders of magnitude
                p[..., 0] += 880.0
            pos[f:f + n * T.nv] = p.reshape(-1, 3)
    cf.positions = pos


def _check_types(cf, types, alive=None, wrong="volume_sign"):
    pos = cf.positions
    alive = np.ones(len(pos), bool) if alive is None else alive
    worst, mut = 0.0, np.inf
    for t, T in types:
        f, n = cf.type_range(t)
        if n == 0:
            continue
        tri = T.tables()["triangles"]
        p = pos[f:f + n * T.nv].reshape(n, T.nv, 3)
        a = alive[f:f + n * T.nv].reshape(n, T.nv)
        g = cf.cell_info(t)
        r = R.cell_info(p, tri, a)
        e = dict(volume=R.excess(g["volume"], r["volume"], r["volume_abs"]), area=R.excess(g["area"], r["area"], r["area_abs"]),
                 position=R.excess(g["position"], r["position"], r["position_abs"]))
        assert max(e.values()) <= 1, (t, e)
        assert np.array_equal(g["bbox"], r["bbox"]), (t, np.abs(g["bbox"] - r["bbox"]).max())
        worst = max(worst, max(e.values()))
        w = R.cell_info(p, tri, a, wrong=wrong)
        key = {"volume_sign": "volume", "centroid_over_nv": "position"}[wrong]
        if wrong == "centroid_over_nv":
            a_inc = ~a.all(axis=1)
            mut = min(mut, R.excess(g[key][a_inc], w[key][a_inc], r[key + "_abs"][a_inc]))
        else:
            mut = min(mut, R.excess(g[key], w[key], r[key + "_abs"]))
    assert mut > MUTATION, mut
    return worst, mut


@pytest.mark.parametrize("state", ["rest", "perturbed", "stretched", "far"])
@pytest.mark.parametrize("mesh", list(MESHES) + ["MIXED", "RBC_x37"])
def test_cell_info_vs_restatement(gpu, mesh, state):
    """hcp_cell_info (volume, area, bbox, centroid) of every cell against the restatement: each mesh alone (2 cells), several types
    in one field (first[type] != 0), and 37 cells of one type (not a multiple of 8, more than one workgroup's worth)"""
    if mesh == "MIXED":
        names, per = ["RBC", "PLT_ELL", "WBC_SPHERE", "MALARIA_STRETCH"], 3
    elif mesh == "RBC_x37":
        names, per = ["RBC"], 37
    else:
        names, per = [mesh], 2
    L, cf, types = _cell_field(gpu, names, per, seed=len(mesh))
    try:
        _apply_state(cf, types, state, np.random.default_rng(11))
        if mesh == "MIXED":
            assert all(cf.type_range(t)[0] > 0 for t, _ in types[1:])
        worst, mut = _check_types(cf, types)
        print("%s/%s: excess %.3g, mutation %.3g" % (mesh, state, worst, mut))
    finally:
        cf.destroy(); L.destroy()
        for _, T in types:
            T.destroy()


def _incomplete_pair(orc, gpu):
    """test_cell_removed_when_it_reaches_the_wall ("particle" mode), stopped at the first particle lost: two RBCs, cell 1 listed
    incomplete, its removed particles still stored at their last positions"""
    nx, ny, nz = 40, 34, 34
    mask, R_ = gpu.pipe_mask(nx, ny, nz)
    Po, Lo, Lg, So, hg = _sim_pair(orc, gpu, nx, ny, nz, (1, 0, 0), mask, k_p=1000, k_m=3)
    hg.cellfields.setDeletionMode("particle")
    assert _add_both(orc, So, hg, 0, (12.0, 16.5, 16.5), (90, 0, 0))
    assert _add_both(orc, So, hg, 0, (30.0, 16.5, 25.0), (90, 0, 0))
    nv = 642
    hg.cellfields.applyConstitutiveModel(0, True)
    hg.iterate(1)
    vel = np.zeros((2 * nv, 3)); vel[nv:, 2] = 0.05
    hg.cellfields.velocities = vel
    for it in range(1, 400):
        hg.iterate(1)
        if hg.cellfields.deletion_counts()[2]:
            break
    cf = hg.cellfields
    assert cf.deletion_counts()[2] == 1 and cf.counts() == (2 * nv, 2, 0)
    return Lo, Lg, hg, cf, nv


def test_incomplete_cell_info_and_vertex_stats(orc, gpu):
    """a cell that lost particles at a wall, before deleteIncompleteCells: centroid and bbox over the particles left (CellPosition,
    helper/cellInfo.cpp:82-100), ParticleInfo over them (helper/particleInfo.cpp), the complete cell unchanged; afterwards the
    info lists exactly the survivors"""
    Lo, Lg, hg, cf, nv = _incomplete_pair(orc, gpu)
    try:
        alive = cf.alive()
        assert alive[:nv].all() and 0 < (~alive[nv:]).sum() < nv
        types = [(0, cf.types[0])]
        pos = cf.positions
        tri = cf.types[0].tables()["triangles"]
        r = R.cell_info(pos.reshape(2, nv, 3), tri, alive.reshape(2, nv))
        g = cf.cell_info(0)
        e = R.excess(g["position"], r["position"], r["position_abs"])
        e_wrong = R.excess(g["position"][1], R.cell_info(pos[nv:], tri, alive[nv:], wrong="centroid_over_nv")["position"], r["position_abs"][1])
        print("incomplete cell: centroid excess %.3g (bound 1), against the centroid over nv %.3g" % (e, e_wrong))
        _check_types(cf, types, alive, wrong="centroid_over_nv")
        # ParticleInfo over the particles left
        for what, arr in ((1, cf.velocities), (2, cf.forces + cf.repulsion_forces)):
            m = _magnitude(arr[alive])
            mn, mx, avg, n = cf.vertex_stats(what)
            assert n == alive.sum() and mn == m.min() and mx == m.max() and abs(avg - m.mean()) <= 1e-14 * m.mean()
        assert cf.deleteIncompleteCells() == 1
        assert cf.cell_ids().tolist() == [0] and cf.counts() == (nv, 1, 1)
        g = cf.cell_info(0)
        assert len(g["volume"]) == 1
        r0 = R.cell_info(cf.positions.reshape(1, nv, 3), tri)
        assert R.excess(g["position"], r0["position"], r0["position_abs"]) <= 1 and np.array_equal(g["bbox"], r0["bbox"])
        assert R.excess(g["volume"], r0["volume"], r0["volume_abs"]) <= 1
    finally:
        Lo.destroy(); Lg.destroy()


def test_facade_cell_information_with_an_incomplete_cell(tmp_path, gpu):
    """CellInformationFunctionals through the facade (tests/drivers/cell_info_incomplete.cpp): the two-argument
    calculateCellInformation and writeCellInfo_CSV leave the incomplete cell out (allCellInformation) and fill stretch; the
    single-property calls run deleteIncompleteCells(false) first, as the reference's do (helper/cellInfo.cpp:263-319)"""
    from tests.test_gpu_compat_driver import _build
    exe = _build(tmp_path, "tests/drivers/cell_info_incomplete.cpp")
    d = str(tmp_path / "case"); shutil.copytree(os.path.join(ROOT, "tests", "golden", "shear_case"), d)
    for fn in os.listdir(d):
        os.chmod(os.path.join(d, fn), 0o644)
    open(os.path.join(d, "RBC.pos"), "w").write("2\n15.0 8.25 8.25 90 0 0\n34.5 8.25 12.5 90 0 0\n")
    r = subprocess.run([exe, "config.xml"], cwd=d, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    lines = [l.split() for l in r.stdout.splitlines()]
    state = [l for l in lines if l[:1] == ["STATE"]][0]
    assert int(state[4]) == 2 and int(state[6]) == 1, state
    tri = np.array([[int(v) for v in l[1:]] for l in lines if l[:1] == ["TRI"]])
    V = np.array([[float(v) for v in l[1:]] for l in lines if l[:1] == ["V"]])
    ids = sorted(set(V[:, 0].astype(int)))
    assert len(ids) == 2
    nv = len(V) // 2
    per = {c: V[V[:, 0] == c] for c in ids}
    ref = {}
    for c in ids:
        v = per[c][np.argsort(per[c][:, 1])]
        ref[c] = R.cell_info(v[:, 3:6], tri, v[:, 2] > 0, v[:, 6:9], stretch=True)
    complete = [c for c in ids if ref[c]["complete"]]
    incomplete = [c for c in ids if not ref[c]["complete"]]
    assert len(complete) == 1 and len(incomplete) == 1
    c0 = complete[0]
    rc = ref[c0]
    info = {int(l[1]): np.array([float(v) for v in l[2:]]) for l in lines if l[:1] == ["INFO"]}
    assert sorted(info) == [c0], info.keys()                             # the incomplete cell is not in the combined call
    vals = info[c0]
    # the facade sums the velocities on the host, one after the other: the worst case of nv sequential adds
    checks = dict(volume=R.excess(vals[0], rc["volume"], rc["volume_abs"]), area=R.excess(vals[1], rc["area"], rc["area_abs"]),
                  position=R.excess(vals[2:5], rc["position"], rc["position_abs"]), stretch=R.excess(vals[5], rc["stretch"], rc["stretch_abs"]),
                  velocity=R.excess(vals[6:9], rc["velocity"], rc["velocity_abs"], k=nv))
    assert max(checks.values()) <= 1, checks
    assert vals[5] > 10.0                                                 # stretch is filled: an RBC is ~15.6 lu across
    assert np.array_equal(vals[9:15], rc["bbox"])
    csv = [l for l in lines if l[:1] == ["CSV"]][0][1]
    rows = [l.split(",") for l in open(os.path.join(d, csv)).read().splitlines()[1:]]
    assert [int(row[6]) for row in rows] == [c0]                         # and not in the CSV
    assert np.allclose([float(v) for v in rows[0][:3]], rc["position"], rtol=1e-5, atol=0)
    assert np.isclose(float(rows[0][4]), rc["volume"], rtol=1e-5)
    # the single-property calls delete the incomplete cell before they look (deleteIncompleteCells(false))
    st = {int(l[1]): float(l[2]) for l in lines if l[:1] == ["STRETCH"]}
    po = {int(l[1]): np.array([float(v) for v in l[2:]]) for l in lines if l[:1] == ["POSITION"]}
    assert sorted(st) == [c0] and sorted(po) == [c0], (st, po)
    assert R.excess(st[c0], rc["stretch"], rc["stretch_abs"]) <= 1 and R.excess(po[c0], rc["position"], rc["position_abs"]) <= 1
    assert "CELLS 1" in r.stdout
