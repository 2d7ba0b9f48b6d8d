"""The three- and four-point IBM kernels (hcp_type_set_ibm_kernel, hemocell_amd/csrc/ibm.hip) against tests/ibm_wide_ref.py,
the extended-precision restatement of the standard phi3 / phi4 inside the reference's interpolationCoefficientsPhi2, on the
crafted geometries of tests/ibm_wide_cases.py.  Every case runs for W = 3 and W = 4 in three kernel forms: per cell (the
default), per vertex (hc_debug_ibm_per_vertex) and the gather form of the spread (hc_set_reproducible_spread).  The oracle
knows two points only; nothing here is compared with it.

Cases (tests/test_ibm_wide_cpu.py asserts with ibm_wide_ref.predict that each sits where it says):
- tile volume <= TILE_CAP3 / TILE_CAP4: tile_19_19_19 and tile_20_20_20 tiled, tile_19_19_20 and tile_20_20_21 take the
  per-vertex path inside the per-cell kernels; node count <= NODE_CAP3 / NODE_CAP4: nodes_2431, nodes_2432 tiled and nodes_2433
  not, nodes_3583, nodes_3584 tiled and nodes_3585 not (disjoint W^3 stencils, the last one partly walled in).
- seams: seam_x, seam_y, seam_z, seam_xyz; a cell leaving a non-periodic face: faces_open; walls that remove part of a stencil:
  walls_7_and_1_of_8, pipe_wall_hug (next to the x seam); positions on nodes and half-nodes and the doubles beside them, both
  signs: exact_positions (there a four-point stencil has an exactly zero weight at f + 2, a three-point one at c + 1, and the
  doubles beside them leave weights at rounding level); removed particles: dead_vertices; FORCE_LIMIT: force_cap.
- types on different kernels in one container: mixed_rbc3_plt4, mixed_rbc2_plt3, mixed_rbc4_plt3, mixed_rbc4_plt2.

Bound: |gpu - ref| <= K 2^-53 abs, K = 16: the rounding figure measured on the CPU
(test_ibm_wide_cpu.py::test_rounding_figure_behind_k) does not exceed 4.  Stencil admission is compared exactly: the nodes the
spread leaves non-zero are the nodes the restatement admits.  Every case must miss the restatement of the other width by 100
bounds, in the spread and in the interpolation."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import ibm_cases as IC
from tests import ibm_wide_cases as WC
from tests import observables_ref as R
from tests.test_gpu_ibm_edges import SENTINEL, _setup
from tests.test_ibm_wide_cpu import FAIL_BY, K, check_expectations, mutation_excess, node_velocities, wrong_kernels

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = ("per_cell", "per_vertex", "gather")
PHI2, PHI3, PHI4 = 2, 3, 4


def _set_kernels(cells, case):
    """the types of the container are the types of the case that have cells, in the order of ibm_cases.TYPES"""
    present = [t for t in IC.TYPES if case["counts"][t]]
    for ti, t in enumerate(present):
        assert cells.ibmKernel(ti) == PHI2
        cells.setIbmKernel(ti, case["kernels"][t])
        assert cells.ibmKernel(ti) == case["kernels"][t]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("W,name", WC.NAMES)
def test_ibm_wide_case(gpu, W, name, form):
    P = gpu.base_parameters()
    case = WC.build(name, W, P.f_limit)
    check_expectations(case)
    lib = gpu.capi.lib()
    pos, frc, alive = case["pos"], case["force"], case["alive"]
    f_limit = P.f_limit if case["limit"] else None
    _, Lg, cells, types = _setup(gpu, case)
    try:
        _set_kernels(cells, case)
        gpu.check(lib.hc_debug_ibm_per_vertex(1 if form == "per_vertex" else 0))
        gpu.check(lib.hc_set_reproducible_spread(1 if form == "gather" else 0))
        # ---- spread
        cells.spreadParticleForce(case["limit"])
        Fg = Lg.ibm_force()
        f_after = cells.forces
        ref = WC.spread_ref(case, f_limit)
        es = R.excess(Fg, ref["F"], ref["F_abs"], K)                              # every node, fluid or not
        ef = R.excess(f_after, ref["force"], ref["force_abs"], K)
        print("%s/%d/%s: spread excess %.3g, capped forces %.3g" % (name, W, form, es, ef))
        assert (Fg[~ref["touched"]] == 0.0).all()                                 # admission, exactly: what the restatement leaves alone is zero ...
        assert (Fg[ref["touched"]] != 0.0).any(axis=1).all()                      # ... and every node it admits received something
        assert es <= 1 and ef <= 1
        assert np.array_equal(f_after[~alive], frc[~alive])                       # removed particles keep their force
        if form == "gather":
            # one sequential double sum per node in (type, cell id, vertex, stencil node) order, added to zero
            dbl = WC.spread_ref(case, f_limit, double=True)
            assert np.array_equal(Fg, dbl["F"]) and np.array_equal(f_after, dbl["force"])
        # ---- interpolate, on the post-stream state the collide leaves and the force it used
        Lg.collideAndStream(1)
        f = Lg.populations()
        cells.interpolateFluidVelocity()
        v = cells.velocities
        u, ua = node_velocities(case, f, Fg + np.array(case["body"])[None, :], extra_kernels=(wrong_kernels(case),))
        rv = WC.interpolate_ref(case, u, ua)
        ev = R.excess(v[alive], rv["v"][alive], rv["v_abs"][alive], K)
        print("%s/%d/%s: interpolation excess %.3g" % (name, W, form, ev))
        assert ev <= 1
        assert (v[~alive] == SENTINEL).all()                                      # removed particles are not written
        if form == "per_cell":
            # the per-cell kernels form the weights and the sums of the per-vertex kernels: the same bits
            gpu.check(lib.hc_debug_ibm_per_vertex(1))
            cells.velocities = np.full(pos.shape, SENTINEL)
            cells.interpolateFluidVelocity()
            assert np.array_equal(cells.velocities, v)
        # ---- the bound can see a wrong kernel: the other width, and each restatement the case names, miss by far
        for wrong, (ws, wv) in mutation_excess(case, f_limit, Fg, v, u, ua).items():
            assert ws > FAIL_BY and (wv is None or wv > FAIL_BY), (name, W, wrong, ws, wv)
        if form == "gather":
            # the gather form repeats bit for bit: the same forces spread again into the next (clean) force buffer
            cells.forces = frc
            cells.spreadParticleForce(case["limit"])
            assert np.array_equal(Lg.ibm_force(), Fg) and np.array_equal(cells.forces, f_after)
    finally:
        gpu.check(lib.hc_debug_ibm_per_vertex(0))
        gpu.check(lib.hc_set_reproducible_spread(0))
        cells.destroy(); Lg.destroy()
        for T in types:
            T.destroy()


# ---- hcp_interpolate_cells: the listed-cells launch of the per-cell kernel
def _listed_cells(gpu, case, calls):
    """calls: (type index, slots of the type, cells of the case those are); after each call exactly the live particles of the
    listed cells hold, bit for bit, what the interpolation of the whole container gave them"""
    lib = gpu.capi.lib()
    alive, sl = case["alive"], IC.cell_slices(case)
    _, Lg, cells, types = _setup(gpu, case)
    try:
        _set_kernels(cells, case)
        Lg.collideAndStream(1)
        cells.interpolateFluidVelocity()
        full = cells.velocities
        assert (full[alive] != SENTINEL).all() and (full[~alive] == SENTINEL).all()
        for ti, slots, listed in calls:
            cells.velocities = np.full(full.shape, SENTINEL)
            s = np.ascontiguousarray(slots, dtype=np.int32)
            gpu.check(lib.hcp_interpolate_cells(cells.ptr, ti, s.ctypes.data_as(C.POINTER(C.c_int)), len(s)))
            v = cells.velocities
            rows = np.zeros(len(full), bool)
            for c in listed:
                rows[sl[c]] = True
            rows &= alive
            assert rows.any() and np.array_equal(v[rows], full[rows])
            assert (v[~rows] == SENTINEL).all()                                   # other cells and removed particles are not written
    finally:
        cells.destroy(); Lg.destroy()
        for T in types:
            T.destroy()


@pytest.mark.parametrize("W", (PHI3, PHI4))
def test_listed_cells_on_wide_kernels(gpu, W):
    """hcp_interpolate_cells on types of three and four points (the slab path, its only caller inside the library, refuses
    them): one RBC on W and two platelets on the other wide kernel, listed one by one and in reverse; then the incomplete cell
    of dead_vertices, whose removed particles keep their velocity."""
    P = gpu.base_parameters()
    case = WC.build("mixed_rbc3_plt4" if W == PHI3 else "mixed_rbc4_plt3", W, P.f_limit)
    assert case["kinds"] == ["rbc", "plt", "plt"]
    _listed_cells(gpu, case, [(1, [1], [2]), (1, [1, 0], [1, 2]), (0, [0], [0])])
    case = WC.build("dead_vertices", W, P.f_limit)
    assert case["kinds"][0] == "rbc" and 0 < case["alive"][IC.cell_slices(case)[0]].sum() < IC.NV["rbc"]
    _listed_cells(gpu, case, [(0, [0], [0])])


# ---- hc_iterate
CH_DIMS, CH_PER, CH_BODY = (32, 24, 24), (True, False, False), (4e-5, 0.0, 1e-5)


def _channel_mask(dims=CH_DIMS):
    m = np.zeros(dims, np.uint8)
    m[:, 0, :] = m[:, -1, :] = 1
    m[:, :, 0] = m[:, :, -1] = 1
    return m


def _channel(gpu, kernels, particle=1, material=1, dims=CH_DIMS, periodic=CH_PER, walls=True):
    """a walled channel along x with one RBC and one PLT; kernels = (RBC's, PLT's), None: the setter is never called"""
    P = gpu.base_parameters()
    L = gpu.Lattice(*dims, periodic, 1.0 / P.tau)
    if walls:
        L.defineBounceBack(_channel_mask(dims))
    L.latticeEquilibrium()
    L.setExternalVector(CH_BODY)
    h = gpu.HemoCell(L, P)
    h.setParticleVelocityUpdateTimeScaleSeparation(particle)
    cf = h.cellfields
    cf.addCellType(gpu.CellType.rbc(P), material)
    cf.addCellType(gpu.CellType.plt(P), material)
    assert cf.addCell(0, (14.3, 11.6, 12.2), (20.0, 0.0, 35.0))
    assert cf.addCell(1, (25.2, 5.1, 17.7), (0.0, 40.0, 0.0))
    for t, k in enumerate(kernels):
        if k is not None:
            cf.setIbmKernel(t, k)
    cf.applyConstitutiveModel(0, True)
    return L, h


def _state(L, h):
    return dict(pos=h.cellfields.positions, vel=h.cellfields.velocities, frc=h.cellfields.forces, f=L.populations())


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("particle,material", [(5, 20), (1, 1)])
def test_iterate_equals_the_phases_one_by_one(gpu, particle, material):
    """40 iterations of hc_iterate on the 32 x 24 x 24 walled channel with the RBC on phi4 and the PLT on phi3 equal the same
    library called phase by phase, bit for bit, with the reproducible spread; and the kernels matter: two points give other bits"""
    lib = gpu.capi.lib()
    gpu.check(lib.hc_set_reproducible_spread(1))
    try:
        L, h = _channel(gpu, (PHI4, PHI3), particle, material)
        try:
            h.iterate(25); h.iterate(15)
            whole = _state(L, h)
        finally:
            h.cellfields.destroy(); L.destroy()
        L, h = _channel(gpu, (PHI4, PHI3), particle, material)
        try:
            cf = h.cellfields
            for it in range(40):
                cf.spreadParticleForce(True)
                L.collideAndStream(1)
                if it % particle == 0:
                    cf.interpolateFluidVelocity()
                cf.advanceParticles(False)
                cf.applyConstitutiveModel(it)
            phased = _state(L, h)
        finally:
            h.cellfields.destroy(); L.destroy()
        assert _same(whole, phased), [k for k in whole if not np.array_equal(whole[k], phased[k])]
        assert np.isfinite(whole["pos"]).all() and np.abs(whole["vel"]).max() > 0
        L, h = _channel(gpu, (PHI2, PHI2), particle, material)
        try:
            h.iterate(40)
            two = _state(L, h)
        finally:
            h.cellfields.destroy(); L.destroy()
        assert not np.array_equal(two["pos"], whole["pos"]) and not np.array_equal(two["f"], whole["f"])
        assert np.abs(two["pos"] - whole["pos"]).max() < 0.05          # another kernel, the same flow
    finally:
        gpu.check(lib.hc_set_reproducible_spread(0))


def test_default_kernel_keeps_its_bits(gpu):
    """a container whose setter is never called, one that sets HC_IBM_PHI2, and one that goes to phi4 / phi3 and back hold the
    same bits after 20 iterations (reproducible spread), and launch the same number of IBM kernels"""
    lib = gpu.capi.lib()
    gpu.check(lib.hc_set_reproducible_spread(1)); gpu.check(lib.hc_profile_enable(1))
    try:
        runs = []
        for kernels in ((None, None), (PHI2, PHI2), "back"):
            L, h = _channel(gpu, (PHI4, PHI3) if kernels == "back" else kernels, 2, 1)
            try:
                if kernels == "back":
                    h.cellfields.setIbmKernel(0, PHI2); h.cellfields.setIbmKernel(1, PHI2)
                assert [h.cellfields.ibmKernel(t) for t in (0, 1)] == [PHI2, PHI2]
                gpu.check(lib.hc_profile_reset())
                h.iterate(20)
                gpu.check(lib.hc_synchronize())
                runs.append((_state(L, h), _profile(lib, "ibm_spread"), _profile(lib, "ibm_interpolate")))
            finally:
                h.cellfields.destroy(); L.destroy()
        for s, ns, ni in runs[1:]:
            assert _same(runs[0][0], s) and (ns, ni) == runs[0][1:]
    finally:
        gpu.check(lib.hc_set_reproducible_spread(0)); gpu.check(lib.hc_profile_enable(0))


def _profile(lib, name):
    import ctypes as C
    ms, n = C.c_double(), C.c_long()
    assert lib.hc_profile_read(name.encode(), C.byref(ms), C.byref(n)) == 0
    return n.value


# ---- combinations that work
def _run_twice_and_on_two_points(gpu, build, n, probe=None):
    """build(kernels) -> (L, h, destroy): the run of n iterations repeats bit for bit on the wide kernels (reproducible spread),
    stays finite, and differs from the run on two points"""
    lib = gpu.capi.lib()
    gpu.check(lib.hc_set_reproducible_spread(1))
    try:
        out = []
        for wide in (True, True, False):
            L, h, destroy = build(wide)
            try:
                h.iterate(n)
                s = _state(L, h)
                if probe is not None:
                    s.update(probe(L, h))
                out.append(s)
            finally:
                destroy()
        assert _same(out[0], out[1]), [k for k in out[0] if not np.array_equal(out[0][k], out[1][k])]
        assert np.isfinite(out[0]["pos"]).all() and np.isfinite(out[0]["f"]).all()
        assert not np.array_equal(out[0]["f"], out[2]["f"])
        return out[0], out[2]
    finally:
        gpu.check(lib.hc_set_reproducible_spread(0))


def _add_unchecked(gpu, cf, t, cell_id, centre):
    gpu.check(gpu.capi.lib().hcp_add_cell_unchecked(cf.ptr, int(t), int(cell_id), gpu.dptr(np.array(centre, dtype=np.float64)), gpu.dptr(np.zeros(3))))


def test_non_periodic_faces_without_walls(gpu):
    """no periodic axis and no wall: a PLT half outside the x = 0 face and an RBC reaching over the y face lose the nodes
    beyond them, the rest is renormalised; the body force drives the flow"""
    def build(wide):
        L, h = _channel(gpu, (PHI4, PHI3) if wide else (PHI2, PHI2), 2, 1, periodic=(False, False, False), walls=False)
        cf = h.cellfields
        _add_unchecked(gpu, cf, 1, 7, (0.4, 12.0, 12.0))
        _add_unchecked(gpu, cf, 0, 8, (20.0, 1.5, 12.0))
        cf.setDeletionMode("cell")
        return L, h, lambda: (cf.destroy(), L.destroy())
    _run_twice_and_on_two_points(gpu, build, 12)


def test_all_four_models(gpu):
    """RbcHighOrderModel on phi4, PltSimpleModel on phi3, WbcHighOrderModel on phi4 and RbcMalariaModel on phi3 in one container"""
    def build(wide):
        P = gpu.base_parameters()
        L = gpu.Lattice(40, 32, 32, (True, True, True), 1.0 / P.tau)
        L.latticeEquilibrium(); L.setExternalVector(CH_BODY)
        h = gpu.HemoCell(L, P)
        cf = h.cellfields
        for T in (gpu.CellType.rbc(P), gpu.CellType.plt(P), gpu.CellType.wbc(P), gpu.CellType.malaria(P)):
            cf.addCellType(T, 1)
        for t, c in enumerate(((9.2, 6.1, 16.3), (30.4, 26.2, 5.7), (28.1, 14.2, 17.9), (9.7, 21.3, 15.1))):
            assert cf.addCell(t, c, (0.0, 0.0, 0.0))
        if wide:
            for t, k in enumerate((PHI4, PHI3, PHI4, PHI3)):
                cf.setIbmKernel(t, k)
        cf.applyConstitutiveModel(0, True)
        return L, h, lambda: (cf.destroy(), L.destroy())
    _run_twice_and_on_two_points(gpu, build, 10)


@pytest.mark.parametrize("mode", ["particle", "cell"])
def test_both_deletion_modes(gpu, mode):
    """a PLT placed across the wall: its particles on boundary nodes go one by one (the rest is still spread and interpolated
    through phi3) or the whole cell goes at once"""
    def build(wide):
        L, h = _channel(gpu, (PHI4, PHI3) if wide else (PHI2, PHI2), 1, 1)
        cf = h.cellfields
        cf.setDeletionMode(mode)
        _add_unchecked(gpu, cf, 1, 5, (8.0, 0.9, 12.0))
        return L, h, lambda: (cf.destroy(), L.destroy())
    probe = lambda L, h: dict(alive=h.cellfields.alive(), counts=np.array(h.cellfields.deletion_counts()))
    wide, _ = _run_twice_and_on_two_points(gpu, build, 10, probe)
    gone_cells, gone_particles = int(wide["counts"][0]), int(wide["counts"][1])
    assert (gone_cells, gone_particles > 0) == ((1, False) if mode == "cell" else (0, True)), wide["counts"]
    if mode == "particle":
        assert (~wide["alive"]).sum() > 0 and wide["alive"].sum() > 642


def test_both_repulsions(gpu):
    """vertex-vertex repulsion between two PLT half a node apart and boundary repulsion of a PLT next to the wall: the
    repulsion force arrays are spread together with the membrane forces"""
    def build(wide):
        L, h = _channel(gpu, (PHI4, PHI3) if wide else (PHI2, PHI2), 1, 1)
        cf = h.cellfields
        assert cf.addCell(1, (25.2, 7.4, 17.7), (0.0, 40.0, 0.0))       # 2.3 above the first PLT, whose half thickness is 1.1
        assert cf.addCell(1, (8.0, 2.1, 12.0), (0.0, 0.0, 0.0))        # its lowest vertices less than a node off the wall nodes y = 0
        cf.setRepulsion(2e-3, 0.7, 1); cf.enableBoundaryParticles(2e-3, 1.0, 1)
        return L, h, lambda: (cf.destroy(), L.destroy())
    probe = lambda L, h: dict(rep=h.cellfields.repulsion_forces)
    wide, _ = _run_twice_and_on_two_points(gpu, build, 10, probe)
    rep = np.abs(wide["rep"]).sum(axis=1)
    assert (rep[642 + 66:642 + 132] > 0).any() and (rep[642 + 132:] > 0).any()


def test_lees_edwards(gpu):
    def build(wide):
        L, h = _channel(gpu, (PHI4, PHI3) if wide else (PHI2, PHI2), 1, 1, periodic=(True, True, True), walls=False)
        L.setLeesEdwards(0.01, -0.01)
        return L, h, lambda: (h.cellfields.destroy(), L.destroy())
    _run_twice_and_on_two_points(gpu, build, 12)


def test_cepac_field(gpu):
    """the scalar field is advected with the velocity that holds the spread force of the wide kernels"""
    def build(wide):
        L, h = _channel(gpu, (PHI4, PHI3) if wide else (PHI2, PHI2), 1, 1)
        S = L.createCEPACfield(0.8)
        S.addSource((2, 4, 8, 14, 8, 14), 2.0)
        h._scalar = S
        return L, h, lambda: (h.cellfields.destroy(), L.destroy())
    probe = lambda L, h: dict(g=h._scalar.populations())
    wide, two = _run_twice_and_on_two_points(gpu, build, 12, probe)
    assert not np.array_equal(wide["g"], two["g"])


def test_solidify(gpu):
    """tests/test_gpu_solidify.py's channel with the platelets on phi4 and the red cell on phi3: the platelet on the floor is
    flagged and solidifies, and the new wall nodes reach the wide kernels (they read the lattice's mask)"""
    from tests.test_gpu_solidify import Channel
    lib = gpu.capi.lib()
    gpu.check(lib.hc_set_reproducible_spread(1))
    try:
        runs = []
        for _ in range(2):
            c = Channel(gpu, 5, 5)
            try:
                c.cf.setIbmKernel(0, PHI4); c.cf.setIbmKernel(1, PHI3)
                c.h.iterate(60)
                runs.append(c.state())
            finally:
                c.destroy()
        assert all(np.array_equal(runs[0][k], runs[1][k]) for k in runs[0])
        assert runs[0]["counts"][0] >= 1 and runs[0]["counts"][1] > 0 and np.isfinite(runs[0]["pos"]).all()
    finally:
        gpu.check(lib.hc_set_reproducible_spread(0))


# ---- combinations that are refused
def _refused(gpu, fn, *words):
    with pytest.raises(gpu.HcError) as e:
        fn()
    for w in words:
        assert w in str(e.value), str(e.value)


def _small(gpu, periodic=(True, False, False), **kw):
    P = gpu.base_parameters()
    L = gpu.Lattice(16, 12, 12, periodic, 1.0 / P.tau, **kw)
    m = np.zeros((kw.get("nx_global", 16), 12, 12), np.uint8)
    m[:, 0, :] = m[:, -1, :] = 1
    L.defineBounceBack(m)
    return P, L


def test_bad_arguments_are_refused(gpu):
    P, L = _small(gpu)
    cf = gpu.Cells(L, P)
    try:
        cf.addCellType(gpu.CellType.plt(P), 1)
        for k in (0, 1, 5, -3):
            _refused(gpu, lambda: cf.setIbmKernel(0, k), "hcp_type_set_ibm_kernel", "HC_IBM_PHI2, HC_IBM_PHI3 or HC_IBM_PHI4")
        _refused(gpu, lambda: cf.setIbmKernel(1, PHI3), "hcp_type_set_ibm_kernel", "unknown cell type")
        _refused(gpu, lambda: cf.ibmKernel(1), "hcp_type_get_ibm_kernel")
        assert cf.ibmKernel(0) == PHI2
    finally:
        cf.destroy(); L.destroy()


@pytest.mark.parametrize("what", ["slabs", "open_boundary", "pre_inlet", "pre_inlet_cells", "interior_viscosity", "sample_scalar"])
@pytest.mark.parametrize("first", ["other", "kernel"])
def test_combinations_are_refused_in_both_orders(gpu, what, first):
    """x-slabs, open-boundary nodes, a pre-inlet (the fluid's and the cells'), interior viscosity and hcp_sample_scalar: refused by
    hcp_type_set_ibm_kernel when the other feature is there, and by the other feature's call when a type is on a wide kernel.
    A refused call changes nothing, and a type that goes back to two points frees the lattice again."""
    extra = []
    if what == "slabs":
        P, L = _small(gpu, x0=0, nx_global=32, n_slabs=2)
    elif what == "open_boundary":
        P, L = _small(gpu, periodic=(False, False, False))
    else:
        P, L = _small(gpu)
    word = dict(slabs="n_slabs", open_boundary="open", pre_inlet="pre-inlet", pre_inlet_cells="pre-inlet", interior_viscosity="interior viscosity",
                sample_scalar="hcp_sample_scalar")[what]
    cf = gpu.Cells(L, P)
    T = gpu.CellType.rbc(P) if what == "interior_viscosity" else gpu.CellType.plt(P)
    cf.addCellType(T, 1)

    def other():
        if what == "open_boundary":
            L.addVelocityBoundary0N((0, 0, 1, 10, 0, 11))
        elif what == "interior_viscosity":
            gpu.check(cf.lib.hcp_type_set_interior_viscosity(cf.ptr, 0, 0.9))
        elif what == "pre_inlet":
            D = gpu.Lattice(16, 12, 12, (False, False, False), 1.0 / P.tau)
            extra.append(D)
            yz = np.array([(y, z) for y in range(1, 11) for z in range(12)])
            extra.insert(0, gpu.PreInlet(L, D, yz, 15, 0, "Xneg", device=True))   # L is the pre-inlet lattice of the pair
        elif what == "pre_inlet_cells":
            D = gpu.Lattice(16, 12, 12, (False, False, False), 1.0 / P.tau)
            extra.append(D)
            dc = gpu.Cells(D, P)
            extra.insert(0, dc)
            dc.addCellType(T, 1)
            yz = np.array([(y, z) for y in range(1, 11) for z in range(12)])
            extra.insert(0, gpu.PreInlet(L, D, yz, 15, 0, "Xneg", device=True, cells=(cf, dc), window=(4.0, 12.0), shift=(-8.0, 0.0, 0.0), id_stride=1000))
    try:
        if what == "slabs":
            _refused(gpu, lambda: cf.setIbmKernel(0, PHI4), "hcp_type_set_ibm_kernel", word)
            assert cf.ibmKernel(0) == PHI2
        elif what == "sample_scalar":
            S = L.createCEPACfield(0.8)
            assert cf.addCell(0, (8.0, 6.0, 6.0))
            before = cf.sampleScalar(S)
            cf.setIbmKernel(0, PHI3)               # the field itself combines with a wide kernel; the sample does not
            _refused(gpu, lambda: cf.sampleScalar(S), word, "three- or four-point")
            cf.setIbmKernel(0, PHI2)
            assert np.array_equal(cf.sampleScalar(S), before)
        elif first == "other":
            other()
            _refused(gpu, lambda: cf.setIbmKernel(0, PHI4), "hcp_type_set_ibm_kernel", word)
            _refused(gpu, lambda: cf.setIbmKernel(0, PHI3), "hcp_type_set_ibm_kernel", word)
            assert cf.ibmKernel(0) == PHI2
            cf.setIbmKernel(0, PHI2)               # the default is never refused
        else:
            cf.setIbmKernel(0, PHI4)
            _refused(gpu, other, word if what != "interior_viscosity" else "three- or four-point")
            assert cf.ibmKernel(0) == PHI4
            cf.setIbmKernel(0, PHI2)               # back on two points: the other feature is accepted
            other()
    finally:
        for e in extra:
            e.destroy()
        cf.destroy(); L.destroy(); T.destroy()


# ---- the facade
def test_facade_example_equals_python_host(gpu, tmp_path):
    """tests/plugin/ibm_kernel_driver.cpp assigns interpolationCoefficientsPhi4 (and, in another run, Phi3 then Phi4) to the
    type's kernelMethod: 20 iterations equal the same case on the Python host with setIbmKernel(0, IBM_PHI4) bit for bit, and
    differ from the host's run on two points"""
    from tests.test_plugin_surface import INC
    libdir = os.path.dirname(gpu.capi.LIB_PATH)
    exe = os.path.join(str(tmp_path), "ibm_kernel_driver")
    r = subprocess.run(["g++", "-std=c++14", "-O1", "-Wall", "-Wno-deprecated-declarations", "-DHEMOCELL_COMPAT_MAIN"] + INC +
                       [os.path.join(ROOT, "tests", "plugin", "ibm_kernel_driver.cpp"), "-o", exe, "-L" + libdir, "-lhemocell_amd", "-Wl,-rpath," + libdir],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    dims, n = (40, 30, 30), 40 * 30 * 30

    def facade(mode):
        d = str(tmp_path / mode)
        shutil.copytree(os.path.join(ROOT, "tests", "golden", "shear_case"), d)
        env = dict(os.environ, HEMOCELL_REPRODUCIBLE_SPREAD="1")
        r = subprocess.run([exe, mode, "config.xml", "20"], cwd=d, capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
        done = [l for l in r.stdout.splitlines() if l.startswith("DONE")][0].split()
        raw = open(os.path.join(d, "ibm_kernel_state.bin"), "rb").read()
        return int(done[-1]), np.frombuffer(raw[:n * 19 * 8], dtype=np.float64).reshape(n, 19), np.frombuffer(raw[n * 19 * 8:], dtype=np.float64).reshape(-1, 3)

    def host(kernel):
        P = gpu.base_parameters(dt=0.5e-7)
        L = gpu.Lattice(*dims, (True, True, True), 1.0 / P.tau)
        lib = gpu.capi.lib()
        gpu.check(lib.hc_set_reproducible_spread(1))
        try:
            L.latticeEquilibrium(1.0, (0.0, 0.0, 0.0))
            h = gpu.HemoCell(L, P)
            h.setParticleVelocityUpdateTimeScaleSeparation(2)
            h.cellfields.addCellType(gpu.CellType.rbc(P), 1)
            h.cellfields.setIbmKernel(0, kernel)
            um = 1e-6 / P.dx
            assert h.cellfields.addCell(0, (9.5 * um, 9.5 * um, 4.5 * um), (90.0, 0.0, 0.0), cell_id=0)
            h.cellfields.applyConstitutiveModel(0, True)
            L.setExternalVector((2e-5, 0.0, -1e-5))
            h.iterate(20)
            return L.populations(), h.cellfields.positions
        finally:
            gpu.check(lib.hc_set_reproducible_spread(0))
            h.cellfields.destroy(); L.destroy()

    k4, f4, p4 = facade("phi4")
    kb, fb, pb = facade("both")
    k3, f3, p3 = facade("phi3")
    assert (k4, kb, k3) == (PHI4, PHI4, PHI3) and len(p4) == 642
    hf4, hp4 = host(PHI4)
    assert np.array_equal(p4, hp4) and np.array_equal(f4, hf4), float(np.abs(p4 - hp4).max())
    assert np.array_equal(pb, p4) and np.array_equal(fb, f4)
    hf3, hp3 = host(PHI3)
    assert np.array_equal(p3, hp3) and np.array_equal(f3, hf3)
    hf2, hp2 = host(PHI2)
    assert not np.array_equal(hf2, hf4) and not np.array_equal(hf3, hf4)
