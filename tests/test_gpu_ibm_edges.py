"""The IBM kernels at the caps, seams and lane-mapping edges of the per-cell kernels (hemocell_amd/csrc/ibm.hip) against
tests/ibm_ref.py, the extended-precision restatement of the reference's interpolationCoefficientsPhi2 / spreadParticleForce /
interpolateFluidVelocity, on the crafted geometries of tests/ibm_cases.py.  Every case runs in three kernel forms: per cell
(the default), per vertex (hc_debug_ibm_per_vertex) and the gather form of the spread (hc_set_reproducible_spread).

Decision points of the per-cell kernels, and the cases on either side (tests/test_ibm_ref_cpu.py asserts with
ibm_ref.predict that each case sits where it says):
- tile volume <= TILE_CAP (5832): tile_18_18_18 (5832) and tile_19_18_17 (5814) tiled, tile_18_18_19 (6156) falls back; the
  thin tiles all have exactly 5832.
- tile no wider than a periodic axis: thin_whole_axis (extent = axis, 1458) tiled, thin_axis_plus_one (1458 on 1457) falls back.
- tile_decode's float reciprocals: thin_2_2_1458, thin_2_1458_2, thin_1458_2_2, thin_3_2_972, thin_2_3_972_seam (every index up to
  5831 with e[2] and e[1] from 2 to 1458), tile_19_18_17 (three different extents).
- tile_is_clear / rebuild_wall_bricks: bricks_64 (64 bricks, one per lane) against bricks_65 (mask path); bricks_lane_63_wall
  (the only boundary node in the brick of lane 63); brick_wall_next_door (tile ends on brick coordinate 7, a boundary node at
  8: clear) against brick_ends_on_8 (the same node inside the tile); faces_open (tiles that leave a non-periodic domain:
  ow = -1 and the last planes) and every seam_* case (a wrapped tile is never clear).
- compact_nodes, ranks across strides of 256 (RBC) and 128 (PLT) entries and NODE_CAP (1536): nodes_1535 and nodes_1536
  tiled, nodes_1537 falls back; every tiled case has marked nodes on both sides of many stride boundaries.
- tile_node / tile_mask wrap once: seam_x, seam_y, seam_z, seam_yz, seam_xyz; seam_negative and seam_far (pmod of the origin:
  negative coordinates, more than a period away); pipe_wall_hug (x seam next to a wall).
- xcd_contiguous for n >= 8: lanes_1, lanes_7 (identity) against lanes_8, lanes_9, lanes_16, lanes_17, lanes_23 (permuted,
  with and without a remainder), RBC and PLT in one run, every cell at its own place with its own forces.
- block size 128 / 256 by nv: PLT (66) and RBC (642) cells throughout; NVPT * nth: big_mesh (2562 vertices, RBC_FROM_SPHERE at
  1300 triangles, takes the per-vertex path inside the per-cell kernels although its tile and node count would fit).
- removed particles of an incomplete cell: dead_vertices (their stored positions would take the tile past 5832; some hold
  forces above the limit; a complete cell beside it, and a cell that has lost every particle: an empty bounding box).
- admission: exact_positions (on nodes, on half-integers, the doubles next to both, both signs), walls_7_and_1_of_8,
  pipe_wall_hug, faces_open (nodes outside the domain dropped, the rest renormalised); force_cap (FORCE_LIMIT).
- the OPEN instantiation of the interpolation: faces_zou_he (a channel with a Zou-He velocity plane and a pressure plane, cells
  within half a node of both and in the corners next to the walls; the completed moments of the plane nodes come from
  open_boundary_ref.observe, which the open-boundary suite pins bit for bit).

Not built: a repulsion force next to the membrane force (the host has no upload for it).  'admit_zero_weight' changes no
sum (a zero weight adds zero), only the node count: tests/test_ibm_ref_cpu.py holds nodes_1537 against it.

Bound: |gpu - ref| <= K 2^-53 abs with abs the sum of the magnitudes of the terms (ibm_ref), K = 22.44.  Measured on the CPU
before any GPU run (test_ibm_ref_cpu.py::test_rounding_figure_behind_k): the largest |double - extended| / (2^-53 abs) of the
plain double restatement, summed in storage order and in the reverse order, over all cases, is 5.61 (spread of nodes_1535);
that exceeds 4, so K is four times it instead of the project's 16.  Every named mutation control has to miss by 100 bounds."""
import zlib

import numpy as np
import pytest

from tests import ibm_cases as IC
from tests import ibm_ref as IR
from tests import observables_ref as R
from tests.test_gpu_parity import _random_populations
from tests.test_ibm_ref_cpu import FAIL_BY, _node_velocity, check_expectations, mutation_excess

pytestmark = pytest.mark.gpu
K = IC.K
FORMS = ("per_cell", "per_vertex", "gather")
SENTINEL = 123.25


def _setup(gpu, case):
    P = gpu.base_parameters()
    lib = gpu.capi.lib()
    Lg = gpu.Lattice(*case["dims"], case["periodic"], 1.0 / 0.9)
    if case["mask"] is not None:
        Lg.defineBounceBack(case["mask"])
    if case["open"] is not None:          # Zou-He planes: the OPEN instantiations of the interpolation kernels
        total = 0
        for kind, box, values in case["open"]["patches"]:
            first, n = (Lg.addVelocityBoundary0N if kind == 0 else Lg.addPressureBoundary0P)(box)
            assert first == total and n == len(values)
            (Lg.setOpenBoundaryVelocitySlots if kind == 0 else Lg.setOpenBoundaryDensitySlots)(first, values)
            total += n
        assert np.array_equal(Lg.openBoundaryValues(0, total), case["open"]["val"])
    rng = np.random.default_rng(zlib.crc32(("s" + case["name"]).encode()))
    Lg.set_populations(_random_populations(rng, Lg.n, 0.01))
    Lg.setExternalVector(case["body"])
    cells = gpu.Cells(Lg, P)
    make = dict(rbc=lambda: gpu.CellType.rbc(P), plt=lambda: gpu.CellType.plt(P), big=lambda: gpu.CellType.rbc(P, min_triangles=IC.BIG_MIN_TRIANGLES))
    types, cid = [], 0
    seat, zero = np.array(case["seat"], dtype=np.float64), np.zeros(3)
    for t in IC.TYPES:
        if case["counts"][t]:
            T = make[t]()
            types.append(T)
            assert T.nv == IC.NV[t]
            ti = cells.addCellType(T, 1)
            for _ in range(case["counts"][t]):       # ids ascend in storage order: the gather form's (type, id, vertex) order
                gpu.check(lib.hcp_add_cell_unchecked(cells.ptr, int(ti), int(cid), gpu.dptr(seat), gpu.dptr(zero)))
                cid += 1
    assert cells.counts()[0] == len(case["pos"])
    if case["kill_pos"] is not None:      # particles whose nearest node is a boundary are removed one by one ("particle" mode)
        cells.setDeletionMode("particle")
        cells.positions = case["kill_pos"]
        cells.velocities = np.zeros_like(case["pos"])
        cells.advanceParticles(True)
    assert np.array_equal(cells.alive(), case["alive"])
    cells.positions = case["pos"]
    cells.forces = case["force"]
    cells.velocities = np.full(case["pos"].shape, SENTINEL)
    return P, Lg, cells, types


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", IC.NAMES)
def test_ibm_edge_case(gpu, name, form):
    P = gpu.base_parameters()
    case = IC.build(name, P.f_limit)
    check_expectations(case)
    lib = gpu.capi.lib()
    geo = (case["dims"], case["periodic"], case["mask"])
    pos, frc, alive = case["pos"], case["force"], case["alive"]
    f_limit = P.f_limit if case["limit"] else None
    _, Lg, cells, types = _setup(gpu, case)
    try:
        gpu.check(lib.hc_debug_ibm_per_vertex(1 if form == "per_vertex" else 0))
        gpu.check(lib.hc_set_reproducible_spread(1 if form == "gather" else 0))
        # ---- spread
        cells.spreadParticleForce(case["limit"])
        Fg = Lg.ibm_force()
        f_after = cells.forces
        ref = IR.spread(pos, frc, None, alive, *geo, f_limit=f_limit)
        es = R.excess(Fg, ref["F"], ref["F_abs"], K)                              # every node, fluid or not
        et = R.excess(R.to_double(R.hp(Fg).sum(axis=0)), ref["total"], ref["total_abs"], K)
        ef = R.excess(f_after, ref["force"], ref["force_abs"], K)
        print("%s/%s: spread excess %.3g, total %.3g, capped forces %.3g" % (name, form, es, et, ef))
        assert (Fg[~ref["touched"]] == 0.0).all()                                 # what the reference leaves alone is exactly zero
        assert es <= 1 and et <= 1 and ef <= 1
        assert np.array_equal(f_after[~alive], frc[~alive])                       # removed particles keep their force
        if form == "gather":
            # one sequential double sum per node in (type, cell id, vertex) order, added to zero: the reference's bits
            dbl = IR.spread_double(pos, frc, None, alive, *geo, f_limit=f_limit)
            assert np.array_equal(Fg, dbl["F"]) and np.array_equal(f_after, dbl["force"])
        # ---- interpolate, on the post-stream state the collide leaves and the force it used
        Lg.collideAndStream(1)
        f = Lg.populations()
        cells.interpolateFluidVelocity()
        v = cells.velocities
        need = [IR.needed_nodes(pos, alive, *geo)]
        for wrong in case["controls"]:
            nodes, _, adm = IR.stencil(pos, *geo, wrong=wrong)
            need.append(nodes[adm])
        u, ua = _node_velocity(case, f, Fg + np.array(case["body"])[None, :], np.unique(np.concatenate(need)))
        rv = IR.interpolate(pos, alive, u, *geo, u_abs=ua)
        ev = R.excess(v[alive], rv["v"][alive], rv["v_abs"][alive], K)
        print("%s/%s: interpolation excess %.3g" % (name, form, ev))
        assert ev <= 1
        assert (v[~alive] == SENTINEL).all()                                      # removed particles are not written
        if form == "per_cell":
            # "same arithmetic and visiting order as phi2_stencil": the per-cell result is the per-vertex result, bit for bit
            gpu.check(lib.hc_debug_ibm_per_vertex(1))
            cells.velocities = np.full(pos.shape, SENTINEL)
            cells.interpolateFluidVelocity()
            assert np.array_equal(cells.velocities, v)
        # ---- the bound can see a wrong kernel: each restatement the case names misses by far
        for wrong, (ws, wv) in mutation_excess(case, f_limit, Fg, v, u, ua).items():
            assert ws > FAIL_BY and (wv is None or wv > FAIL_BY), (name, wrong, ws, wv)
    finally:
        gpu.check(lib.hc_debug_ibm_per_vertex(0))
        gpu.check(lib.hc_set_reproducible_spread(0))
        cells.destroy(); Lg.destroy()
        for T in types:
            T.destroy()
