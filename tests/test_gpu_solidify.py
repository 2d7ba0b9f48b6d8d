"""Solidify mechanics on the GPU against tests/solidify_ref.py: the binding-site rule, the Tresca observer, the flag pass, the
prepare pass with the wall set growing on the device (mask, binding field, wall bricks, counts), the check inside hc_iterate
against the same library driven phase by phase, and the refusals."""
import ctypes as C
import os

import numpy as np
import pytest

import interior_viscosity_ref as IV
import solidify_ref as SR
from tests import ibm_ref as IR
from tests import observables_ref as R
from tests.ibm_cases import K

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = os.path.join(ROOT, "tests", "golden", "solidify_case")
T_Q = np.array([1 / 3] + [1 / 18] * 3 + [1 / 36] * 6 + [1 / 18] * 3 + [1 / 36] * 6)
C_Q = np.array([(0, 0, 0), (-1, 0, 0), (0, -1, 0), (0, 0, -1), (-1, -1, 0), (-1, 1, 0), (-1, 0, -1), (-1, 0, 1), (0, -1, -1), (0, -1, 1),
                (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, -1, 0), (1, 0, 1), (1, 0, -1), (0, 1, 1), (0, 1, -1)], dtype=np.float64)


def _profile(lib, name):
    ms, n = C.c_double(), C.c_long()
    assert lib.hc_profile_read(name.encode(), C.byref(ms), C.byref(n)) == 0
    return n.value


def _add_unchecked(gpu, cf, t, cell_id):
    c, a = np.array([8.0, 8.0, 8.0]), np.zeros(3)
    gpu.check(gpu.capi.lib().hcp_add_cell_unchecked(cf.ptr, int(t), int(cell_id), gpu.dptr(c), gpu.dptr(a)))


def _random_populations(rng, n, amp):
    return amp * rng.standard_normal((n, 19)) * T_Q[None, :]


def _off_equilibrium(P6):
    """the 19 stored populations with rhoBar = 0, j = 0 and PiNeq = P6 (xx, xy, xz, yy, yz, zz): t_i 9/2 (c c - I/3) : Pi"""
    xx, xy, xz, yy, yz, zz = P6
    cc = (C_Q[:, 0] ** 2 * xx + C_Q[:, 1] ** 2 * yy + C_Q[:, 2] ** 2 * zz
          + 2 * (C_Q[:, 0] * C_Q[:, 1] * xy + C_Q[:, 0] * C_Q[:, 2] * xz + C_Q[:, 1] * C_Q[:, 2] * yz))
    return T_Q * 4.5 * (cc - (xx + yy + zz) / 3.0)


# ---- 1. binding sites

BDIMS, BPER = (12, 10, 9), (True, True, False)


def _binding_mask():
    m = np.zeros(BDIMS, np.uint8)
    m[:, :, 0] = 1                 # the floor
    m[5, 5, 1:3] = 1               # a two-node pillar
    m[7:10, 2:5, 1] = 1            # a slab on the floor: the floor node (8, 3, 0) under its middle has no fluid neighbour
    return m


@pytest.mark.parametrize("boxes", [[(0, 11, 0, 9, 0, 0)], [(-3, 5, 4, 20, 0, 4)], [(0, 5, 0, 9, 0, 0), (4, 9, 2, 6, 1, 2)]],
                         ids=["floor", "partly_outside", "union"])
def test_binding_sites_equal_restatement(gpu, boxes):
    """12 x 10 x 9, periodic along x and y: the floor, a pillar and an enclosed floor node; the floor box, a box partly outside
    the lattice, and two calls whose sites add up.  Byte for byte."""
    L = gpu.Lattice(*BDIMS, BPER, 1.0)
    try:
        mask = _binding_mask()
        L.defineBounceBack(mask)
        assert not L.bindingSites().any()                     # before the first call: no site anywhere
        want = np.zeros(BDIMS, np.uint8)
        for b in boxes:
            L.populateBindingSites(b)
            SR.populate(want, mask, BPER, b)
        got = L.bindingSites()
        assert np.array_equal(got, want), int((got != want).sum())
        assert want.any() and not want[mask == 0].any()
        if boxes[0] == (0, 11, 0, 9, 0, 0):
            assert want[8, 3, 0] == 0 and want[8, 2, 0] == 1 and want[0, 0, 0] == 1 and want.sum() == 12 * 10 - 1
        if len(boxes) == 2:
            assert want[5, 5, 1] == 1 and want[5, 5, 2] == 1 and want[8, 3, 1] == 1 and want[10, 0, 0] == 0
        L.clearBindingSites()
        assert not L.bindingSites().any()
        L.setBindingSites(want)
        assert np.array_equal(L.bindingSites(), want)
    finally:
        L.destroy()


# ---- 2. Tresca

def test_tresca_matches_eigvalsh(gpu):
    """8 x 7 x 6 with a few wall nodes; equilibrium plus a 1e-3 random part, and nodes overwritten with exact equilibrium, a
    pure shear, a uniaxial state (two equal eigenvalues) and an isotropic one.  Against numpy.linalg.eigvalsh on S built from
    the downloaded pi_neq and rho, within 1e-12 ||S||_F per node: both sides are a handful of fp64 roundings of size
    eps ||S||, which leaves a few hundred times that.  Wall nodes give exactly 0."""
    dims, per, omega = (8, 7, 6), (True, False, True), 1.0 / 0.9
    L = gpu.Lattice(*dims, per, omega)
    try:
        mask = np.zeros(dims, np.uint8)
        mask[:, 0, :] = 1
        mask[:, -1, :] = 1
        mask[3, 3, 2] = 1
        mask[6, 2, 4] = 1
        L.defineBounceBack(mask)
        rng = np.random.default_rng(5)
        f = _random_populations(rng, L.n, 1e-3).reshape(dims + (19,))
        special = {(1, 3, 1): np.zeros(19),                                            # exact equilibrium at rest: S = 0
                   (2, 4, 3): _off_equilibrium((0.0, 2.0 ** -12, 0.0, 0.0, 0.0, 0.0)),  # pure shear
                   (4, 2, 2): _off_equilibrium((2.0 ** -11, 0, 0, -2.0 ** -12, 0, -2.0 ** -12)),   # uniaxial
                   (5, 4, 4): _off_equilibrium((2.0 ** -12, 0, 0, 2.0 ** -12, 0, 2.0 ** -12)),     # isotropic
                   (6, 4, 1): _off_equilibrium((3e-4, 1e-4, 0, 3e-4, 0, -6e-4))}                  # two close eigenvalues, rotated
        for node, v in special.items():
            f[node] = v
        L.set_populations(f.reshape(-1, 19))
        pi, (rho, _) = L.pi_neq(), L.rho_u()
        want, norm = SR.tresca(pi, rho, omega, mask)
        got = L.tresca()
        err = np.abs(got - want)
        fluid = mask.reshape(-1) == 0
        worst = float((err[fluid] / np.where(norm[fluid] > 0, norm[fluid], 1.0)).max())
        print("tresca: worst error %.3g ||S||_F" % worst)
        assert np.all(err <= 1e-12 * norm), worst
        assert np.all(got[~fluid] == 0.0) and np.all(got[fluid] >= 0.0)
        idx = {n: np.ravel_multi_index(n, dims) for n in special}
        assert got[idx[(1, 3, 1)]] == 0.0
        assert abs(got[idx[(2, 4, 3)]] - abs(-omega * 1.5 * 2.0 ** -12)) <= 1e-12 * norm[idx[(2, 4, 3)]]
        assert got[idx[(5, 4, 4)]] <= 1e-12 * norm[idx[(5, 4, 4)]] and norm[idx[(5, 4, 4)]] > 1e-4
        assert got[fluid].max() > 1e-5
    finally:
        L.destroy()


# ---- 3. the flag pass

DIST = 1.25


def _flag_scene(gpu):
    P = gpu.base_parameters()
    L = gpu.Lattice(*BDIMS, BPER, 1.0 / P.tau)
    mask = _binding_mask()
    L.defineBounceBack(mask)
    L.populateBindingSites((0, 11, 0, 9, 0, 0))
    L.populateBindingSites((5, 5, 5, 5, 1, 2))       # the pillar
    cf = gpu.Cells(L, P)
    plt, rbc = gpu.CellType.plt(P), gpu.CellType.rbc(P)
    cf.addCellType(plt, 1)
    cf.addCellType(rbc, 1)
    _add_unchecked(gpu, cf, 0, 0)
    _add_unchecked(gpu, cf, 1, 1)
    return P, L, cf, mask, plt, rbc


def _flag_positions(rng, nv):
    """the vertices placed by hand, then random ones in the two layers above the floor"""
    crafted = [(3.0, 4.0, DIST),                                   # exactly at the threshold above the site (3, 4, 0)
               (3.0, 4.0, float(np.nextafter(DIST, 2.0))),         # one ulp farther
               (4.5, 2.5, 0.75),                                   # x.5 rounds up: nearest node (5, 3, 1)
               (11.7, 9.8, 1.0),                                   # nearest node (12, 10, 1): across both periodic seams
               (-0.4, 5.0, 1.0),                                   # negative coordinate: floor, not truncation
               (6.2, 3.3, 8.2),                                    # under the non-periodic top: no site in reach
               (6.2, 3.3, 8.6),                                    # nearest node beyond the top: not in the grid
               (2.0, 7.0, 0.3),                                    # nearest node is a wall node: Tresca 0
               (5.0, 5.0, 3.6),                                    # above the pillar: the site (5, 5, 2) at 1.6
               (5.6, 5.0, 2.5)]                                    # beside the pillar's top: the site (5, 5, 2) in reach
    rest = np.stack([rng.uniform(-1.0, 13.0, nv - len(crafted)), rng.uniform(-1.0, 11.0, nv - len(crafted)),
                     rng.uniform(0.6, 2.4, nv - len(crafted))], axis=1)
    return np.concatenate([np.array(crafted), rest])


@pytest.mark.parametrize("quantile", [0.3, 0.7])
def test_flag_pass_equals_restatement(gpu, quantile):
    """The lattice of test 1 with the floor's sites, one platelet (enabled) and one RBC (not enabled) with uploaded positions.
    The shear threshold is put between two neighbouring candidate values, at the 30 % and the 70 % quantile, so that some
    candidates lie above it and some below; the restatement asserts that no candidate lies within 1e-9 (relative) of it.
    Flags equal the restatement exactly, the RBC's stay 0, and a second pass over a fluid at rest leaves set flags set."""
    P, L, cf, mask, plt, rbc = _flag_scene(gpu)
    try:
        rng = np.random.default_rng(17)
        L.set_populations(_random_populations(rng, L.n, 1e-3))
        pos_p = _flag_positions(rng, plt.nv)
        pos_r = np.stack([rng.uniform(0.0, 12.0, rbc.nv), rng.uniform(0.0, 10.0, rbc.nv), rng.uniform(0.6, 2.4, rbc.nv)], axis=1)
        cf.positions = np.concatenate([pos_p, pos_r])
        binding = L.bindingSites()
        T, _ = SR.tresca(L.pi_neq(), L.rho_u()[0], 1.0 / P.tau, mask)
        _, cand = SR.flag(np.zeros(plt.nv, bool), pos_p, np.ones(plt.nv, bool), binding, mask, BPER, T, DIST, 0.0, margin=0.0)
        assert list(cand[:10]) == [True, False, True, True, True, False, False, True, False, True]
        near = SR.nearest(pos_p[cand])
        _, nw = IV.wrap(near, BDIMS, BPER)
        values = np.unique(np.abs(T.reshape(BDIMS)[nw[:, 0], nw[:, 1], nw[:, 2]] / 1e-7))
        assert len(values) > 8
        k = int(quantile * len(values))
        shear = 0.5 * (values[k - 1] + values[k])
        cf.enableSolidifyMechanics(0, DIST, shear)
        want, cand = SR.flag(np.zeros(plt.nv, bool), pos_p, np.ones(plt.nv, bool), binding, mask, BPER, T, DIST, shear)
        assert 0 < want.sum() < cand.sum()
        assert not cf.solidifyFlags().any()
        cf.solidifyCells()
        got = cf.solidifyFlags()
        assert np.array_equal(got[:plt.nv], want), (np.flatnonzero(got[:plt.nv] != want), cand.sum())
        assert not got[plt.nv:].any()
        assert not want[1] and not want[7]
        assert cf.solidify_counts() == (0, 0, int(want.sum()))
        L.latticeEquilibrium(1.0, (0.0, 0.0, 0.0))              # no shear anywhere: nobody is flagged anew, nobody loses the flag
        cf.solidifyCells()
        assert np.array_equal(cf.solidifyFlags(), got)
        assert np.array_equal(cf.positions, np.concatenate([pos_p, pos_r]))
    finally:
        cf.destroy(); L.destroy()


# ---- 4. the prepare pass

PDIMS, PPER = (24, 24, 24), (True, True, False)


def _centred(vertices):
    return vertices - 0.5 * (vertices.min(axis=0) + vertices.max(axis=0))


class PrepareScene:
    """24^3, periodic along x and y, a floor.  platelets: [(centre, flagged vertices, removed vertex or None)]; an optional
    small red cell (radius 1 um, not enabled) at rbc_centre."""

    def __init__(self, gpu, platelets, min_triangles=66, rbc_centre=None):
        self.gpu, self.P = gpu, gpu.base_parameters()
        self.L = gpu.Lattice(*PDIMS, PPER, 1.0 / self.P.tau)
        self.mask = np.zeros(PDIMS, np.uint8)
        self.mask[:, :, 0] = 1
        self.L.defineBounceBack(self.mask)
        self.L.populateBindingSites((0, 23, 0, 23, 0, 0))
        self.cf = gpu.Cells(self.L, self.P)
        self.plt = gpu.CellType.plt(self.P, min_triangles=min_triangles, solidify=(1.5, 100.0))
        self.cf.addCellType(self.plt, 1)
        self.tab = self.plt.tables()
        shape = _centred(self.tab["vertices"])
        self.pos = [np.asarray(c, dtype=np.float64)[None, :] + shape for c, _, _ in platelets]
        for k in range(len(platelets)):
            _add_unchecked(gpu, self.cf, 0, k)
        allpos = list(self.pos)
        self.rbc = None
        if rbc_centre is not None:
            self.rbc = gpu.CellType.rbc(self.P, radius=1.0e-6)
            self.cf.addCellType(self.rbc, 1)
            _add_unchecked(gpu, self.cf, 1, 100)
            self.rbc_pos = np.asarray(rbc_centre, dtype=np.float64)[None, :] + _centred(self.rbc.tables()["vertices"])
            allpos.append(self.rbc_pos)
        self.cf.positions = np.concatenate(allpos)
        self.cf.velocities = np.zeros((self.cf.counts()[0], 3))
        removed = [r for _, _, r in platelets]
        if any(r is not None for r in removed):   # one particle of the cell is taken out at the wall ("particle" mode)
            self.cf.setDeletionMode("particle")
            moved = np.concatenate(allpos)
            for k, r in enumerate(removed):
                if r is not None:
                    moved[k * self.plt.nv + r] = (3.0, 3.0, 0.2)
            self.cf.positions = moved
            self.cf.advanceParticles(True)
            self.cf.positions = np.concatenate(allpos)
        self.flags = np.zeros(self.cf.counts()[0], bool)
        for k, (_, fl, _) in enumerate(platelets):
            self.flags[[k * self.plt.nv + i % self.plt.nv for i in fl]] = True
        self.cf.setSolidifyFlags(self.flags)
        self.cells = [dict(pos=self.pos[k], tri=self.tab["triangles"], flags=self.flags[k * self.plt.nv:(k + 1) * self.plt.nv],
                           complete=removed[k] is None, enabled=True) for k in range(len(platelets))]

    def destroy(self):
        self.cf.destroy(); self.L.destroy()


CASES = {
    # (a) a platelet at the centre of an 8^3 brick that starts wall-free, a second one that overlaps its box, both flagged in
    # one check; a third one without a flag stays
    "a_overlap": dict(platelets=[((10.0, 12.0, 12.0), [3], None), ((11.5, 12.5, 12.25), [0, 7], None), ((4.0, 4.0, 6.0), [], None)]),
    # (b) across the periodic seam in x and y
    "b_seam": dict(platelets=[((23.6, -0.4, 9.0), [5], None)]),
    # (c) resting on the floor: its inner wall nodes are untouched and uncounted
    "c_floor": dict(platelets=[((8.0, 15.0, 0.6), [1], None)]),
    # (d) flagged, but one vertex removed: incomplete cells are skipped
    "d_incomplete": dict(platelets=[((10.0, 12.0, 12.0), [3], 4), ((16.0, 6.0, 8.0), [2], None)]),
    # (e) a finer mesh: the loops over vertices and nodes cross the workgroup size
    "e_fine": dict(platelets=[((10.3, 12.1, 11.7), [-1], None)], min_triangles=300, block=64),
}


@pytest.mark.parametrize("name", list(CASES))
def test_prepare_pass_equals_restatement(gpu, name):
    """mask, binding field and counts equal the restatement exactly, the solidified cells are gone, hcl_node_counts moved by
    the node count"""
    case = CASES[name]
    lib = gpu.capi.lib()
    s = PrepareScene(gpu, case["platelets"], case.get("min_triangles", 66))
    try:
        gpu.check(lib.hc_debug_solidify_block(case.get("block", 256)))
        if name == "e_fine":
            assert s.plt.nv > 64 * 2
        mask, binding = s.mask.copy(), s.L.bindingSites()
        assert np.array_equal(binding, (s.mask != 0).astype(np.uint8))
        gone, nodes = SR.prepare(s.cells, mask, binding, PPER)
        before = s.L.node_counts()
        assert before[1] == 24 * 24 * 23
        s.cf.prepareSolidification()
        got_mask = s.L.mask()
        assert np.array_equal(got_mask != 0, mask != 0) and np.array_equal(got_mask[mask != s.mask], np.ones(nodes, np.uint8))
        assert np.array_equal(s.L.bindingSites(), binding)
        kept = [k for k in range(len(s.cells)) if not gone[k]]
        assert s.cf.solidify_counts()[:2] == (int(gone.sum()), nodes)
        assert s.cf.counts()[1] == len(kept) and list(s.cf.cell_ids()) == kept
        assert s.cf.counts()[2] == 0                       # not a wall deletion
        assert np.array_equal(s.cf.positions, np.concatenate([s.pos[k] for k in kept]) if kept else np.zeros((0, 3)))
        assert np.array_equal(s.cf.solidifyFlags(), np.concatenate([s.cells[k]["flags"] for k in kept]) if kept else np.zeros(0, bool))
        after = s.L.node_counts()
        assert after == (before[0], before[1] - nodes, before[2])
        if name == "a_overlap":
            one = [SR.prepare([c], s.mask.copy(), np.zeros(PDIMS, np.uint8), PPER)[1] for c in s.cells[:2]]
            assert list(gone) == [True, True, False] and 0 < nodes < one[0] + one[1] and min(one) > 3   # shared nodes count once
        if name == "b_seam":
            new = mask != s.mask
            assert new[0].any() and new[-1].any() and new[:, 0].any() and new[:, -1].any()
        if name == "c_floor":
            inside = IV.interior_nodes(s.cells[0]["pos"], s.cells[0]["tri"])
            assert (inside[:, 2] == 0).any() and nodes == int((inside[:, 2] > 0).sum()) and gone[0]
        if name == "d_incomplete":
            assert list(gone) == [False, True] and s.cf.deletion_counts()[2:] == (1, 1)
        if name == "e_fine":
            assert nodes > 10
        s.cf.prepareSolidification()                       # nobody is flagged any more among complete cells: nothing moves
        assert np.array_equal(s.L.mask(), got_mask) and s.cf.solidify_counts()[:2] == (int(gone.sum()), nodes)
    finally:
        gpu.check(lib.hc_debug_solidify_block(256))
        s.destroy()


def _bricks_of(nodes_padded):
    return {tuple(int(v) >> 3 for v in n) for n in nodes_padded}


def test_new_walls_reach_the_ibm_kernels_and_the_collide(gpu):
    """After case (a): a small red cell whose stencil tile lay in wall-free 8^3 bricks sits next to the new wall.  A stale brick
    byte would let the per-cell IBM kernels skip the mask there: the spread force and the interpolated velocity equal
    tests/ibm_ref.py with the new mask (conditioned bound of tests/ibm_cases.py), and what the restatement leaves alone is
    exactly 0.  Then 20 collideAndStream steps equal, bit for bit, a fresh lattice given the final mask through hcl_set_mask
    and the same populations."""
    s = PrepareScene(gpu, CASES["a_overlap"]["platelets"], rbc_centre=(11.0, 12.0, 11.5))
    B = None
    try:
        # the bricks (padded x = x + 2) under the red cell's stencil nodes: none is at a lattice edge, none holds a wall yet
        # (a stencil holds the nodes floor(p) and floor(p) + 1 on every axis; brick 0 and the last one along x hold halo planes,
        # those along the non-periodic z touch its ends, those along the periodic y touch nothing)
        lo, hi = np.floor(s.rbc_pos.min(axis=0)).astype(int), np.floor(s.rbc_pos.max(axis=0)).astype(int) + 1
        box = np.mgrid[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1].reshape(3, -1).T
        bricks = _bricks_of(box + (2, 0, 0))
        assert all(1 <= bx <= 2 and 0 <= by <= 2 and bz == 1 for bx, by, bz in bricks), (lo, hi)
        assert not s.mask[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, 8:16].any()
        rng = np.random.default_rng(23)
        s.L.set_populations(_random_populations(rng, s.L.n, 0.01))
        s.cf.prepareSolidification()
        mask = s.L.mask()
        new = (mask != 0) & (s.mask == 0)
        assert _bricks_of(np.argwhere(new) + (2, 0, 0)) & bricks
        assert s.cf.counts()[1] == 2                       # the unflagged platelet and the red cell
        pos = s.cf.positions
        nodes, _, adm = IR.stencil(pos, PDIMS, PPER, s.mask)
        hit = new.reshape(-1)[np.where(adm, nodes, 0)] & adm
        assert hit[s.plt.nv:].any()                        # vertices of the red cell whose stencil holds a new wall node
        geo = (PDIMS, PPER, (mask != 0).astype(np.uint8))
        frc = 1e-4 * rng.standard_normal(pos.shape)
        s.cf.forces = frc
        s.cf.spreadParticleForce(False)
        Fg = s.L.ibm_force()
        ref = IR.spread(pos, frc, None, None, *geo)
        assert (Fg[~ref["touched"]] == 0.0).all() and (Fg[new.reshape(-1)] == 0.0).all()
        es = R.excess(Fg, ref["F"], ref["F_abs"], K)
        stale = IR.spread(pos, frc, None, None, PDIMS, PPER, s.mask)
        print("spread next to the new wall: excess %.3g; with the old mask %.3g" % (es, R.excess(Fg, stale["F"], ref["F_abs"], K)))
        assert es <= 1 and R.excess(Fg, stale["F"], ref["F_abs"], K) > 100
        s.L.collideAndStream(1)
        f = s.L.populations()
        s.cf.interpolateFluidVelocity()
        v = s.cf.velocities
        need = IR.needed_nodes(pos, None, *geo)
        u, ua = np.zeros((s.L.n, 3)), np.zeros((s.L.n, 3))
        ru = R.rho_u(f[need], Fg[need])
        u[need], ua[need] = ru["u"], ru["u_abs"]
        rv = IR.interpolate(pos, None, u, *geo, u_abs=ua)
        ev = R.excess(v, rv["v"], rv["v_abs"], K)
        print("interpolation next to the new wall: excess %.3g" % ev)
        assert ev <= 1
        # the collide: the same populations on a fresh lattice that got the final mask the usual way
        S = s.L.populations()
        B = gpu.Lattice(*PDIMS, PPER, 1.0 / s.P.tau)
        B.defineBounceBack((mask != 0).astype(np.uint8))
        s.gpu.check(s.gpu.capi.lib().hcl_zero_ibm_force(s.L.ptr))
        s.L.set_populations(S); B.set_populations(S)
        s.L.collideAndStream(20); B.collideAndStream(20)
        fa, fb = s.L.populations(), B.populations()
        fluid = mask.reshape(-1) == 0
        assert np.array_equal(fa[fluid], fb[fluid]) and not np.array_equal(fa[fluid], S[fluid])
        assert B.node_counts()[1] == s.L.node_counts()[1]
    finally:
        if B is not None:
            B.destroy()
        s.destroy()


# ---- 5. hc_iterate

IDIMS, IPER = (15, 15, 15), (True, True, False)
U_TOP = 600.0 * 1e-7 * 15.0      # <shearRate> 600 1/s of the fixture's config times nz, in lattice units, as the reference's driver sets it


class Channel:
    """the fixture's 15^3 channel: floor, moving top wall, binding sites on the floor, its three platelets and one red cell"""

    def __init__(self, gpu, every, particle, solidify=True):
        self.gpu, self.P = gpu, gpu.base_parameters()
        m = gpu.read_material(os.path.join(CASE, "PLT.xml"))
        self.dist, self.shear = m["distanceThreshold"], m["shearThreshold"]
        self.L = gpu.Lattice(*IDIMS, IPER, 1.0 / self.P.tau)
        self.mask = np.zeros(IDIMS, np.uint8)
        self.mask[:, :, 0] = 1
        self.mask[:, :, -1] = 3
        self.L.defineBounceBack(self.mask)
        self.L.setBoundaryVelocity(3, (U_TOP, 0.0, 0.0))
        z = np.broadcast_to(np.arange(15.0)[None, None, :], IDIMS).reshape(-1)
        u = np.stack([U_TOP * np.clip((z - 0.5) / 13.0, 0.0, 1.0), 0 * z, 0 * z], axis=1)
        self.L.set_populations(R.to_double(R.equilibrium(R.hp(np.ones(len(z))), R.hp(u))))   # the developed Couette profile
        self.h = gpu.HemoCell(self.L, self.P)
        self.h.setParticleVelocityUpdateTimeScaleSeparation(particle)
        self.cf = self.h.cellfields
        self.plt = gpu.CellType.plt(self.P, min_triangles=int(m["minNumTriangles"]), kLink=m["kLink"], kArea=m["kArea"], kVolume=m["kVolume"],
                                    kBend=m["kBend"], eta_m=m["eta_m"], aspect_ratio=m["aspectRatio"], inner_edges=m["inner_edges"],
                                    solidify=(self.dist, self.shear) if solidify else None)
        self.rbc = gpu.CellType.rbc(self.P, radius=1.5e-6)
        self.cf.addCellType(self.plt, 1)
        self.cf.addCellType(self.rbc, 1)
        rows = [l.split() for l in open(os.path.join(CASE, "PLT.pos")).read().splitlines()[1:] if l.strip()]
        self.lifted = []
        for r in rows:
            c = [float(v) * 1e-6 / self.P.dx for v in r[:3]]
            lift = 0.0     # a row whose rotated platelet reaches a wall node is rejected, here as in the reference: lifted until it fits
            while not self.cf.addCell(0, (c[0], c[1], c[2] + lift), [float(v) for v in r[3:6]]):
                lift += 0.25
                assert lift < 2.0
            self.lifted.append(lift)
        assert len(rows) == 3 and self.cf.counts()[1] == 3
        assert self.cf.addCell(1, (10.0, 10.0, 8.0))
        if solidify:
            self.L.populateBindingSites((0, 14, 0, 14, 0, 0))
            self.cf.setSolidifyTimeScaleSeparation(every)
        self.every, self.particle = every, particle

    def state(self):
        return dict(pos=self.cf.positions, vel=self.cf.velocities, f=self.L.populations(), mask=self.L.mask(), binding=self.L.bindingSites(),
                    flags=self.cf.solidifyFlags(), ids=self.cf.cell_ids(), counts=self.cf.solidify_counts())

    def destroy(self):
        self.cf.destroy(); self.L.destroy()


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a)


def _restated_check(c, log):
    """one check on the downloaded state of channel c, by the restatement: (mask, binding, flags of the platelets that stay)"""
    nv = c.plt.nv
    pos, flags, ids = c.cf.positions, c.cf.solidifyFlags(), c.cf.cell_ids()
    alive = c.cf.alive()
    n_plt = c.cf.type_range(0)[1]
    mask, binding = c.L.mask(), c.L.bindingSites()
    tri = c.plt.tables()["triangles"]
    cells = [dict(pos=pos[k * nv:(k + 1) * nv], tri=tri, flags=flags[k * nv:(k + 1) * nv], complete=bool(alive[k * nv:(k + 1) * nv].all()),
                  enabled=True) for k in range(n_plt)]
    m01 = (mask != 0).astype(np.uint8)
    gone, nodes = SR.prepare(cells, m01, binding, IPER)
    T, _ = SR.tresca(c.L.pi_neq(), c.L.rho_u()[0], 1.0 / c.P.tau, m01)
    keep = [k for k in range(n_plt) if not gone[k]]
    want = []
    for k in keep:
        fl, _ = SR.flag(cells[k]["flags"].copy(), cells[k]["pos"], alive[k * nv:(k + 1) * nv], binding, m01, IPER, T, c.dist, c.shear)
        want.append(fl)
    log.append((int(gone.sum()), nodes, int(sum(f.any() for f in want))))
    return m01, binding, (np.concatenate(want) if want else np.zeros(0, bool)), [int(ids[k]) for k in keep]


@pytest.mark.parametrize("every, particle", [(1, 1), (5, 5), (3, 5)])
def test_iterate_equals_the_phases_in_the_reference_order(gpu, every, particle):
    """300 iterations of hc_iterate equal the same library driven phase by phase with the check between the interpolation and
    the advance (core/hemoCell.cpp:327-342), bit for bit in positions, populations, mask, binding field and flags, with
    reproducible spread on; two hc_iterate runs give the same bits; at every check the mask, the binding field and the flags
    equal the restatement evaluated on the state downloaded just before it.
    Thresholds: the fixture's own (distanceThreshold 1.5 lu, shearThreshold 100).  The developed Couette flow of the fixture's
    shear rate, 600 1/s, has a Tresca value of 300 in those units everywhere, so the platelet the fixture puts on the floor is
    flagged at the first check and solidifies at the second; between the two it is flagged and not yet solidified.  (Rotated as
    its row says, that platelet reaches below z = 0.5, where the placement rule rejects it; Channel lifts it in steps of a
    quarter node until it is placed.)"""
    lib = gpu.capi.lib()
    gpu.check(lib.hc_set_reproducible_spread(1))
    runs = []
    try:
        for _ in range(2):
            c = Channel(gpu, every, particle)
            try:
                for _ in range(6):
                    c.h.iterate(50)
                runs.append(c.state())
                assert c.L.node_counts()[1] == int((runs[-1]["mask"] == 0).sum())    # the host mask followed
            finally:
                c.destroy()
        assert _same(runs[0], runs[1])
        c = Channel(gpu, every, particle)
        try:
            log = []
            for it in range(300):
                c.cf.spreadParticleForce(True)
                c.L.collideAndStream(1)
                if it % particle == 0:
                    c.cf.interpolateFluidVelocity()
                if it % every == 0:
                    m01, binding, flags, ids = _restated_check(c, log)
                    c.cf.prepareSolidification()
                    c.cf.solidifyCells()
                    n_plt = c.cf.type_range(0)[1]
                    assert np.array_equal(c.L.mask() != 0, m01 != 0) and np.array_equal(c.L.bindingSites(), binding), it
                    assert list(c.cf.cell_ids()[:n_plt]) == ids and np.array_equal(c.cf.solidifyFlags()[:n_plt * c.plt.nv], flags), it
                c.cf.advanceParticles(False)
                c.cf.applyConstitutiveModel(it)
            phased = c.state()
        finally:
            c.destroy()
        print("checks (cells solidified, nodes, platelets flagged after): first %s, solidifying %s" %
              (log[:3], [(k, e) for k, e in enumerate(log) if e[0]]))
        assert _same(runs[0], phased), [k for k in phased if not np.array_equal(phased[k], runs[0][k])]
        assert sum(e[0] for e in log) >= 1 and phased["counts"][0] == sum(e[0] for e in log) and phased["counts"][1] == sum(e[1] for e in log) > 0
        assert any(e[2] > 0 for e in log)                  # a check that left a platelet flagged and not yet solidified
        assert not phased["flags"][-c.rbc.nv:].any()
    finally:
        gpu.check(lib.hc_set_reproducible_spread(0))


def test_feature_off_launches_the_kernels_of_today(gpu):
    """the same container with the feature never enabled: the profiler counts of 40 iterations are those of the kernels that ran
    before the feature existed, the solidify entries stay 0, and nothing is solidified; with the feature on, one entry per check"""
    lib = gpu.capi.lib()
    gpu.check(lib.hc_profile_enable(1))
    try:
        counts = {}
        for on in (False, True):
            c = Channel(gpu, 5, 5, solidify=on)
            try:
                gpu.check(lib.hc_profile_reset())
                c.h.iterate(40)
                gpu.check(lib.hc_synchronize())
                counts[on] = {k: _profile(lib, k) for k in ("collide_stream", "ibm_spread", "ibm_interpolate", "advance", "mechanics",
                                                            "solidify_prepare", "solidify_flag")}
                if not on:
                    assert not c.L.bindingSites().any() and not c.cf.solidifyFlags().any() and c.cf.solidify_counts() == (0, 0, 0)
            finally:
                c.destroy()
        assert counts[False]["collide_stream"] == 40 and counts[False]["ibm_interpolate"] == 8 and counts[False]["advance"] > 0
        assert counts[False]["solidify_prepare"] == 0 and counts[False]["solidify_flag"] == 0
        assert counts[True] == dict(counts[False], solidify_prepare=8, solidify_flag=8)
    finally:
        gpu.check(lib.hc_profile_enable(0))


# ---- 6. beside the CEPAC scalar

def _scalar_scene(gpu):
    """the 12 x 10 x 9 lattice with a floor, a driven flow, a CEPAC field with a source box and one platelet in mid-channel
    whose flags are uploaded; the check runs every 10 iterations and the count starts at 1, so it solidifies at iteration 10"""
    P = gpu.base_parameters()
    L = gpu.Lattice(*BDIMS, BPER, 1.0 / P.tau)
    mask = np.zeros(BDIMS, np.uint8)
    mask[:, :, 0] = 1
    L.defineBounceBack(mask)
    L.latticeEquilibrium()
    L.setExternalVector(SBODY)
    S = L.createCEPACfield(0.8)
    S.addSource(SBOX, 2.0)
    h = gpu.HemoCell(L, P)
    plt = gpu.CellType.plt(P, solidify=(1.5, 1e30))     # nobody is flagged by the flag pass
    h.cellfields.addCellType(plt, 1)
    _add_unchecked(gpu, h.cellfields, 0, 0)
    h.cellfields.positions = np.array([6.2, 5.1, 4.4])[None, :] + _centred(plt.tables()["vertices"])
    fl = np.zeros(plt.nv, bool)
    fl[3] = True
    h.cellfields.setSolidifyFlags(fl)
    h.cellfields.setSolidifyTimeScaleSeparation(10)
    h.iter = 1
    return P, L, S, h, mask, plt


SBODY, SBOX = (2e-5, 0.0, 0.0), (2, 3, 3, 6, 3, 5)


def test_scalar_bounces_back_from_a_node_that_turned_to_wall(gpu):
    """30 iterations, the platelet solidifies at iteration 10.  The concentration and the field's populations equal
    tests/scalar_ref.py run with the mask switched after that iteration's step (the scalar's step precedes the check), bit for
    bit on fluid nodes: once through the phases one by one, which give the restatement its flow populations and forces, and once
    through one hc_iterate call of all 30."""
    import scalar_ref as SC
    lib = gpu.capi.lib()
    gpu.check(lib.hc_set_reproducible_spread(1))
    try:
        P, L, S, h, mask, plt = _scalar_scene(gpu)
        try:
            cf = h.cellfields
            src = SC.Sources(BDIMS)
            src.add(SBOX, 2.0)
            g = SC.equilibrium(BDIMS, 1.0, mask)
            m = mask.copy()
            switched = None
            for it in range(1, 31):
                cf.spreadParticleForce(True)
                F = L.ibm_force().reshape(BDIMS + (3,))
                L.collideAndStream(1)
                f = L.populations().reshape(BDIMS + (19,))
                S.collideAndStream()
                g = SC.step(g, m, BPER, 1.0 / 0.8, SC.velocity(f, m, SBODY, F=F), src)
                got = S.populations().reshape(g.shape)
                assert np.array_equal(got[m == 0], g[m == 0]), it
                cf.interpolateFluidVelocity()
                if it % 10 == 0:
                    cf.prepareSolidification(); cf.solidifyCells()
                    now = (L.mask() != 0).astype(np.uint8)
                    if switched is None and not np.array_equal(now, m):
                        switched = it
                    m = now
                cf.advanceParticles(False)
                cf.applyConstitutiveModel(it)
            assert switched == 10 and cf.counts()[1] == 0 and int((m != mask).sum()) == cf.solidify_counts()[1] > 3
            want_C = SC.concentration(g, m, src)
            assert np.array_equal(S.concentration().reshape(BDIMS)[m == 0], want_C[m == 0])
            assert want_C[2, 4, 4] == 2.0 and 1.0 < want_C[5, 5, 4] < 2.0       # the source holds, and the field has reached the platelet's place
            phased_g = g
        finally:
            h.cellfields.destroy(); L.destroy()
        P, L, S, h, mask, plt = _scalar_scene(gpu)
        try:
            h.iterate(30)
            assert h.iter == 31 and h.cellfields.counts()[1] == 0
            assert np.array_equal(L.mask() != 0, m != 0)
            got = S.populations().reshape(phased_g.shape)
            assert np.array_equal(got[m == 0], phased_g[m == 0])
            assert np.array_equal(S.concentration().reshape(BDIMS)[m == 0], want_C[m == 0])
        finally:
            h.cellfields.destroy(); L.destroy()
    finally:
        gpu.check(lib.hc_set_reproducible_spread(0))


# ---- 7. refusals

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


@pytest.mark.parametrize("what", ["slabs", "open_boundary", "lees_edwards", "interior_viscosity", "pre_inlet"])
@pytest.mark.parametrize("first", ["other", "solidify"])
def test_combinations_are_refused_in_both_orders(gpu, what, first):
    """slabs, open boundaries, Lees-Edwards, interior viscosity and a pre-inlet: refused by the solidify entry points when the
    other feature is there already, and by hc_iterate when it came second.  Nothing is changed by a refused call."""
    extra = []
    if what == "slabs":
        P, L = _small(gpu, x0=0, nx_global=32, n_slabs=2)
    elif what == "lees_edwards":
        P = gpu.base_parameters()
        L = gpu.Lattice(16, 12, 12, (True, True, True), 1.0 / P.tau)
    elif what == "open_boundary":
        P, L = _small(gpu, periodic=(False, False, False))
    else:
        P, L = _small(gpu)

    def other():
        if what == "open_boundary":
            L.addVelocityBoundary0N((0, 0, 1, 10, 0, 11))
        elif what == "lees_edwards":
            L.setLeesEdwards(0.01, -0.01)
        elif what == "interior_viscosity":
            L.enableInteriorViscosity([0.8])
        elif what == "pre_inlet":
            D = gpu.Lattice(16, 12, 12, (False, False, False), 1.0 / P.tau)
            extra.append(D)
            yz = np.array([(y, z) for y in range(1, 11) for z in range(12)])
            extra.insert(0, gpu.PreInlet(L, D, yz, 8, 0, "Xneg", device=True))   # L is the pre-inlet lattice of the pair
    cf = None
    try:
        cf = gpu.Cells(L, P)
        cf.addCellType(gpu.CellType.plt(P), 1)
        word = dict(slabs="one domain", open_boundary="open boundaries", lees_edwards="Lees-Edwards", interior_viscosity="interior viscosity",
                    pre_inlet="pre-inlet")[what]
        if first == "other" or what == "slabs":
            other()
            _refused(gpu, lambda: L.populateBindingSites((0, 15, 0, 0, 0, 11)), "solidify", word)
            _refused(gpu, lambda: cf.enableSolidifyMechanics(0, 1.5, 100.0), "solidify", word)
            _refused(gpu, cf.prepareSolidification, "solidify")
            _refused(gpu, cf.solidifyCells, "solidify")
            assert not L.bindingSites().any() and cf.solidify_counts() == (0, 0, 0)
        else:
            L.populateBindingSites((0, 15, 0, 0, 0, 11))
            cf.enableSolidifyMechanics(0, 1.5, 100.0)
            sites = L.bindingSites()
            assert sites.any() or what == "lees_edwards"
            other()
            h = gpu.HemoCell(L, P)
            h.cellfields.destroy()
            h.cellfields = cf
            f0 = L.populations()
            _refused(gpu, lambda: h.iterate(1), "hc_iterate", "solidify", word)
            assert h.iter == 0 and np.array_equal(L.populations(), f0) and np.array_equal(L.bindingSites(), sites)
    finally:
        for e in extra:
            e.destroy()
        if cf is not None:
            cf.destroy()
        L.destroy()


def test_wrong_model_and_thresholds_are_refused(gpu):
    P, L = _small(gpu)
    cf = gpu.Cells(L, P)
    try:
        cf.addCellType(gpu.CellType.rbc(P), 1)
        cf.addCellType(gpu.CellType.plt(P), 1)
        _refused(gpu, lambda: cf.enableSolidifyMechanics(0, 1.5, 100.0), "HC_MODEL_PLT_SIMPLE")
        _refused(gpu, lambda: cf.enableSolidifyMechanics(1, -0.1, 100.0), "negative")
        _refused(gpu, lambda: cf.enableSolidifyMechanics(1, 1.5, -1.0), "negative")
        _refused(gpu, lambda: cf.enableSolidifyMechanics(1, float("nan"), 1.0), "negative")
        _refused(gpu, lambda: cf.enableSolidifyMechanics(2, 1.5, 100.0), "unknown cell type")
        _refused(gpu, lambda: cf.setSolidifyTimeScaleSeparation(0), "timescale")
        _refused(gpu, cf.prepareSolidification, "hcp_type_set_solidify")
        _refused(gpu, lambda: cf.setSolidifyFlags(np.zeros(0, bool)), "hcp_type_set_solidify")
        assert cf.solidify_counts() == (0, 0, 0)
        cf.enableSolidifyMechanics(1, 1.5, 100.0)
        cf.prepareSolidification()                         # no cells yet: nothing to do, nothing refused
        cf.solidifyCells()
    finally:
        cf.destroy(); L.destroy()
