"""tests/repulsion_ref.py against the CPU oracle at every periodic and open edge (no GPU).

The oracle's orc_sim_repulsion, orc_sim_boundary_repulsion and orc_sim_advance (both deletion modes) against the
plain restatement on all eight periodicity triples of a 12 x 10 x 11 lattice and on a periodic axis of length 3, where
bins wrap both ways.  The inputs are those of tests/test_gpu_repulsion_edges.py, and the conditions that keep a
comparison from passing on nothing are asserted here from the restatement alone, so the GPU tests inherit inputs
known to be sufficient."""
import ctypes as C
import itertools

import numpy as np
import pytest

from oracle import oracle as O
from tests import repulsion_ref as R

TRIPLES = list(itertools.product((0, 1), repeat=3))
CASES = [(p, R.DIMS) for p in TRIPLES] + [((0, 1, 0), (12, 3, 11))]
IDS = ["".join(map(str, p)) + ("" if d == R.DIMS else "-ny3") for p, d in CASES]
K_REP, K_WALL = 2e-6, 3e-6


class OracleCase:
    """an oracle lattice and simulation that hold the cells of a built case at the case's positions"""

    def __init__(self, orc, case, dims, periodic, mask=None, mode="particle"):
        self.orc = orc
        self.P = O.make_params(orc)
        self.L = O.OracleLattice(orc, dims[0], dims[1], dims[2], periodic, 1.0 / self.P.tau)
        self.L.init_equilibrium()
        self.S = orc.orc_sim_create(self.L.ptr, C.byref(self.P))
        self.types = [O.make_rbc(orc, self.P), O.make_plt(orc, self.P)]
        for T in self.types:
            orc.orc_sim_add_type(self.S, T)
        centre, angles = np.array([5.0, 5.0, 5.0]), np.zeros(3)
        for nv in case["sizes"]:                     # placed before the mask is set: nothing is refused
            assert orc.orc_sim_add_cell(self.S, {R.NV_RBC: 0, R.NV_PLT: 1}[nv], O.dptr(centre), O.dptr(angles), 0.0)
        if mask is not None:
            self.L.set_mask(mask)
        self.S.contents.deletion_mode = {"particle": 0, "cell": 1}[mode]
        self.set(0, case["pos"])

    def set(self, what, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        assert a.shape == (self.S.contents.np, 3)
        self.orc.orc_sim_set(self.S, what, O.dptr(a))

    def get(self, what):
        out = np.zeros((self.S.contents.np, 3))
        self.orc.orc_sim_get(self.S, what, O.dptr(out))
        return out

    def alive(self):
        a = np.ones(self.S.contents.np, dtype=np.uint8)
        self.orc.orc_sim_get_alive(self.S, a.ctypes.data)
        return a.astype(bool)

    def advance(self, vel=None):
        self.set(1, np.zeros((self.S.contents.np, 3)) if vel is None else vel)
        self.orc.orc_sim_advance(self.S)

    def destroy(self):
        self.orc.orc_sim_destroy(self.S)
        for T in self.types:
            self.orc.orc_celltype_destroy(T)
        self.L.destroy()


_built = {}


def built(periodic, dims):
    """the case, its mask, what the restatement says of it, and the counts that show it sufficient; computed once"""
    key = (tuple(periodic), tuple(dims))
    if key not in _built:
        case, mask = R.build_case(periodic, dims), R.block_mask(dims)
        alive = ~R.tagged(case["pos"], mask, periodic)
        ref = R.repulsion(case["pos"], case["cell_of"], alive, dims, periodic, K_REP, R.CUTOFF)
        wrong = {w: R.repulsion(case["pos"], case["cell_of"], alive, dims, periodic, K_REP, R.CUTOFF, wrong=w) for w in R.WRONG}
        cond = R.conditions(ref, wrong["bin_outside"], case["pos"], alive, dims, periodic, case)
        _built[key] = dict(case=case, mask=mask, alive=alive, ref=ref, wrong=wrong, cond=cond)
    return _built[key]


def ratio(got, ref):
    """largest |got - ref| in units of the bound; a vertex without terms has to read exactly 0"""
    b = R.bound(ref)
    d = np.abs(got - ref["sum"])
    assert (d[b == 0] == 0).all()
    return float((d[b > 0] / b[b > 0]).max()) if (b > 0).any() else 0.0


def wrong_by(got, ref_wrong):
    """largest |got - wrong restatement| in units of the bound"""
    b = R.bound(ref_wrong)
    d = np.abs(got - ref_wrong["sum"])
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(d > 0, d / b, 0.0)
    return float(q.max())


def test_builder_properties():
    """spacing, bin occupancy, ties and the cut-off pair, as the issue of the inputs states them"""
    for periodic, dims in CASES:
        case = R.build_case(periodic, dims)
        pos, n = case["pos"], np.array(dims, dtype=np.float64)
        assert len(pos) == sum(case["sizes"]) and case["sizes"][0] == R.NV_RBC and set(case["sizes"][1:]) == {R.NV_PLT}
        assert np.array_equal(case["cell_of"], np.repeat(np.arange(len(case["sizes"])), case["sizes"]))
        per = np.array(periodic, dtype=bool)
        closest = np.inf
        for i in range(len(pos) - 1):
            d = pos[i] - pos[i + 1:]
            d[:, per] -= n[per] * np.rint(d[:, per] / n[per])
            closest = min(closest, np.sqrt((d * d).sum(axis=1)).min())
        assert closest >= 0.05
        node = R.nearest_node(pos)
        inside = R.in_grid(node, dims, periodic)
        _, counts = np.unique(np.mod(node[inside], dims), axis=0, return_counts=True)
        assert counts.max() <= 10
        assert (np.mod(pos, 1.0) == 0.5).sum() >= 8                         # ties of floor(x + 0.5)
        for a in range(3):
            got = set(node[:, a]) if not periodic[a] else set()
            assert periodic[a] or {-3, -2, -1, dims[a], dims[a] + 1} <= got
        (i, j), (k, l) = case["cut"], case["twin"]
        assert pos[j, 0] - pos[i, 0] == R.CUTOFF and np.array_equal(pos[i, 1:], pos[j, 1:])
        assert pos[l, 2] - pos[k, 2] == np.nextafter(R.CUTOFF, 0.0) and np.array_equal(pos[k, :2], pos[l, :2])
        if per.any():                                                       # whole cells on other laps
            lap = np.round((pos[case["cell_of"] == 1].mean(0) - pos[case["cell_of"] == 3].mean(0)) / n)
            assert np.array_equal(lap[per], 2 * np.ones(per.sum()))
            lap = np.round((pos[case["cell_of"] == 2].mean(0) - pos[case["cell_of"] == 3].mean(0)) / n)
            assert np.array_equal(lap[per], -np.ones(per.sum()))


@pytest.mark.parametrize("periodic,dims", CASES, ids=IDS)
def test_inputs_are_sufficient(periodic, dims):
    """>= 50 interacting pairs, >= 5 same-bin pairs, >= 5 pairs through every periodic face, >= 5 out-of-grid vertices
    that binning them would make interact, the exact cut-off pair silent and its twin not; every wrong restatement
    moves a vertex by >= 100 x the bound where the case can show it"""
    b = built(periodic, dims)
    R.check_conditions(b["cond"], periodic)
    assert (~b["alive"]).sum() >= 20
    for w, res in b["wrong"].items():
        if (w == "no_min_image" and not any(periodic)) or (w == "bin_outside" and all(periodic)):
            assert np.array_equal(res["sum"], b["ref"]["sum"])              # nothing for it to get wrong here
            continue
        assert wrong_by(b["ref"]["sum"], res) >= 100.0, w


@pytest.mark.parametrize("periodic,dims", CASES, ids=IDS)
def test_oracle_tagging_and_repulsion(orc, periodic, dims):
    """advance in particle mode removes exactly tagged(); the repulsion of what is left is within the bound of the
    restatement, which agrees with its all-longdouble twin to the rounding of the terms"""
    b = built(periodic, dims)
    case, ref = b["case"], b["ref"]
    oc = OracleCase(orc, case, dims, periodic, b["mask"])
    try:
        oc.advance()
        assert np.array_equal(oc.get(0), case["pos"])
        assert np.array_equal(oc.alive(), b["alive"]) and oc.S.contents.particles_deleted == (~b["alive"]).sum()
        oc.set(3, np.full(case["pos"].shape, 7.0))                          # applyRepulsionForce zeroes what it does not touch
        orc.orc_sim_repulsion(oc.S, K_REP, R.CUTOFF)
        r = oc.get(3)
    finally:
        oc.destroy()
    q = ratio(r, ref)
    print("oracle / bound", q)
    assert q <= 1.0
    assert np.abs(r.sum(0)).max() <= 4 * ref["k"].sum() * R.U * ref["abs"].sum(0).max()   # action = reaction
    for i in case["cut"]:
        assert not r[i].any()
    for i in case["twin"]:
        assert r[i, 2] != 0.0
    # coordinates stay below 64, so a separation carries at most 2^-53 * 64 of rounding, against distances >= 0.05:
    # the float64 terms are within 3 * 7.2e-15 / 0.05 + a few 2^-53 < 1e-12 of the exact ones
    full = R.repulsion(case["pos"], case["cell_of"], b["alive"], dims, periodic, K_REP, R.CUTOFF, full=True)
    assert np.abs(np.abs(case["pos"]).max()) < 64.0
    assert (np.abs(full["sum"] - ref["sum"]) <= 1e-12 * ref["abs"]).all()
    for w, res in b["wrong"].items():                                       # the oracle is none of the wrong ones
        if not np.array_equal(res["sum"], ref["sum"]):
            assert wrong_by(r, res) >= 100.0, w


@pytest.mark.parametrize("periodic,dims", CASES, ids=IDS)
def test_oracle_boundary_repulsion_bit_for_bit(orc, periodic, dims):
    b = built(periodic, dims)
    case, mask = b["case"], b["mask"]
    flag = R.boundary_flags(mask, periodic)
    if periodic[0]:
        assert flag[0, 2, 5]                                                # its only fluid neighbours lie across the x seam
    elif dims[1] > 5:
        assert mask[0, 2, 5] and not flag[0, 2, 5] and flag[1, 4, 5]
    oc = OracleCase(orc, case, dims, periodic, mask)
    try:
        oc.advance()
        r0 = np.zeros(case["pos"].shape)
        for call in (1, 2):
            orc.orc_sim_boundary_repulsion(oc.S, K_WALL, R.CUTOFF)
            r, r_hp = R.boundary_repulsion(case["pos"], b["alive"], mask, periodic, K_WALL, R.CUTOFF, r0)
            got = oc.get(3)
            assert np.array_equal(got, r), call
            assert np.abs(r - r_hp).max() <= 64 * R.U * np.abs(r_hp).max()  # at most 2 x 27 terms of a few roundings each
            r0 = r
        touched = np.abs(r).sum(1) > 0
        outside = ~R.in_grid(R.nearest_node(case["pos"]), dims, periodic)
        assert touched.sum() >= 20 and not touched[~b["alive"]].any() and not touched[outside].any()
    finally:
        oc.destroy()


@pytest.mark.parametrize("periodic,dims", CASES, ids=IDS)
def test_oracle_cell_mode_tagging(orc, periodic, dims):
    """cell mode: a cell with a tagged vertex is gone at once"""
    b = built(periodic, dims)
    case = b["case"]
    gone = np.array([(~b["alive"])[case["cell_of"] == c].any() for c in range(len(case["sizes"]))])
    oc = OracleCase(orc, case, dims, periodic, b["mask"], mode="cell")
    try:
        oc.advance()
        assert oc.S.contents.cells_deleted == gone.sum() and oc.S.contents.np == sum(s for s, g in zip(case["sizes"], gone) if not g)
        assert np.array_equal(oc.get(0), case["pos"][~gone[case["cell_of"]]])
    finally:
        oc.destroy()


@pytest.mark.parametrize("mode", ["particle", "cell"])
def test_oracle_gone_and_incomplete_cells(orc, mode):
    """a cell that loses vertices at a wall in one advance: the lost ones (the whole cell in cell mode) neither push
    nor are pushed, in both repulsions"""
    g = R.build_gone_case()
    periodic, dims = (1, 1, 0), R.DIMS
    end = g["pos"] + g["vel"]
    lost = R.tagged(end, g["mask"], periodic)
    assert 10 <= lost.sum() < R.NV_PLT and not lost[R.NV_PLT:].any()
    alive = ~lost if mode == "particle" else g["cell_of"] != 0
    ref = R.repulsion(end, g["cell_of"], alive, dims, periodic, K_REP, R.CUTOFF)
    push = R.repulsion(end, g["cell_of"], alive, dims, periodic, K_REP, R.CUTOFF, wrong="dead_push")
    assert (ref["k"][R.NV_PLT:2 * R.NV_PLT] > 0).sum() >= 10 and wrong_by(ref["sum"], push) >= 100.0
    oc = OracleCase(orc, g, dims, periodic, g["mask"], mode)
    try:
        oc.advance(g["vel"])
        keep = np.ones(len(end), dtype=bool) if mode == "particle" else g["cell_of"] != 0
        assert np.array_equal(oc.get(0), end[keep]) and np.array_equal(oc.alive(), alive[keep])
        orc.orc_sim_repulsion(oc.S, K_REP, R.CUTOFF)
        r = oc.get(3)
        sub = dict(sum=ref["sum"][keep], abs=ref["abs"][keep], k=ref["k"][keep])
        assert ratio(r, sub) <= 1.0
        orc.orc_sim_boundary_repulsion(oc.S, K_WALL, R.CUTOFF)
        rb, _ = R.boundary_repulsion(end, alive, g["mask"], periodic, K_WALL, R.CUTOFF, ref["sum"] * 0 + _scatter(r, keep, len(end)))
        assert np.array_equal(oc.get(3), rb[keep]) and np.abs(rb[keep] - r).max() > 0
    finally:
        oc.destroy()


def _scatter(r, keep, n):
    out = np.zeros((n, 3))
    out[keep] = r
    return out
