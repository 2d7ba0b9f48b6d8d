"""tests/ibm_ref.py and tests/ibm_cases.py without a GPU: the restatement against the CPU oracle on every crafted case, the
cases' preconditions (ibm_ref.predict against the caps of hemocell_amd/csrc/ibm_common.h, so that a changed TILE_CAP or NODE_CAP
fails here instead of moving the edges silently), the mutation controls against the right restatement, and the pinned
constants and visiting orders."""
import ctypes as C
import os
import re
import zlib

import numpy as np
import pytest

from oracle import oracle as O
from tests import ibm_cases as IC
from tests import ibm_ref as IR
from tests import observables_ref as R
from tests import open_boundary_ref as OB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = IC.K              # the constant of the conditioned bound (observables_ref.excess); see test_rounding_figure_behind_k
FAIL_BY = 100.0       # a wrong restatement must miss the bound by this factor


def _src(*path):
    return open(os.path.join(ROOT, *path)).read()


def test_pinned_constants_and_orders(orc):
    ibm, common, cells_h = _src("hemocell_amd", "csrc", "ibm.hip"), _src("hemocell_amd", "csrc", "common.h"), _src("hemocell_amd", "csrc", "cells.h")
    ibm_h = _src("hemocell_amd", "csrc", "ibm_common.h")
    assert int(re.search(r"constexpr int TILE_CAP = (\d+);", ibm_h).group(1)) == IC.TILE_CAP == 18 ** 3
    assert int(re.search(r"constexpr int NODE_CAP = (\d+);", ibm_h).group(1)) == IC.NODE_CAP
    assert int(re.search(r"constexpr int NVPT = (\d+);", ibm_h).group(1)) == IC.NVPT
    assert int(re.search(r"constexpr int HALO = (\d+);", common).group(1)) == IC.HALO
    assert (ibm + ibm_h).count("dim3(nv > 128 ? 256 : 128)") == 1            # the block size rule of ibm_cases.BLOCK, stated once
    assert "nb[0] * nb[1] * nb[2] > 64" in ibm_h and "n >> 3" in ibm          # 64 bricks per wave, 8 XCD ranges
    assert "const int idx = i * 4 + j * 2 + k;" in cells_h                    # the kernels' visiting order: OFFSETS
    assert [tuple(o) for o in IR.OFFSETS] == [(i, j, k) for i in range(2) for j in range(2) for k in range(2)]
    # D3Q19: observables_ref.C is the oracle's orc_c (test_observables_cpu checks the copy); the stencil order is the oracle's
    # ascending (dx, dy, dz) loop: at a generic interior point both list the same 8 nodes in the same order
    L = O.OracleLattice(orc, 9, 8, 7, (0, 0, 0), 1.0)
    p = np.array([4.3, 3.6, 2.2])
    nodes, w = np.zeros(8, np.int64), np.zeros(8)
    assert orc.orc_phi2_stencil(L.ptr, O.dptr(p), O.lptr(nodes), O.dptr(w)) == 8
    rn, rw, ra = IR.stencil(p[None], (9, 8, 7), (0, 0, 0), None)
    assert ra.all() and np.array_equal(rn[0], nodes) and R.excess(w, R.to_double(rw[0]), R.to_double(rw[0]), 4) <= 1
    L.destroy()


def _f_limit(orc):
    return O.make_params(orc).f_limit


def tiled(case, c, pred):
    kind = case["kinds"][c]
    return bool(pred["vol"] <= IC.TILE_CAP and not pred["exceeds"] and pred["nodes"] <= IC.NODE_CAP and IC.NV[kind] <= IC.NVPT * IC.BLOCK[kind])


def check_expectations(case):
    """every cell the case makes a claim about sits where the claim puts it"""
    sl = IC.cell_slices(case)
    for c, want in case["expect"].items():
        pred = IR.predict(case["pos"][sl[c]], case["alive"][sl[c]], case["dims"], case["periodic"], case["mask"], pad_x=IC.HALO)
        for key, val in want.items():
            if key == "tiled":
                assert tiled(case, c, pred) == val, (case["name"], c, pred)
            elif key == "vol_all_gt":
                assert IR.predict(case["pos"][sl[c]], None, case["dims"], case["periodic"], case["mask"])["vol"] > val, (case["name"], c)
            else:
                assert pred[key] == val, (case["name"], c, key, pred)
    # no particle with all its nodes masked or outside: the weights would be 0 / 0 in the reference too
    nodes, _, adm = IR.stencil(case["pos"], case["dims"], case["periodic"], case["mask"])
    assert adm[case["alive"]].any(axis=1).all(), case["name"]


@pytest.mark.parametrize("name", IC.NAMES)
def test_case_preconditions(orc, name):
    case = IC.build(name, _f_limit(orc))
    check_expectations(case)
    assert case["controls"], name
    n = sum(IC.NV[k] for k in case["kinds"])
    assert case["pos"].shape == case["force"].shape == (n, 3) and case["alive"].shape == (n,)
    if case["kill_pos"] is not None:       # the particles to remove, and only they, start on a boundary node
        b = np.floor(case["kill_pos"] + 0.5).astype(int)
        solid = case["mask"][b[:, 0] % case["dims"][0], b[:, 1], b[:, 2]] != 0
        assert np.array_equal(solid, ~case["alive"])


def test_caps_from_both_sides(orc):
    """the cases around TILE_CAP and NODE_CAP differ from their neighbours by what the names say, and a zero-weight node
    does not count: with 'admit_zero_weight' the vertex on a node would bring 8 nodes instead of 1"""
    fl = _f_limit(orc)
    def pred(name, wrong=None):
        c = IC.build(name, fl)
        return IR.predict(c["pos"], None, c["dims"], c["periodic"], c["mask"], wrong=wrong)
    assert pred("tile_18_18_18")["vol"] == IC.TILE_CAP and pred("tile_19_18_17")["vol"] == 5814 and pred("tile_18_18_19")["vol"] == 6156
    assert [pred(n)["nodes"] for n in ("nodes_1535", "nodes_1536", "nodes_1537")] == [IC.NODE_CAP - 1, IC.NODE_CAP, IC.NODE_CAP + 1]
    assert pred("nodes_1537", "admit_zero_weight")["nodes"] == IC.NODE_CAP + 8
    assert pred("nodes_1535", "admit_zero_weight")["nodes"] > IC.NODE_CAP
    assert pred("bricks_64")["bricks"] == 64 and pred("bricks_65")["bricks"] == 65
    for n in ("thin_2_2_1458", "thin_2_1458_2", "thin_1458_2_2", "thin_3_2_972", "thin_2_3_972_seam", "thin_whole_axis", "thin_axis_plus_one"):
        assert pred(n)["vol"] == IC.TILE_CAP and pred(n)["nodes"] <= IC.NODE_CAP, n


def _oracle_case(orc, case):
    Po = O.make_params(orc)
    Lo = O.OracleLattice(orc, *case["dims"], case["periodic"], 1.0 / 0.9)
    if case["mask"] is not None:
        Lo.set_mask(case["mask"])
    if case["open"] is not None:
        Lo.set_open_boundary(case["open"]["code"], case["open"]["val"])
    So = orc.orc_sim_create(Lo.ptr, C.byref(Po))
    make = dict(rbc=lambda: O.make_rbc(orc, Po), plt=lambda: O.make_plt(orc, Po), big=lambda: O.make_rbc(orc, Po, min_tri=IC.BIG_MIN_TRIANGLES))
    seat, zero = np.array(case["seat"], dtype=np.float64), np.zeros(3)
    types = []
    for t in IC.TYPES:
        if case["counts"][t]:
            T = make[t]()
            assert T.contents.nv == IC.NV[t]
            ti = orc.orc_sim_add_type(So, T)
            types.append(T)
            for _ in range(case["counts"][t]):
                assert orc.orc_sim_add_cell(So, ti, O.dptr(seat), O.dptr(zero), 0.0)
    assert So.contents.np == len(case["pos"])
    return Po, Lo, So, types


def _random_state(case):
    rng = np.random.default_rng(zlib.crc32(("s" + case["name"]).encode()))
    n = int(np.prod(case["dims"]))
    t = np.array([1 / 3] + [1 / 18] * 3 + [1 / 36] * 6 + [1 / 18] * 3 + [1 / 36] * 6)
    return 0.01 * rng.standard_normal((n, 19)) * t[None, :]


def _node_velocity(case, f, F, need):
    """observables_ref.rho_u (post-stream populations f, body plus spread force F) on the nodes an interpolation reads
    -> (u, u_abs) [nodes][3], zero elsewhere.  A fluid node of a Zou-He plane shows the moments of its completed populations
    (open_boundary_ref.observe, plain double in the kernels' order: the completion has no extended-precision restatement);
    their error scale is that of the plain moments plus |u|."""
    u, ua = np.zeros((len(f), 3)), np.zeros((len(f), 3))
    ru = R.rho_u(f[need], F[need])
    u[need], ua[need] = ru["u"], ru["u_abs"]
    if case["open"] is not None:
        dims, code = tuple(case["dims"]), case["open"]["code"]
        _, uo, _ = OB.observe(f.reshape(dims + (19,)), case["mask"], case["periodic"], (0.0, 0.0, 0.0), F.reshape(dims + (3,)), code, case["open"]["val"])
        completed = need[((code.reshape(-1) >= 0) & (case["mask"].reshape(-1) == 0))[need]]
        u[completed] = uo.reshape(-1, 3)[completed]
        ua[completed] += np.abs(u[completed])
    return u, ua


@pytest.mark.parametrize("name", IC.NAMES)
def test_restatement_vs_oracle(orc, name):
    """orc_sim_spread / orc_sim_interpolate on the case: every node's force, the capped forces and every particle's velocity
    within the conditioned bound (the oracle is plain double in the reference's order; bit equality is not asked for)"""
    case = IC.build(name, _f_limit(orc))
    Po, Lo, So, types = _oracle_case(orc, case)
    try:
        pos, frc, alive = case["pos"], case["force"], case["alive"]
        geo = (case["dims"], case["periodic"], case["mask"])
        orc.orc_sim_set(So, 0, O.dptr(pos)); orc.orc_sim_set(So, 2, O.dptr(np.ascontiguousarray(frc)))
        sentinel = np.full(pos.shape, 123.25)
        orc.orc_sim_set(So, 1, O.dptr(sentinel))
        dead = (~alive).astype(np.uint8)
        C.memmove(So.contents.dead, dead.ctypes.data, len(dead))
        So.contents.force_limit_enabled = 1 if case["limit"] else 0
        Lo.f[:] = _random_state(case)
        orc.orc_sim_spread(So)
        ref = IR.spread(pos, frc, None, alive, *geo, f_limit=Po.f_limit if case["limit"] else None)
        Fo = Lo.force.copy()
        assert R.excess(Fo, ref["F"], ref["F_abs"], K) <= 1
        assert (Fo[~ref["touched"]] == 0.0).all()
        f_after = np.zeros_like(pos); orc.orc_sim_get(So, 2, O.dptr(f_after))
        assert R.excess(f_after, ref["force"], ref["force_abs"], K) <= 1
        assert np.array_equal(f_after[~alive], frc[~alive])
        # the plain double restatement in storage order is what the oracle holds, bit for bit
        dbl = IR.spread_double(pos, frc, None, alive, *geo, f_limit=Po.f_limit if case["limit"] else None)
        assert np.array_equal(dbl["F"], Fo) and np.array_equal(dbl["force"], f_after)
        Lo.force[:] += np.array(case["body"])[None, :]
        Ftot = Lo.force.copy()
        orc.orc_sim_interpolate(So)
        v = np.zeros_like(pos); orc.orc_sim_get(So, 1, O.dptr(v))
        u, ua = _node_velocity(case, Lo.f, Ftot, IR.needed_nodes(pos, alive, *geo))
        rv = IR.interpolate(pos, alive, u, *geo, u_abs=ua)
        assert R.excess(v[alive], rv["v"][alive], rv["v_abs"][alive], K) <= 1
        assert np.array_equal(v[~alive], sentinel[~alive])
    finally:
        orc.orc_sim_destroy(So); Lo.destroy()
        for T in types:
            orc.orc_celltype_destroy(T)


def mutation_excess(case, f_limit, F, v, u, ua):
    """for every control of the case: how far the values F (node forces) and v (particle velocities, NaN where a
    particle was not written) miss the WRONG restatement, in units of the bound of the right one -> {control: (spread, interpolate)}"""
    geo = (case["dims"], case["periodic"], case["mask"])
    pos, frc, alive = case["pos"], case["force"], case["alive"]
    right = IR.spread(pos, frc, None, alive, *geo, f_limit=f_limit)
    right_v = IR.interpolate(pos, alive, u, *geo, u_abs=ua)
    out = {}
    for wrong in case["controls"]:
        ws = IR.spread(pos, frc, None, alive, *geo, f_limit=f_limit, wrong=wrong)
        es = R.excess(F, ws["F"], right["F_abs"], K)
        if wrong == "no_cap":
            out[wrong] = (es, None)
            continue
        wv = IR.interpolate(pos, alive, u, *geo, u_abs=ua, wrong=wrong)
        written = alive if wrong != "dead_take_part" else np.ones(len(pos), bool)
        scale = np.where(alive[:, None], right_v["v_abs"], np.abs(wv["v"]))       # a removed particle has no right value
        with np.errstate(invalid="ignore"):
            ev = R.excess(np.where(np.isnan(v), 1e30, v)[written], wv["v"][written], scale[written], K)
        out[wrong] = (es, ev)
    return out


@pytest.mark.parametrize("name", IC.NAMES)
def test_mutation_controls_vs_right_restatement(orc, name):
    """the right restatement (standing in for a right kernel) misses each wrong one the case names by at least FAIL_BY bounds"""
    fl = _f_limit(orc)
    case = IC.build(name, fl)
    geo = (case["dims"], case["periodic"], case["mask"])
    F = IR.spread(case["pos"], case["force"], None, case["alive"], *geo, f_limit=fl)["F"]
    u = 0.01 * np.random.default_rng(5).standard_normal(F.shape)       # any node velocities will do here
    ua = np.abs(u)
    v = IR.interpolate(case["pos"], case["alive"], u, *geo, u_abs=ua)["v"]
    v[~case["alive"]] = np.nan
    for wrong, (es, ev) in mutation_excess(case, fl, F, v, u, ua).items():
        assert es > FAIL_BY and (ev is None or ev > FAIL_BY), (name, wrong, es, ev)


def test_rounding_figure_behind_k(orc):
    """the largest |double - extended| / (2^-53 * abs) of the plain double restatement, summed in storage order and the
    other way round, over every case.  It is 5.61 (spread, nodes_1535); the project's k = 16 is less than four times
    that, so K is four times the figure, 22.44: the kernels add in hardware order and round 1 / total once more"""
    fl = _f_limit(orc)
    worst = 0.0
    for name in IC.NAMES:
        case = IC.build(name, fl)
        geo = (case["dims"], case["periodic"], case["mask"])
        pos, frc, alive = case["pos"], case["force"], case["alive"]
        ref = IR.spread(pos, frc, None, alive, *geo, f_limit=fl)
        f = _random_state(case)
        need = IR.needed_nodes(pos, alive, *geo)
        u, ua = _node_velocity(case, f, ref["F"] + np.array(case["body"])[None, :], need)
        rv = IR.interpolate(pos, alive, u, *geo, u_abs=ua)
        for rev in (False, True):
            d = IR.spread_double(pos, frc, None, alive, *geo, f_limit=fl, reverse=rev)
            worst = max(worst, R.excess(d["F"], ref["F"], ref["F_abs"], 1.0), R.excess(d["force"], ref["force"], ref["force_abs"], 1.0))
            dv = IR.interpolate_double(pos, alive, u, *geo, reverse=rev)
            worst = max(worst, R.excess(dv[alive], rv["v"][alive], rv["v_abs"][alive], 1.0))
    print("largest |double - extended| / (2^-53 abs) over %d cases, two orders: %.3f" % (len(IC.NAMES), worst))
    assert 4.0 * worst <= K < 4.0 * worst + 0.1
