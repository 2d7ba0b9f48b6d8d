"""tests/ibm_wide_ref.py and tests/ibm_wide_cases.py without a GPU: the properties of the three- and four-point delta
functions, where their branches and the floor ties sit, the cases' preconditions against the caps of
hemocell_amd/csrc/ibm_common.h (a changed cap fails here instead of moving an edge silently), the mutation control of every
case (the other width) against the right restatement, the rounding figure behind the bound of the GPU tests, and a facade
driver that assigns both new names to HemoCellField::kernelMethod.

Nothing here is compared with the oracle, which knows the two-point kernel only."""
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import oracle as O
from tests import ibm_cases as IC
from tests import ibm_ref as IR
from tests import ibm_wide_cases as WC
from tests import ibm_wide_ref as WR
from tests import observables_ref as R
from tests.test_ibm_ref_cpu import _node_velocity, _random_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 16.0              # the project's constant of the conditioned bound; see test_rounding_figure_behind_k
FAIL_BY = 100.0       # a restatement of the wrong width must miss the bound by this factor
SUM_SQUARES = {3: 0.5, 4: 0.375}


def _src(*path):
    return open(os.path.join(ROOT, *path)).read()


def _f_limit(orc):
    return O.make_params(orc).f_limit


def test_pinned_constants():
    wide, hdr = _src("hemocell_amd", "csrc", "ibm_common.h"), _src("include", "hemocell_amd.h")
    for W in WR.WIDTHS:
        assert int(re.search(r"constexpr int TILE_CAP%d = (\d+);" % W, wide).group(1)) == WC.TILE_CAP[W] == (16 + W) ** 3
        assert int(re.search(r"constexpr int NODE_CAP%d = (\d+);" % W, wide).group(1)) == WC.NODE_CAP[W]
        assert int(re.search(r"#define HC_IBM_PHI%d (\d)" % W, hdr).group(1)) == W
    assert int(re.search(r"#define HC_IBM_PHI2 (\d)", hdr).group(1)) == 2
    assert int(re.search(r"constexpr int NVPT = (\d+);", wide).group(1)) == IC.NVPT
    assert (wide + _src("hemocell_amd", "csrc", "ibm.hip")).count("dim3(nv > 128 ? 256 : 128)") == 1   # the block size rule of ibm_cases.BLOCK, stated once for all widths
    # LDS of a per-cell workgroup: slots, mask tile / node list, three doubles per node; within the 160 KB of a CU
    for W in WR.WIDTHS:
        lds = 2 * WC.TILE_CAP[W] + max(WC.TILE_CAP[W], 2 * WC.NODE_CAP[W]) + 24 * WC.NODE_CAP[W] + 104
        assert lds <= 160 * 1024
    assert [tuple(o) for o in WR.offsets(3)][:4] == [(0, 0, 0), (0, 0, 1), (0, 0, 2), (0, 1, 0)]     # ascending x, then y, then z


@pytest.mark.parametrize("W", WR.WIDTHS)
def test_caps_hold_a_red_cell_in_any_orientation(orc, W):
    """the count behind NODE_CAP3 / NODE_CAP4 and the tile caps: the RBC_FROM_SPHERE mesh (642 vertices, radius 7.82 lu) at 300
    random orientations and offsets, every second one stretched by 10 % along an axis, stays below both caps of its width (the
    comment next to the constants quotes the maxima over 2000: 2234 and 3015 nodes, boxes of 5508 and 6498)"""
    T = O.make_rbc(orc, O.make_params(orc))
    try:
        V = T.contents.arr("vertices").copy()
    finally:
        orc.orc_celltype_destroy(T)
    assert len(V) == IC.NV["rbc"]
    V -= V.mean(axis=0)
    rng = np.random.default_rng(1)
    off = WR.offsets(W)
    most, box = 0, 0
    for it in range(300):
        q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        p = (V * np.array([1.0 if it % 2 == 0 else 1.1, 1.0, 1.0])) @ q.T + rng.uniform(0, 1, 3) + 40.0
        b = WR.base(p, W)
        g = (b[:, None, :] + off[None]).reshape(-1, 3) - b.min(axis=0)
        most = max(most, len(np.unique((g[:, 0] * 64 + g[:, 1]) * 64 + g[:, 2])))
        box = max(box, int(np.prod(b.max(axis=0) + W - b.min(axis=0))))
    print("W = %d: at most %d distinct nodes (cap %d), box of %d nodes (cap %d)" % (W, most, WC.NODE_CAP[W], box, WC.TILE_CAP[W]))
    assert 0.8 * WC.NODE_CAP[W] < most <= WC.NODE_CAP[W] and box <= WC.TILE_CAP[W]


def _probe_points():
    """a fine grid over two cells, and the doubles next to every node and half-node, both signs"""
    p = list(np.linspace(-2.0, 2.0, 1601) + 7.0) + list(np.linspace(-2.0, 2.0, 1601) - 7.0)
    for s in np.arange(-9.0, 9.5, 0.5):
        if abs(s) >= 2.0:                      # the doubles next to it have |p| >= 1: every p - node is exact
            p += [s, np.nextafter(s, np.inf), np.nextafter(s, -np.inf)]
    return np.array(p)


@pytest.mark.parametrize("W", WR.WIDTHS)
def test_phi_properties(W):
    """per axis: the weights sum to 1, their first moment about the particle is 0 and their squares sum to 1/2 (three points)
    or 3/8 (four): in extended precision to its rounding, in the kernel's doubles to a few units of 2^-53"""
    p = _probe_points()
    b = WR.base(p, W)
    g = b[:, None] + np.arange(W)[None, :]
    d = p[:, None] - g                                                   # exact: |p| >= 1
    assert (R.hp(d) == R.hp(p)[:, None] - R.hp(g)).all()
    ext, ext_abs = WR.phi_hp(np.abs(R.hp(d)), d, W)
    dbl = WR.phi_double(d, W)
    one, zero = R.hp(1.0), R.hp(0.0)
    eps_hp = float(np.finfo(np.longdouble).eps) if R.HP is np.longdouble else 2.0 ** -110
    scale = R.to_double(ext_abs.sum(axis=1))
    assert (np.abs(R.to_double(ext.sum(axis=1) - one)) <= 8 * eps_hp * scale).all()
    assert (np.abs(R.to_double((ext * R.hp(d)).sum(axis=1) - zero)) <= 16 * eps_hp * scale).all()
    assert (np.abs(R.to_double((ext * ext).sum(axis=1) - R.hp(SUM_SQUARES[W]))) <= 16 * eps_hp * scale).all()
    assert (np.abs(dbl.sum(axis=1) - 1.0) <= 8 * 2.0 ** -53 * scale).all()
    assert (np.abs((dbl * d).sum(axis=1)) <= 16 * 2.0 ** -53 * scale).all()
    assert (np.abs((dbl * dbl).sum(axis=1) - SUM_SQUARES[W]) <= 16 * 2.0 ** -53 * scale).all()
    # the double the kernel forms lies within its error scale of the extended value: what phi_abs is for
    assert (np.abs(dbl - R.to_double(ext)) <= WR.PHI_ROUNDINGS * 2.0 ** -53 * R.to_double(ext_abs)).all()
    assert (R.to_double(ext) >= -1e-18).all() and (R.to_double(ext) <= 2.0 / 3.0 + 1e-15).all()


def test_branch_switches_and_floor_ties():
    up, dn = (lambda x: np.nextafter(x, np.inf)), (lambda x: np.nextafter(x, -np.inf))
    # phi3: inner branch up to and including 0.5, outer up to and including 1.5 (where it is exactly 0), nothing beyond
    f3 = lambda r: float(WR.phi_double(np.array([r]), 3)[0])
    assert f3(0.0) == 2.0 / 3.0 and f3(0.5) == (1.0 + np.sqrt(1.0 - 3.0 * 0.5 * 0.5)) / 3.0 == 0.5
    assert f3(up(0.5)) == (5.0 - 3.0 * up(0.5) - np.sqrt(-2.0 + 6.0 * up(0.5) - 3.0 * up(0.5) * up(0.5))) / 6.0
    assert f3(1.0) == 1.0 / 6.0 and f3(-1.0) == 1.0 / 6.0
    assert f3(1.5) == 0.0 and f3(-1.5) == 0.0 and f3(up(1.5)) == 0.0 and f3(2.0) == 0.0 and abs(f3(dn(1.5))) < 1e-15
    # phi4: inner up to and including 1, outer up to and including 2 (exactly 0), nothing beyond
    f4 = lambda r: float(WR.phi_double(np.array([r]), 4)[0])
    assert f4(0.0) == 0.5 and f4(1.0) == 0.25 and f4(-1.0) == 0.25
    assert f4(up(1.0)) == (5.0 - 2.0 * up(1.0) - np.sqrt(-7.0 + 12.0 * up(1.0) - 4.0 * up(1.0) * up(1.0))) / 8.0
    assert f4(2.0) == 0.0 and f4(-2.0) == 0.0 and f4(up(2.0)) == 0.0 and f4(2.5) == 0.0 and abs(f4(dn(2.0))) < 1e-15
    # nodes: c - 1 .. c + 1 with c = floor(p + 0.5): the tie 2.5 goes up, -2.5 goes up too (floor, not truncation)
    b3 = lambda x: int(WR.base(np.array([x]), 3)[0])
    assert [b3(2.5), b3(dn(2.5)), b3(up(2.5)), b3(3.0)] == [2, 1, 2, 2]
    assert [b3(-2.5), b3(dn(-2.5)), b3(up(-2.5)), b3(-3.0)] == [-3, -4, -3, -4]
    # nodes: f - 1 .. f + 2 with f = floor(p)
    b4 = lambda x: int(WR.base(np.array([x]), 4)[0])
    assert [b4(3.0), b4(dn(3.0)), b4(up(3.0)), b4(3.5)] == [2, 1, 2, 2]
    assert [b4(-3.0), b4(dn(-3.0)), b4(up(-3.0)), b4(-2.5)] == [-4, -5, -4, -4]
    # on a node the four-point stencil has a zero weight at f + 2 and admits 3 nodes per axis; on a half-node the
    # three-point stencil has a zero weight at c + 1 and admits 2
    n4, _, a4 = WR.stencil(np.array([[5.0, 6.0, 7.0]]), (16, 16, 16), (1, 1, 1), None, 4)
    assert a4.sum() == 27 and not a4[0, 3] and a4[0, 2]
    n3, _, a3 = WR.stencil(np.array([[5.5, 6.5, 7.5]]), (16, 16, 16), (1, 1, 1), None, 3)
    assert a3.sum() == 8 and not a3[0, 2] and a3[0, 1]
    # ... and the visiting order is ascending x, then y, then z: node index z + nz (y + ny x)
    n3, _, a3 = WR.stencil(np.array([[5.2, 6.2, 7.2]]), (16, 16, 16), (1, 1, 1), None, 3)
    assert a3.all() and list(n3[0, :4]) == [(4 * 16 + 5) * 16 + 6, (4 * 16 + 5) * 16 + 7, (4 * 16 + 5) * 16 + 8, (4 * 16 + 6) * 16 + 6]


def check_expectations(case):
    """every cell sits on the side of its caps that the case says, and no live particle is left without a node"""
    for c, want in case["expect"].items():
        pred = WC.predict(case, c)
        for key, val in want.items():
            if key == "tiled":
                assert WC.tiled(case, c, pred) == val, (case["name"], c, pred)
            else:
                assert pred[key] == val, (case["name"], c, key, pred)
    nodes = WC.needed(case)
    assert len(nodes) > 0
    geo = (case["dims"], case["periodic"], case["mask"])
    for t, sl in WC._by_type(case):
        W = case["kernels"][t]
        adm = (WR.stencil(case["pos"][sl], *geo, W) if W != 2 else IR.stencil(case["pos"][sl], *geo))[2]
        assert adm[case["alive"][sl]].any(axis=1).all(), case["name"]


@pytest.mark.parametrize("W,name", WC.NAMES)
def test_case_preconditions(orc, W, name):
    case = WC.build(name, W, _f_limit(orc))
    check_expectations(case)
    n = sum(IC.NV[k] for k in case["kinds"])
    assert case["pos"].shape == case["force"].shape == (n, 3) and case["alive"].shape == (n,)
    assert set(case["kernels"][k] for k in case["kinds"]) - {2} != set(), "a case without a wide kernel"
    WC.spread_ref(case, _f_limit(orc), double=True)          # asserts that two types never touch one node


def test_caps_from_both_sides(orc):
    fl = _f_limit(orc)
    pred = lambda W, name: WC.predict(WC.build(name, W, fl), 0)
    assert [pred(3, n)["vol"] for n in ("tile_19_19_19", "tile_19_19_20")] == [WC.TILE_CAP[3], WC.TILE_CAP[3] + 361]
    assert [pred(4, n)["vol"] for n in ("tile_20_20_20", "tile_20_20_21")] == [WC.TILE_CAP[4], WC.TILE_CAP[4] + 400]
    for W, names in ((3, ("tile_19_19_19", "tile_19_19_20")), (4, ("tile_20_20_20", "tile_20_20_21"))):
        for n in names:                                   # the tile alone decides: the node count is below its cap
            assert pred(W, n)["nodes"] <= WC.NODE_CAP[W] and not pred(W, n)["exceeds"]
    assert [pred(3, n)["nodes"] for n in ("nodes_2431", "nodes_2432", "nodes_2433")] == [WC.NODE_CAP[3] - 1, WC.NODE_CAP[3], WC.NODE_CAP[3] + 1]
    assert [pred(4, n)["nodes"] for n in ("nodes_3583", "nodes_3584", "nodes_3585")] == [WC.NODE_CAP[4] - 1, WC.NODE_CAP[4], WC.NODE_CAP[4] + 1]
    for W, names in ((3, ("nodes_2431", "nodes_2432", "nodes_2433")), (4, ("nodes_3583", "nodes_3584", "nodes_3585"))):
        for n in names:                                   # the node count alone decides: the box is below the tile cap
            assert pred(W, n)["vol"] <= WC.TILE_CAP[W]


def node_velocities(case, f, F, extra_kernels=()):
    """(u, u_abs) on every node that the case's kernels, or any of extra_kernels, read"""
    need = [WC.needed(case)] + [WC.needed(case, k) for k in extra_kernels]
    return _node_velocity(case, f, F, np.unique(np.concatenate(need)))


def wrong_kernels(case):
    return {t: WC.other_width(w) for t, w in case["kernels"].items()}


def _excess(*args):
    """observables_ref.excess where a miss may be too large for a double (a bound at rounding level of a weight near zero)"""
    with np.errstate(over="ignore", invalid="ignore"):
        return R.excess(*args)


def mutation_excess(case, f_limit, F, v, u, ua):
    """how far the values F (node forces) and v (particle velocities) miss the restatements that must not pass -- the other
    width, and the controls the case names -- in units of the bound of the right one -> {control: (spread, interpolate)}"""
    right = WC.spread_ref(case, f_limit)
    right_v = WC.interpolate_ref(case, u, ua)
    alive = case["alive"]
    out = {}
    ws = WC.spread_ref(case, f_limit, kernels=wrong_kernels(case))
    wv = WC.interpolate_ref(case, u, ua, kernels=wrong_kernels(case))
    own = right["touched"]                    # on the nodes of the right width alone, with its bound: nothing to do with the nodes only the wrong one reaches
    out["other_width"] = (_excess(F[own], ws["F"][own], right["F_abs"][own], K),
                          _excess(v[alive], wv["v"][alive], right_v["v_abs"][alive], K))
    for wrong in case["controls"]:
        ws = WC.spread_ref(case, f_limit, wrong=wrong)
        both = right["touched"] | ws["touched"]
        es = _excess(F[both], ws["F"][both], np.maximum(right["F_abs"], 1e-300)[both], K)
        if wrong == "no_cap":
            out[wrong] = (es, None)
            continue
        wv = WC.interpolate_ref(case, u, ua, wrong=wrong)
        written = alive if wrong != "dead_take_part" else np.ones(len(alive), bool)
        scale = np.where(alive[:, None], right_v["v_abs"], np.abs(wv["v"]))       # a removed particle has no right value
        ev = _excess(np.where(np.isnan(v), 1e30, v)[written], wv["v"][written], scale[written], K)
        out[wrong] = (es, ev)
    return out


@pytest.mark.parametrize("W,name", WC.NAMES)
def test_mutation_controls_vs_right_restatement(orc, W, name):
    """the right restatement (standing in for a right kernel) misses the other width, and each wrong restatement the case
    names, by at least FAIL_BY bounds"""
    fl = _f_limit(orc)
    case = WC.build(name, W, fl)
    F = WC.spread_ref(case, fl)["F"]
    u = 0.01 * np.random.default_rng(5).standard_normal(F.shape)       # any node velocities will do here
    ua = np.abs(u)
    v = WC.interpolate_ref(case, u, ua)["v"]
    v[~case["alive"]] = np.nan
    for wrong, (es, ev) in mutation_excess(case, fl, F, v, u, ua).items():
        assert es > FAIL_BY and (ev is None or ev > FAIL_BY), (name, W, wrong, es, ev)


def test_rounding_figure_behind_k(orc):
    """the largest |double - extended| / (2^-53 * abs) of the plain double restatement, summed in storage order and the other
    way round, over every case of both widths.  It is 3.63 (mixed_rbc4_plt2); that does not exceed 4, so K is the project's 16."""
    fl = _f_limit(orc)
    worst, where = 0.0, None
    for W, name in WC.NAMES:
        case = WC.build(name, W, fl)
        ref = WC.spread_ref(case, fl)
        f = _random_state(case)
        u, ua = node_velocities(case, f, ref["F"] + np.array(case["body"])[None, :])
        rv = WC.interpolate_ref(case, u, ua)
        alive = case["alive"]
        for rev in (False, True):
            d = WC.spread_ref(case, fl, double=True, reverse=rev)
            dv = WC.interpolate_ref(case, u, ua, double=True, reverse=rev)
            for e in (R.excess(d["F"], ref["F"], ref["F_abs"], 1.0), R.excess(d["force"], ref["force"], ref["force_abs"], 1.0),
                      R.excess(dv[alive], rv["v"][alive], rv["v_abs"][alive], 1.0)):
                if e > worst:
                    worst, where = e, (W, name)
    print("largest |double - extended| / (2^-53 abs) over %d cases, two orders: %.3f at %s" % (len(WC.NAMES), worst, where))
    assert worst <= 4.0 and K == 16.0


def test_facade_driver_with_both_kernel_names_compiles(tmp_path):
    from tests.test_plugin_surface import INC
    from hemocell_amd import capi
    libdir = os.path.dirname(capi.LIB_PATH)
    exe = os.path.join(str(tmp_path), "ibm_kernel_driver")
    r = subprocess.run(["g++", "-std=c++14", "-O1", "-Wall", "-Wno-deprecated-declarations", "-DHEMOCELL_COMPAT_MAIN"] + INC +
                       [os.path.join(ROOT, "tests", "plugin", "ibm_kernel_driver.cpp"), "-o", exe, "-L" + libdir, "-lhemocell_amd", "-Wl,-rpath," + libdir],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
