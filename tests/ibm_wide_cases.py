"""Crafted geometries for the three- and four-point IBM kernels (tests/test_ibm_wide_cpu.py, tests/test_gpu_ibm_wide.py).

build(name, W, f_limit) returns a case in the format of tests/ibm_cases.py with one more key, kernels {type name: 2, 3 or 4}.
Cases that do not depend on the caps are those of ibm_cases, taken by import with every type on W (REUSED); the cases around
the caps of hemocell_amd/csrc/ibm_common.h (TILE_CAP3/4, NODE_CAP3/4; tests/test_ibm_wide_cpu.py checks the copies below) and
the container with types on different kernels are made here.  expect {cell: {'tiled': bool, 'vol': ..., 'nodes': ...}} is what
ibm_wide_ref.predict must say of the cell.

spread_ref / interpolate_ref / needed: the restatement of a whole case, type by type with the kernel of each (ibm_ref for a
type on two points).  The cells of a mixed case touch disjoint nodes, so a node's force has one type's terms.
"""
import zlib

import numpy as np

from tests import ibm_cases as IC
from tests import ibm_ref as IR
from tests import ibm_wide_ref as WR

TILE_CAP = {2: IC.TILE_CAP, 3: 19 ** 3, 4: 20 ** 3}
NODE_CAP = {2: IC.NODE_CAP, 3: 2432, 4: 3584}
WBOX = dict(dims=(40, 40, 40), periodic=(1, 1, 1))
REUSED = ("seam_x", "seam_y", "seam_z", "seam_xyz", "faces_open", "walls_7_and_1_of_8", "pipe_wall_hug", "exact_positions",
          "dead_vertices", "force_cap")


def other_width(w):
    """the wrong width of the mutation control"""
    return {2: 3, 3: 4, 4: 3}[w]


def _wfill(rng, lows, nv, W):
    """nv vertices; the stencil of vertex i starts at node lows[i % len] and all its W^3 weights are non-zero"""
    assert len(lows) <= nv, "every stencil needs a vertex"
    b = np.asarray(lows, dtype=np.float64)[np.arange(nv) % len(lows)]
    return b + 1.0 + (rng.uniform(-0.3, 0.3, size=(nv, 3)) if W == 3 else rng.uniform(0.2, 0.8, size=(nv, 3)))


def _wbox_lows(rng, o, e, W, m):
    """distinct lowest nodes whose stencils span exactly the box of origin o and extents e: its 8 corners and up to m inside"""
    o, e = np.array(o), np.array(e)
    corners = np.array([o + (e - W) * np.array(c) for c in np.ndindex(2, 2, 2)])
    inner = o + rng.integers(0, e - W + 1, size=(m, 3))
    return np.unique(np.vstack([corners, inner]), axis=0)


def _tile(name, W, e, kind, tiled, m):
    def b(rng, fl):
        o = (-30, -29, -28)      # negative coordinates: the box wraps to (10, 11, 12) without crossing a face
        p = _wfill(rng, _wbox_lows(rng, o, e, W, m), IC.NV[kind], W)
        return IC._case(name, fl, WBOX, [(kind, p)], expect={0: dict(e=e, vol=int(np.prod(e)), tiled=tiled, wraps=(False, False, False))})
    return b


def _nodes(name, W, blocks, masked, nodes, tiled):
    """`blocks` disjoint W^3 stencils, the first `masked` nodes of the last one turned into wall"""
    def b(rng, fl):
        o = np.array((2, 3, 5))
        side = 6 if W == 3 else 5                                      # 18 and 20 nodes along an axis: inside the tile cap
        grid = np.array([(i, j, k) for k in range(side) for j in range(side) for i in range(side)])[:blocks]
        lows = o + W * grid
        mask = np.zeros(WBOX["dims"], np.uint8)
        for d in WR.offsets(W)[:masked]:
            mask[tuple(lows[-1] + d)] = 1
        p = _wfill(rng, lows, IC.NV["rbc"], W)
        return IC._case(name, fl, WBOX, [("rbc", p)], mask=mask if masked else None, seat=(30.0, 30.0, 30.0),
                        expect={0: dict(nodes=nodes, tiled=tiled)})
    return b


def _mixed(name, k_rbc, k_plt):
    """one RBC and two PLT, far enough apart that no node is touched by two types; forces above the limit in both types"""
    def b(rng, fl):
        cells = [IC._cell(rng, "rbc", (3, 3, 4), (6, 6, 6), 30), IC._cell(rng, "plt", (14, 4, 11), (5, 5, 5), 20),
                 IC._cell(rng, "plt", (15, 10, 2), (4, 4, 5), 20)]
        n = IC.NV["rbc"] + 2 * IC.NV["plt"]
        f = IC._forces(rng, n, fl)
        for i, s in ((0, 1.5), (256, 1e3), (641, 2.0), (642, 3.0), (n - 1, 1.0 + 1e-9)):
            f[i] *= s * fl / np.sqrt((f[i] * f[i]).sum())
        c = IC._case(name, fl, IC.SEAM, cells, force=f, expect={0: dict(tiled=True), 1: dict(tiled=True), 2: dict(tiled=True)})
        c["kernels"] = dict(rbc=k_rbc, plt=k_plt, big=2)
        return c
    return b


def _builders(W):
    cap, t = NODE_CAP[W], W ** 3
    if W == 3:
        out = {
            "tile_19_19_19": _tile("tile_19_19_19", 3, (19, 19, 19), "rbc", True, 60),
            "tile_19_19_20": _tile("tile_19_19_20", 3, (19, 19, 20), "rbc", False, 60),
            "nodes_2431": _nodes("nodes_2431", 3, 91, 26, cap - 1, True),
            "nodes_2432": _nodes("nodes_2432", 3, 91, 25, cap, True),
            "nodes_2433": _nodes("nodes_2433", 3, 91, 24, cap + 1, False),
            "mixed_rbc3_plt4": _mixed("mixed_rbc3_plt4", 3, 4),
            "mixed_rbc2_plt3": _mixed("mixed_rbc2_plt3", 2, 3),
        }
    else:
        out = {
            "tile_20_20_20": _tile("tile_20_20_20", 4, (20, 20, 20), "rbc", True, 40),
            "tile_20_20_21": _tile("tile_20_20_21", 4, (20, 20, 21), "plt", False, 40),
            "nodes_3583": _nodes("nodes_3583", 4, 56, 1, cap - 1, True),
            "nodes_3584": _nodes("nodes_3584", 4, 56, 0, cap, True),
            "nodes_3585": _nodes("nodes_3585", 4, 57, t - 1, cap + 1, False),
            "mixed_rbc4_plt3": _mixed("mixed_rbc4_plt3", 4, 3),
            "mixed_rbc4_plt2": _mixed("mixed_rbc4_plt2", 4, 2),
        }
    return out


BUILDERS = {W: _builders(W) for W in WR.WIDTHS}
NAMES = [(W, n) for W in WR.WIDTHS for n in list(BUILDERS[W]) + list(REUSED)]
_cache = {}


def build(name, W, f_limit):
    key = (name, W, float(f_limit))
    if key not in _cache:
        if name in REUSED:
            c = dict(IC.build(name, f_limit))
            c["kernels"] = {t: W for t in IC.TYPES}
            c["expect"] = {i: dict(tiled=True) for i in range(len(c["kinds"]))}     # none of them is near a cap of the wide kernels
            c["controls"] = tuple(w for w in c["controls"] if w in ("no_renormalise", "admit_walls", "dead_take_part", "no_cap"))
        else:
            c = BUILDERS[W][name](np.random.default_rng(zlib.crc32(("%s/%d" % (name, W)).encode())), float(f_limit))
            c.setdefault("kernels", {t: W for t in IC.TYPES})
            c["controls"] = ()
        _cache[key] = c
    return _cache[key]


def tiled(case, c, pred):
    """does cell c take the LDS tile of its kernel (pred: ibm_wide_ref.predict of the cell)"""
    kind = case["kinds"][c]
    W = case["kernels"][kind]
    return bool(pred["vol"] <= TILE_CAP[W] and not pred["exceeds"] and pred["nodes"] <= NODE_CAP[W] and IC.NV[kind] <= IC.NVPT * IC.BLOCK[kind])


# ----------------------------------------------------------------------------------------------------------------------
def _by_type(case, kernels=None):
    """[(type name, slice of the vertices of the type)] in storage order; with kernels, types that follow each other on one
    kernel form one entry (their terms at a shared node are then summed before anything is rounded)"""
    out, o = [], 0
    for t in IC.TYPES:
        n = case["counts"][t] * IC.NV[t]
        if n:
            if kernels is not None and out and kernels[out[-1][0]] == kernels[t]:
                out[-1] = (out[-1][0], slice(out[-1][1].start, o + n))
            else:
                out.append((t, slice(o, o + n)))
        o += n
    return out


def _kernels(case, kernels):
    return case["kernels"] if kernels is None else kernels


def spread_ref(case, f_limit, kernels=None, wrong=None, double=False, reverse=False):
    """the whole case -> dict(F, F_abs, touched, force, force_abs) (double: dict(F, force) of the plain double restatement)"""
    geo = (case["dims"], case["periodic"], case["mask"])
    N = int(np.prod(case["dims"]))
    out = dict(F=np.zeros((N, 3)), F_abs=np.zeros((N, 3)), touched=np.zeros(N, bool), force=np.zeros_like(case["pos"]), force_abs=np.zeros_like(case["pos"]))
    for t, sl in _by_type(case, _kernels(case, kernels)):
        W = _kernels(case, kernels)[t]
        args = (case["pos"][sl], case["force"][sl], None, case["alive"][sl]) + geo
        if double:
            r = IR.spread_double(*args, f_limit=f_limit, reverse=reverse) if W == 2 else WR.spread_double(*args, W, f_limit=f_limit, reverse=reverse)
            assert not (out["touched"] & (r["F"] != 0).any(axis=1)).any(), "two types touch one node"
            out["touched"] |= (r["F"] != 0).any(axis=1)
            out["F"] += r["F"]; out["force"][sl] = r["force"]
            continue
        r = IR.spread(*args, f_limit=f_limit, wrong=wrong) if W == 2 else WR.spread(*args, W, f_limit=f_limit, wrong=wrong)
        assert not (out["touched"] & r["touched"]).any(), "two types touch one node"
        out["F"] += r["F"]; out["F_abs"] += r["F_abs"]; out["touched"] |= r["touched"]
        out["force"][sl], out["force_abs"][sl] = r["force"], r["force_abs"]
    return out


def needed(case, kernels=None):
    geo = (case["dims"], case["periodic"], case["mask"])
    parts = []
    for t, sl in _by_type(case, _kernels(case, kernels)):
        W = _kernels(case, kernels)[t]
        parts.append(IR.needed_nodes(case["pos"][sl], case["alive"][sl], *geo) if W == 2 else WR.needed_nodes(case["pos"][sl], case["alive"][sl], *geo, W))
    return np.unique(np.concatenate(parts))


def interpolate_ref(case, u, ua, kernels=None, wrong=None, double=False, reverse=False):
    """-> dict(v, v_abs) (double: v of the plain double restatement)"""
    geo = (case["dims"], case["periodic"], case["mask"])
    v, va = np.zeros_like(case["pos"]), np.zeros_like(case["pos"])
    for t, sl in _by_type(case, _kernels(case, kernels)):
        W = _kernels(case, kernels)[t]
        p, al = case["pos"][sl], case["alive"][sl]
        if double:
            v[sl] = IR.interpolate_double(p, al, u, *geo, reverse=reverse) if W == 2 else WR.interpolate_double(p, al, u, *geo, W, reverse=reverse)
            continue
        r = IR.interpolate(p, al, u, *geo, u_abs=ua, wrong=wrong) if W == 2 else WR.interpolate(p, al, u, *geo, W, u_abs=ua, wrong=wrong)
        v[sl], va[sl] = r["v"], r["v_abs"]
    return v if double else dict(v=v, v_abs=va)


def predict(case, c):
    sl = IC.cell_slices(case)[c]
    W = case["kernels"][case["kinds"][c]]
    geo = (case["dims"], case["periodic"], case["mask"])
    if W == 2:
        return IR.predict(case["pos"][sl], case["alive"][sl], *geo, pad_x=IC.HALO)
    return WR.predict(case["pos"][sl], case["alive"][sl], *geo, W)
