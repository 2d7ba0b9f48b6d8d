"""Cell packing without a GPU: the restatement (tests/packing_ref.py) against the reference's own pair numbers
(tests/golden/packing_pairs.json, recorded from tools/packCells), packing_plan against what the reference printed, the
.pos output, the Euler angles and the restatement's invariants on the smallest shape."""
import json
import os

import numpy as np
import pytest

import packing_ref as R
from hemocell_amd import packing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "packing_pairs.json")
SCALE = 1.2 / 8.4
SIZES = np.array([[8.4, 4.4, 8.4], [2.4, 1.05, 2.4]]) * SCALE


@pytest.fixture(scope="module")
def pairs():
    return json.load(open(FIXTURE))["pairs"]


def test_fixture_covers_the_cases(pairs):
    assert 150 <= len(pairs) <= 200
    tags = [p["tag"] for p in pairs]
    for combo in ("RBC-RBC", "RBC-PLT", "PLT-RBC", "PLT-PLT", "WBC-RBC", "RBC-WBC", "TINY-RBC"):
        for orient in ("identity", "random"):
            for kind in ("deep", "near_in", "near_out", "far"):
                assert any(t == "%s/%s/%s" % (combo, orient, kind) for t in tags), (combo, orient, kind)
    assert {p["rotate"] for p in pairs} == {0, 1}
    near = [p["f_AB"] for p in pairs if "near" in p["tag"]]
    assert all(abs(f - 1) < 1e-3 for f in near) and min(near) < 1 < max(near)


def test_restatement_equals_reference_bit_for_bit(pairs):
    """same IEEE operations in the same order on a build without FMA: every recorded number is reproduced exactly"""
    kinds = set()
    for p in pairs:
        D2 = p["Douter"] * p["Douter"]
        o = R.pair(p["sizeA"], p["qA"], p["sizeB"], p["qB"], p["rij"], D2, p["rotate"])
        assert o["capped"] == 0 and o["evals"] < 128, p["tag"]
        assert o["kind"] in (1, 2), p["tag"]
        kinds.add(o["kind"])
        assert o["lambda"] == p["lambda"], p["tag"]
        assert o["fscl"] / D2 == p["f_AB"], p["tag"]
        assert (o["fscl"] if o["kind"] == 2 else D2) == p["Dinner2"], p["tag"]   # the minimum runs over overlapping pairs only
        for k in ("n", "fA", "tA", "fB", "tB"):
            assert np.array_equal(o[k], np.array(p[k])), (p["tag"], k)
        assert np.array_equal(o["fA"], -o["fB"])
        if not p["rotate"] or o["kind"] == 1:
            assert not o["tA"].any() and not o["tB"].any()
    assert kinds == {1, 2}


def test_anchor_record(pairs):
    a = pairs[0]
    assert a["tag"] == "anchor" and a["Douter"] == 1.05
    assert a["sizeA"] == [1.2, 4.4 * 1.2 / 8.4, 1.2] and a["qA"] == [0.9, 0.1, -0.3, 0.2]
    assert a["sizeB"] == [2.4 * 1.2 / 8.4, 1.05 * 1.2 / 8.4, 2.4 * 1.2 / 8.4] and a["qB"] == [0.5, -0.4, 0.2, 0.6]
    assert a["rij"] == [0.45, 0.2, -0.3]
    o = R.pair(a["sizeA"], a["qA"], a["sizeB"], a["qB"], a["rij"], 1.05 * 1.05, 1)
    assert o["lambda"] == 0.83620154980623351
    assert o["fscl"] / (1.05 * 1.05) == 0.58158853031933755
    assert o["fscl"] == 0.64120135467706962
    assert list(o["fA"]) == [-0.36644797187836176, -0.11109570053400646, 0.16864693056627403]


def test_tiny_sphere_takes_the_degenerate_branch(pairs):
    """A = a sphere of scaled size 0.1, B = an RBC: det(A_AB) ~ 1e-6, so ellipsoid.h:358-363 builds the polynomials"""
    tiny = [p for p in pairs if p["tag"].startswith("TINY-RBC")]
    assert len(tiny) >= 10
    for p in tiny:
        rb = np.array(p["sizeB"])
        assert 0.1 ** 6 / np.prod(rb) ** 2 < 1e-5   # det(A_AB) = det(XA_m1) det(XB_12)^2, whatever the orientations


@pytest.mark.parametrize("size, kw, counts, grid, fraction", [
    (24, dict(hematocrit=0.30), (43, 3), (4, 4, 4), 0.506331),
    (18, dict(hematocrit=0.30), None, (3, 3, 3), 0.502267),
    (12, dict(cells=[("RBC", 4), ("PLT", 2)]), (4, 2), (2, 2, 2), 0.379958),
    (24, dict(hematocrit=0.40), None, None, 0.671188),
    (60, dict(hematocrit=0.42), None, (9, 9, 9), 0.704621),
    (100, dict(hematocrit=0.40), (4124, 289), None, None),
])
def test_packing_plan_matches_the_reference(size, kw, counts, grid, fraction):
    p = packing.packing_plan((size,) * 3, **kw)
    assert p.names == ["RBC", "PLT"]
    if counts is not None:
        assert tuple(p.counts) == counts
    if grid is not None:
        assert p.grid == grid
    if fraction is not None:
        assert abs(p.nominal_fraction - fraction) <= 5e-7   # the last digit the reference printed
    assert (p.warning is not None) == (p.nominal_fraction > 0.7)
    assert p.scale == (1. / 8.4) * 1.2
    assert np.allclose(p.box_um, np.array(p.grid) / p.scale, rtol=1e-15)


def test_packing_plan_details():
    p = packing.packing_plan((24, 24, 24), hematocrit=0.30)
    assert p.box_um[0] == pytest.approx(28.0, abs=1e-12) and p.size_um == (24.0, 24.0, 24.0)   # 4 cells: larger than requested
    assert packing.packing_plan((60, 60, 60), hematocrit=0.42).warning
    # the first of the most numerous types sets the scale; a custom type carries its own sizes
    q = packing.packing_plan((30, 30, 30), cells=[("WBC", 1), ("PLT", 50), ("blob", 50, (3.0, 2.0, 1.0))])
    assert q.scale == (1. / 2.4) * 1.2 and q.names == ["WBC", "PLT", "blob"] and q.count("blob") == 50
    assert np.array_equal(q.sizes_um[2], [3.0, 2.0, 1.0])
    assert packing.packing_plan((24, 24, 24), hematocrit=0.3, scale=0.25).grid == (6, 6, 6)
    # hematocrit adds RBC and PLT after the named types; a ratio that rounds to no platelet adds none
    r = packing.packing_plan((24, 24, 24), hematocrit=0.3, cells=[("WBC", 1)])
    assert r.names == ["WBC", "RBC", "PLT"] and r.counts == [1, 43, 3]
    assert packing.packing_plan((24, 24, 24), hematocrit=0.3, plt_ratio=0.01).names == ["RBC"]
    for name, dims in (("RBC", (8.4, 4.4, 8.4)), ("PLT", (2.4, 1.05, 2.4)), ("WBC", (8.4, 8.4, 8.4)), ("vRBC", (3.5, 6.0, 11.0)),
                       ("RBC_m", (5.8, 3.4, 5.8)), ("PLT_m", (1.84, 1.05, 1.84)), ("PLT_mko", (1.71, 1.71, 1.71))):
        assert packing.CELL_SIZES_UM[name] == dims


def test_packing_plan_refusals():
    with pytest.raises(ValueError, match="mutually exclusive"):
        packing.packing_plan((24, 24, 24), hematocrit=0.3, cells=[("RBC", 5)])
    with pytest.raises(ValueError, match="mutually exclusive"):
        packing.packing_plan((24, 24, 24), hematocrit=0.3, cells=[("WBC", 1), ("PLT", 5)])
    with pytest.raises(ValueError, match="at least a cell type or the hematocrit"):
        packing.packing_plan((24, 24, 24))
    with pytest.raises(ValueError):
        packing.packing_plan((24, 24, 24), cells=[("nameless", 3)])
    with pytest.raises(ValueError):
        packing.packing_plan((24, 0, 24), hematocrit=0.3)
    with pytest.raises(ValueError):
        packing.packing_plan((24, 24, 24), cells=[("RBC", 0)])   # nothing to pack


def test_command_line_refuses_like_the_reference(capsys):
    assert packing._main(["24", "24", "24", "--hematocrit", "0.3", "--rbc", "4"]) == 1
    assert "mutually exclusive" in capsys.readouterr().err
    assert packing._main(["24", "24"]) == 1
    assert packing._main(["--help"]) == 1
    err = capsys.readouterr().err
    assert err.startswith("USAGE:") and "--noRotate" in err and "--seed" in err


def _rot(a, b, c):
    """Rz(c) Ry(b) Rx(a): what a .pos reader builds from the angles of a line (radians)"""
    ca, sa, cb, sb, cc, sc = np.cos(a), np.sin(a), np.cos(b), np.sin(b), np.cos(c), np.sin(c)
    Rx = np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]])
    Ry = np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]])
    Rz = np.array([[cc, -sc, 0], [sc, cc, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def test_euler_angles_invert_the_reader():
    """the ellipsoid's matrix is Q^T diag Q, so countQ() maps world to body; the reader's body-to-world rotation built from the
    written angles must be its transpose"""
    rng = np.random.default_rng(5)
    q = rng.normal(size=(200, 4))
    q /= np.linalg.norm(q, axis=1)[:, None]
    q[0] = (1, 0, 0, 0)
    ang = np.radians(packing.euler_angles_deg(q))
    Q = packing.quaternion_matrix(q)
    assert np.array_equal(packing.euler_angles_deg(q[0]), [0, 0, 0])
    for k in range(len(q)):
        assert np.abs(Q[k] @ Q[k].T - np.eye(3)).max() < 1e-12
        assert np.abs(_rot(*ang[k]) - Q[k].T).max() < 1e-12


def test_write_pos_round_trip(tmp_path):
    plan = packing.packing_plan((12, 12, 12), cells=[("RBC", 4), ("PLT", 2)])
    rng = np.random.default_rng(2)
    pos = rng.random((6, 3)) * plan.box_um
    q = rng.normal(size=(6, 4))
    q /= np.linalg.norm(q, axis=1)[:, None]
    status = np.array([17, 1, 0.98, 0.98, 0.37, 0.37, 0.0, 1e-6, 3, 0, 19, 0], dtype=np.float64)
    res = packing.PackResult(plan, pos, q, status, seed=2)
    assert res.steps == 17 and res.finished and res.inner_diameter == res.outer_diameter == 0.98 and res.density == 0.37
    assert res.box_um == plan.box_um
    paths = res.write_pos(str(tmp_path / "out"))
    assert [os.path.basename(p) for p in paths] == ["RBC.pos", "PLT.pos"]
    lines = open(paths[0]).read().splitlines()
    assert lines[0] == "4" and len(lines) == 5 and all(len(l.split()) == 6 for l in lines[1:])
    at = 0
    for path, name, n in zip(paths, plan.names, plan.counts):
        c, a = packing.read_pos(path)
        assert c.shape == a.shape == (n, 3)
        assert np.abs(c - pos[at:at + n]).max() < 1e-8 and np.array_equal(res.positions[name], pos[at:at + n])
        assert np.abs(a - packing.euler_angles_deg(q[at:at + n])).max() < 1e-7
        at += n


@pytest.mark.parametrize("rotate", [True, False])
def test_restatement_invariants_on_the_smallest_shape(rotate):
    """12^3 um, 4 RBC + 2 PLT on a 2^3 grid: forces are sums of bitwise opposite pair terms, and the finished state has no
    overlapping pair by brute force over all pairs"""
    grid, counts = (2, 2, 2), (4, 2)
    plan = packing.packing_plan((12, 12, 12), cells=[("RBC", 4), ("PLT", 2)])
    assert plan.grid == grid and np.array_equal(plan.sizes_scaled, SIZES)
    pos0 = R.initial_positions(grid, 6, 1)
    S = R.Packing(grid, SIZES, counts, pos0, None, plan.nominal_fraction, rotate)
    st = S.status()
    assert st["steps"] == 0 and st["pairs"] == 15 and st["Dinner"] <= st["Douter"]
    # the forces of the first state from the pair function alone, added in ascending partner index
    pos, quat, f, t = S.state()
    spec = [0, 0, 0, 0, 1, 1]
    want = np.zeros((6, 3))
    box = np.array(grid, dtype=np.float64)
    for A in range(6):
        for B in range(A):
            r = pos[B] - pos[A]
            r = np.where(r < -box / 2, r + box, np.where(r > box / 2, r - box, r))
            o = R.pair(SIZES[spec[A]], quat[A], SIZES[spec[B]], quat[B], r, st["Douter"] * st["Douter"], rotate)
            assert np.array_equal(o["fA"], -o["fB"])   # bitwise opposite
            want[A] += o["fA"]; want[B] += o["fB"]
    assert np.array_equal(f, want) and f.any()
    assert np.abs(f.sum(axis=0)).max() < 1e-14
    assert t.any() == bool(rotate)
    st = S.run(1000)
    assert st["finished"] == 1 and st["error"] == 0 and 0 < st["steps"] < 200 and st["maxeval"] < 128
    assert st["Force_step"] == 0.0 and st["Dinner"] == st["Douter"]
    pos, quat, f, t = S.state()
    assert not f.any() and not t.any()
    best, overlapping, skipped = R.min_contact(grid, SIZES, counts, pos, quat, st["Douter"])
    assert overlapping == 0 and skipped == 0 and best >= 1.0
    assert (pos >= 0).all() and (pos <= box).all()
    assert np.abs(np.linalg.norm(quat, axis=1) - 1).max() < 1e-10
    assert np.array_equal(quat[:, 0] == 1.0, np.ones(6, bool)) == (not rotate)   # rotation off: identity throughout


def test_to_the_end_shape_finishes_well_inside_the_cap():
    """24^3 um at 0.40 (57 RBC + 4 PLT), the shape tests/test_gpu_packing.py runs to the end under max_iter = 1000: the
    restatement ends seed 1 in 152 iterations (the bound below is half the cap, not that count, which the last bit of the
    host's pow() could move)"""
    plan = packing.packing_plan((24, 24, 24), hematocrit=0.40)
    assert plan.counts == [57, 4] and plan.grid == (4, 4, 4)
    S = R.Packing(plan.grid, plan.sizes_scaled, plan.counts, R.initial_positions(plan.grid, 61, 1), None, plan.nominal_fraction, True)
    st = S.run(1000)
    print("24^3 at 0.40, seed 1: finished after %d iterations" % st["steps"])
    assert st["finished"] == 1 and st["steps"] <= 500 and st["error"] == 0


# ------------------------------------------------------------------------------------------------------------------------------
# The conditions the starts of tests/packing_cases.py rest on (tests/test_gpu_packing_shapes.py runs them on the device)
import functools
import hashlib

import packing_cases as PC


@functools.lru_cache(maxsize=None)
def _walk(name, rotate, marks=(0, 1, 5, 20)):
    """the restatement on a case: [(status, state)] after each of marks iterations"""
    c = PC.build(name)
    S = R.Packing(c.grid, c.sizes_scaled, c.counts, c.pos, c.quat, c.nominal_fraction, rotate)
    out, done = [], 0
    for upto in marks:
        st = S.run(upto - done)
        done = upto
        out.append((st, S.state()))
    return c, out


def _inside(case, pos):
    return (pos >= 0).all() and (pos <= np.array(case.grid, dtype=np.float64)).all()


@pytest.mark.parametrize("rotate", [True, False])
@pytest.mark.parametrize("name", PC.UNEVEN)
def test_uneven_cases_reach_what_they_claim(name, rotate):
    """grids with three different axes, a sphere, given orientations, N past a wave and past a block: the path of every species
    from the rule itself, the pair counts of the restatement against an independent count in numpy (packing_cases.partner_matrix),
    nothing outside the box, no error, and root searches far below the 128 the device tests allow (33 at the most here)"""
    c, walk = _walk(name, rotate)
    n, all_pairs = c.n, c.n * (c.n - 1) // 2
    assert n == {"uneven288": 288, "uneven134": 134, "uneven70": 70}[name] and n > 64 and n % 64
    assert len(set(c.grid)) == 3 and np.abs(np.linalg.norm(c.quat, axis=1) - 1).max() < 1e-15
    st0 = walk[0][0]
    assert st0["Douter"] == PC.first_diameter(c)
    for st, state in walk:
        mode = PC.modes(c, st["Douter"])
        assert mode == PC.UNEVEN_MODES[name]
        assert st["pairs"] == PC.partner_matrix(c, state[0], st["Douter"]).sum()
        if "part" in mode:
            assert 0 < st["pairs"] < all_pairs
        else:
            assert st["pairs"] == all_pairs
        assert _inside(c, state[0]) and st["error"] == 0 and st["maxeval"] <= 40
        assert not st["finished"]
    assert [st["steps"] for st, _ in walk] == [0, 1, 5, 20]
    counts = PC.partner_counts(c, c.pos, st0["Douter"])
    if name == "uneven288":
        assert n > 256 and -(-n // 64) == 5
        assert st0["pairs"] == 6369 and counts.max() == 72 and PC.list_capacity(c) == 274 < n - 1
    elif name == "uneven134":
        assert st0["pairs"] == 7597 and PC.list_capacity(c) == n - 1   # the seed-5 start; it walks through 7614 a few steps on
    else:
        assert counts.min() == n - 1 and PC.list_capacity(c) == n - 1
    # the sphere: no torque of its own and an orientation that stays; the RBCs have both
    state = walk[-1][1]
    assert not state[3][c.rows("WBC")].any() and np.array_equal(state[1][c.rows("WBC")], c.quat[c.rows("WBC")])
    assert state[2][c.rows("WBC")].any()
    assert state[3][c.rows("RBC")].any() == bool(rotate)
    assert np.array_equal(state[1], c.quat) == (not rotate)


@pytest.mark.parametrize("rotate", [True, False])
def test_uneven288_finishes_well_inside_the_cap(rotate):
    """the (5, 6, 8) start of seed 5 runs to the end under a cap of 1000 on the device: the restatement ends it after 94
    iterations with rotation and 312 without (the bound is half the cap, not those counts)"""
    c = PC.build("uneven288")
    S = R.Packing(c.grid, c.sizes_scaled, c.counts, c.pos, c.quat, c.nominal_fraction, rotate)
    st = S.run(1000)
    print("(5, 6, 8) with 288 particles, seed 5, rotate %d: finished after %d iterations" % (rotate, st["steps"]))
    assert st["finished"] == 1 and st["steps"] <= 500 and st["error"] == 0 and st["maxeval"] < 128
    assert _inside(c, S.state()[0])


@pytest.mark.parametrize("rotate", [True, False])
def test_cluster_start_needs_longer_lists(rotate):
    """200 particles inside a cube of edge 0.9 on 8^3: both species are on the cell list, yet every particle is every other's
    partner (199 each, 19900 pairs) while hc_packing_create starts with lists of 161.  The first step then scatters them
    (Force_step about 61) and the lists shrink to about 40; nothing leaves the box in 20 iterations."""
    c, walk = _walk("cluster", rotate)
    st0, state0 = walk[0]
    assert PC.modes(c, st0["Douter"]) == ["part", "part"]
    assert PC.list_capacity(c) == 161
    counts = PC.partner_counts(c, c.pos, st0["Douter"])
    assert counts.min() == counts.max() == 199 > 161 and st0["pairs"] == 19900
    assert PC.grown_capacity(c, 199) == 199
    for st, state in walk:
        assert _inside(c, state[0]) and st["error"] == 0 and not st["finished"]
        assert st["pairs"] == PC.partner_matrix(c, state[0], st["Douter"]).sum()
    assert 50 < walk[1][0]["Force_step"] < 70
    assert PC.partner_counts(c, walk[1][1][0], walk[1][0]["Douter"]).max() < 50
    assert walk[-1][0]["steps"] == 20 and walk[-1][0]["maxeval"] == (19 if rotate else 18)


@pytest.mark.parametrize("rotate", [True, False])
def test_faces_start(rotate):
    """deviation 8: a particle exactly on an upper face has no cell.  Particle 0 is the lowest index, so it is never an A; as B
    it is in nobody's range, and it neither feels a force nor moves.  Particle 1, at the origin, does."""
    c, walk = _walk("faces", rotate)
    assert walk[0][0]["pairs"] == 828 and PC.partner_counts(c, c.pos, walk[0][0]["Douter"])[0] == 0
    box = np.array(c.grid, dtype=np.float64)
    for st, state in walk:
        assert st["error"] == 0 and st["maxeval"] <= 19 and _inside(c, state[0]) and not st["finished"]
        assert not state[2][0].any() and not state[3][0].any() and np.array_equal(state[0][0], c.pos[0])
        assert st["pairs"] == PC.partner_matrix(c, state[0], st["Douter"]).sum()
    assert walk[0][1][2][1].any()
    assert (walk[-1][1][0] == box).sum() == 3 and walk[-1][1][0][0, 0] == 4.0
    # no two particles at the same point modulo the box
    wrapped = np.mod(c.pos, box)
    assert len(np.unique(wrapped, axis=0)) == c.n


def test_coincident_start_ends_in_the_error_flag():
    """rows 1 and 45 are the same point modulo the box: rij = 0, the contact polynomials vanish, the search returns lambda = 1
    at once and the force is 0 / 0.  Create goes through (nothing reaches the cap); the first iteration moves both to NaN and
    every search with them runs into the cap."""
    c = PC.build("coincident")
    assert not np.mod(c.pos[1] - c.pos[45], 4.0).any()
    S = R.Packing(c.grid, c.sizes_scaled, c.counts, c.pos, None, c.nominal_fraction, True)
    st = S.status()
    assert st["error"] == 0 and st["maxeval"] < 128 and st["Dinner"] == 0.0
    f = S.state()[2]
    assert np.isnan(f[1]).all() and np.isnan(f[45]).all() and np.isfinite(np.delete(f, (1, 45), axis=0)).all()
    st = S.run(5)
    assert st["error"] == 1 and st["maxeval"] == 256 and st["steps"] == 1   # the restatement counts the iteration that failed
    assert S.run(5)["steps"] == 1


def test_thrown_start_leaves_the_box():
    """deviation 11: 320 particles within half a cell on 8^3.  The first step is longer than the box, pbc wraps once, and
    coordinates stay outside for two iterations.  Outside, a particle has a cell only where (int)x is in 0..grid-1, and its
    range as A is taken by the floor modulo: the restatement's pair count equals the numpy count of that rule at every step."""
    c, walk = _walk("thrown", True, (0, 1, 2, 4))
    box = np.array(c.grid, dtype=np.float64)
    outside = [int(((s[0] < 0) | (s[0] > box)).sum()) for _, s in walk]
    print("coordinates outside the box after 0, 1, 2 and 4 iterations:", outside)
    assert outside[0] == 0 and outside[1] > 100 and outside[2] > 0
    low = min((s[0] + box - 0.55 * st["Douter"] * 2 * c.sizes_scaled[:, 0].max()).min() for st, s in walk)
    assert low < -1.0   # a range that starts below zero: where a truncating and a floor modulo part
    assert PC.partner_counts(c, c.pos, walk[0][0]["Douter"]).min() == 319 > PC.list_capacity(c) == 182
    for st, state in walk:
        assert st["error"] == 0 and st["maxeval"] < 128 and np.isfinite(state[0]).all()
        assert st["pairs"] == PC.partner_matrix(c, state[0], st["Douter"]).sum()


def _digest(S):
    st = S.status()
    h = hashlib.sha256()
    for a in S.state():
        h.update(np.ascontiguousarray(a).tobytes())
    return dict(steps=st["steps"], finished=st["finished"], Nsf=st["Nsf"], pairs=st["pairs"], maxeval=st["maxeval"],
                Douter=float(st["Douter"]).hex(), Dinner=float(st["Dinner"]).hex(), Force_step=float(st["Force_step"]).hex(),
                state_sha256=h.hexdigest())


def test_restatement_unchanged_inside_the_box():
    """tests/golden/packing_restatement_runs.json holds the restatement's trajectories on the shapes of the tests above and of
    tests/test_gpu_packing.py (start, 20 iterations, the end), recorded while active() still compared leap % grid with the cell.
    Inside the box x + grid - Rcut is positive and the two rules are one: every number and every bit of the states is the same."""
    runs = json.load(open(os.path.join(ROOT, "tests", "golden", "packing_restatement_runs.json")))["runs"]
    assert len(runs) == 12
    for r in runs:
        kw = dict(r["plan"])
        if "cells" in kw:
            kw["cells"] = [tuple(x) for x in kw["cells"]]
        plan = packing.packing_plan((r["size"],) * 3, **kw)
        S = R.Packing(plan.grid, plan.sizes_scaled, plan.counts, R.initial_positions(plan.grid, sum(plan.counts), r["seed"]), None,
                      plan.nominal_fraction, r["rotate"])
        where = (r["size"], r["seed"], r["rotate"])
        assert _digest(S) == r["start"], where
        S.run(20)
        assert _digest(S) == r["after20"], where
        S.run(1000)
        assert _digest(S) == r["end"] and r["end"]["finished"] == 1, where
