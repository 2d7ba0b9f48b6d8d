"""Packing inside walls without a GPU: the plan for a lumen, the mirror image, the wall contact scale against the closed form
for an ellipsoid and a plane, the host-side refusals, the distance passes against the definition, and the restatement
(tests/packing_wall_ref.py) packing the pipe of tests/test_gpu_packing_walls.py to the end.

End state (PIPE below: radius 20 um, length 24 um, dx 0.5 um, margin 1.0 um, seed 1, cap 5000 iterations).  The restatement
alone, started as pack_pipe starts the device:
  hematocrit 0.30 (93 RBC + 7 PLT): not finished after 5000 iterations (Douter 1.0926, Dinner 0.6393, force per particle 0.336)
  hematocrit 0.25 (78 RBC + 5 PLT): finished after 4392 iterations, Douter = Dinner = 1.1072590236464144
so the end-state tests run at HEMATOCRIT = 0.25.  The cap is a condition of the test, not a tuning: at Relax = Douter0 / 204800
per iteration, 5000 iterations take the outer diameter down by 2.4 %, and a target that needs more than that is too dense
for this start."""
import numpy as np
import pytest

import packing_ref as R
import packing_wall_cases as cases
import packing_wall_ref as W
from hemocell_amd import packing

SCALE = 1.2 / 8.4
RBC = np.array([8.4, 4.4, 8.4]) * SCALE
PLT = np.array([2.4, 1.05, 2.4]) * SCALE
WBC = np.array([8.4, 8.4, 8.4]) * SCALE

PIPE, HEMATOCRIT, ITERATION_CAP, END_STEPS, pipe_start = cases.PIPE, cases.HEMATOCRIT, cases.ITERATION_CAP, cases.END_STEPS, cases.pipe_start
# the one tolerance the packing tests hold a summed quantity to (tests/test_gpu_packing.py, Force_step): 1e-12 relative.  The
# root search ends within 2e-15 of its lambda, where f_AB is stationary, so what is left is the rounding of the contact
# polynomials' coefficients; the recorded pairs themselves are reproduced with difference 0, which a closed form cannot be.
CONTACT_RTOL = 1e-12


def test_plan_counts_come_from_the_lumen():
    """24 x 41 x 41 um holds 40344 um^3, the pipe's lumen 30078 um^3 (240624 fluid nodes of 0.125 um^3).  By hand, with the
    hematocrit in single precision: 0.3 * 40344 / 97 = 124.8 -> 125 RBC, 8.75 -> 9 PLT; 0.3 * 30078 / 97 = 93.02 -> 93 RBC,
    6.51 -> 7 PLT; 0.25 * 30078 / 97 = 77.5 -> 78 RBC, 5.46 -> 5 PLT.  Grid and sizing factor do not move."""
    box = packing.packing_plan((24, 41, 41), hematocrit=0.30)
    lumen = packing.packing_plan((24, 41, 41), hematocrit=0.30, volume_um3=30078.0)
    assert box.counts == [125, 9] and lumen.counts == [93, 7]
    assert packing.packing_plan((24, 41, 41), hematocrit=0.25, volume_um3=30078.0).counts == [78, 5]
    assert lumen.grid == box.grid and lumen.scale == box.scale and lumen.box_um == box.box_um
    assert lumen.nominal_fraction == pytest.approx(box.nominal_fraction * (93 * 8.4 * 4.4 * 8.4 + 7 * 2.4 * 1.05 * 2.4)
                                                   / (125 * 8.4 * 4.4 * 8.4 + 9 * 2.4 * 1.05 * 2.4), rel=1e-14)
    explicit = packing.packing_plan((24, 41, 41), cells=[("RBC", 5)], volume_um3=30078.0)
    assert explicit.counts == [5]   # no hematocrit: the volume decides nothing
    with pytest.raises(ValueError):
        packing.packing_plan((24, 41, 41), hematocrit=0.3, volume_um3=0.0)
    mask = packing.pipe_mask(24.0, 20.0, 0.5, 0)
    assert mask.shape == (48, 83, 83) and int((mask == 0).sum()) == 240624
    plan = pipe_start(0.30)[0]
    assert plan.counts == [93, 7] and plan.grid == (4, 7, 7) and plan.scale == pytest.approx(1 / 6.0, rel=1e-15)


def _random_unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1)[:, None]


def test_image_is_a_proper_rotation_of_the_reflected_ellipsoid():
    """Q' = countQ of the image's quaternion is orthogonal with determinant +1, and its shape matrix Q'^T D Q' is H A H"""
    rng = np.random.Generator(np.random.PCG64(3))
    q = rng.normal(size=(40, 4))
    q /= np.linalg.norm(q, axis=1)[:, None]
    q[0] = (1, 0, 0, 0)
    n = _random_unit(rng, 40)
    n[1], n[2] = (0, 0, 1), (0, -1, 0)
    D = np.diag(RBC ** 2)
    for k in range(40):
        qi = W.image_quat(q[k], n[k])
        assert abs(np.linalg.norm(qi) - 1) < 1e-15
        Q, Qi = packing.quaternion_matrix(q[k]), packing.quaternion_matrix(qi)
        assert np.abs(Qi @ Qi.T - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(Qi) - 1) < 1e-14
        H = np.eye(3) - 2 * np.outer(n[k], n[k])
        assert np.abs(Qi.T @ D @ Qi - H @ (Q.T @ D @ Q) @ H).max() < 1e-14
        assert np.abs(Qi.T - H @ Q.T @ np.diag([1.0, 1.0, -1.0])).max() < 1e-14   # body to world: H R diag(1, 1, -1)


def test_wall_contact_scale_equals_the_closed_form():
    """An ellipsoid x^T A^-1 x <= sigma^2 (A = R diag(semi-axes^2) R^T) touches the plane at distance s along -n when
    sigma = s / sqrt(n^T A n).  The wall slot's 4 f_AB(lambda) is sigma^2 of the pair with the mirror image."""
    rng = np.random.Generator(np.random.PCG64(4))
    rows = []
    for size in (RBC, PLT, WBC):
        rows.append((size, np.array([1.0, 0, 0, 0]), np.array([0.0, 0, 1.0]), 0.4))       # axis-aligned
        rows.append((size, np.array([1.0, 0, 0, 0]), np.array([0.0, -1.0, 0]), 0.2))
    while len(rows) < 50:
        size = (RBC, PLT, WBC)[len(rows) % 3]
        q = rng.normal(size=4)
        rows.append((size, q / np.linalg.norm(q), _random_unit(rng, 1)[0], float(rng.uniform(0.05, 1.2)) * size.max()))
    worst = 0.0
    for size, q, n, s in rows:
        o = W.wall(size, q, s, n, 1.0, 1)
        assert o["capped"] == 0 and o["kind"] in (1, 2) and o["evals"] < 128
        Q = packing.quaternion_matrix(q)
        A = Q.T @ np.diag((0.5 * size) ** 2) @ Q
        sigma = s / np.sqrt(n @ A @ n)
        err = abs(np.sqrt(o["fscl"]) - sigma) / sigma
        worst = max(worst, err)
        assert err <= CONTACT_RTOL, (size, q, n, s, err)
        assert (o["kind"] == 2) == (sigma < 1.0)
        if o["kind"] == 2:   # pushed off the wall along n, by 1 - f_AB
            assert np.abs(o["f"] - n * (1 - sigma * sigma)).max() < 1e-9
            assert np.isfinite(o["t"]).all()
    print("\nlargest relative difference of the wall contact scale to s / sqrt(n^T A n): %.3e" % worst)


def test_axis_along_the_normal_gives_no_torque():
    """X n parallel to n: the pair function's torque direction is 0/0 there; the wall slot returns zero"""
    o = W.wall(RBC, [1.0, 0, 0, 0], 0.2, [0.0, 0, 1.0], 1.0, 1)
    assert o["kind"] == 2 and not o["t"].any() and o["f"][2] > 0 and not o["f"][:2].any()
    tilted = W.wall(RBC, [0.9, 0.3, 0.1, 0.2], 0.2, [0.0, 0, 1.0], 1.0, 1)
    assert tilted["kind"] == 2 and tilted["t"].any()


def test_distance_passes_equal_the_definition():
    """the three integer passes (the restatement's and packing.wall_distance_field) against the brute-force minimum over all
    wall nodes on the mask of the GPU test: slabs on y and z, a sphere across the periodic x face"""
    mask = cases.field_mask()
    for R_nodes in (3, 6):
        want = W.brute_force_field(mask, (True, False, False), R_nodes)
        assert np.array_equal(W.field(mask, (True, False, False), R_nodes), want)
        assert np.array_equal(packing.wall_distance_field(mask, (True, False, False), R_nodes), want)
    assert want.min() == -0.5 and want.max() == 5.5
    assert (want[mask != 0] == -0.5).all() and (want[mask == 0] >= 0.5).all()


def test_sample_of_a_plane_is_exact():
    """between two plates the trilinear sample is the distance to the halfway surface, and the normal is +-z"""
    mask = np.zeros((8, 8, 17), dtype=np.uint8)
    mask[:, :, 0] = mask[:, :, -1] = 1
    f = W.field(mask, (True, True, False), 20)
    s, n, ok = W.sample(f, (True, True, False), 0.5, 0.1, [1.3, 3.9, 1.7])
    assert ok and s == pytest.approx(1.7 - 0.25 - 0.1, abs=1e-15) and np.array_equal(n, [0, 0, 1])
    s, n, ok = W.sample(f, (True, True, False), 0.5, 0.1, [3.99, 0.01, 7.1])   # wraps in x and y
    assert ok and s == pytest.approx(8 - 7.1 - 0.25 - 0.1, abs=1e-14) and np.array_equal(n, [0, 0, -1])
    flat = W.field(mask, (True, True, False), 3)   # truncated at 3 nodes: a plateau between the plates, no gradient
    assert flat[0, 0, 3] == 2.5 == flat[0, 0, 8] and flat[0, 0, 2] == 1.5
    assert not W.sample(flat, (True, True, False), 0.5, 0.1, [1.0, 1.0, 4.2])[2]
    assert W.sample(flat, (True, True, False), 0.5, 0.1, [1.0, 1.0, 1.2])[2]


def test_refusals_on_the_host():
    m = np.zeros((8, 8, 9), dtype=np.uint8)
    m[:, :, 0] = m[:, :, -1] = 1
    cells = [("RBC", 2)]
    open_face = m.copy(); open_face[3, 4, 0] = 0
    with pytest.raises(ValueError, match="axis z is not periodic and has an open face"):
        packing.pack_cells((4, 4, 4), cells=cells, wall_mask=open_face, mask_dx_um=0.5, periodic=(True, True, False))
    with pytest.raises(ValueError, match="axis x is not periodic and has an open face"):
        packing.pack_cells((4, 4, 4), cells=cells, wall_mask=m, mask_dx_um=0.5, periodic=(False, True, False))
    with pytest.raises(ValueError, match="the mask and the box disagree: axis x is periodic"):
        packing.pack_cells((5, 4, 4), cells=cells, wall_mask=m, mask_dx_um=0.5, periodic=(True, True, False))
    with pytest.raises(ValueError, match="the mask and the box disagree: the mask is longer than the box along z"):
        packing.pack_cells((4, 4, 3), cells=cells, wall_mask=m, mask_dx_um=0.5, periodic=(True, True, False))
    with pytest.raises(ValueError, match="mask_dx_um"):
        packing.pack_cells((4, 4, 4), cells=cells, wall_mask=m, periodic=(True, True, False))
    with pytest.raises(ValueError, match="whole number of grid cells"):
        packing.wall_plan((24, 25, 4), np.zeros((48, 50, 9), dtype=np.uint8) + m[:1, :1, :], 0.5, (True, True, False), cells=cells)
    with pytest.raises(ValueError, match="whole number of dx_um"):
        packing.pipe_mask(24.2, 20.0, 0.5)


def test_wall_start_keeps_to_the_rule():
    """every centre lies on a node further from the wall than its species' smallest semi-axis at the first diameter, the draws
    are the seed's stream, and without rejections they are the periodic start"""
    plan, mask, periodic, pos, spacing, margin = pipe_start()
    n = sum(plan.counts)
    douter0 = (4 * 7 * 7 / (3.141592653589793 / 6.) / n * plan.nominal_fraction) ** (1. / 3.)
    s_node = packing.wall_distance_field(mask, periodic, 14) * spacing - margin
    node = np.floor(pos / spacing + 0.5).astype(int)
    node[:, 0] %= mask.shape[0]
    s = s_node[node[:, 0], node[:, 1], node[:, 2]]
    spec = np.repeat([0, 1], plan.counts)
    assert (s > 0.5 * plan.sizes_scaled[spec].min(axis=1) * douter0).all()
    stream = np.random.Generator(np.random.PCG64(PIPE["seed"])).random((400, 3)) * np.array(plan.grid, dtype=np.float64)
    at = 0
    for p in pos:   # every centre is a candidate of the stream, in order
        while not np.array_equal(stream[at], p):
            at += 1
        at += 1
    assert at > n   # some were rejected
    plan2, m2, per2, _ = packing.wall_plan((28, 28, 28), np.zeros((56, 56, 56), dtype=np.uint8), 0.5, (True, True, True), cells=[("RBC", 9)])
    pos2 = packing.wall_start(plan2, m2, 0.5, per2, 0.5, np.random.Generator(np.random.PCG64(2)))[0]
    assert np.array_equal(pos2, R.initial_positions(plan2.grid, 9, 2))


@pytest.fixture(scope="module")
def pipe_end():
    plan, mask, periodic, pos, spacing, margin = pipe_start()
    S = W.WallPacking(plan.grid, plan.sizes_scaled, plan.counts, pos, None, plan.nominal_fraction, True, mask, spacing, periodic, margin)
    first = S.status()
    st = S.run(ITERATION_CAP)
    return plan, S, first, st


def test_restatement_packs_the_pipe_to_the_end(pipe_end):
    plan, S, first, st = pipe_end
    assert plan.counts == [78, 5] and first["wall_slots"] > 0 and first["truncation"] == 14
    assert st["finished"] == 1 and st["error"] == 0 and st["steps"] == END_STEPS <= ITERATION_CAP
    assert st["Dinner"] == st["Douter"] == 1.1072590236464144 and st["maxeval"] < 128
    pos, quat, f, t = S.state()
    assert not f.any() and not t.any()
    best, pairs, walls, nothing, no_normal = S.check(pos, quat, st["Dinner"])
    assert pairs == 0 and walls == 0 and nothing == 0 and best >= 1.0
    assert 0 < no_normal < sum(plan.counts)   # cells in the core are beyond the field's truncation: no wall partner


def test_wall_node_error_has_its_own_code():
    """a particle pushed through the margin onto a wall node ends the run with error 2, not clamped"""
    mask = np.zeros((8, 8, 9), dtype=np.uint8)
    mask[:, :, 0] = mask[:, :, -1] = 1
    # two RBCs on top of each other right at the lower plate; with a margin as thick as the gap the wall pushes the wrong way
    pos = np.array([[2.0, 2.0, 0.30], [2.0, 2.0, 0.45]])
    S = W.WallPacking((4, 4, 4), [RBC], [2], pos, None, 0.05, False, mask, 0.5, (True, True, False), 1.0, epsilon=5.0)
    st = S.run(50)
    assert st["error"] == 2 and st["finished"] == 0 and st["steps"] < 50


def test_plates_case_is_live_and_the_probe_inputs_cover_the_kinds():
    """the conditions the GPU trajectory and probe tests rest on: 40 iterations between the plates without an error, with wall
    slots, overlaps and torques all the way; the probe rows reach overlap, no overlap, the floor and the zero torque"""
    c = cases.plates()
    S = W.WallPacking(c.grid, c.sizes, c.counts, c.pos, c.quat, c.nominal, True, c.mask, c.spacing, c.periodic, c.margin)
    st = S.status()
    assert 4.0 < st["Douter"] < 4.1 and st["wall_slots"] >= 15 and 0 < st["pairs"] < 30 * 29 // 2   # the platelets use the cell list
    for k in range(6):
        st = S.run(7 if k < 5 else 5)
        pos, quat, f, t = S.state()
        assert st["error"] == 0 and not st["finished"] and st["wall_slots"] >= 15
        assert np.abs(f).max() > 0.1 and np.abs(t).max() > 0.1 and np.isfinite(pos).all() and np.isfinite(quat).all()
        assert (pos[:, 2] > 0.25).all() and (pos[:, 2] < 7.75).all()
    assert st["steps"] == 40
    size, quat, s, normal, d2, tags = cases.probe_inputs()
    kinds = {}
    for k in range(60):
        o = W.wall(size[k], quat[k], s[k], normal[k], d2[k], 1)
        assert o["capped"] == 0, tags[k]
        kinds[tags[k].split("/")[-1]] = kinds.get(tags[k].split("/")[-1], set()) | {o["kind"]}
        if "identity" in tags[k]:
            assert not o["t"].any(), tags[k]
    assert kinds["deep"] == {2} and kinds["near_in"] == {2} and kinds["near_out"] == {1} and kinds["far"] == {1}
    assert kinds["deep@0"] == {2} and kinds["deep@neg"] == {2} and kinds["deep@floor"] == {2}
    a, b = W.wall(size[0], quat[0], 0.0, normal[0], d2[0], 1), W.wall(size[0], quat[0], 1e-6, normal[0], d2[0], 1)
    assert np.array_equal(a["f"], b["f"]) and a["fscl"] == b["fscl"]
