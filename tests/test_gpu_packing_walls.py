"""Packing inside walls on the GPU (hc_packing_set_walls, hc_packing_wall_field, hc_packing_walls, pack_pipe) against the
restatement in tests/packing_wall_ref.py: the distance field against a brute-force minimum, the wall probe, a trajectory
between two plates with a batch boundary and a list growth mid-run, a pipe packed to the end and taken into a lattice with
the same mask, and the periodic packing unchanged without walls.  Cases: tests/packing_wall_cases.py; the end state's
hematocrit and iteration count are recorded in tests/test_packing_wall_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import packing_cases
import packing_ref as R
import packing_wall_cases as cases
import packing_wall_ref as W
from hemocell_amd import packing

pytestmark = pytest.mark.gpu
IP = C.POINTER(C.c_int)
STATUS = R.STATUS + ("grow",)
INTS = ("steps", "finished", "Nsf", "error", "maxeval", "grow")


def _ip(a):
    return a.ctypes.data_as(IP)


class Device:
    """hc_packing_* on one packing; walls = (mask, spacing, periodic, margin) or None"""

    def __init__(self, gpu, grid, sizes, counts, pos, quat, nominal, rotate, walls=None, epsilon=0.0):
        self.gpu, self.lib = gpu, gpu.capi.lib()
        self.n = int(sum(counts))
        grid, counts = np.array(grid, dtype=np.int32), np.array(counts, dtype=np.int32)
        sizes, pos = np.ascontiguousarray(sizes, dtype=np.float64), np.ascontiguousarray(pos, dtype=np.float64)
        self.h = C.c_void_p()
        gpu.check(self.lib.hc_packing_create(C.byref(self.h), _ip(grid), len(counts), gpu.dptr(sizes), _ip(counts), gpu.dptr(pos),
                                             None if quat is None else gpu.dptr(np.ascontiguousarray(quat)), float(nominal), int(rotate), 0,
                                             float(epsilon)))
        if walls is not None:
            rc = self.set_walls(*walls)
            if rc != 0:
                self.destroy()
                gpu.check(rc)

    def set_walls(self, mask, spacing, periodic, margin):
        mask = np.ascontiguousarray(mask, dtype=np.uint8)
        self.dims = mask.shape
        dims, per = np.array(mask.shape, dtype=np.int32), np.array([int(bool(p)) for p in periodic], dtype=np.int32)
        return self.lib.hc_packing_set_walls(self.h, mask.ctypes.data, _ip(dims), float(spacing), _ip(per), float(margin))

    def run(self, steps, check=True):
        st = np.zeros(12)
        rc = self.lib.hc_packing_run(self.h, int(steps), self.gpu.dptr(st))
        if check:
            self.gpu.check(rc)
        d = dict(zip(STATUS, st))
        for k in INTS:
            d[k] = int(d[k])
        d["rc"] = rc
        return d

    def state(self):
        out = [np.zeros((self.n, 3)), np.zeros((self.n, 4)), np.zeros((self.n, 3)), np.zeros((self.n, 3))]
        self.gpu.check(self.lib.hc_packing_state(self.h, *[self.gpu.dptr(a) for a in out]))
        return out

    def field(self):
        out = np.zeros(self.dims)
        self.gpu.check(self.lib.hc_packing_wall_field(self.h, self.gpu.dptr(out)))
        return out

    def capacity(self):
        n, k = C.c_int(), C.c_int()
        self.gpu.check(self.lib.hc_packing_count(self.h, C.byref(n), C.byref(k)))
        return k.value

    def destroy(self):
        if self.h:
            self.lib.hc_packing_destroy(self.h)
        self.h = C.c_void_p()


def _compare(dev_st, dev_state, ref_st, ref_state, where):
    for k in ("steps", "finished", "Douter", "Dinner", "Relax", "Nsf", "Pactual", "DensityNominal", "error"):
        assert dev_st[k] == ref_st[k], (where, k, dev_st[k], ref_st[k])
    # the device adds |f| in a tree, the restatement in particle order: the one tolerance of tests/test_gpu_packing.py
    assert abs(dev_st["Force_step"] - ref_st["Force_step"]) <= 1e-12 * abs(ref_st["Force_step"]), where
    assert dev_st["maxeval"] == ref_st["maxeval"] and dev_st["maxeval"] < 128, where
    for name, a, b in zip(("positions", "quaternions", "forces", "torques"), dev_state, ref_state):
        assert np.array_equal(a, b), (where, name, np.abs(a - b).max())


def test_distance_field_equals_brute_force(gpu):
    """24 x 20 x 16 nodes, periodic in x, slabs on y and z and a sphere across the periodic face: bit for bit the minimum over
    all wall nodes, truncated at R.  Two RBCs at a first diameter of 3.6 make R = 7, below the widest gap's 7.5 nodes, so both
    truncated and untruncated nodes are compared."""
    mask = cases.field_mask()
    pos = np.array([[6.0, 5.0, 4.0], [2.5, 7.0, 2.0]])
    dev = Device(gpu, (12, 10, 8), [cases.RBC], [2], pos, None, 0.05, True, (mask, 0.5, (True, False, False), 0.1))
    try:
        R_nodes = W.truncation(dev.run(0)["Douter"], [cases.RBC], 0.5, 0.1)
        assert R_nodes == 7
        got = dev.field()
    finally:
        dev.destroy()
    want = W.brute_force_field(mask, (True, False, False), R_nodes)
    assert np.array_equal(got, want)
    assert (want == R_nodes - 0.5).sum() > 0 and (want == -0.5).sum() == int(mask.sum())
    assert len(np.unique(want)) > 20   # off-axis distances: square roots of sums of two and three squares
    assert np.array_equal(got, W.field(mask, (True, False, False), R_nodes))


@pytest.mark.parametrize("rotate", [1, 0])
def test_wall_probe_equals_restatement_bit_for_bit(gpu, rotate):
    size, quat, s, normal, d2, tags = cases.probe_inputs()
    n = len(tags)
    force, torque = np.zeros((n, 3)), np.zeros((n, 3))
    cand, ev, kind = np.zeros(n), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    D = gpu.dptr
    gpu.check(gpu.capi.lib().hc_packing_walls(n, D(size), D(quat), D(s), D(normal), D(d2), rotate, D(force), D(torque), D(cand), _ip(ev), _ip(kind)))
    assert set(kind) == {1, 2}
    for k in range(n):
        o = W.wall(size[k], quat[k], s[k], normal[k], d2[k], rotate)
        assert (kind[k], ev[k]) == (o["kind"], o["evals"]), tags[k]
        assert np.array_equal(force[k], o["f"]) and np.array_equal(torque[k], o["t"]) and cand[k] == o["candidate"], tags[k]
        assert (cand[k] == d2[k]) == (kind[k] == 1), tags[k]
        if kind[k] == 2:
            assert force[k] @ normal[k] > 0, tags[k]   # off the wall
    assert torque.any() == bool(rotate) and np.isfinite(torque).all() and ev.max() < 128


def test_trajectory_between_plates(gpu):
    """30 particles, not periodic in z, 40 iterations in batches of 7: positions, quaternions, forces, torques and the status
    block equal the restatement after every batch; a second run whose lists start at 4 slots has to grow them once, with an
    iteration interrupted behind its motion, and ends on the same bits"""
    c = cases.plates()
    walls = (c.mask, c.spacing, c.periodic, c.margin)
    ref = W.WallPacking(c.grid, c.sizes, c.counts, c.pos, c.quat, c.nominal, True, c.mask, c.spacing, c.periodic, c.margin)
    dev = Device(gpu, c.grid, c.sizes, c.counts, c.pos, c.quat, c.nominal, True, walls)
    small = Device(gpu, c.grid, c.sizes, c.counts, c.pos, c.quat, c.nominal, True, walls)
    try:
        _compare(dev.run(0), dev.state(), ref.status(), ref.state(), "start")
        assert ref.status()["wall_slots"] >= 15 and dev.state()[2].any() and dev.state()[3].any()
        gpu.check(small.lib.hc_packing_reserve_lists(small.h, 4))
        assert small.capacity() == 4
        done, grows = 0, 0
        for batch in (7, 7, 7, 7, 7, 5):
            ref_st, dev_st = ref.run(batch), dev.run(batch)
            done += batch
            assert dev_st["steps"] == done and dev_st["grow"] == 0 and not dev_st["finished"]
            state = dev.state()
            _compare(dev_st, state, ref_st, ref.state(), "after %d" % done)
            assert (state[0][:, 2] > 0.25).all() and (state[0][:, 2] < 7.75).all()   # between the plates' surfaces
            st = small.run(batch)
            while st["steps"] < done:
                assert st["grow"] == 1
                grows += 1
                st = small.run(done - st["steps"])
            _compare(st, small.state(), ref_st, ref.state(), "small lists, after %d" % done)
        assert grows == 1 and 4 < small.capacity() <= 29
    finally:
        dev.destroy(); small.destroy()


@pytest.fixture(scope="module")
def pipe(gpu):
    return packing.pack_pipe(cases.PIPE["length_um"], cases.PIPE["radius_um"], cases.HEMATOCRIT, dx_um=cases.PIPE["dx_um"], axis=0,
                             wall_margin_um=cases.PIPE["wall_margin_um"], seed=cases.PIPE["seed"], max_iter=cases.ITERATION_CAP)


def test_pipe_packs_to_the_end(gpu, pipe):
    """radius 20 um, length 24 um at the hematocrit the restatement reaches: finished in the restatement's iterations, and by
    its brute force over all pairs and all wall slots nothing overlaps at Dinner"""
    res = pipe
    assert res.counts == [78, 5] and res.plan.grid == (4, 7, 7) and res.wall_mask.shape == (48, 83, 83)
    assert res.finished and res.steps == cases.END_STEPS and res.max_root_evaluations < 128
    assert res.force_per_particle == 0.0 and res.inner_diameter == res.outer_diameter == 1.1072590236464144
    assert res.lumen_volume_um3 == 240624 * 0.125
    plan, mask, periodic, pos0, spacing, margin = cases.pipe_start()
    ref = W.WallPacking(plan.grid, plan.sizes_scaled, plan.counts, pos0, None, plan.nominal_fraction, True, mask, spacing, periodic, margin)
    pos = np.concatenate([res.positions[n] for n in res.names]) * plan.scale
    quat = np.concatenate([res.quaternions[n] for n in res.names])
    best, pairs, wall_slots, nothing, _ = ref.check(pos, quat, res.inner_diameter)
    assert pairs == 0 and wall_slots == 0 and nothing == 0 and best >= 1.0
    r = np.hypot(res.positions["RBC"][:, 1] - 20.5, res.positions["RBC"][:, 2] - 20.5)
    print("\ncentres of the RBCs: radial position %.2f .. %.2f um in a lumen of radius 20 um" % (r.min(), r.max()))
    assert r.max() < 19.0 - 2.2 * 1.107 + 0.5   # margin and thin semi-axis off the wall (half a node of staircase)


def test_pipe_packing_into_a_lattice(gpu, pipe):
    """every packed cell goes through host.Cells.addCell into a lattice with the pipe's mask: all placed, no vertex on a wall
    node, nothing removed by the first deletion check.  Packing the enclosing periodic box instead leaves cells across the wall."""
    res = pipe
    dx = res.mask_dx_um
    P = gpu.base_parameters()
    nx, ny, nz = res.wall_mask.shape
    L = gpu.Lattice(nx, ny, nz, (True, False, False), 1.0 / P.tau)
    h = None
    try:
        L.defineBounceBack(res.wall_mask)
        L.latticeEquilibrium()
        h = gpu.HemoCell(L, P)
        h.cellfields.addCellType(gpu.CellType.rbc(P), 1)
        h.cellfields.addCellType(gpu.CellType.plt(P), 1)
        for t, name in enumerate(("RBC", "PLT")):
            for centre, angles in zip(res.positions[name], res.angles[name]):
                assert h.cellfields.addCell(t, centre / dx, angles)
        nv, nc, _ = h.cellfields.counts()
        assert nc == 83
        node = np.floor(h.cellfields.positions + 0.5).astype(int)
        node[:, 0] %= nx
        assert (node[:, 1:] >= 0).all() and (node[:, 1] < ny).all() and (node[:, 2] < nz).all()
        assert not res.wall_mask[node[:, 0], node[:, 1], node[:, 2]].any()
        h.cellfields.applyConstitutiveModel(0, True)
        h.iterate(1)
        assert h.cellfields.deletion_counts() == (0, 0, 0, 0) and h.cellfields.alive().all()
        assert h.cellfields.counts()[:2] == (nv, nc) and np.isfinite(h.cellfields.positions).all()
    finally:
        if h is not None:
            h.cellfields.destroy()
        L.destroy()


def test_command_line_pipe_and_mask(gpu, tmp_path, capsys):
    """--pipe and --mask / --mask-dx / --periodic reach pack_cells: the same start gives the same .pos files either way"""
    args = ["16", "0", "0", "--rbc", "4", "--plt", "2", "--maxiter", "60", "--seed", "3"]
    assert packing._main(args + ["--pipe", "10", "--outdir", str(tmp_path / "pipe")]) == 0
    out = capsys.readouterr().out
    assert "Walls: mask 32 x 43 x 43 nodes at 0.5 um, periodic in x" in out and "Resolution of collision check: 3 x 4 x 4" in out
    np.save(str(tmp_path / "mask.npy"), packing.pipe_mask(16.0, 10.0, 0.5, 0))
    assert packing._main(["16", "21", "21"] + args[3:] + ["--mask", str(tmp_path / "mask.npy"), "--mask-dx", "0.5", "--periodic", "x",
                                                           "--outdir", str(tmp_path / "mask")]) == 0
    for name, n in (("RBC", 4), ("PLT", 2)):
        a, b = packing.read_pos(str(tmp_path / "pipe" / (name + ".pos"))), packing.read_pos(str(tmp_path / "mask" / (name + ".pos")))
        assert len(a[0]) == n and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert (np.hypot(a[0][:, 1] - 10.5, a[0][:, 2] - 10.5) < 10.0).all()
    assert packing._main(args + ["--pipe", "10", "--mask", "x.npy"]) == 1 and packing._main(args + ["--mask", str(tmp_path / "none.npy")]) == 1


def test_without_walls_nothing_changes(gpu):
    """no hc_packing_set_walls: the bits of the periodic trajectory case uneven134 of tests/packing_cases.py"""
    c = packing_cases.build("uneven134")
    ref = R.Packing(c.grid, c.sizes_scaled, c.counts, c.pos, c.quat, c.nominal_fraction, True)
    dev = Device(gpu, c.grid, c.sizes_scaled, c.counts, c.pos, c.quat, c.nominal_fraction, True)
    try:
        _compare(dev.run(0), dev.state(), ref.status(), ref.state(), "start")
        for upto, batch in ((3, 3), (10, 7)):
            ref_st, dev_st = ref.run(batch), dev.run(batch)
            assert dev_st["steps"] == upto and dev_st["grow"] == 0
            _compare(dev_st, dev.state(), ref_st, ref.state(), "after %d" % upto)
        assert dev.lib.hc_packing_wall_field(dev.h, gpu.dptr(np.zeros(8))) == 2 and b"no walls are set" in dev.lib.hc_last_error()
    finally:
        dev.destroy()


def test_refusals_and_the_wall_node_error(gpu):
    mask = np.zeros((8, 8, 9), dtype=np.uint8)
    mask[:, :, 0] = mask[:, :, -1] = 1
    per = (True, True, False)
    pos = np.array([[2.0, 2.0, 1.0], [1.0, 3.0, 3.0]])
    dev = Device(gpu, (4, 4, 4), [cases.RBC], [2], pos, None, 0.05, True)
    err = dev.lib.hc_last_error
    try:
        open_face = mask.copy(); open_face[3, 4, 8] = 0
        assert dev.set_walls(open_face, 0.5, per, 0.1) == 2 and b"axis z is not periodic and has an open face" in err()
        assert dev.set_walls(mask, 0.5, (False, True, False), 0.1) == 2 and b"axis x is not periodic and has an open face" in err()
        assert dev.set_walls(mask, 0.6, per, 0.1) == 2 and b"the mask and the box disagree" in err()
        assert dev.set_walls(mask[:, :, :5], 1.5, (False, False, False), 0.1) == 2 and b"the mask and the box disagree" in err()
        assert dev.set_walls(mask, 0.5, per, -1.0) == 2 and dev.set_walls(mask, 0.5, per, np.nan) == 2
        blocked = mask.copy(); blocked[4, 4, 2] = 1   # the first particle's node
        assert dev.set_walls(blocked, 0.5, per, 0.1) == 2 and b"starts on a wall node" in err()
        assert dev.set_walls(mask, 0.5, per, 0.1) == 0
        assert dev.set_walls(mask, 0.5, per, 0.1) == 2 and b"already set" in err()
    finally:
        dev.destroy()
    late = Device(gpu, (4, 4, 4), [cases.RBC], [2], pos, None, 0.05, True)
    try:
        late.run(0)
        assert late.set_walls(open_face, 0.5, per, 0.1) == 2 and b"open face" in err()   # run(0) queued nothing: still allowed to try
        late.run(1)
        assert late.set_walls(mask, 0.5, per, 0.1) == 2 and b"before the first hc_packing_run" in err()
    finally:
        late.destroy()
    # two RBCs on top of each other at the lower plate, a margin as thick as the gap and long steps: one is pushed onto a wall node
    low = np.array([[2.0, 2.0, 0.30], [2.0, 2.0, 0.45]])
    ref = W.WallPacking((4, 4, 4), [cases.RBC], [2], low, None, 0.05, False, mask, 0.5, per, 1.0, epsilon=5.0)
    assert ref.run(50)["error"] == 2
    hit = Device(gpu, (4, 4, 4), [cases.RBC], [2], low, None, 0.05, False, (mask, 0.5, per, 1.0), epsilon=5.0)
    try:
        st = hit.run(50, check=False)
        assert st["rc"] == 3 and st["error"] == 2 and st["finished"] == 0 and st["steps"] == ref.status()["steps"]
        assert b"reached a wall node" in err()
        assert hit.run(5, check=False)["rc"] == 3   # sticky
    finally:
        hit.destroy()
