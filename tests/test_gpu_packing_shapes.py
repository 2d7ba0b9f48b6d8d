"""The packing kernels (hemocell_amd/csrc/packing.hip) past one wave, one block and one grid size, against the restatement in
tests/packing_ref.py bit for bit, on the starts of tests/packing_cases.py: pk_list's carry from chunk to chunk, second blocks of
pk_motion / pk_bin / pk_sum / pk_probe, the stride and the tree of pk_control, grids with three different axes, a sphere among
the species, orientations given to create, lists that grow in create, particles on the faces and outside the box, the
null outputs of hc_packing_state and the sticky error flag.  tests/test_packing_cpu.py checks what every start rests on."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import packing_cases as PC
import packing_ref as R
from test_gpu_packing import DevicePacking, _compare, _ip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _capacity(dev):
    n, k = C.c_int(), C.c_int()
    dev.gpu.check(dev.lib.hc_packing_count(dev.h, C.byref(n), C.byref(k)))
    assert n.value == dev.n
    return k.value


def _walk(gpu, case, rotate, marks, each=None, to_end=False):
    """device and restatement side by side: compared after each of marks iterations (0 = what create left), then to the end"""
    ref = R.Packing(case.grid, case.sizes_scaled, case.counts, case.pos, case.quat, case.nominal_fraction, rotate)
    dev = DevicePacking(gpu, case, case.pos, rotate, case.quat)
    try:
        done = 0
        for upto in marks:
            ref_st, dev_st = ref.run(upto - done), dev.run(upto - done)
            done = upto
            assert ref_st["steps"] == upto and dev_st["grow"] == 0
            dev_state, ref_state = dev.state(), ref.state()
            _compare(dev_st, dev_state, ref_st, ref_state, "%s after %d" % (case.name, upto))
            assert dev_state[2].any() and not dev_st["finished"]   # a live state
            if each is not None:
                each(upto, dev, dev_st, dev_state, ref_st)
        if to_end:
            ref_st, dev_st = ref.run(1000 - done), dev.run(1000 - done)
            assert ref_st["finished"] == 1 and done < ref_st["steps"] <= 500 and dev_st["grow"] == 0
            _compare(dev_st, dev.state(), ref_st, ref.state(), "%s at the end" % case.name)
    finally:
        dev.destroy()


@pytest.mark.parametrize("rotate", [True, False])
@pytest.mark.parametrize("name", PC.UNEVEN)
def test_uneven_grids_past_one_wave(gpu, name, rotate):
    """grids (5, 6, 8) and (3, 6, 8) with RBC, PLT and a spherical WBC, orientations given to create, N = 288, 134 and 70: after
    0, 1, 5 and 20 iterations everything equals the restatement bitwise (Force_step within 1e-12, deviation 6), and the
    288-particle start also at its end.  A swapped axis in pk_bin or partner(), a wrong prefix across pk_list's chunks or a
    second block that never ran would each move a bit."""
    case = PC.build(name)
    n, all_pairs = case.n, case.n * (case.n - 1) // 2
    wbc, rbc = case.rows("WBC"), case.rows("RBC")
    K = PC.list_capacity(case)

    def each(upto, dev, dev_st, state, ref_st):
        mode = PC.modes(case, ref_st["Douter"])   # the rule itself, packing.h:390-393
        assert mode == PC.UNEVEN_MODES[name]
        if "part" in mode:
            assert 0 < ref_st["pairs"] < all_pairs
        else:
            assert ref_st["pairs"] == all_pairs
        if upto == 0 and name == "uneven288":
            assert ref_st["pairs"] == 6369   # about 6300 of 41328
        assert np.array_equal(state[1][wbc], case.quat[wbc])   # the sphere never turns
        assert not state[3][wbc].any()                         # and carries no torque of its own
        assert state[3][rbc].any() == bool(rotate)
        if upto > 0:
            assert (not np.array_equal(state[1][rbc], case.quat[rbc])) == bool(rotate)
        assert _capacity(dev) == K

    _walk(gpu, case, rotate, (0, 1, 5, 20), each, to_end=name == "uneven288")


@pytest.mark.parametrize("rotate", [True, False])
def test_lists_grow_in_create(gpu, rotate):
    """200 particles within a cube of edge 0.9 on 8^3: create starts with lists of 161, every particle has 199 partners, pk_list
    truncates and raises grow, everything behind it is skipped, and create retries with 199 + 199 / 4 + 16 capped at N - 1.
    What create leaves equals the restatement's 19900 pairs bitwise, as do the states after 1, 5 and 20 iterations, over which
    the lists shrink from everyone to about 40."""
    case = PC.build("cluster")
    assert PC.list_capacity(case) == 161 and PC.grown_capacity(case, 199) == 199

    def each(upto, dev, dev_st, state, ref_st):
        assert _capacity(dev) == 199
        assert ref_st["pairs"] == 19900 if upto == 0 else ref_st["pairs"] < 3000

    _walk(gpu, case, rotate, (0, 1, 5, 20), each)


@pytest.mark.parametrize("rotate", [True, False])
def test_particles_on_the_faces(gpu, rotate):
    """deviation 8 of DESIGN section 6: a particle exactly on an upper face has no cell and is nobody's partner as B.  Particle 0
    (x = 4.0, the lowest index, so never an A) has exactly zero force at every compared step and does not move; particle 1
    at the origin is pushed from the start."""
    case = PC.build("faces")

    def each(upto, dev, dev_st, state, ref_st):
        assert not state[2][0].any() and not state[3][0].any()
        assert np.array_equal(state[0][0], case.pos[0]) and state[0][0, 0] == 4.0
        if upto == 0:
            assert state[2][1].any() and ref_st["pairs"] == 828
        if upto == 20:
            assert (state[0] == 4.0).sum() == 3

    _walk(gpu, case, rotate, (0, 1, 5, 20), each)


def test_positions_thrown_outside_the_box(gpu):
    """deviation 11: 320 particles within half a cell on 8^3 (the lists grow to 319 in create); the first step is longer than
    the box, so coordinates lie outside it after 1 and 2 iterations, where only a cell with (int)x in 0..grid-1 counts and
    A's range is taken by the floor modulo"""
    case = PC.build("thrown")
    box = np.array(case.grid, dtype=np.float64)
    outside = []

    def each(upto, dev, dev_st, state, ref_st):
        outside.append(int(((state[0] < 0) | (state[0] > box)).sum()))
        assert _capacity(dev) == 319

    _walk(gpu, case, True, (0, 1, 2, 4), each)
    assert outside[0] == 0 and outside[1] > 100 and outside[2] > 0


def test_pair_probe_past_two_blocks(gpu):
    """hc_packing_pairs on the fixture's pairs of one rotate value repeated to 600: three blocks of pk_probe, the last with 88
    threads at work.  Every row equals the restatement bitwise, and a pair gives the same wherever it stands."""
    pairs = json.load(open(os.path.join(ROOT, "tests", "golden", "packing_pairs.json")))["pairs"]
    lib = gpu.capi.lib()
    n = 600
    for rotate in (1, 0):
        sel = [p for p in pairs if p["rotate"] == rotate]
        m = len(sel)
        assert 60 <= m < 256 and n > 2 * 256 and n % 256 and n % m
        want = [R.pair(p["sizeA"], p["qA"], p["sizeB"], p["qB"], p["rij"], p["Douter"] * p["Douter"], rotate) for p in sel]
        rep = [sel[k % m] for k in range(n)]
        arr = lambda k: np.ascontiguousarray([p[k] for p in rep], dtype=np.float64)
        sa, qa, sb, qb, rij = arr("sizeA"), arr("qA"), arr("sizeB"), arr("qB"), arr("rij")
        d2 = np.array([p["Douter"] * p["Douter"] for p in rep])
        lam, fscl = np.full(n, np.nan), np.full(n, np.nan)
        nv, fA, tA, fB, tB = (np.full((n, 3), np.nan) for _ in range(5))
        ev, kind = np.full(n, -7, dtype=np.int32), np.full(n, -7, dtype=np.int32)
        D = gpu.dptr
        gpu.check(lib.hc_packing_pairs(n, D(sa), D(qa), D(sb), D(qb), D(rij), D(d2), rotate, D(lam), D(fscl), D(nv), D(fA), D(tA), D(fB), D(tB),
                                       _ip(ev), _ip(kind)))
        for k in range(n):
            o, tag = want[k % m], rep[k]["tag"]
            assert (kind[k], ev[k]) == (o["kind"], o["evals"]), (k, tag)
            assert lam[k] == o["lambda"] and fscl[k] == o["fscl"], (k, tag)
            for got, key in ((nv, "n"), (fA, "fA"), (tA, "tA"), (fB, "fB"), (tB, "tB")):
                assert np.array_equal(got[k], o[key]), (k, tag, key)
        for got in (lam, fscl, nv, fA, tA, fB, tB, ev, kind):
            assert np.array_equal(got[:n - m], got[m:])   # rows k and k + len(sel)


def test_state_with_null_outputs(gpu):
    """hc_packing_state with one output at a time and the other three null returns what the call with all four returned"""
    case = PC.build("uneven288")
    dev = DevicePacking(gpu, case, case.pos, True, case.quat)
    try:
        dev.run(3)
        full = dev.state()
        assert all(a.any() for a in full)
        for at, a in enumerate(full):
            one = np.full(a.shape, np.nan)
            args = [None] * 4
            args[at] = gpu.dptr(one)
            gpu.check(dev.lib.hc_packing_state(dev.h, *args))
            assert np.array_equal(one, a), at
        gpu.check(dev.lib.hc_packing_state(dev.h, None, None, None, None))
    finally:
        dev.destroy()


def test_error_flag_is_sticky_and_ends_cleanly(gpu):
    """two particles at the same point modulo the box: rij = 0 and the pair's force is 0 / 0.  Create goes through, as in the
    restatement; the first iteration moves both to NaN, every root search with them runs into the cap of 256, and
    hc_packing_run returns HC_ERR_STATE with the flag set, now and on every later call.  The device skips the rest of an
    iteration once the flag is up, so its count of steps done stays 0 where the restatement, which walks iterate() to its
    end, counts the failed one.  Flags and step counts only: the state is NaN."""
    case = PC.build("coincident")
    ref = R.Packing(case.grid, case.sizes_scaled, case.counts, case.pos, None, case.nominal_fraction, True)
    assert ref.status()["error"] == 0
    ref_st = ref.run(5)
    assert (ref_st["error"], ref_st["maxeval"], ref_st["steps"]) == (1, 256, 1)
    dev = DevicePacking(gpu, case, case.pos, True)
    lib = dev.lib
    try:
        st = dev.run(0)
        assert st["error"] == 0 and st["steps"] == 0 and st["maxeval"] < 128
        status = np.zeros(12)
        for _ in range(2):
            assert lib.hc_packing_run(dev.h, 5, gpu.dptr(status)) == 3   # HC_ERR_STATE
            assert b"root search" in lib.hc_last_error()
            assert status[9] == 1 == ref_st["error"] and status[10] == 256 == ref_st["maxeval"]
            assert status[0] == 0 == ref_st["steps"] - 1 and status[1] == 0 and status[11] == 0
    finally:
        assert lib.hc_packing_destroy(dev.h) == 0
        dev.h = None
