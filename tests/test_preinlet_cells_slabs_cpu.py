"""The inputs of tests/test_gpu_preinlet_cells_slabs.py (tests/preinlet_cells_slabs_scene.py) are what that file claims, from
tests/preinlet_cells_ref.py and numpy alone -- every cell stands as the eight corners of its bounding box -- and the collective
entry point is declared and bound."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import preinlet_cells_ref as PC
import preinlet_cells_slabs_scene as SC
from hemocell_amd import capi, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [("Xneg", 2), ("Xpos", 2), ("Xneg", 3), ("Xpos", 3)]
NV = {0: 8, 1: 8}


def test_entry_point_is_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "hemocell_amd.h")).read()
    assert re.search(r"\bint hcp_preinlet_create_slab\(", header)
    assert capi.SIGNATURES["hcp_preinlet_create_slab"] == capi.SIGNATURES["hcp_preinlet_create"]
    assert capi.SIGNATURES["hcp_preinlet_create_slab"][0] is C.c_int
    for name in ("iterate", "applyPreInletCells", "cell_counts", "destroy"):
        assert callable(getattr(host.PreInletPeer, name))
    assert SC.REC == host.Cells.SV_DTYPE


def test_scene_geometry():
    assert SC.domain(2) == (96, 48) and SC.domain(3) == (120, 40)
    assert SC.slab_of(1, 3) == (40, 80)
    assert (SC.inlet_rank("Xneg", 3), SC.far_rank("Xneg", 3), SC.inlet_rank("Xpos", 3), SC.far_rank("Xpos", 3)) == (0, 2, 2, 0)


@pytest.mark.parametrize("direction, world", CASES)
def test_static_candidates_collision_and_margin(direction, world):
    sign = SC.SIGN[direction]
    nxg, _ = SC.domain(world)
    shift = SC.static_shift(direction, world)
    pre = SC.box_records(SC.static_pre_cells(), SC.STATIC_LAPS)
    residents = SC.static_residents(direction, world)
    dom = SC.box_records(residents)
    # which candidates lie in the window, in ascending (type, slot) order
    cand = PC.select(pre, NV, 0, SC.PRE[0], SC.STATIC_WINDOW)
    assert [(t, i, lap) for t, i, _, lap in cand] == [(0, 5007, 0), (1, 5011, 2), (1, 5014, 0), (1, 5015, 0)]
    x = {int(i): r["position"][:, 0] for (t, i), r in PC.by_id(pre).items()}
    assert x[5012].min() < SC.STATIC_WINDOW[1] < x[5012].max() and x[5013].max() < SC.STATIC_WINDOW[0]
    # what arrives: 5014 leaves the domain in y, the far rank's resident holds 5015's new id
    offered = set()
    out, ids, rejected = PC.inject(pre, dom, NV, 0, sign, SC.PRE[0], SC.STATIC_WINDOW, shift, SC.STRIDE, (nxg,) + SC.CROSS, offered)
    assert ids == [(0, PC.new_id(5007, 0, sign, SC.STRIDE)), (1, PC.new_id(5011, 2, sign, SC.STRIDE))] and rejected == 1
    collide = (1, PC.new_id(5015, 0, sign, SC.STRIDE))
    assert collide in offered and collide not in ids and residents[2][:2] == collide
    y14 = PC.by_id(pre)[(1, 5014)]["position"][:, 1]
    assert y14.max() + shift[1] > SC.CROSS[0] - 1
    # ... and only the far rank holds that resident; the others live on the inlet rank alone
    assert SC.holders(residents[2], world) == [SC.far_rank(direction, world)]
    assert SC.holders(residents[0], world) == SC.holders(residents[1], world) == [SC.inlet_rank(direction, world)]
    # the arrivals lie in the inlet rank's slab, off its envelope, and the window respects the margin
    assert SC.margin_ok(direction, world, SC.STATIC_WINDOW, shift)
    x0, x1 = SC.slab_of(SC.inlet_rank(direction, world), world)
    for key in ids:
        p = PC.by_id(out)[key]["position"][:, 0]
        assert x0 + (SC.E_SHARE if sign > 0 else 0) <= p.min() and p.max() <= x1 - (SC.E_SHARE if sign < 0 else 0)
    # the 70 further PLTs all lie in the window and arrive
    more = SC.box_records(SC.static_more_cells())
    out2, ids2, rejected2 = PC.inject(more, out, NV, 0, sign, SC.PRE[0], SC.STATIC_WINDOW, shift, SC.STRIDE, (nxg,) + SC.CROSS, offered)
    assert ids2 == [(1, PC.new_id(5300 + k, 0, sign, SC.STRIDE)) for k in range(70)] and rejected2 == 0
    assert 70 > 64 + 2 // 4   # more than the slots the inlet rank's PLT region was allocated with for its one resident


def test_refused_window_is_within_the_envelope():
    for direction, world in CASES:
        shift = list(SC.static_shift(direction, world))
        x0, x1 = SC.slab_of(SC.inlet_rank(direction, world), world)
        # moved until it ends one plane inside the envelope of the inner face
        shift[0] = (x1 - SC.E_SHARE + 1.0 - SC.STATIC_WINDOW[1]) if SC.SIGN[direction] < 0 else (x0 + SC.E_SHARE - 1.0 - SC.STATIC_WINDOW[0])
        a, b = SC.image(SC.STATIC_WINDOW, shift)
        assert x0 <= a and b <= x1 and not SC.margin_ok(direction, world, SC.STATIC_WINDOW, shift)


@pytest.mark.parametrize("world", [2, 3])
def test_coupled_scene(world):
    shift = SC.coupled_shift(world)
    assert SC.margin_ok("Xneg", world, SC.COUPLED_WINDOW, shift)
    _, face = SC.slab_of(0, world)
    assert SC.image(SC.COUPLED_WINDOW, shift)[1] == face - SC.E_SHARE          # as close to the face as create allows
    pre = SC.box_records(SC.coupled_pre_cells())
    assert PC.select(pre, NV, 0, SC.PRE[0], SC.COUPLED_WINDOW) == []               # not yet: the trailing vertex is upstream of the window
    x = pre["position"][:, 0]
    assert abs(x.min() - (SC.COUPLED_WINDOW[0] - 0.3)) < 1e-12 and x.max() < SC.COUPLED_WINDOW[1]
    moved = pre.copy(); moved["position"][:, 0] += 0.3
    assert [(t, i) for t, i, _, _ in PC.select(moved, NV, 0, SC.PRE[0], SC.COUPLED_WINDOW)] == [(1, 5040)]
    assert SC.holders(SC.coupled_residents(world)[0], world) == [1]


def test_sink_and_stale_scenes():
    face = SC.slab_of(0, 2)[1]
    assert SC.SINK_PLANE == face + 2
    # 3: the PLT starts two planes upstream of the plane, on both ranks, and still straddles the face when its leading vertex
    # reaches the plane: vertices on both sides of x = face - 0.5, where the nearest node changes rank
    a, b = SC.sink_residents()
    rec = SC.box_records([a])
    assert abs(rec["position"][:, 0].max() - (SC.SINK_PLANE - 2.0)) < 1e-12 and SC.holders(a, 2) == [0, 1] and SC.holders(b, 2) == [0]
    assert PC.sink(SC.box_records([a, b]), 0, -1, SC.SINK_PLANE)[1] == []
    rec["position"][:, 0] += 2.0 + 1e-9
    x = rec["position"][:, 0]
    assert x.min() < face - 0.5 < x.max() and PC.sink(rec, 0, -1, SC.SINK_PLANE)[1] == [(1, 5)]
    idle = SC.box_records(SC.sink_pre_cells())
    assert PC.select(idle, NV, 0, SC.PRE[0], SC.STALE_WINDOW) == [] and idle["position"][:, 0].min() + 150 * 0.03 < SC.STALE_WINDOW[0]
    # 4: the first check takes PLT 5 (past the plane, rank 1's, a pure copy on rank 0) and brings PLT 5040: rank 0 holds two PLTs
    # before and after, and PLT 6, across the face and short of the plane even 0.5 planes further on, moves into the slot of 5
    res = SC.stale_residents()
    assert SC.holders(res[0], 2) == [0, 1] and SC.owners(res[0], 2) == [1] and SC.holders(res[1], 2) == SC.owners(res[1], 2) == [0, 1]
    x6 = SC.box_records([res[1]])["position"][:, 0]
    assert x6.max() + 0.5 < SC.SINK_PLANE and x6.max() >= face - SC.E_SHARE
    kept, gone = PC.sink(SC.box_records(res), 0, -1, SC.SINK_PLANE)
    assert gone == [(1, 5)]
    out, ids, rejected = PC.inject(SC.box_records(SC.stale_pre_cells()), kept, NV, 0, -1, SC.PRE[0], SC.STALE_WINDOW, SC.STALE_SHIFT, SC.STRIDE,
                                   (96,) + SC.CROSS, set())
    assert ids == [(1, 6040)] and rejected == 0
    assert sorted(set(out["cellId"])) == [6, 6040] and len(set(kept["cellId"])) + 1 == len(res)
    assert SC.margin_ok("Xneg", 2, SC.STALE_WINDOW, SC.STALE_SHIFT)
