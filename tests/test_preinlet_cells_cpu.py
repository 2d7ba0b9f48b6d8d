"""The pre-inlet's cells without a GPU: the new entry points are declared and bound, the restatement's lap, window and id
arithmetic on hand-made records, and host.PreInlet without cells= is the object it was."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import preinlet_cells_ref as PC
from hemocell_amd import capi, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hcp_preinlet_create", "hcp_preinlet_set_sink", "hcp_preinlet_apply", "hcp_preinlet_counts", "hcp_preinlet_destroy",
       "hc_preinlet_iterate")
SV = host.Cells.SV_DTYPE


@pytest.fixture(autouse=True)
def _entry_points():
    """the restatement restates entry points: it is only worth something next to them"""
    missing = [n for n in NEW if n not in capi.SIGNATURES]
    assert not missing, "not bound in capi.SIGNATURES: %s" % missing


def test_new_symbols_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "hemocell_amd.h")).read()
    assert "typedef struct hc_preinlet_cells hc_preinlet_cells;" in header
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in capi.SIGNATURES, name
        assert capi.SIGNATURES[name][0] is C.c_int
    assert len(capi.SIGNATURES["hcp_preinlet_create"][1]) == 9
    assert capi.SIGNATURES["hcp_preinlet_create"][1][5:7] == [C.c_double, C.c_double]
    assert len(capi.SIGNATURES["hc_preinlet_iterate"][1]) == 8
    assert len(capi.SIGNATURES["hcp_preinlet_apply"][1]) == 3
    # the fluid entry points keep their signatures
    assert capi.SIGNATURES["hcl_preinlet_iterate"] == (C.c_int, [capi.VP, C.c_int])
    for name in ("applyPreInletCells", "cell_counts"):
        assert callable(getattr(host.PreInlet, name))


def _cell(celltype, cell_id, xs, y=5.0, z=6.0, order=None):
    """records of one cell with the given x coordinates"""
    rec = np.zeros(len(xs), dtype=SV)
    rec["position"][:, 0] = xs
    rec["position"][:, 1] = y + 0.25 * np.arange(len(xs))
    rec["position"][:, 2] = z - 0.125 * np.arange(len(xs))
    rec["v"] = 0.001 * (1 + np.arange(3 * len(xs)).reshape(-1, 3))
    rec["force"] = -0.002 * (1 + np.arange(3 * len(xs)).reshape(-1, 3))
    rec["cellId"], rec["celltype"] = cell_id, celltype
    rec["vertexId"] = np.arange(len(xs))
    return rec if order is None else rec[list(order)]


LP, WINDOW, STRIDE = 40, (10.0, 30.0), 1000


@pytest.mark.parametrize("lap", [0, 2, -1])
def test_lap_window_and_id(lap):
    xs = np.array([12.5, 14.0, 13.25, 17.75]) + lap * LP
    got_lap, inside = PC.lap_and_window(xs.min(), xs.max(), LP, WINDOW)
    assert (got_lap, inside) == (lap, True)
    assert PC.new_id(7, lap, -1, STRIDE) == 7 + (lap + 1) * STRIDE    # *neg: the offset of lap 0 is positive
    assert PC.new_id(5007, lap, 1, STRIDE) == 5007 + (lap - 1) * STRIDE
    t = PC.translation(lap, 0, LP, (-8.0, 1.5, -2.0))
    assert t == [np.float64(-8.0) - np.float64(lap) * np.float64(LP), 1.5, -2.0]
    t = PC.translation(lap, 2, LP, (-8.0, 1.5, -2.0))
    assert t == [-8.0, 1.5, np.float64(-2.0) - np.float64(lap) * np.float64(LP)]


def test_window_edges_and_lap_boundary():
    # touching window_hi exactly is inside; one ulp beyond is not
    assert PC.lap_and_window(12.0, 30.0, LP, WINDOW) == (0, True)
    assert PC.lap_and_window(12.0, np.nextafter(30.0, 31.0), LP, WINDOW) == (0, False)
    assert PC.lap_and_window(10.0, 20.0, LP, WINDOW) == (0, True)
    assert PC.lap_and_window(np.nextafter(10.0, 9.0), 20.0, LP, WINDOW) == (0, False)
    assert PC.lap_and_window(12.0 + 3 * LP, 30.0 + 3 * LP, LP, WINDOW) == (3, True)
    # a cell straddling the lap boundary belongs to the lap of its lowest vertex and cannot lie in a window inside [0, Lp]
    assert PC.lap_and_window(38.0, 42.0, LP, (0.0, 40.0)) == (0, False)
    assert PC.lap_and_window(-2.0, 3.0, LP, (0.0, 40.0)) == (-1, False)
    assert PC.lap_and_window(78.5, 81.0, LP, (0.0, 40.0)) == (1, False)
    # ... while one that ends on the boundary is whole in its lap
    assert PC.lap_and_window(36.0, 40.0, LP, (0.0, 40.0)) == (0, True)
    assert PC.lap_and_window(40.0, 44.0, LP, (0.0, 40.0)) == (1, True)


def test_injection_and_sink_on_records():
    nv = {0: 4, 1: 3}
    pre = np.concatenate([
        _cell(1, 21, [15.0, 16.0, 17.0]),                         # in the window, lap 0
        _cell(0, 11, np.array([12.0, 13.0, 14.0, 15.0]) + 2 * LP, order=(2, 0, 3, 1)),   # lap 2, records shuffled
        _cell(1, 22, [28.0, 29.0, 31.0]),                         # straddles window_hi
        _cell(1, 23, [3.0, 4.0, 5.0]),                            # outside
        _cell(1, 24, [20.0, 21.0, 22.0], y=31.0),                 # in the window, leaves the domain in y
        _cell(1, 25, [20.0, 21.0]),                               # incomplete
        _cell(1, 26, [18.0, 19.0, 20.0]),                         # the domain holds its new id
    ])
    dom = np.concatenate([_cell(0, 11, [30.0, 31.0, 32.0, 33.0]), _cell(1, 1026, [40.0, 41.0, 42.0])])
    shift, dims = (-8.0, 2.0, 0.0), (48, 34, 34)
    cand = PC.select(pre, nv, 0, LP, WINDOW)
    assert [(t, i, lap) for t, i, _, lap in cand] == [(0, 11, 2), (1, 21, 0), (1, 24, 0), (1, 26, 0)]   # ascending (type, slot)
    assert list(pre["vertexId"][cand[0][2]]) == [0, 1, 2, 3]
    offered = set()
    out, ids, rejected = PC.inject(pre, dom, nv, 0, -1, LP, WINDOW, shift, STRIDE, dims, offered)
    assert ids == [(0, 11 + 3 * STRIDE), (1, 21 + STRIDE)] and rejected == 1
    assert offered == {(0, 3011), (1, 1021), (1, 1024), (1, 1026)}
    assert np.array_equal(out[:len(dom)], dom) and len(out) == len(dom) + 7
    a = out[out["cellId"] == 3011]
    src = _cell(0, 11, np.array([12.0, 13.0, 14.0, 15.0]) + 2 * LP)
    assert np.array_equal(a["position"][:, 0], src["position"][:, 0] + (np.float64(-8.0) - np.float64(2.0) * np.float64(LP)))
    assert np.array_equal(a["position"][:, 1], src["position"][:, 1] + 2.0)
    assert np.array_equal(a["position"][:, 2], src["position"][:, 2] + 0.0)
    assert np.array_equal(a["v"], src["v"]) and np.array_equal(a["force"], src["force"])
    assert set(a["celltype"]) == {0} and list(a["vertexId"]) == [0, 1, 2, 3]
    # a second check offers nothing new
    again, ids2, rejected2 = PC.inject(pre, out, nv, 0, -1, LP, WINDOW, shift, STRIDE, dims, offered)
    assert ids2 == [] and rejected2 == 0 and again is out
    # the sink
    kept, gone = PC.sink(out, 0, -1, 41.5)
    assert gone == [(1, 1026)] and len(kept) == len(out) - 3 and 1026 not in kept["cellId"]
    kept, gone = PC.sink(out, 0, 1, 6.5)
    assert gone == [(0, 3011)]   # 12 + 80 - 8 - 80 = 4 < 6.5
    kept, gone = PC.sink(out, 0, -1, 100.0)
    assert gone == [] and np.array_equal(kept, out)


class _FakeLattice:
    def __init__(self, nx, ny, nz):
        self.nx, self.ny, self.nz, self.ptr, self.declared = nx, ny, nz, None, None

    def addOpenBoundaryNodes(self, kind, orientation, nodes, axis=0):
        self.declared = (kind, orientation, np.array(nodes), axis)
        return 17


def test_preinlet_without_cells_is_the_object_it_was():
    pre, dom = _FakeLattice(10, 12, 12), _FakeLattice(20, 16, 16)
    p = host.PreInlet(pre, dom, [[3, 4], [5, 6]], 9, 0, direction="Xneg", pre_origin=(2, 2))
    assert set(vars(p)) == {"pre", "domain", "axis", "device", "ptr", "pre_yz", "pre_x", "domain_x", "domain_nodes", "first"}
    assert (p.axis, p.device, p.ptr, p.pre_x, p.domain_x, p.first) == (0, False, None, 9, 0, 17)
    assert np.array_equal(p.pre_yz, [1 * 12 + 2, 3 * 12 + 4]) and p.pre_yz.dtype == np.int32
    assert np.array_equal(p.domain_nodes, [[0, 3, 4], [0, 5, 6]])
    assert dom.declared[0] == 0 and dom.declared[1] == -1 and dom.declared[3] == 0
    p.destroy()   # nothing to free
    for call in (p.applyPreInletCells, p.cell_counts):
        with pytest.raises(host.HcError, match="no cell coupling"):
            call()
    # cells cross on the device only; refused before anything is declared on the domain
    dom2 = _FakeLattice(20, 16, 16)
    with pytest.raises(host.HcError, match="cells= needs device=True"):
        host.PreInlet(pre, dom2, [[3, 4]], 9, 0, direction="Xneg", pre_origin=(2, 2), cells=(object(), object()),
                      window=(1.0, 5.0), id_stride=10)
    with pytest.raises(host.HcError, match="window="):
        host.PreInlet(pre, dom2, [[3, 4]], 9, 0, direction="Xneg", pre_origin=(2, 2), device=True, cells=(object(), object()))
    with pytest.raises(host.HcError, match="cells_every"):
        host.PreInlet(pre, dom2, [[3, 4]], 9, 0, direction="Xneg", pre_origin=(2, 2), device=True, cells=(object(), object()),
                      window=(1.0, 5.0), id_stride=10, cells_every=0)
    assert dom2.declared is None
