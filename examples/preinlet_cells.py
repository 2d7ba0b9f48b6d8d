"""python examples/preinlet_cells.py [--iterations 2000] [--cells-every 20] [--repeat 7]

A periodic, driven pre-inlet channel with a few cells feeds a walled domain channel (host.PreInlet(device=True, cells=...),
direction Xneg): the fluid through the domain's velocity inlet, the cells by injection of whole cells found in the
pre-inlet's window, and a sink in front of the domain's pressure outlet takes them out again.  Prints one JSON line: the cell
counts of the run, its wall time per iteration, and the wall time of one hcp_preinlet_apply (one check) with zero candidates
and with one candidate that is injected -- each the median of --repeat calls on an idle stream, timed with a host clock from
the call to the end of a wait for the stream."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from hemocell_amd import capi, host   # noqa: E402

PRE, DOM = (48, 34, 34), (96, 34, 34)
WINDOW, SHIFT, STRIDE, SINK = (6.0, 44.0), (-4.0, 0.0, 0.0), 100000, 88.0
U0 = 0.03


def channel_mask(dims):
    m = np.zeros(dims, np.uint8)
    m[:, 0, :] = m[:, -1, :] = m[:, :, 0] = m[:, :, -1] = 1
    return m


def time_check(lib, pc, dc, window, repeat, expect):
    """median wall time [us] of one hcp_preinlet_apply that injects `expect` cells (a fresh handle each time, whose blocks
    hcp_preinlet_create allocated; what arrived is taken out of the domain again)"""
    sh = np.array(SHIFT)
    times = []
    for _ in range(repeat + 1):   # the first call brings the containers to the device and sizes the staging: not counted
        X = C.c_void_p()
        host.check(lib.hcp_preinlet_create(C.byref(X), pc.ptr, dc.ptr, 0, -1, window[0], window[1], host.dptr(sh), STRIDE))
        host.check(lib.hc_synchronize())
        n_inj, n_rem = C.c_long(), C.c_long()
        t0 = time.perf_counter()
        host.check(lib.hcp_preinlet_apply(X, C.byref(n_inj), C.byref(n_rem)))
        host.check(lib.hc_synchronize())
        times.append((time.perf_counter() - t0) * 1e6)
        assert (n_inj.value, n_rem.value) == (expect, 0), (n_inj.value, n_rem.value)
        host.check(lib.hcp_preinlet_destroy(X))
        if expect:   # the arrivals are the last cells of their type
            n = dc.type_range(1)[1]
            slots = np.arange(n - expect, n, dtype=np.int32)
            host.check(lib.hcp_remove_cells(dc.ptr, 1, slots.ctypes.data_as(C.POINTER(C.c_int)), expect))
    times = times[1:]
    return statistics.median(times), max(times) - min(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=2000)
    ap.add_argument("--cells-every", type=int, default=20)
    ap.add_argument("--repeat", type=int, default=7)
    a = ap.parse_args()

    host.init(0)
    lib = capi.lib()
    P = host.base_parameters()
    omega = 1.0 / P.tau
    pre = host.Lattice(*PRE, (True, False, False), omega)
    dom = host.Lattice(*DOM, (False, False, False), omega)
    pmask, dmask = channel_mask(PRE), channel_mask(DOM)
    area = int((pmask[0] == 0).sum())
    # the force that sustains a mean velocity of about U0 / 2 in the pre-inlet (preinlet_driving_force scaled by the Reynolds number)
    radius = np.sqrt(area / np.pi)
    _, _, F = host.preinlet_driving_force_vector(U0 * 2 * radius / P.nu_lbm, P.nu_lbm, area, "Xneg")
    pre.defineBounceBack(pmask); pre.setExternalVector(F); pre.latticeEquilibrium(1.0, (U0, 0.0, 0.0))
    dom.defineBounceBack(dmask); dom.latticeEquilibrium(1.0, (U0, 0.0, 0.0))
    types = [host.CellType.rbc(P), host.CellType.plt(P)]
    pc, dc = host.Cells(pre, P), host.Cells(dom, P)
    for t in types:
        pc.addCellType(t, 1); dc.addCellType(t, 1)
    # the pre-inlet's cells: one PLT in the window already, the others upstream of it
    assert pc.addCell(1, (12.0, 16.5, 16.5), (10.0, 20.0, 30.0), cell_id=0)
    assert pc.addCell(1, (2.0, 11.0, 22.0), (40.0, 0.0, 10.0), cell_id=1)
    assert pc.addCell(1, (1.5, 22.0, 11.0), (0.0, 30.0, 60.0), cell_id=2)
    assert pc.addCell(0, (-4.0, 16.5, 16.5), (90.0, 0.0, 0.0), cell_id=3)   # across the periodic seam, lap -1
    assert dc.addCell(0, (60.0, 16.5, 16.5), (90.0, 0.0, 0.0), cell_id=50)
    for c in (pc, dc):
        c.applyConstitutiveModel(0, True)

    zero_us, zero_spread = time_check(lib, pc, dc, (20.0, 40.0), a.repeat, 0)   # no cell lies in this window
    one_us, one_spread = time_check(lib, pc, dc, WINDOW, a.repeat, 1)

    g = np.stack(np.nonzero(pmask[0] == 0), axis=1)
    coupling = host.PreInlet(pre, dom, g, PRE[0] - 1, 0, direction="Xneg", device=True, cells=(pc, dc), window=WINDOW,
                             shift=SHIFT, id_stride=STRIDE, sink=SINK, cells_every=a.cells_every)
    dom.setOpenBoundaryVelocitySlots(coupling.first, np.tile((U0, 0.0, 0.0), (len(g), 1)))
    dom.addPressureBoundary0P((DOM[0] - 1, DOM[0] - 1, 0, DOM[1] - 1, 0, DOM[2] - 1))
    coupling.iterate(a.cells_every)   # warm-up: the first check allocates
    host.check(lib.hc_synchronize())
    t0 = time.perf_counter()
    coupling.iterate(a.iterations)
    host.check(lib.hc_synchronize())
    per_iteration = (time.perf_counter() - t0) / a.iterations * 1e6
    injected, rejected, removed, checks = coupling.cell_counts()
    assert np.isfinite(dc.positions).all() and np.isfinite(dom.populations()).all()
    print(json.dumps({"example": "preinlet_cells", "pre": PRE, "domain": DOM, "iterations": a.iterations,
                      "cells_every": a.cells_every, "injected": injected, "rejected": rejected, "removed_by_sink": removed,
                      "checks": checks, "cells_in_preinlet": pc.counts()[1], "cells_in_domain": dc.counts()[1],
                      "domain_cell_ids": [int(i) for i in dc.cell_ids()], "us_per_iteration": round(per_iteration, 2),
                      "check_us_zero_candidates": round(zero_us, 2), "check_us_zero_candidates_spread": round(zero_spread, 2),
                      "check_us_one_candidate": round(one_us, 2), "check_us_one_candidate_spread": round(one_spread, 2),
                      "build_tag": lib.hc_build_tag().decode()}))
    coupling.destroy()
    pc.destroy(); dc.destroy(); pre.destroy(); dom.destroy()
    for t in types:
        t.destroy()


if __name__ == "__main__":
    main()
