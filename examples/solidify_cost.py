"""What the solidify check costs on the benchmark's workload: the pipe of bench.py (default 256^3, 10 % haematocrit, velocity
update every 5, material model every 20) with a ring of platelets next to the wall, through the Python host, in one process.

Prints one JSON line.  Per iteration, from a host clock around hc_iterate + synchronise with the event pairs off: the whole
iteration with the feature off, with the check every iteration, with the check every 5 iterations, and with it off again.
With the feature on the wall is the binding box and the platelets carry the thresholds of the reference's PLT.xml (1.5 lattice
units, 100), so platelets that get flagged do solidify; the counts are printed.  Per launch, from hipEvent pairs
(hc_profile_read) in a second, shorter run of each setting: the prepare and the flag pass.  DESIGN.md section 7 quotes it.

    python examples/solidify_cost.py [--n 256] [--steps 200] [--warmup 20] [--tree DIR] [--off-only]

--tree DIR: import hemocell_amd from another checkout (the same run on the parent commit: use it with --off-only).
"""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time


def per_launch(host, name):
    ms, n = C.c_double(), C.c_long()
    host.check(host.capi.lib().hc_profile_read(name.encode(), C.byref(ms), C.byref(n)))
    return (ms.value / n.value if n.value else None), n.value


def run(host, pack_pipe_rbc, n, steps, warmup, every):
    """every: 0 = the feature off"""
    lib = host.capi.lib()
    P = host.base_parameters()
    L = host.Lattice(n, n, n, (True, False, False), 1.0 / P.tau)
    try:
        mask, R = host.pipe_mask(n, n, n)
        L.defineBounceBack(mask)
        L.latticeEquilibrium(1.0, (0.0, 0.0, 0.0))
        u_max = 0.5 * P.nu_lbm / (2 * R)   # poiseuilleForce of examples/pipeflow/pipeflow.cpp:80 at Re = 0.5, as bench.py
        L.setExternalVector((8.0 * P.nu_lbm * (u_max * 0.5) / (R * R), 0.0, 0.0))
        h = host.HemoCell(L, P)
        h.setParticleVelocityUpdateTimeScaleSeparation(5)
        cf = h.cellfields
        cf.addCellType(host.CellType.rbc(P), 20)
        cf.addCellType(host.CellType.plt(P, solidify=(1.5, 100.0)) if every else host.CellType.plt(P), 20)
        centres, angles = pack_pipe_rbc(n, n, n, 0.10)
        cells = sum(bool(cf.addCell(0, c, a, 0.0, cell_id=i)) for i, (c, a) in enumerate(zip(centres, angles)))
        # platelets lying against the wall: rings of 24 every 8 planes, their flat side towards it, 4 nodes inside the radius
        platelets, c0 = 0, (n - 1) / 2.0
        for x in range(4, n - 4, 8):
            for k in range(24):
                a = 2.0 * math.pi * k / 24.0
                pos = (float(x), c0 + (R - 4.0) * math.cos(a), c0 + (R - 4.0) * math.sin(a))
                platelets += bool(cf.addCell(1, pos, (90.0 - math.degrees(a), 0.0, 0.0), 0.0, cell_id=10 ** 6 + platelets))
        if every:
            L.populateBindingSites((0, n - 1, 0, n - 1, 0, n - 1))
            cf.setSolidifyTimeScaleSeparation(every)
        cf.applyConstitutiveModel(0, True)
        h.iterate(warmup)
        h.synchronize()
        t0 = time.perf_counter()
        h.iterate(steps)
        h.synchronize()
        out = dict(rbc=cells, platelets=platelets, every=every, iteration_ms=(time.perf_counter() - t0) * 1e3 / steps)
        if every:
            host.check(lib.hc_profile_enable(1))
            host.check(lib.hc_profile_reset())
            h.iterate(5 * every)
            h.synchronize()
            out["prepare_ms_per_check"], out["checks"] = per_launch(host, "solidify_prepare")
            out["flag_ms_per_check"], _ = per_launch(host, "solidify_flag")
            host.check(lib.hc_profile_enable(0))
            out["solidified_cells"], out["solidified_nodes"], out["flagged_vertices"] = cf.solidify_counts()
        return out
    finally:
        L.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--off-only", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, a.tree)
    from hemocell_amd import host
    from hemocell_amd.packing import pack_pipe_rbc
    host.init(0)
    settings = (0, 0) if a.off_only else (0, 1, 5, 0)
    runs = [run(host, pack_pipe_rbc, a.n, a.steps, a.warmup, every) for every in settings]
    print(json.dumps(dict(n=a.n, steps=a.steps, runs=runs, build=host.capi.lib().hc_build_tag().decode())))


if __name__ == "__main__":
    main()
