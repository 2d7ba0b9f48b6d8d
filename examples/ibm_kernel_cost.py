"""What the three- and four-point IBM kernels cost on the benchmark's workload: the pipe of bench.py (default 256^3, 10 %
haematocrit, velocity update every 5, material model every 20) through the Python host, in one process, with the red cells on
HC_IBM_PHI2, HC_IBM_PHI3, HC_IBM_PHI4 and HC_IBM_PHI2 again (the spread between the two runs on two points is the noise).

Prints one JSON line.  Per width: the spread (hcp_spread) and the interpolation (hcp_interpolate) alone, launch after launch on
the state that `warmup` iterations left, from hipEvent pairs around every launch (hc_profile_read), after a first round that
warms both up; and the whole iteration from a host clock around hc_iterate + synchronise with the event pairs off.  A vertex
has 8, 27 or 64 stencil nodes, so the LDS adds and the blend grow 3.4 and 8 times; the node velocities of the interpolation and
the global atomics of the spread grow with the distinct nodes of a cell, about 1.6 and 2.1 times.  DESIGN.md section 7 quotes it.

    python examples/ibm_kernel_cost.py [--n 256] [--steps 100] [--warmup 20] [--kernel-launches 50]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from hemocell_amd import host  # noqa: E402
from hemocell_amd.packing import pack_pipe_rbc  # noqa: E402


def per_launch(name):
    ms, n = C.c_double(), C.c_long()
    host.check(host.capi.lib().hc_profile_read(name.encode(), C.byref(ms), C.byref(n)))
    return (ms.value / n.value if n.value else None), n.value


def run(n, steps, warmup, kernel_launches, kernel):
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
        cf.setIbmKernel(0, kernel)
        centres, angles = pack_pipe_rbc(n, n, n, 0.10)
        cells = sum(bool(cf.addCell(0, c, a, 0.0, cell_id=i)) for i, (c, a) in enumerate(zip(centres, angles)))
        cf.applyConstitutiveModel(0, True)
        h.iterate(warmup)
        h.synchronize()
        t0 = time.perf_counter()
        h.iterate(steps)
        h.synchronize()
        out = dict(kernel=kernel, cells=cells, iteration_ms=(time.perf_counter() - t0) * 1e3 / steps)
        # the two phases alone: event pairs around every launch; the spread adds into one force buffer again and again, which
        # costs what a first spread costs (the atomics do not depend on the values)
        host.check(lib.hc_profile_enable(1))
        for k in range(2):   # the first round warms both up
            host.check(lib.hc_profile_reset())
            for _ in range(kernel_launches):
                cf.spreadParticleForce(True)
            for _ in range(kernel_launches):
                cf.interpolateFluidVelocity()
            h.synchronize()
        spread_ms, ns = per_launch("ibm_spread")
        interp_ms, ni = per_launch("ibm_interpolate")
        host.check(lib.hc_profile_enable(0))
        out.update(spread_ms_per_call=spread_ms, spread_calls=ns, interpolate_ms_per_call=interp_ms, interpolate_calls=ni)
        return out
    finally:
        L.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--kernel-launches", type=int, default=50)
    a = ap.parse_args()
    host.init(0)
    runs = [run(a.n, a.steps, a.warmup, a.kernel_launches, k) for k in (host.IBM_PHI2, host.IBM_PHI3, host.IBM_PHI4, host.IBM_PHI2)]
    base = runs[0]
    for r in runs[1:]:
        r["spread_over_phi2"] = r["spread_ms_per_call"] / base["spread_ms_per_call"]
        r["interpolate_over_phi2"] = r["interpolate_ms_per_call"] / base["interpolate_ms_per_call"]
        r["iteration_over_phi2"] = r["iteration_ms"] / base["iteration_ms"]
    print(json.dumps(dict(n=a.n, steps=a.steps, phi2=runs[0], phi3=runs[1], phi4=runs[2], phi2_again=runs[3],
                          build=host.capi.lib().hc_build_tag().decode())))


if __name__ == "__main__":
    main()
