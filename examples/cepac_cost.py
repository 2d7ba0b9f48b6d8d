"""What the CEPAC scalar field costs on the benchmark's workload: the pipe of bench.py (default 256^3, 10 % haematocrit,
velocity update every 5, material model every 20) through the Python host, in one process.

Prints one JSON line.  Per kernel, from hipEvent pairs around every launch (hc_profile_read), on the lattice with its cells
bound: the flow's collide alone (hcl_collide_stream, nothing beside it) and the scalar step alone (hcl_scalar_step), launch
after launch, and their ratio -- by bytes the step moves 19 + 19 + 19 populations, a mask and a class byte, about 458 B per
node (the force record comes on top where cells spread) against the collide's 353 B, a ratio of 1.30.  Per iteration, from a
host clock around hc_iterate + synchronise with the event pairs off: the whole iteration without the field, with it, and
without it again.  DESIGN.md section 7 quotes it.

    python examples/cepac_cost.py [--n 256] [--steps 200] [--warmup 20] [--kernel-launches 100]
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

SCALAR_BYTES_PER_NODE = 19 * 8 * 3 + 2   # flow populations read, scalar populations read and written, mask and class byte


def per_launch(name):
    ms, n = C.c_double(), C.c_long()
    host.check(host.capi.lib().hc_profile_read(name.encode(), C.byref(ms), C.byref(n)))
    return (ms.value / n.value if n.value else None), n.value


def run(n, steps, warmup, kernel_launches, field):
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
        centres, angles = pack_pipe_rbc(n, n, n, 0.10)
        cells = sum(bool(cf.addCell(0, c, a, 0.0, cell_id=i)) for i, (c, a) in enumerate(zip(centres, angles)))
        S = None
        if field:
            S = L.createCEPACfield(0.8)
            S.initializeAtEquilibrium(1.0)
            S.addSource((n // 2 - 2, n // 2 + 2, n // 2 - 2, n // 2 + 2, n // 2 - 2, n // 2 + 2), 2.0)
        cf.applyConstitutiveModel(0, True)
        h.iterate(warmup)
        h.synchronize()
        t0 = time.perf_counter()
        h.iterate(steps)
        h.synchronize()
        out = dict(cells=cells, iteration_ms=(time.perf_counter() - t0) * 1e3 / steps, active_nodes=None)
        if field:
            # the two kernels alone, on the state the iterations left (its IBM force included): event pairs around every launch
            host.check(lib.hc_profile_enable(1))
            for k in range(2):   # the first round warms both up
                host.check(lib.hc_profile_reset())
                L.collideAndStream(kernel_launches)
                for _ in range(kernel_launches):
                    S.collideAndStream()
                h.synchronize()
            collide_ms, nc = per_launch("collide_stream")
            scalar_ms, ns = per_launch("scalar_step")
            host.check(lib.hc_profile_enable(0))
            counts = (C.c_long * 3)()
            host.check(lib.hcl_node_counts(L.ptr, counts))
            total, lo, hi = S.stats()
            out.update(collide_ms_per_launch=collide_ms, collide_launches=nc, scalar_ms_per_launch=scalar_ms, scalar_launches=ns,
                       scalar_over_collide=scalar_ms / collide_ms, active_nodes=counts[2],
                       collide_bytes_per_node=L.bytes_per_node(), scalar_bytes_per_node=SCALAR_BYTES_PER_NODE,
                       collide_TBps=L.bytes_per_node() * counts[2] / (collide_ms * 1e-3) / 1e12,
                       scalar_TBps=SCALAR_BYTES_PER_NODE * counts[2] / (scalar_ms * 1e-3) / 1e12,
                       C_sum=total, C_min=lo, C_max=hi)
        return out
    finally:
        L.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--kernel-launches", type=int, default=100)
    a = ap.parse_args()
    host.init(0)
    runs = [run(a.n, a.steps, a.warmup, a.kernel_launches, field) for field in (False, True, False)]
    print(json.dumps(dict(n=a.n, steps=a.steps, without=runs[0], with_field=runs[1], without_again=runs[2],
                          build=host.capi.lib().hc_build_tag().decode())))


if __name__ == "__main__":
    main()
