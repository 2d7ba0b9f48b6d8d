"""What the running statistics cost on the benchmark's workload: the pipe of bench.py (default 256^3, 10 % haematocrit,
velocity update every 5, material model every 20) through the Python host, in one process.

Prints one JSON line.  Per kernel, from hipEvent pairs around every launch (hc_profile_read), on the state the iterations left:
the flow's collide alone (hcl_collide_stream), one fluid sample with all three fluid sets (stats_fluid_kernel), one
cell-density sample and one inside sample (hc_stats_sample, launch after launch).  By bytes a fluid sample reads 19 populations,
the mask-free force record (3 doubles) and reads and writes 16 fp64 accumulators per node: 19 * 8 + 24 + 2 * 16 * 8 = 432 B
against the collide's 353 B, a ratio of 1.22.  Per iteration, from a host clock around hc_iterate + synchronise with the event
pairs off: without a handle, with all five sets at every = 10, 100 and 1000, and without a handle again.  DESIGN.md section 7
quotes it.

    python examples/statistics_cost.py [--n 256] [--steps 1000] [--warmup 20] [--kernel-launches 50]
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

FLUID_SAMPLE_BYTES_PER_NODE = 19 * 8 + 3 * 8 + 2 * 16 * 8   # populations, force record, 16 accumulators read and written


def per_launch(name):
    ms, n = C.c_double(), C.c_long()
    host.check(host.capi.lib().hc_profile_read(name.encode(), C.byref(ms), C.byref(n)))
    return (ms.value / n.value if n.value else None), n.value


def build(n):
    P = host.base_parameters()
    L = host.Lattice(n, n, n, (True, False, False), 1.0 / P.tau)
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
    cf.applyConstitutiveModel(0, True)
    return L, h, cells


def timed(h, steps):
    h.synchronize()
    t0 = time.perf_counter()
    h.iterate(steps)
    h.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--kernel-launches", type=int, default=50)
    a = ap.parse_args()
    host.init(0)
    lib = host.capi.lib()
    L, h, cells = build(a.n)
    st = None
    try:
        h.iterate(a.warmup)
        out = dict(n=a.n, steps=a.steps, cells=cells, iteration_ms={})
        out["iteration_ms"]["no_handle"] = timed(h, a.steps)
        st = host.Statistics(L, h.cellfields, what=31)
        for every in (10, 100, 1000):
            st.setEvery(every)
            st.reset()
            out["iteration_ms"]["every_%d" % every] = timed(h, a.steps)
            out["samples_every_%d" % every] = st.samples
        st.setEvery(0)
        # the kernels alone, on the state the iterations left: event pairs around every launch; the first round warms them up
        host.check(lib.hc_profile_enable(1))
        for _ in range(2):
            host.check(lib.hc_profile_reset())
            L.collideAndStream(a.kernel_launches)
            for _ in range(a.kernel_launches):
                st.sample()
            h.synchronize()
        kernels = {}
        for name in ("collide_stream", "stats_fluid", "stats_cell_density", "stats_inside"):
            ms, n = per_launch(name)
            kernels[name] = dict(ms_per_launch=ms, launches=n)
        host.check(lib.hc_profile_enable(0))
        counts = (C.c_long * 3)()
        host.check(lib.hcl_node_counts(L.ptr, counts))
        nodes = counts[0]
        out.update(kernels=kernels, nodes=nodes, active_nodes=counts[2], collide_bytes_per_node=L.bytes_per_node(),
                   fluid_sample_bytes_per_node=FLUID_SAMPLE_BYTES_PER_NODE,
                   fluid_sample_over_collide=kernels["stats_fluid"]["ms_per_launch"] / kernels["collide_stream"]["ms_per_launch"],
                   collide_TBps=L.bytes_per_node() * counts[2] / (kernels["collide_stream"]["ms_per_launch"] * 1e-3) / 1e12,
                   fluid_sample_TBps=FLUID_SAMPLE_BYTES_PER_NODE * nodes / (kernels["stats_fluid"]["ms_per_launch"] * 1e-3) / 1e12)
        st.destroy(); st = None
        out["iteration_ms"]["no_handle_again"] = timed(h, a.steps)
        out["build"] = lib.hc_build_tag().decode()
        print(json.dumps(out))
    finally:
        if st is not None:
            st.destroy()
        h.cellfields.destroy()
        L.destroy()


if __name__ == "__main__":
    main()
