"""What interior viscosity costs on the benchmark's workload: the pipe of bench.py (default 256^3, 10 % haematocrit, velocity
update every 5, material model every 20) through the Python host, once without the feature and once with viscosity ratio 5,
the membrane pass every 10 and the entire-grid pass every 1000 iterations, in one process.

Prints one JSON line: the collide's time per launch of the plain instantiation and of the interior-viscosity one (hipEvent
pairs around every launch, hc_profile_read), the time of one membrane pass and of one entire-grid pass (event pairs around
the kernels of a pass), and the number of tagged nodes.  DESIGN.md section 7 quotes it.

    python examples/interior_viscosity.py [--n 256] [--steps 200] [--warmup 20]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from hemocell_amd import host  # noqa: E402
from hemocell_amd.packing import pack_pipe_rbc  # noqa: E402


def profile(name):
    ms, n = C.c_double(), C.c_long()
    host.check(host.capi.lib().hc_profile_read(name.encode(), C.byref(ms), C.byref(n)))
    return ms.value, n.value


def per_launch(name):
    ms, n = profile(name)
    return ms / n if n else None


def run(n, steps, warmup, ratio):
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
        kw = {} if ratio is None else dict(interior_viscosity=True, viscosity_ratio=ratio)
        cf.addCellType(host.CellType.rbc(P, **kw), 20)
        centres, angles = pack_pipe_rbc(n, n, n, 0.10)
        cells = sum(bool(cf.addCell(0, c, a, 0.0, cell_id=i)) for i, (c, a) in enumerate(zip(centres, angles)))
        if ratio is not None:
            cf.setInteriorViscosityTimeScaleSeparation(10, 1000)
        cf.applyConstitutiveModel(0, True)
        h.iterate(warmup)            # iteration 0 runs both passes
        h.synchronize()
        host.check(lib.hc_profile_enable(1))
        host.check(lib.hc_profile_reset())
        h.iterate(steps)
        h.synchronize()
        out = dict(cells=cells, collide_ms_per_launch=per_launch("collide_stream"), collide_launches=profile("collide_stream")[1],
                   interior_launches=profile("collide_stream_interior")[1], bytes_per_node=L.bytes_per_node())
        if ratio is not None:
            out["membrane_pass_ms"] = per_launch("interior_membrane")
            out["membrane_passes"] = profile("interior_membrane")[1]
            host.check(lib.hc_profile_reset())
            cf.findInternalParticleGridPoints()
            cf.findInternalParticleGridPoints()
            h.synchronize()
            out["entire_grid_pass_ms"] = per_launch("interior_find")
            out["tagged_nodes"] = int(np.count_nonzero(L.interiorClasses()))
        host.check(lib.hc_profile_enable(0))
        return out
    finally:
        L.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--ratio", type=float, default=5.0)
    a = ap.parse_args()
    host.init(0)
    plain = run(a.n, a.steps, a.warmup, None)
    visc = run(a.n, a.steps, a.warmup, a.ratio)
    plain_again = run(a.n, a.steps, a.warmup, None)
    print(json.dumps(dict(n=a.n, steps=a.steps, ratio=a.ratio, plain=plain, interior=visc, plain_again=plain_again,
                          build=host.capi.lib().hc_build_tag().decode())))


if __name__ == "__main__":
    main()
