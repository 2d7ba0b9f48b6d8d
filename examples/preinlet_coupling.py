"""python examples/preinlet_coupling.py [--mode host|device] [--iterations 500] [--warmup 50] [--repeat 3]
                                       [--pre 64 128 128] [--domain 256 128 128] [--direction Xneg]

Wall time per iteration of a coupled pre-inlet / domain run (fluid only, host.PreInlet): a walled pre-inlet channel, periodic
along the direction's axis and driven by host.preinlet_driving_force's force, feeds the velocity inlet of a walled domain
channel with a pressure outlet on its far face.  --mode host is the loop PreInlet.iterate(1) x iterations, which reads the
plane velocities back and sets the domain's slots from the host in every iteration; --mode device is one
PreInlet(device=True).iterate(iterations), which queues everything on the library's stream.  Each repetition is timed with a
host clock between two waits for the stream, after the warm-up iterations.  Prints one JSON line.

The two in-plane extents of --pre and --domain must agree (the cross-sections are matched node by node)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # after PYTHONPATH: another build can be timed

from hemocell_amd import capi, host   # noqa: E402

AXES = {"X": 0, "Y": 1, "Z": 2}


def channel_mask(dims, axis):
    m = np.zeros(dims, np.uint8)
    for ax in range(3):
        if ax != axis:
            idx = [slice(None)] * 3
            idx[ax] = 0; m[tuple(idx)] = 1
            idx[ax] = -1; m[tuple(idx)] = 1
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["host", "device"], default="host")
    ap.add_argument("--iterations", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--pre", type=int, nargs=3, default=[64, 128, 128])
    ap.add_argument("--domain", type=int, nargs=3, default=[256, 128, 128])
    ap.add_argument("--direction", default="Xneg")
    a = ap.parse_args()
    axis, neg = AXES[a.direction[0]], a.direction.endswith("neg")
    if axis != 0 and a.mode == "host" and not hasattr(host.Lattice, "planeVelocityAxis"):
        raise SystemExit("this build couples along x only")
    pre_dims, dom_dims = tuple(a.pre), tuple(a.domain)
    others = [d for d in range(3) if d != axis]
    assert all(pre_dims[d] == dom_dims[d] for d in others), "the cross-sections must agree"

    host.init(0)
    lib = capi.lib()
    omega = 1.0
    pre = host.Lattice(*pre_dims, tuple(d == axis for d in range(3)), omega)
    dom = host.Lattice(*dom_dims, (False, False, False), omega)
    pmask, dmask = channel_mask(pre_dims, axis), channel_mask(dom_dims, axis)
    area = int((np.take(pmask, 0, axis=axis) == 0).sum())
    F = [0.0, 0.0, 0.0]
    F[axis] = host.preinlet_driving_force(0.5, (1.0 / omega - 0.5) / 3.0, area, "Xneg" if neg else "Xpos")[2]
    pre.defineBounceBack(pmask); pre.setExternalVector(F); pre.latticeEquilibrium()
    dom.defineBounceBack(dmask); dom.latticeEquilibrium()
    la, lb = np.nonzero(np.take(pmask, 0, axis=axis) == 0)
    g = np.stack([la, lb], axis=1)
    pre_plane = pre_dims[axis] - 1 if neg else 0
    dom_plane, out_plane = (0, dom_dims[axis] - 1) if neg else (dom_dims[axis] - 1, 0)
    kw = {"device": True} if a.mode == "device" else {}
    coupling = host.PreInlet(pre, dom, g, pre_plane, dom_plane, direction=a.direction, **kw)
    box = [0, dom_dims[0] - 1, 0, dom_dims[1] - 1, 0, dom_dims[2] - 1]
    box[2 * axis] = box[2 * axis + 1] = out_plane
    nodes = np.mgrid[box[0]:box[1] + 1, box[2]:box[3] + 1, box[4]:box[5] + 1].reshape(3, -1).T
    dom.addOpenBoundaryNodes(1, 1 if neg else -1, nodes, **({"axis": axis} if axis else {}))

    def run(n):
        if a.mode == "device":
            coupling.iterate(n)
        else:
            for _ in range(n):
                coupling.iterate(1)

    run(a.warmup)
    host.check(lib.hc_synchronize())
    times = []
    for _ in range(a.repeat):
        t0 = time.perf_counter()
        run(a.iterations)
        host.check(lib.hc_synchronize())
        times.append((time.perf_counter() - t0) / a.iterations * 1e6)
    sent = dom.openBoundaryValues(coupling.first, len(g))[:, :3]
    assert np.isfinite(sent).all() and (sent[:, axis].mean() > 0) == neg
    print(json.dumps({"example": "preinlet_coupling", "mode": a.mode, "direction": a.direction, "pre": pre_dims, "domain": dom_dims,
                      "coupled_nodes": len(g), "iterations": a.iterations, "warmup": a.warmup,
                      "us_per_iteration": [round(t, 2) for t in times], "median_us": round(statistics.median(times), 2),
                      "spread_us": round(max(times) - min(times), 2), "mean_inlet_velocity": float(sent[:, axis].mean()),
                      "build_tag": lib.hc_build_tag().decode()}))
    if hasattr(coupling, "destroy"):
        coupling.destroy()
    pre.destroy(); dom.destroy()


if __name__ == "__main__":
    main()
