"""python examples/preinlet_slabs.py [--ranks 2] [--domain 192 66 66] [--pre 32 66 66] [--cells 3] [--iterations 200]
                                    [--warmup 20] [--transport tcp|rccl]

An inlet-fed channel with a pressure outlet on N x-slabs: a walled pre-inlet channel, periodic and driven along x, lives whole
on rank 0 and feeds the Zou-He velocity inlet on plane 0 of rank 0's slab (host.PreInlet, direction Xneg, on the device); the
last rank's last plane is a pressure outlet.  --domain is the GLOBAL domain, cut into --ranks equal slabs.  With --cells > 0
that many red blood cells are spread evenly along the channel axis (2 * ranks - 1 of them put one across every slab face; the
cells do not depend on --ranks, so --ranks 1 is the same run on one lattice) and every rank steps with
HemoCell.iterate(1) -- rank 0 between its pre-inlet's step and applyPreInlet -- so that the velocity update exchanges the
face-velocity message of an open lattice; with --cells 0 the run is fluid only, rank 0 queues PreInlet.iterate(n) and the other
ranks collideAndStream(n).

The script starts its own ranks as child processes, one per GPU (ranks that share a GPU talk through the host-staged transport),
and prints one JSON line with the wall time per iteration in ms, timed on rank 0 between two waits for the device."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def channel_mask(dims):
    m = np.zeros(dims, np.uint8)
    m[:, 0, :] = m[:, -1, :] = 1
    m[:, :, 0] = m[:, :, -1] = 1
    return m


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ranks", type=int, default=2)
    ap.add_argument("--domain", type=int, nargs=3, default=[192, 66, 66])
    ap.add_argument("--pre", type=int, nargs=3, default=[32, 66, 66])
    ap.add_argument("--cells", type=int, default=3)
    ap.add_argument("--iterations", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--transport", choices=["tcp", "rccl"], default=None)
    return ap.parse_args()


def launch_ranks(a):
    port = 29600 + os.getpid() % 2000
    procs = []
    for r in range(a.ranks):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(a.ranks), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=None if r == 0 else subprocess.DEVNULL))
    rcs = [p.wait() for p in procs]
    if any(rcs):
        sys.exit("preinlet_slabs.py: ranks exited with %s" % rcs)


def main():
    a = parse()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world == 1 and a.ranks > 1:
        return launch_ranks(a)
    if world != a.ranks:
        sys.exit("preinlet_slabs.py --ranks %d was started in a world of %d ranks" % (a.ranks, world))
    nxg, ny, nz = a.domain
    if nxg % world or tuple(a.pre[1:]) != (ny, nz):
        sys.exit("preinlet_slabs.py: the domain's planes must divide into the ranks, and the cross-sections must agree")
    # stdout carries the JSON line only (RCCL prints a banner there)
    sys.stdout.flush()
    result_fd = os.dup(1)
    os.dup2(2, 1)
    if a.transport:
        os.environ["HEMOCELL_TRANSPORT"] = a.transport

    from hemocell_amd import host, slab

    lib = host.capi.lib()
    if world > 1:
        rank, world = slab.comm_init_env()
    else:
        rank = 0
        host.init(0)
    P = host.base_parameters()
    omega = 1.0 / P.tau
    nx = nxg // world
    r = slab.SlabRunner(nx, ny, nz, rank, world, P, periodic=(False, False, False), particle_timescale=5, material_timescale=20,
                        fluid_only=a.cells == 0)
    r.define_bounce_back(channel_mask((nxg, ny, nz)))
    r.lattice.latticeEquilibrium()
    pre = coupling = None
    if rank == 0:   # the pre-inlet, whole, beside rank 0's slab; the inlet is the local plane 0
        pre_dims = tuple(a.pre)
        pmask = channel_mask(pre_dims)
        area = int((pmask[0] == 0).sum())
        pre = host.Lattice(*pre_dims, (True, False, False), omega)
        pre.defineBounceBack(pmask)
        pre.setExternalVector((host.preinlet_driving_force(0.5, (1.0 / omega - 0.5) / 3.0, area, "Xneg")[2], 0.0, 0.0))
        pre.latticeEquilibrium()
        ly, lz = np.nonzero(pmask[0] == 0)
        coupling = host.PreInlet(pre, r.lattice, np.stack([ly, lz], axis=1), pre_dims[0] - 1, 0, direction="Xneg", device=True)
    r.add_open_boundary(1, 0, 1, (nxg - 1, nxg - 1, 0, ny - 1, 0, nz - 1))   # the pressure outlet, global coordinates: the last rank keeps it
    n_cells = 0
    if a.cells:
        r.add_cell_type(host.CellType.rbc(P))
        # evenly spaced along the axis, the same cells whatever the number of ranks: with --cells 2 * ranks - 1 every
        # slab face has a cell across it
        xs = [nxg * (k + 1.0) / (a.cells + 1) + 0.3 for k in range(a.cells)]
        r.load_cells(0, [np.array([x, ny / 2.0, nz / 2.0]) for x in xs], [np.array([90.0, 0.0, 0.0])] * len(xs))
        n_cells = int(r.sync_placement()[0])
        r.prepare()

    def run(n):
        if a.cells:
            for _ in range(n):
                if pre is not None:
                    pre.collideAndStream(1)
                r.run(1)                     # collective: every rank steps its slab
                if coupling is not None:
                    coupling.applyPreInlet()
        elif coupling is not None:
            coupling.iterate(n)              # n x (pre-inlet step, collective domain step, apply), queued in one call
        else:
            r.run(n)

    run(a.warmup)
    host.check(lib.hc_synchronize())
    if world > 1:
        slab.barrier()
    t0 = time.perf_counter()
    run(a.iterations)
    host.check(lib.hc_synchronize())
    ms = (time.perf_counter() - t0) / a.iterations * 1e3
    mn, mx, mean, n_nodes = r.fluid_stats(0)   # reduced over the slabs
    if rank == 0:
        sent = coupling.sent()
        assert np.isfinite(sent).all() and np.isfinite([mn, mx, mean]).all() and sent[:, 0].mean() > 0
        os.write(result_fd, (json.dumps({"example": "preinlet_slabs", "ranks": world, "domain": [nxg, ny, nz], "pre": list(a.pre),
                                         "cells": n_cells, "iterations": a.iterations, "warmup": a.warmup,
                                         "ms_per_iteration": round(ms, 4), "mean_inlet_velocity": float(sent[:, 0].mean()),
                                         "max_velocity": float(mx), "fluid_nodes": int(n_nodes),
                                         "build_tag": lib.hc_build_tag().decode()}) + "\n").encode())
        coupling.destroy()
        pre.destroy()
    if world > 1:
        slab.barrier()
        slab.comm_finalize()
    r.lattice.destroy()


if __name__ == "__main__":
    main()
