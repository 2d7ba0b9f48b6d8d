"""python examples/preinlet_cells_slabs.py [--ranks 2] [--iterations 1000] [--cells-every 20] [--repeat 15] [--transport tcp|rccl]

The channel of examples/preinlet_cells.py -- a periodic, driven pre-inlet with a few cells feeds a walled 96 x 34 x 34 domain
through its velocity inlet, whole cells are injected from the pre-inlet's window, and a sink in front of the pressure outlet takes
them out again -- with the domain cut into --ranks x-slabs, one process per slab.  The pre-inlet lives whole on rank 0, which
holds host.PreInlet(device=True, cells=(pre_cells, slab_cells)); the other ranks hold host.PreInletPeer and make the same calls.
Ranks that share a GPU talk through the host-staged transport (the default here).

The script starts its own processes: first the same run on ONE domain (--ranks 1 of this script), then the ranks.  It prints one
JSON line with both: cell counts, wall time per iteration, and the wall time of one check (applyPreInletCells) with no candidate
left -- with the sink, which on slabs costs two rounds over the control plane, and without it, which costs one -- each the
median of --repeat calls on an idle stream between a barrier and the end of a wait for the stream, on rank 0."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PRE, DOM = (48, 34, 34), (96, 34, 34)
WINDOW, SHIFT, STRIDE, SINK = (6.0, 40.0), (-4.0, 0.0, 0.0), 100000, 88.0   # the window's image [2, 36] keeps the envelope off x = 48
U0 = 0.03


def channel_mask(dims):
    m = np.zeros(dims, np.uint8)
    m[:, 0, :] = m[:, -1, :] = m[:, :, 0] = m[:, :, -1] = 1
    return m


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ranks", type=int, default=2)
    ap.add_argument("--iterations", type=int, default=1000)
    ap.add_argument("--cells-every", type=int, default=20)
    ap.add_argument("--repeat", type=int, default=15)
    ap.add_argument("--transport", choices=["tcp", "rccl"], default="tcp")
    return ap.parse_args()


def launch(a):
    """one domain first, then the ranks; both JSON lines merged into one"""
    me = [sys.executable, os.path.abspath(__file__)]
    args = ["--iterations", str(a.iterations), "--cells-every", str(a.cells_every), "--repeat", str(a.repeat), "--transport", a.transport]
    single = subprocess.run(me + ["--ranks", "1"] + args, env=dict(os.environ, HEMOCELL_EXAMPLE_CHILD="1"), stdout=subprocess.PIPE, check=True)
    port = 29700 + os.getpid() % 2000
    procs = []
    for r in range(a.ranks):
        env = dict(os.environ, HEMOCELL_EXAMPLE_CHILD="1", RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(a.ranks), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port))
        procs.append(subprocess.Popen(me + ["--ranks", str(a.ranks)] + args, env=env, stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL))
    out = procs[0].communicate()[0]
    rcs = [p.wait() for p in procs]
    if any(rcs):
        sys.exit("preinlet_cells_slabs.py: ranks exited with %s" % rcs)
    one, slabs = json.loads(single.stdout.decode().strip().splitlines()[-1]), json.loads(out.decode().strip().splitlines()[-1])
    print(json.dumps({"example": "preinlet_cells_slabs", "one_domain": one, "slabs": slabs}))


def main():
    a = parse()
    if not os.environ.get("HEMOCELL_EXAMPLE_CHILD"):
        return launch(a)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != a.ranks or DOM[0] % world:
        sys.exit("preinlet_cells_slabs.py --ranks %d was started in a world of %d ranks" % (a.ranks, world))
    sys.stdout.flush()
    result_fd = os.dup(1)   # stdout carries the JSON line only
    os.dup2(2, 1)
    os.environ["HEMOCELL_TRANSPORT"] = a.transport

    from hemocell_amd import host, slab

    lib = host.capi.lib()
    if world > 1:
        rank, world = slab.comm_init_env()
    else:
        rank = 0
        host.init(0)
    P = host.base_parameters()
    nx = DOM[0] // world
    r = slab.SlabRunner(nx, DOM[1], DOM[2], rank, world, P, periodic=(False, False, False), particle_timescale=1, material_timescale=1)
    r.define_bounce_back(channel_mask(DOM))
    r.lattice.latticeEquilibrium(1.0, (U0, 0.0, 0.0))
    types = [host.CellType.rbc(P), host.CellType.plt(P)]
    for t in types:
        r.add_cell_type(t)
    r.cells.addCell(0, (60.0, 16.5, 16.5), (90.0, 0.0, 0.0), cell_id=50)   # every rank offers it; the rank whose slab holds it keeps it
    r.sync_placement()
    r.prepare()
    kw = dict(window=WINDOW, shift=SHIFT, id_stride=STRIDE, sink=SINK, cells_every=a.cells_every)
    pre = pc = None
    if rank == 0:
        pmask = channel_mask(PRE)
        area = int((pmask[0] == 0).sum())
        radius = np.sqrt(area / np.pi)
        _, _, F = host.preinlet_driving_force_vector(U0 * 2 * radius / P.nu_lbm, P.nu_lbm, area, "Xneg")
        pre = host.Lattice(*PRE, (True, False, False), 1.0 / P.tau)
        pre.defineBounceBack(pmask); pre.setExternalVector(F); pre.latticeEquilibrium(1.0, (U0, 0.0, 0.0))
        pc = host.Cells(pre, P)
        for t in types:
            pc.addCellType(t, 1)
        assert pc.addCell(1, (12.0, 16.5, 16.5), (10.0, 20.0, 30.0), cell_id=0)
        assert pc.addCell(1, (2.0, 11.0, 22.0), (40.0, 0.0, 10.0), cell_id=1)
        assert pc.addCell(1, (1.5, 22.0, 11.0), (0.0, 30.0, 60.0), cell_id=2)
        assert pc.addCell(0, (-4.0, 16.5, 16.5), (90.0, 0.0, 0.0), cell_id=3)   # across the periodic seam, lap -1
        pc.applyConstitutiveModel(0, True)
        g = np.stack(np.nonzero(pmask[0] == 0), axis=1)
        coupling = host.PreInlet(pre, r.lattice, g, PRE[0] - 1, 0, direction="Xneg", device=True, cells=(pc, r.cells), **kw)
        r.lattice.setOpenBoundaryVelocitySlots(coupling.first, np.tile((U0, 0.0, 0.0), (len(g), 1)))
    else:
        coupling = host.PreInletPeer(r.cells, direction="Xneg", **kw)
    r.add_open_boundary(1, 0, 1, (DOM[0] - 1, DOM[0] - 1, 0, DOM[1] - 1, 0, DOM[2] - 1))

    def sync():
        host.check(lib.hc_synchronize())
        if world > 1:
            slab.barrier()

    coupling.iterate(a.cells_every)   # warm-up: the first check allocates
    sync()
    t0 = time.perf_counter()
    coupling.iterate(a.iterations)
    host.check(lib.hc_synchronize())
    per_iteration = (time.perf_counter() - t0) / a.iterations * 1e6
    counts = coupling.cell_counts()

    def time_check(sink_on):
        """median wall time [us] of one check that finds no new candidate and nothing past the plane"""
        host.check(lib.hcp_preinlet_set_sink(coupling.cells_ptr, int(sink_on), SINK))
        times = []
        for _ in range(a.repeat + 1):
            sync()
            t = time.perf_counter()
            got = coupling.applyPreInletCells()
            host.check(lib.hc_synchronize())
            times.append((time.perf_counter() - t) * 1e6)
            assert got == (0, 0), got
        return statistics.median(times[1:]), max(times[1:]) - min(times[1:])

    with_sink, without = time_check(True), time_check(False)
    held = r.cells.counts()[1]
    assert np.isfinite(r.cells.positions).all() and np.isfinite(r.populations()).all()
    if rank == 0:
        os.write(result_fd, (json.dumps({"ranks": world, "transport": a.transport if world > 1 else None, "pre": PRE, "domain": DOM,
                                         "iterations": a.iterations, "cells_every": a.cells_every, "injected": counts[0], "rejected": counts[1],
                                         "removed_by_sink": counts[2], "checks": counts[3], "cells_held_by_rank_0": held,
                                         "us_per_iteration": round(per_iteration, 2),
                                         "check_us_with_sink": round(with_sink[0], 2), "check_us_with_sink_spread": round(with_sink[1], 2),
                                         "check_us_without_sink": round(without[0], 2), "check_us_without_sink_spread": round(without[1], 2),
                                         "build_tag": lib.hc_build_tag().decode()}) + "\n").encode())
    coupling.destroy()
    if pc is not None:
        pc.destroy(); pre.destroy()
    if world > 1:
        slab.barrier()
        slab.comm_finalize()
    r.lattice.destroy()


if __name__ == "__main__":
    main()
