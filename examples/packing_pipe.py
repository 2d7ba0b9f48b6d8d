"""Pack a pipe, load the cells into a lattice with the pipe's mask, step it, and say what the wall term costs.

pack_pipe packs the enclosing ellipsoids of RBCs and platelets inside a straight pipe, periodic along x, to the requested
hematocrit of the lumen ("packing walls").  Every cell then goes through host.Cells.addCell into a
host.Lattice that carries the same mask, and the suspension runs a few hc_iterate steps.  One JSON line is printed: the cells,
the iterations, the time per iteration with the wall term and without it, the hematocrit over the lumen, and how many cells the
lattice kept.

The time per iteration is a host clock between the first and the last wait of hc_packing_run over the iterations done between
them (each wait ends in a stream synchronise), as in examples/packing_cost.py: it leaves out create, the distance field and
the first batch, which loads the code objects.  "Without the wall term" is the same cells packed into the enclosing periodic
box on the same grid (same sizing factor, so the same lists and launch sizes) by the kernels' <false> instances, with pk_wall
not launched.  That packing is sparse and ends after some tens of iterations, so both packings queue only --steps-per-wait 8
iterations per host wait, the same for both since a wait costs as much as an iteration; its window is a few milliseconds, and
the figures are per iteration, not totals.  Both packings run --repeats times in turn and every figure is printed.  A small
packing runs first as warm-up.  DESIGN.md section 7 quotes the figures.

    python examples/packing_pipe.py [--radius 20] [--length 24] [--hematocrit 0.25] [--dx 0.5] [--margin 1.0] [--seed 1] [--steps 10]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from hemocell_amd import host, packing  # noqa: E402


def timed(fn, **kw):
    marks = []
    t0 = time.perf_counter()
    res = fn(progress=lambda st: marks.append((time.perf_counter(), int(st[0]))), **kw)
    total = time.perf_counter() - t0
    per = None
    if len(marks) >= 2 and marks[-1][1] > marks[0][1]:
        per = round(1e3 * (marks[-1][0] - marks[0][0]) / (marks[-1][1] - marks[0][1]), 4)
    return res, total, per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--radius", type=float, default=20.0)
    ap.add_argument("--length", type=float, default=24.0)
    ap.add_argument("--hematocrit", type=float, default=0.25)
    ap.add_argument("--dx", type=float, default=0.5)
    ap.add_argument("--margin", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--max-iter", type=int, default=20000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps-per-wait", type=int, default=8)
    a = ap.parse_args()
    host.init(0)
    packing.pack_cells((24, 24, 24), hematocrit=0.3, seed=0, max_iter=200)   # warm-up
    per_wall, per_free = [], []
    for _ in range(a.repeats):   # the two packings alternate, so that a drift of the machine shows in both
        res, total, per = timed(lambda **kw: packing.pack_pipe(a.length, a.radius, a.hematocrit, dx_um=a.dx, wall_margin_um=a.margin,
                                                               seed=a.seed, max_iter=a.max_iter, steps_per_wait=a.steps_per_wait, **kw))
        per_wall.append(per)
        cells = list(zip(res.names, res.counts))
        box = [(n - 1) * a.dx for n in res.wall_mask.shape]
        box[0] = a.length
        free, _, per = timed(lambda **kw: packing.pack_cells(box, cells=cells, scale=res.plan.scale, seed=a.seed, max_iter=res.steps,
                                                             steps_per_wait=a.steps_per_wait, **kw))
        per_free.append(per)

    P = host.base_parameters()
    nx, ny, nz = res.wall_mask.shape
    L = host.Lattice(nx, ny, nz, res.periodic, 1.0 / P.tau)
    L.defineBounceBack(res.wall_mask)
    L.latticeEquilibrium()
    h = host.HemoCell(L, P)
    types = {"RBC": host.CellType.rbc(P), "PLT": host.CellType.plt(P)}
    placed = 0
    for t, name in enumerate(res.names):
        h.cellfields.addCellType(types[name], 1)
        for centre, angles in zip(res.positions[name], res.angles[name]):
            placed += bool(h.cellfields.addCell(t, centre / a.dx, angles))
    node = np.floor(h.cellfields.positions + 0.5).astype(int)
    node[:, 0] %= nx
    on_wall = int(res.wall_mask[node[:, 0], np.clip(node[:, 1], 0, ny - 1), np.clip(node[:, 2], 0, nz - 1)].sum())
    h.cellfields.applyConstitutiveModel(0, True)
    h.iterate(a.steps)
    removed = h.cellfields.deletion_counts()
    n_rbc = res.counts[res.names.index("RBC")] if "RBC" in res.names else 0
    print(json.dumps({
        "pipe_um": {"radius": a.radius, "length": a.length, "dx": a.dx, "wall_margin": a.margin}, "seed": a.seed,
        "cells": dict(cells), "grid": res.plan.grid, "finished": res.finished, "iterations": res.steps,
        "outer_diameter": res.outer_diameter, "total_s": round(total, 4), "ms_per_iteration_walls": per_wall,
        "periodic_box_um": [round(v, 3) for v in free.plan.size_um], "periodic_box_grid": free.plan.grid,
        "periodic_box_iterations": free.steps, "ms_per_iteration_no_walls": per_free,
        "lumen_um3": res.lumen_volume_um3, "hematocrit_requested": a.hematocrit,
        "hematocrit_lumen": round(n_rbc * packing.RBC_VOLUME_NOMINAL_UM3 / res.lumen_volume_um3, 6),
        "cells_placed": placed, "vertices_on_wall_nodes": on_wall, "lattice_steps": a.steps,
        "cells_removed": removed[0], "particles_removed": removed[1]}), flush=True)
    h.cellfields.destroy()
    L.destroy()


if __name__ == "__main__":
    main()
