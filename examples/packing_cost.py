"""What packing costs on the device: 100^3 um and 200^3 um at hematocrit 0.40 packed to the end with pack_cells.

Prints one JSON line per box: cells, grid, iterations, the total wall time of pack_cells (plan, initial state, create with
the first force evaluation, every iteration, download) and the time per iteration.  The time per iteration is a host clock
between the first and the last wait of hc_packing_run (each ends in a stream synchronise), over the iterations done between
them, so it leaves out create and the first batch, which loads the code objects; the last batch holds the launches queued
behind the end, which return at once.  A small packing runs first as warm-up.  DESIGN.md section 7 quotes the figures.

    python examples/packing_cost.py [--sizes 100 200] [--hematocrit 0.40] [--seed 0] [--steps-per-wait 64]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from hemocell_amd.packing import pack_cells  # noqa: E402


def run(size, hematocrit, seed, steps_per_wait, max_iter):
    marks = []
    t0 = time.perf_counter()
    res = pack_cells((size,) * 3, hematocrit=hematocrit, seed=seed, steps_per_wait=steps_per_wait, max_iter=max_iter,
                     progress=lambda st: marks.append((time.perf_counter(), int(st[0]))))
    total = time.perf_counter() - t0
    out = {"box_um": size, "hematocrit": hematocrit, "seed": seed, "cells": dict(zip(res.names, res.counts)), "grid": res.plan.grid,
           "packed_box_um": round(res.box_um[0], 6), "iterations": res.steps, "finished": res.finished, "density": res.density,
           "max_root_evaluations": res.max_root_evaluations, "total_s": round(total, 4), "waits": len(marks)}
    if len(marks) >= 2 and marks[-1][1] > marks[0][1]:
        out["ms_per_iteration"] = round(1e3 * (marks[-1][0] - marks[0][0]) / (marks[-1][1] - marks[0][1]), 4)
    else:
        out["ms_per_iteration"] = None   # one wait only: nothing to difference
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[100, 200])
    ap.add_argument("--hematocrit", type=float, default=0.40)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--steps-per-wait", type=int, default=64)
    ap.add_argument("--max-iter", type=int, default=5000)
    a = ap.parse_args()
    pack_cells((24, 24, 24), hematocrit=0.3, seed=0, max_iter=200)   # warm-up
    for size in a.sizes:
        print(json.dumps(run(size, a.hematocrit, a.seed, a.steps_per_wait, a.max_iter)), flush=True)


if __name__ == "__main__":
    main()
