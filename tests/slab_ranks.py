"""Ranks for the slab tests -- test infrastructure only: N processes on GPU 0 that talk through the library's TCP data plane
(RCCL refuses two ranks on one device), each running one function and handing its arrays back through an .npz file.

run(fn, world, tmp_path, *args): fn(rank, world, *args) -> {name: array} runs on every rank between comm_init and a barrier;
fn is a module-level function of the calling test module (the children import it by name).  Returns the ranks' dicts in rank
order.  A rank that raises reports its traceback; its peers then run into HEMOCELL_COMM_TIMEOUT on their sockets, and the
parent's waits are bounded."""
import multiprocessing as mp
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_RANKS = 4


def _entry(fn, rank, world, port, out, args, q):
    try:
        sys.path.insert(0, ROOT)
        from hemocell_amd import slab
        slab.comm_init(rank, world, local_rank=0, port=port, transport="tcp")   # every rank on GPU 0
        res = fn(rank, world, *args)
        np.savez(os.path.join(out, "rank%d.npz" % rank), **res)
        slab.barrier()
        slab.comm_finalize()
        q.put((rank, "ok"))
    except BaseException as e:   # noqa: BLE001 -- the parent reports it
        import traceback
        q.put((rank, "FAILED: %r\n%s" % (e, traceback.format_exc())))


def run(fn, world, tmp_path, *args, salt=0):
    assert 2 <= world <= MAX_RANKS
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 32000 + (os.getpid() * 7 + world * 101 + salt * 397 + 11) % 20000
    os.environ["HEMOCELL_COMM_TIMEOUT"] = "60"
    ps = [ctx.Process(target=_entry, args=(fn, r, world, port, str(tmp_path), args, q)) for r in range(world)]
    for p in ps:
        p.start()
    try:
        res = [q.get(timeout=240) for _ in ps]
    finally:
        for p in ps:
            p.join(30)
        for p in ps:
            if p.is_alive():
                p.kill()
    assert sorted(r[0] for r in res) == list(range(world)) and all(r[1] == "ok" for r in res), res
    return [dict(np.load(os.path.join(str(tmp_path), "rank%d.npz" % k), allow_pickle=False)) for k in range(world)]
