"""x-slab decomposition of the pipe across the GPUs of one node (one process per GPU).

Reference equivalent: Palabos atomic blocks + envelopes (core/hemoCell.cpp:142 fluid envelope,
core/hemoCellFields.cpp:377-499 syncEnvelopes).  Here every rank owns ONE slab along x (the pipe axis).  The whole
schedule -- faces of the 5 crossing populations every step, particle envelopes at every velocity update, both
travelling beside the interior collide -- runs inside libhemocell_amd.so (csrc/slab.hip over csrc/comm.hip: RCCL
point-to-point between x-neighbours, or the same messages through the library's TCP mesh when ranks share a GPU).
This module only creates the objects and calls hc_iterate / hcl_collide_stream; no step is scheduled from Python.

world == 1 runs the loop on one GPU with the periodic wrap done in-kernel.
"""
import ctypes as C
import os

import numpy as np

from . import host

TRANSPORT = {"none": 0, "rccl": 1, "tcp": 2, "auto": 3}


def comm_init_env():
    """connect the ranks named by RANK / WORLD_SIZE / LOCAL_RANK / MASTER_ADDR / MASTER_PORT (torch.distributed.run's
    variables) and select this rank's GPU; a no-op for a one-rank world.  Returns (rank, world)."""
    lib = host.capi.lib()
    host.check(lib.hc_comm_init_env())
    return comm_info()[:2]


def comm_init(rank, world, local_rank=None, addr="127.0.0.1", port=30417, transport="rccl", init_device=True):
    host.check(host.capi.lib().hc_comm_init(int(rank), int(world), int(rank if local_rank is None else local_rank),
                                           addr.encode(), int(port), TRANSPORT[transport], int(bool(init_device))))


def comm_info():
    r, w, t = C.c_int(), C.c_int(), C.c_int()
    host.check(host.capi.lib().hc_comm_info(C.byref(r), C.byref(w), C.byref(t)))
    return r.value, w.value, t.value


def barrier():
    host.check(host.capi.lib().hc_comm_barrier())


def allreduce(values, op="sum"):
    v = np.ascontiguousarray(values, dtype=np.float64).copy()
    host.check(host.capi.lib().hc_comm_allreduce(host.dptr(v), v.size, {"sum": 0, "min": 1, "max": 2}[op]))
    return v


def comm_finalize():
    host.check(host.capi.lib().hc_comm_finalize())


def open_boundary_rows(where_global, x0, nx, nc=None, values=None):
    """The part of an open-boundary declaration that falls on the slab [x0, x0 + nx).  where_global: an inclusive box
    (x0, x1, y0, y1, z0, z1) or an [n][3] node list, GLOBAL node coordinates; its nodes are taken in box order (x outermost, z
    innermost) or list order.  Returns (box, nodes, rows, values): the box clipped to the slab and translated to local
    coordinates (None for a node list, or where the box misses the slab), the slab's nodes [m][3] in local coordinates, their
    rows in the global order -- ascending, so the per-rank lists concatenated in rank order are the global order of a box --
    and, with nc and values (one value or one per node, nc components each), this slab's rows of them [m][nc].  Pure numpy."""
    w = np.asarray(where_global, dtype=np.int64)
    box = None
    if w.shape == (6,):
        g = np.mgrid[w[0]:w[1] + 1, w[2]:w[3] + 1, w[4]:w[5] + 1].reshape(3, -1).T
        lo, hi = max(int(w[0]), x0), min(int(w[1]), x0 + nx - 1)
        if lo <= hi and w[2] <= w[3] and w[4] <= w[5]:
            box = (lo - x0, hi - x0, int(w[2]), int(w[3]), int(w[4]), int(w[5]))
    else:
        g = w.reshape(-1, 3)
    rows = np.flatnonzero((g[:, 0] >= x0) & (g[:, 0] < x0 + nx))
    nodes = g[rows] - np.array([x0, 0, 0], dtype=np.int64)
    vals = None
    if values is not None:
        v = np.asarray(values, dtype=np.float64)
        v = np.broadcast_to(v.reshape(-1, nc) if v.size != nc else v.reshape(1, nc), (len(g), nc))
        vals = np.ascontiguousarray(v[rows])
    return box, nodes, rows, vals


class SlabRunner:
    def __init__(self, nx_local, ny, nz, rank, world, P, periodic=(True, False, False), particle_timescale=5,
                 material_timescale=20, deletion_check_every=1, fluid_only=False, n_slabs=None):
        self.rank, self.world = rank, world
        self.nx, self.ny, self.nz = nx_local, ny, nz
        self.nx_global = nx_local * world
        self.x0 = rank * nx_local
        self.P = P
        self.periodic = periodic
        self.k_p, self.k_m = particle_timescale, material_timescale
        # n_slabs > 1 with world == 1: a rank that is its own periodic neighbour over the data plane (transport tests)
        self.n_slabs = world if n_slabs is None else n_slabs
        self.lattice = host.Lattice(nx_local, ny, nz, periodic, 1.0 / P.tau, x0=self.x0, nx_global=self.nx_global,
                                    n_slabs=self.n_slabs)
        self.fluid_only = fluid_only   # no membrane cells: the lattice then never touches the IBM force buffers
        if fluid_only:
            self.hemocell, self.cells = None, None
        else:
            self.hemocell = host.HemoCell(self.lattice, P)
            self.hemocell.setParticleVelocityUpdateTimeScaleSeparation(particle_timescale)
            self.hemocell.deletion_check_every = deletion_check_every
            self.cells = self.hemocell.cellfields

    def define_bounce_back(self, mask_global):
        self.lattice.defineBounceBack(mask_global)

    # ---- Zou-He open boundaries in GLOBAL node coordinates: every rank makes the same call and keeps what lies on its slab
    # (open_boundary_rows); the slots are the slab's own
    def add_open_boundary(self, kind, axis, orientation, box_global):
        """kind 0 = velocity, 1 = pressure; axis 0, 1, 2; orientation -1 = N, +1 = P; box_global inclusive.  Returns
        (first_slot, n) on this slab, its nodes in box order; n == 0 where the box misses the slab."""
        _, nodes, _, _ = open_boundary_rows(box_global, self.x0, self.nx)
        first = self.lattice.addOpenBoundaryNodes(kind, orientation, nodes, axis=axis)
        return first, len(nodes)

    def set_open_velocity(self, where_global, u):
        """setBoundaryVelocity on a global box or [n][3] node list: one velocity or one per node in that global order"""
        _, nodes, _, vals = open_boundary_rows(where_global, self.x0, self.nx, 3, u)
        if len(nodes):
            self.lattice.setBoundaryVelocity(nodes, vals)

    def set_open_density(self, where_global, rho):
        """setBoundaryDensity likewise: one density or one per node"""
        _, nodes, _, vals = open_boundary_rows(where_global, self.x0, self.nx, 1, rho)
        if len(nodes):
            self.lattice.setBoundaryDensity(nodes, vals)

    def add_cell_type(self, celltype):
        return self.cells.addCellType(celltype, self.k_m)

    def set_envelope(self, particle_envelope_lu):
        """<domain><particleEnvelope> of the configuration (core/hemoCell.cpp:139), after the cell types and before the cells;
        returns the distance from a slab face within which whole cells are replicated"""
        used = C.c_double()
        host.check(host.capi.lib().hcp_set_envelope(self.cells.ptr, float(particle_envelope_lu), C.byref(used)))
        return used.value

    def envelope(self):
        """(share in use [lu], copies that arrived late so far)"""
        used, late = C.c_double(), C.c_long()
        host.check(host.capi.lib().hcp_envelope(self.cells.ptr, C.byref(used), C.byref(late)))
        return used.value, late.value

    def load_cells(self, t, centres, angles, min_dist_um=0.0):
        """offer every cell to this rank (hcp_add_cell keeps what its slab has to hold, periodic images included);
        call sync_placement() after the last type.  Returns the number of cells kept on this rank."""
        n = 0
        for i, (c, a) in enumerate(zip(centres, angles)):
            n += bool(self.cells.addCell(t, c, a, min_dist_um, cell_id=i))
        return n

    def sync_placement(self):
        """drop everywhere the cells some rank rejected at a wall; distinct cells per type over all slabs"""
        out = np.zeros(max(len(self.cells.types), 1), dtype=np.int64)
        host.check(host.capi.lib().hcp_slab_sync_placement(self.cells.ptr, host.lptr(out)))
        return out[:len(self.cells.types)]

    def owned_vertices(self):
        if self.fluid_only:
            return 0
        n = C.c_long()
        host.check(host.capi.lib().hcp_owned_vertices(self.cells.ptr, C.byref(n)))
        return n.value

    def prepare(self):
        """what the drivers do before the loop: forces of the initial configuration"""
        if not self.fluid_only:
            self.cells.applyConstitutiveModel(0, True)

    def run(self, n):
        if self.fluid_only:
            self.lattice.collideAndStream(n)
        else:
            self.hemocell.iterate(n)

    def slab_stats(self, reset=False):
        """counters of the native slab schedule (hc_slab_stats)"""
        o = np.zeros(8)
        host.check(host.capi.lib().hc_slab_stats(self.lattice.ptr, host.dptr(o), int(reset)))
        names = ("cells_sent", "cells_new", "cells_dropped", "cells_deleted", "iterations", "host_s", "header_wait_s", "particle_steps")
        return dict(zip(names, o.tolist()))

    # ---- diagnostics across slabs: the reference gathers per-block statistics (HemoCellGatheringFunctional,
    # core/hemoCellFunctional.h:101-112); here a few scalars are reduced over the control plane at output cadence
    def _reduce(self, mn, mx, total, count):
        if self.world == 1:
            return mn, mx, total, count
        big = 1e300
        lo = allreduce([mn if count else big], "min")[0]
        hi = allreduce([mx if count else -big], "max")[0]
        sm = allreduce([total, float(count)], "sum")
        n = int(sm[1])
        return (float(lo) if n else 0.0), (float(hi) if n else 0.0), float(sm[0]), n

    def fluid_stats(self, what=0):
        """FluidInfo statistics over the whole domain: (min, max, mean, nodes)"""
        mn, mx, avg, n = self.lattice.fluid_stats(what)
        mn, mx, total, n = self._reduce(mn, mx, avg * n, n)
        return mn, mx, (total / n if n else 0.0), n

    def vertex_stats(self, what=2):
        """ParticleInfo statistics over all owned vertices of all slabs: (min, max, mean, vertices)"""
        mn, mx, avg, n = self.cells.vertex_stats(what) if not self.fluid_only else (0.0, 0.0, 0.0, 0)
        mn, mx, total, n = self._reduce(mn, mx, avg * n, n)
        return mn, mx, (total / n if n else 0.0), n

    # ---- inspection helpers (tests / output): gather-free, per rank
    def populations(self):
        """post-stream populations of this slab (the library refreshes the halo planes the view pulls from)"""
        return self.lattice.populations()

    def owned_vertex_table(self, t=0):
        """(cell id, vertex id, position) of the vertices whose nearest node lies in this slab"""
        pos = self.cells.positions
        ids = self.cells.cell_ids()
        f, n = self.cells.type_range(t)
        nv = self.cells.types[t].nv
        p = pos[f:f + n * nv].reshape(n, nv, 3)
        first = sum(self.cells.type_range(u)[1] for u in range(t))
        cid = ids[first:first + n]
        g = np.floor(p[:, :, 0] + 0.5).astype(np.int64) - self.x0
        own = (g >= 0) & (g < self.nx)
        ci, vi = np.nonzero(own)
        return cid[ci], vi, p[ci, vi]
