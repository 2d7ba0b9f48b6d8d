"""The pre-inlet's cells on the GPU (csrc/preinlet.hip: hcp_preinlet_*, hc_preinlet_iterate; host.PreInlet(cells=...)) against the
numpy restatement tests/preinlet_cells_ref.py on the record API.  Every comparison of positions, velocities, forces and
populations is bit for bit: the select kernel reduces with fmin / fmax, which are exact, and the copy adds one double per
coordinate in the restatement's operand order."""
import ctypes as C

import numpy as np
import pytest

import open_boundary_axis_ref as AX
import preinlet_cells_ref as PC

pytestmark = pytest.mark.gpu

NONPER = (False, False, False)
DIRECTIONS = {"Xneg": (0, -1), "Xpos": (0, 1), "Yneg": (1, -1), "Ypos": (1, 1), "Zneg": (2, -1), "Zpos": (2, 1)}
STRIDE = 1000
FIELDS = ("position", "v", "force", "force_repulsion", "cellId", "vertexId", "restime", "celltype")


@pytest.fixture(autouse=True)
def _reproducible_spread(gpu):
    lib = gpu.capi.lib()
    gpu.check(lib.hc_set_reproducible_spread(1))
    try:
        yield
    finally:
        gpu.check(lib.hc_set_reproducible_spread(0))


def _same(a, b):
    """two record arrays equal field by field, bit for bit (floats compared as bits, so -0.0 and NaN count)"""
    if len(a) != len(b):
        return False
    for f in FIELDS:
        x, y = np.ascontiguousarray(a[f]), np.ascontiguousarray(b[f])
        if x.dtype.kind == "f":
            x, y = x.view(np.uint64), y.view(np.uint64)
        if not np.array_equal(x, y):
            return False
    return True


def _dims(axis, n_axis, n_a, n_b):
    d = [0, 0, 0]
    others = [a for a in range(3) if a != axis]
    d[axis], d[others[0]], d[others[1]] = n_axis, n_a, n_b
    return tuple(d)


def _rows(cells, t, slot):
    """the rows of cell (type t, slot) in positions / velocities / forces"""
    first, _ = cells.type_range(t)
    nv = cells.types[t].nv
    return slice(first + slot * nv, first + (slot + 1) * nv)


class _System:
    """a pre-inlet (periodic along the direction's axis, walled across) and a domain (walled across, its far face a pressure
    outlet) of the same cross-section with their cell containers, coupled by host.PreInlet(device=True, cells=...)"""

    def __init__(self, gpu, direction, pre_dims, dom_dims, kinds, window, shift, sink=None, cells_every=1, u0=None,
                 with_cells=True):
        self.gpu, self.direction = gpu, direction
        self.axis, self.sign = DIRECTIONS[direction]
        axis = self.axis
        self.pre_dims, self.dom_dims, self.window, self.shift = pre_dims, dom_dims, window, shift
        self.P = gpu.base_parameters()
        omega = 1.0 / self.P.tau
        self.pre = self.dom = self.pc = self.dc = self.coupling = None
        self.types = []
        try:
            self.pmask, self.dmask = AX.channel_mask(pre_dims, axis), AX.channel_mask(dom_dims, axis)
            self.pre = gpu.Lattice(*pre_dims, tuple(a == axis for a in range(3)), omega)
            self.dom = gpu.Lattice(*dom_dims, NONPER, omega)
            u = (0.0, 0.0, 0.0) if u0 is None else u0
            self.pre.defineBounceBack(self.pmask); self.pre.latticeEquilibrium(1.0, u)
            self.dom.defineBounceBack(self.dmask); self.dom.latticeEquilibrium(1.0, u)
            self.types = [getattr(gpu.CellType, k)(self.P) for k in kinds]
            self.nv = {t: ct.nv for t, ct in enumerate(self.types)}
            self.pc, self.dc = gpu.Cells(self.pre, self.P), gpu.Cells(self.dom, self.P)
            for ct in self.types:
                self.pc.addCellType(ct, 1); self.dc.addCellType(ct, 1)
            la, lb = np.nonzero(np.take(self.pmask, 0, axis=axis) == 0)
            self.g = np.stack([la, lb], axis=1)
            self.pre_plane = pre_dims[axis] - 1 if self.sign < 0 else 0
            self.dom_plane = 0 if self.sign < 0 else dom_dims[axis] - 1
            kw = dict(cells=(self.pc, self.dc), window=window, shift=shift, id_stride=STRIDE, sink=sink,
                      cells_every=cells_every) if with_cells else {}
            self.coupling = gpu.PreInlet(self.pre, self.dom, self.g, self.pre_plane, self.dom_plane, direction=direction,
                                         device=True, **kw)
            if u0 is not None:
                self.dom.setOpenBoundaryVelocitySlots(self.coupling.first, np.tile(np.asarray(u0, float), (len(self.g), 1)))
            box = [0, dom_dims[0] - 1, 0, dom_dims[1] - 1, 0, dom_dims[2] - 1]
            box[2 * axis] = box[2 * axis + 1] = dom_dims[axis] - 1 if self.sign < 0 else 0
            self.dom._add_open_box(1, -self.sign, box, axis)
        except Exception:
            self.destroy()
            raise

    def inject_ref(self, offered, dom_rec=None):
        """the restatement's injection on the containers' records as they are"""
        return PC.inject(self.pc.records(), self.dc.records() if dom_rec is None else dom_rec, self.nv, self.axis, self.sign,
                         self.pre_dims[self.axis], self.window, self.shift, STRIDE, self.dom_dims, offered)

    def step(self, it, fluid=True):
        """one iteration of the reference driver's loop through the separate entry points; returns the advanced iteration"""
        lib = self.gpu.capi.lib()
        for L, cells in ((self.pre, self.pc), (self.dom, self.dc)):
            i = C.c_long(it)
            self.gpu.check(lib.hc_iterate(L.ptr, cells.ptr, C.byref(i), 1, 1, 1, 1))
            assert i.value == it + 1
        if fluid:
            self.coupling.applyPreInlet()
        return it + 1

    def destroy(self):
        if self.coupling is not None:
            self.coupling.destroy()
        for c in (self.pc, self.dc):
            if c is not None:
                c.destroy()
        for L in (self.pre, self.dom):
            if L is not None:
                L.destroy()
        for ct in self.types:
            ct.destroy()


def _randomise(cells, seed):
    """non-zero velocities and forces on every vertex"""
    rng = np.random.default_rng(seed)
    n = cells.counts()[0]
    cells.velocities = rng.uniform(-1e-3, 1e-3, size=(n, 3))
    cells.forces = rng.uniform(-1e-4, 1e-4, size=(n, 3))


# ---- 1: static selection and copy

PRE, DOM = (40, 34, 34), (48, 34, 34)
WINDOW, SHIFT = (10.0, 36.0), (-8.0, 6.0, 0.0)


def test_static_selection_and_copy(gpu):
    """pre-inlet 40 x 34 x 34 periodic in x, domain 48 x 34 x 34, RBC (type 0) and PLT (type 1).  Of five cells in the pre-inlet --
    an RBC in the window, a PLT in the window two laps on, a PLT across window_hi, a PLT before the window and a PLT in the
    window that the in-plane shift puts outside the domain -- exactly the first two arrive; then 70 more PLTs in the window,
    more than the 65 slots the domain's PLT region was allocated with for its one resident (n + n / 4 + 64), so the region
    grows through the host staging."""
    s = _System(gpu, "Xneg", PRE, DOM, ("rbc", "plt"), WINDOW, SHIFT)
    try:
        pc, dc, Lp = s.pc, s.dc, PRE[0]
        assert pc.addCell(0, (23.0, 13.0, 16.5), (90.0, 0.0, 0.0), cell_id=7)
        for cid, centre in ((11, (14.0, 12.0, 20.0)), (12, (36.0, 12.0, 12.0)), (13, (5.0, 14.0, 14.0)), (14, (20.0, 28.0, 16.0))):
            assert pc.addCell(1, centre, (10.0, 20.0, 30.0), cell_id=cid)
        pos = pc.positions
        pos[_rows(pc, 1, 0), 0] += 2 * Lp
        pc.positions = pos
        _randomise(pc, 3)
        assert dc.addCell(0, (30.0, 16.5, 16.5), (90.0, 0.0, 0.0), cell_id=1) and dc.addCell(1, (10.0, 12.0, 20.0), cell_id=2)
        _randomise(dc, 4)
        pre_rec, dom_rec = pc.records(), dc.records()
        # the five cases are what they are meant to be
        x = {int(i): r["position"][:, 0] for (t, i), r in PC.by_id(pre_rec).items()}
        y14 = PC.by_id(pre_rec)[(1, 14)]["position"][:, 1]
        assert WINDOW[0] < x[7].min() and x[7].max() < WINDOW[1]
        assert 2 * Lp + WINDOW[0] < x[11].min() and x[11].max() < 2 * Lp + WINDOW[1]
        assert x[12].min() < WINDOW[1] < x[12].max() and x[13].max() < WINDOW[0]
        assert WINDOW[0] < x[14].min() and x[14].max() < WINDOW[1] and y14.max() + SHIFT[1] > DOM[1] - 1
        offered = set()
        want, ids, rejected = s.inject_ref(offered)
        assert ids == [(0, 7 + STRIDE), (1, 11 + 3 * STRIDE)] and rejected == 1

        assert s.coupling.applyPreInletCells() == (2, 0)
        got = dc.records()
        assert _same(got, PC.canonical(want))
        cells = PC.by_id(got)
        assert sorted(cells) == [(0, 1), (0, 1007), (1, 2), (1, 3011)]
        src = PC.by_id(pre_rec)
        for (t, new), old, lap in (((0, 1007), 7, 0), ((1, 3011), 11, 2)):
            a, b = cells[(t, new)], src[(t, old)]
            assert np.array_equal(a["position"][:, 0], b["position"][:, 0] + (np.float64(SHIFT[0]) - np.float64(lap) * np.float64(Lp)))
            assert np.array_equal(a["position"][:, 1], b["position"][:, 1] + SHIFT[1])
            assert np.array_equal(a["position"][:, 2], b["position"][:, 2] + SHIFT[2])
            assert np.array_equal(a["v"], b["v"]) and np.array_equal(a["force"], b["force"])
            assert np.all(a["v"] != 0.0) and np.all(a["force"] != 0.0)
        residents = PC.by_id(dom_rec)
        assert _same(cells[(0, 1)], residents[(0, 1)]) and _same(cells[(1, 2)], residents[(1, 2)])
        assert dc.alive().all() and dc.deletion_counts()[2] == 0
        assert _same(pc.records(), pre_rec)   # the pre-inlet keeps its cells
        assert s.coupling.cell_counts() == (2, 1, 0, 1)
        # a second check injects nothing
        assert s.coupling.applyPreInletCells() == (0, 0)
        assert s.coupling.cell_counts() == (2, 1, 0, 2)
        assert _same(dc.records(), got)

        # the slow path: 70 PLTs at once into a region of 65 slots that holds 2
        rng = np.random.default_rng(9)
        for k in range(70):
            assert pc.addCell(1, (20.0, 14.0, 14.0), (10.0, 20.0, 30.0), cell_id=300 + k)
        pos = pc.positions
        for k in range(70):
            pos[_rows(pc, 1, 4 + k)] += rng.uniform(-3.0, 3.0, size=3) * (1.0, 0.5, 1.0)
        pc.positions = pos
        vel, frc = pc.velocities, pc.forces
        tail = slice(_rows(pc, 1, 4).start, None)
        vel[tail] = rng.uniform(-1e-3, 1e-3, size=vel[tail].shape); frc[tail] = rng.uniform(-1e-4, 1e-4, size=frc[tail].shape)
        pc.velocities = vel; pc.forces = frc
        want2, ids2, rejected2 = s.inject_ref(offered, got)
        assert ids2 == [(1, 300 + k + STRIDE) for k in range(70)] and rejected2 == 0
        assert s.coupling.applyPreInletCells() == (70, 0)
        got2 = dc.records()
        assert _same(got2, PC.canonical(want2))
        after = PC.by_id(got2)
        for key in cells:   # the residents and the earlier arrivals survive the growth
            assert _same(after[key], cells[key]), key
        assert dc.counts()[1] == 74 and dc.alive().all()
        assert s.coupling.cell_counts() == (72, 1, 0, 3)
        assert s.coupling.applyPreInletCells() == (0, 0)
        assert _same(dc.records(), got2)
    finally:
        s.destroy()


# ---- 2: every direction

@pytest.mark.parametrize("direction, laps", [("Xpos", (-1, 0, -3)), ("Yneg", (0, 2, 1)), ("Zpos", (-2, -1, 0))])
def test_every_direction(gpu, direction, laps):
    """PLTs only, boxes of 11 x 12 across and 13 along the axis, the pre-inlet periodic on that axis: three PLTs in the window at
    the given laps (negative ones for *pos) arrive with id' = id + (lap - orientation) * stride and the restatement's bits; a
    fourth across the lap boundary does not"""
    axis, sign = DIRECTIONS[direction]
    dims = _dims(axis, 13, 11, 12)
    window = (2.0, 11.5)
    shift = [0.25, -0.5, 0.125]; shift[axis] = 0.5
    s = _System(gpu, direction, dims, dims, ("plt",), window, tuple(shift))
    try:
        centre = [5.0, 5.5, 5.5]; centre[axis] = 6.5
        edge = list(centre); edge[axis] = 12.5
        for k in range(3):
            assert s.pc.addCell(0, centre, (10.0, 20.0, 30.0), cell_id=5000 + k)
        assert s.pc.addCell(0, edge, (10.0, 20.0, 30.0), cell_id=5003)
        pos = s.pc.positions
        for k, lap in enumerate(laps):
            pos[_rows(s.pc, 0, k), axis] += lap * 13 + 0.5 * k
        pos[_rows(s.pc, 0, 3), axis] += laps[0] * 13
        s.pc.positions = pos
        _randomise(s.pc, 21)
        assert s.dc.addCell(0, centre, cell_id=1)
        _randomise(s.dc, 22)
        dom_rec = s.dc.records()
        want, ids, rejected = s.inject_ref(set())
        assert ids == [(0, 5000 + k + (lap - sign) * STRIDE) for k, lap in enumerate(laps)] and rejected == 0
        assert s.coupling.applyPreInletCells() == (3, 0)
        got = s.dc.records()
        assert _same(got, PC.canonical(want))
        assert list(s.dc.cell_ids()) == [1] + [i for _, i in ids]
        cells = PC.by_id(got)
        assert _same(cells[(0, 1)], PC.by_id(dom_rec)[(0, 1)])
        for _, i in ids:
            p = cells[(0, i)]["position"]
            assert np.all(p.min(axis=0) >= 0.0) and np.all(p.max(axis=0) <= np.array(dims) - 1.0)
        assert s.coupling.cell_counts() == (3, 0, 0, 1)
        assert s.coupling.applyPreInletCells() == (0, 0) and _same(s.dc.records(), got)
    finally:
        s.destroy()


# ---- 3: coupled run, device against restatement

U0 = (0.04, 0.0, 0.0)
C_WINDOW, C_SHIFT, N_ITER, EVERY = (12.0, 34.0), (-10.0, 0.0, 0.0), 30, 2


def _coupled(gpu, with_cells):
    s = _System(gpu, "Xneg", PRE, DOM, ("rbc", "plt"), C_WINDOW, C_SHIFT, cells_every=EVERY, u0=U0, with_cells=with_cells)
    try:
        assert s.pc.addCell(1, (16.0, 16.5, 16.5), (10.0, 20.0, 30.0), cell_id=40)
        pos = s.pc.positions
        pos[:, 0] -= pos[:, 0].min() - (C_WINDOW[0] - 0.3)   # the trailing edge starts 0.3 nodes upstream of window_lo
        s.pc.positions = pos
        assert s.dc.addCell(0, (30.0, 16.5, 16.5), (90.0, 0.0, 0.0), cell_id=1)
        for c in (s.pc, s.dc):
            c.applyConstitutiveModel(0, True)
    except Exception:
        s.destroy()
        raise
    return s


def _state(s):
    return s.pre.populations(), s.dom.populations(), s.pc.records(), s.dc.records()


def test_coupled_run_device_against_restatement(gpu):
    """the lattices of test 1 with a 0N velocity inlet fed by the fluid coupling and a 0P pressure outlet, both at equilibrium
    with u_x = 0.04; a PLT in the pre-inlet whose trailing edge starts 0.3 nodes upstream of window_lo, an RBC resident in the
    domain, cells checked every 2nd iteration, 30 iterations.  Run A: hc_preinlet_iterate, once iteration by iteration and once
    as one call.  Run B: fresh objects and the loop hc_iterate(pre), hc_iterate(domain), fluid apply, and at the same
    iterations the restatement through records() / set_records()."""
    a = _coupled(gpu, True)
    a1 = b = None
    try:
        injected_at = None
        for i in range(N_ITER):
            assert a.coupling.iterate(1) is None and a.coupling.iter == i + 1
            if injected_at is None and a.coupling.cell_counts()[0] == 1:
                injected_at = i + 1
        assert a.coupling.cell_counts() == (1, 0, 0, N_ITER // EVERY)
        A = _state(a)
        a1 = _coupled(gpu, True)
        a1.coupling.iterate(N_ITER)
        assert a1.coupling.iter == N_ITER and a1.coupling.cell_counts() == (1, 0, 0, N_ITER // EVERY)
        A1 = _state(a1)

        b = _coupled(gpu, False)
        offered, it, ref_at = set(), 0, None
        for i in range(N_ITER):
            it = b.step(it)
            if it % EVERY == 0:
                new, ids, rejected = b.inject_ref(offered)
                assert rejected == 0
                if ids:
                    assert ids == [(1, 40 + STRIDE)] and ref_at is None
                    ref_at = it
                    b.dc.set_records(PC.canonical(new))
        B = _state(b)
        print("injected at iteration %s (device) / %s (restatement) of %d" % (injected_at, ref_at, N_ITER))
        assert injected_at == ref_at
        assert 0 < ref_at < N_ITER and ref_at % EVERY == 0
        for name, X in (("iteration by iteration", A), ("one call", A1)):
            for k in (0, 1):
                assert np.isfinite(B[k]).all()
                assert np.array_equal(X[k], B[k]), (name, "populations", k)
            for k, cells in ((2, b.pc), (3, b.dc)):
                assert cells.alive().all() and cells.deletion_counts()[2] == 0
                gb, gx = PC.by_id(B[k]), PC.by_id(X[k])
                assert sorted(gb) == sorted(gx), (name, k)
                for key in gb:
                    assert np.isfinite(gb[key]["position"]).all() and np.isfinite(gb[key]["force"]).all()
                    assert len(gb[key]) == b.nv[key[0]]
                    assert _same(gx[key], gb[key]), (name, k, key)
            assert sorted(PC.by_id(X[3])) == [(0, 1), (1, 40 + STRIDE)]   # exactly one more cell than the domain started with
        assert a.dc.alive().all() and a.pc.alive().all() and a.dc.counts()[1] == 2 == b.dc.counts()[1] and b.pc.counts()[1] == 1
        # the arrival moved on with the domain's fluid
        arrived = PC.by_id(B[3])[(1, 40 + STRIDE)]["position"][:, 0]
        origin = PC.by_id(B[2])[(1, 40)]["position"][:, 0]
        assert arrived.mean() > C_WINDOW[0] + C_SHIFT[0] and not np.array_equal(arrived, origin + C_SHIFT[0])
    finally:
        for s in (a, a1, b):
            if s is not None:
                s.destroy()


# ---- 4: the sink

SINK_PLANE = 40.0


def _sink_system(gpu, sink):
    s = _System(gpu, "Xneg", (13, 34, 34), DOM, ("rbc", "plt"), (1.0, 12.0), (0.0, 0.0, 0.0), sink=sink, u0=(0.05, 0.0, 0.0))
    try:
        assert s.dc.addCell(1, (35.0, 16.5, 16.5), (10.0, 20.0, 30.0), cell_id=5)
        assert s.dc.addCell(1, (14.0, 16.5, 16.5), (10.0, 20.0, 30.0), cell_id=6)
        pos = s.dc.positions
        rows = _rows(s.dc, 1, 0)
        pos[rows, 0] -= pos[rows, 0].max() - (SINK_PLANE - 2.0)   # two nodes upstream of the plane
        s.dc.positions = pos
        s.dc.applyConstitutiveModel(0, True)
    except Exception:
        s.destroy()
        raise
    return s


def _domain_step(s, it):
    i = C.c_long(it)
    s.gpu.check(s.gpu.capi.lib().hc_iterate(s.dom.ptr, s.dc.ptr, C.byref(i), 1, 1, 1, 1))
    return i.value


def test_sink(gpu):
    """a domain with a uniform inflow of 0.05: a PLT two nodes upstream of the sink plane drifts across it, a second PLT sits
    mid-channel.  Without a check nothing is removed; the crossing iteration k is read off that run.  With the sink, checked
    after every iteration, the first PLT goes at iteration k, and 5 iterations later -- before its absence can have reached
    the second PLT, 19 nodes upstream, at one node per iteration -- the second equals the undisturbed run bit for bit.  With
    the sink off both remain."""
    ref = _sink_system(gpu, None)
    on = off = None
    try:
        it, k, states = 0, None, {}
        for _ in range(80):
            it = _domain_step(ref, it)
            rec = ref.dc.records()
            if k is None and PC.by_id(rec)[(1, 5)]["position"][:, 0].max() > SINK_PLANE:
                k = it
            if k is not None and it == k + 5:
                break
        assert k is not None and 10 < k and it == k + 5, (k, it)
        want = PC.by_id(rec)
        assert sorted(want) == [(1, 5), (1, 6)] and ref.dc.alive().all()
        assert want[(1, 6)]["position"][:, 0].max() < SINK_PLANE - 19.0
        print("the PLT crosses the sink plane at iteration %d" % k)

        on = _sink_system(gpu, SINK_PLANE)
        it, removed_at = 0, None
        for _ in range(k + 5):
            it = _domain_step(on, it)
            inj, rem = on.coupling.applyPreInletCells()
            assert inj == 0
            if rem:
                assert rem == 1 and removed_at is None
                removed_at = it
        assert removed_at == k
        got = PC.by_id(on.dc.records())
        assert sorted(got) == [(1, 6)] and _same(got[(1, 6)], want[(1, 6)])
        assert on.coupling.cell_counts() == (0, 0, 1, k + 5)
        assert list(on.dc.cell_ids()) == [6] and on.dc.alive().all() and on.dc.counts()[1] == 1

        off = _sink_system(gpu, None)
        it = 0
        for _ in range(k + 5):
            it = _domain_step(off, it)
            assert off.coupling.applyPreInletCells() == (0, 0)
        got = PC.by_id(off.dc.records())
        assert sorted(got) == [(1, 5), (1, 6)] and _same(got[(1, 5)], want[(1, 5)]) and _same(got[(1, 6)], want[(1, 6)])
        assert off.coupling.cell_counts() == (0, 0, 0, k + 5)
        assert np.array_equal(off.dom.populations(), ref.dom.populations())
    finally:
        for s in (ref, on, off):
            if s is not None:
                s.destroy()


# ---- 5: refusals

def _create(gpu, pre, dom, axis=0, orientation=-1, lo=2.0, hi=11.0, shift=(0.5, 0.0, 0.0), stride=STRIDE):
    ptr = C.c_void_p()
    sh = np.array(shift, dtype=np.float64)
    rc = gpu.capi.lib().hcp_preinlet_create(C.byref(ptr), pre.ptr, dom.ptr, int(axis), int(orientation), float(lo), float(hi),
                                             gpu.dptr(sh), int(stride))
    assert (rc == 0) == bool(ptr.value)   # a refused call hands out nothing
    gpu.check(rc)
    return ptr


def test_refusals(gpu):
    lib = gpu.capi.lib()
    dims = (13, 11, 12)
    s = _System(gpu, "Xneg", dims, dims, ("plt",), (2.0, 11.0), (0.5, 0.0, 0.0))
    extra = []
    try:
        P = s.P
        plt, rbc, rbc_small = s.types[0], gpu.CellType.rbc(P), gpu.CellType.rbc(P, min_triangles=300)
        extra += [rbc, rbc_small]
        assert rbc.nv != rbc_small.nv
        assert s.pc.addCell(0, (6.5, 5.0, 5.5), (10.0, 20.0, 30.0), cell_id=5000)
        assert s.dc.addCell(0, (6.5, 5.0, 5.5), cell_id=1)
        slab = gpu.Lattice(8, 11, 12, (True, True, True), 1.0, x0=0, nx_global=16, n_slabs=2); extra.append(slab)
        walled = gpu.Lattice(*dims, NONPER, 1.0); extra.append(walled)

        def container(L, types, repulsion=False):
            c = gpu.Cells(L, P); extra.insert(0, c)
            for t in types:
                c.addCellType(t, 1)
            if repulsion:
                c.setRepulsion(1e-3, 0.5, 1)
            return c

        before = (s.pc.counts(), s.dc.counts(), s.coupling.cell_counts())
        assert before[2] == (0, 0, 0, 0)
        ok = _create(gpu, s.pc, s.dc)
        gpu.check(lib.hcp_preinlet_destroy(ok))
        for pre, dom, match in ((container(slab, [plt]), s.dc, "n_slabs = 1"), (s.pc, container(slab, [plt]), "n_slabs = 1"),
                                (container(walled, [plt]), s.dc, "periodic"),
                                (s.pc, container(s.dom, [plt, rbc]), "numbers of cell types"),
                                (s.pc, container(s.dom, [rbc]), "model or vertices"),
                                (container(s.pre, [rbc]), container(s.dom, [rbc_small]), "model or vertices"),
                                (s.pc, container(s.dom, [plt], repulsion=True), "one container only"),
                                (container(s.pre, [plt], repulsion=True), s.dc, "one container only")):
            with pytest.raises(gpu.HcError, match=match):
                _create(gpu, pre, dom)
        with pytest.raises(gpu.HcError, match="periodic"):
            _create(gpu, s.pc, s.dc, axis=1)   # the pre-inlet is walled in y
        for lo, hi in ((-0.5, 11.0), (2.0, 13.5), (6.0, 6.0), (7.0, 6.0)):
            with pytest.raises(gpu.HcError, match="window"):
                _create(gpu, s.pc, s.dc, lo=lo, hi=hi)
        gpu.check(lib.hcp_preinlet_destroy(_create(gpu, s.pc, s.dc, lo=0.0, hi=13.0)))   # the whole box is a window
        for stride in (0, -5):
            with pytest.raises(gpu.HcError, match="id_stride"):
                _create(gpu, s.pc, s.dc, stride=stride)
        for axis in (-1, 3):
            with pytest.raises(gpu.HcError, match="axis must be"):
                _create(gpu, s.pc, s.dc, axis=axis)
        with pytest.raises(gpu.HcError, match="orientation"):
            _create(gpu, s.pc, s.dc, orientation=0)
        # cells_every < 1: nothing steps
        S_pre, S_dom = s.pre.populations(), s.dom.populations()
        for every in (0, -2):
            it = C.c_long(0)
            rc = lib.hc_preinlet_iterate(s.coupling.ptr, s.coupling.cells_ptr, C.byref(it), 3, 1, 1, 1, every)
            assert rc != 0 and it.value == 0
            with pytest.raises(gpu.HcError, match="cells_every"):
                gpu.check(rc)
        with pytest.raises(gpu.HcError, match="cells= needs device=True"):
            gpu.PreInlet(s.pre, s.dom, s.g, 12, 0, direction="Xneg", cells=(s.pc, s.dc), window=(2.0, 11.0), id_stride=STRIDE)
        assert (s.pc.counts(), s.dc.counts(), s.coupling.cell_counts()) == before
        assert np.array_equal(s.pre.populations(), S_pre) and np.array_equal(s.dom.populations(), S_dom)
        # the fluid handle is the one it was: hcl_preinlet_iterate still runs, and so does the whole iteration
        gpu.check(lib.hcl_preinlet_iterate(s.coupling.ptr, 2))
        assert np.isfinite(s.dom.populations()).all() and s.coupling.cell_counts() == before[2]
        s.coupling.iterate(2)
        assert s.coupling.iter == 2 and s.coupling.cell_counts() == (1, 0, 0, 2)
    finally:
        for c in extra:
            if isinstance(c, gpu.Cells):
                c.destroy()
        s.destroy()
        for c in extra:
            if not isinstance(c, gpu.Cells):
                c.destroy()
