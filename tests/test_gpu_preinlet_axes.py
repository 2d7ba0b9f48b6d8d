"""The pre-inlet's fluid coupling in the reference's six directions on the GPU: hcl_plane_velocity_axis on x, y and z planes, the
host path of host.PreInlet and the device path (hcl_preinlet_*), against numpy moments of the downloaded populations and the
restatements tests/open_boundary_ref.py and tests/open_boundary_axis_ref.py.

Every comparison of velocities and populations is bit for bit; the one bound, 1e-14 against the prescribed values on velocity
nodes, is that of the existing observer tests."""
import ctypes as C

import numpy as np
import pytest

import open_boundary_axis_ref as AX
import open_boundary_ref as OB

pytestmark = pytest.mark.gpu

NONPER = (False, False, False)
DIRECTIONS = {"Xneg": (0, -1), "Xpos": (0, 1), "Yneg": (1, -1), "Ypos": (1, 1), "Zneg": (2, -1), "Zpos": (2, 1)}


def _others(axis):
    return [a for a in range(3) if a != axis]


def _dims(axis, n_axis, n_a, n_b):
    """extents with n_axis along `axis` and (n_a, n_b) along the two other axes in ascending axis order"""
    d = [0, 0, 0]
    d[axis] = n_axis
    d[_others(axis)[0]], d[_others(axis)[1]] = n_a, n_b
    return tuple(d)


def _plane(A, axis, plane):
    """the plane coordinate[axis] == plane of A [nx][ny][nz][...], flattened in the in-plane index order of
    hcl_plane_velocity_axis: the axis removed, the remaining axes in lattice order"""
    P = np.take(A, plane, axis=axis)
    return P.reshape((P.shape[0] * P.shape[1],) + P.shape[2:])


def _plane_velocity_ref(S, mask, axis, plane, idx, body):
    """_plane_velocity_ref of tests/test_gpu_preinlet.py for any axis: the kernels' moments() and u = j / rho + F / 2 on the
    listed nodes of a plane of the post-stream state S [nx][ny][nz][19]; bounce-back nodes answer 0"""
    idx = np.asarray(idx, dtype=np.int64)
    f = _plane(S, axis, plane)[idx]
    r = np.zeros(len(idx)); j = [np.zeros(len(idx)) for _ in range(3)]
    for q in range(19):
        r = r + f[:, q]
        for d in range(3):
            if OB.C[q][d] == 1: j[d] = j[d] + f[:, q]
            elif OB.C[q][d] == -1: j[d] = j[d] + (-f[:, q])
    invRho = 1.0 / (1.0 + r)
    u = np.stack([j[d] * invRho + body[d] / 2.0 for d in range(3)], axis=1)
    u[_plane(mask, axis, plane)[idx] != 0] = 0.0
    return u


# ---- 1: plane velocity on every axis, bit for bit

BOX = (11, 12, 13)
BOX_BODY = (2e-6, -3e-6, 1.5e-6)


@pytest.mark.parametrize("periodic_axis, padding", [(0, 0), (1, 0), (2, 0), (1, 1), (1, -1)])
def test_plane_velocity_on_every_axis(gpu, periodic_axis, padding):
    """an 11 x 12 x 13 box walled on two axes and periodic on the third, body force with three non-zero components, random
    populations, 5 steps: planes 0, 5 and last of every axis, the whole plane, a shuffled list with a repeated index, n = 1 and
    n = 0; bounce-back nodes answer exactly 0 (the first and last plane of a walled axis are bounce-back throughout); axis 0 is
    planeVelocity.  Once more with the planes padded and unpadded."""
    lib = gpu.capi.lib()
    per = tuple(a == periodic_axis for a in range(3))
    mask = AX.channel_mask(BOX, periodic_axis)
    gpu.check(lib.hc_debug_force_plane_padding(padding))
    L = None
    try:
        L = gpu.Lattice(*BOX, per, 1.0 / 0.8)
        L.defineBounceBack(mask)
        L.setExternalVector(BOX_BODY)
        L.set_populations(np.random.default_rng(31).uniform(-0.005, 0.005, size=(L.n, 19)))
        L.collideAndStream(5)
        S = L.populations().reshape(BOX + (19,))
        assert np.isfinite(S).all()
        rng = np.random.default_rng(5)
        for axis in range(3):
            size = BOX[_others(axis)[0]] * BOX[_others(axis)[1]]
            assert size % 256 != 0
            for plane in (0, 5, BOX[axis] - 1):
                whole = np.arange(size)
                want = _plane_velocity_ref(S, mask, axis, plane, whole, BOX_BODY)
                solid = _plane(mask, axis, plane) != 0
                # planes 0 and last of a walled axis are bounce-back throughout; every other plane holds walls and fluid
                assert solid.any() and (~solid).any() == (axis == periodic_axis or plane == 5)
                assert np.all(want[~solid] != 0.0) and np.all(want[solid] == 0.0)
                got = L.planeVelocityAxis(axis, plane, whole)
                assert np.array_equal(got, want), (axis, plane)
                assert np.all(got[solid] == 0.0)
                shuffled = rng.permutation(size)
                shuffled = np.concatenate([shuffled[:40], shuffled[7:8], shuffled[40:]])   # one index twice
                assert np.array_equal(L.planeVelocityAxis(axis, plane, shuffled), want[shuffled]), (axis, plane)
                one = [int(np.flatnonzero(~solid)[3])] if (~solid).any() else [size - 1]
                assert np.array_equal(L.planeVelocityAxis(axis, plane, one), want[one])
                assert L.planeVelocityAxis(axis, plane, []).shape == (0, 3)
                if axis == 0:
                    assert np.array_equal(L.planeVelocity(plane, whole), got)
    finally:
        gpu.check(lib.hc_debug_force_plane_padding(0))
        if L is not None:
            L.destroy()


# ---- 2: planes of an open lattice report completed moments

FACADE = {(k, a): "add%sBoundary%d%s" % ("Velocity" if k in (OB.VEL_0N, OB.VEL_0P) else "Pressure", a,
                                         "N" if k in (OB.VEL_0N, OB.PRES_0N) else "P") for k in range(4) for a in range(3)}


@pytest.mark.parametrize("axis", [1, 2])
def test_planes_of_an_open_lattice_report_completed_moments(gpu, axis):
    """the walled y and z channels of open_boundary_axis_ref with a velocity N inlet plane and a pressure P outlet: the inlet
    plane itself, the plane next to it and an x plane that crosses both faces equal AX.observe() bit for bit; velocity nodes
    report u_bc + F / 2 to 1e-14"""
    dims = AX.CHANNEL_DIMS[axis]
    mask, patches = AX.channel_mask(dims, axis), AX.channel_patches("original", axis, dims)
    code, axes, val = AX.declaration(dims, patches)
    L = gpu.Lattice(*dims, NONPER, AX.OMEGA)
    try:
        L.defineBounceBack(mask)
        L.setExternalVector(AX.BODY)
        for kind, a, box, values in patches:
            first, n = getattr(L, FACADE[(kind, a)])(box)
            (L.setOpenBoundaryVelocitySlots if kind in (OB.VEL_0N, OB.VEL_0P) else L.setOpenBoundaryDensitySlots)(first, values)
        assert np.array_equal(L.openBoundaryValues(0, len(val)), val)
        L.set_populations(AX.initial_state(dims).reshape(-1, 19))
        L.collideAndStream(7)
        S = L.populations().reshape(dims + (19,))
        assert np.isfinite(S).all()
        rho_ref, u_ref, _ = AX.observe(S, mask, NONPER, AX.BODY, None, code, axes, val)
        assert float(np.abs(rho_ref[mask == 0] - 1.0).max()) < 0.1
        _, u_plain, _ = OB.observe(S, mask, NONPER, AX.BODY)
        half = np.asarray(AX.BODY, np.longdouble) / 2
        for a, plane in ((axis, 0), (axis, 1), (0, dims[0] // 2)):
            fluid = _plane(mask, a, plane) == 0
            idx = np.flatnonzero(fluid)
            want = _plane(u_ref, a, plane)[idx]
            got = L.planeVelocityAxis(a, plane, idx)
            assert np.array_equal(got, want), (a, plane)
            c = _plane(code, a, plane)[idx]
            if (a, plane) != (axis, 1):
                assert (c >= 0).any() and not np.array_equal(want, _plane(u_plain, a, plane)[idx])   # the plane holds open nodes
            vel = (c >= 0) & ((c & 3) == OB.VEL_0N)
            if (a, plane) == (axis, 0):
                assert vel.all()
            if vel.any():
                err = np.abs(got[vel].astype(np.longdouble) - (val[c[vel] >> 2][:, :3].astype(np.longdouble) + half))
                print("axis %d plane %d: largest error against u_bc + F / 2 %.3e" % (a, plane, float(err.max())))
                assert float(err.max()) <= 1e-14
            walls = np.flatnonzero(~fluid)[:9]
            assert np.all(L.planeVelocityAxis(a, plane, walls) == 0.0)
    finally:
        L.destroy()


# ---- 3, 4: the coupling

OMEGA_C = 1.0
N_PRE = 12


def _driving(gpu, direction, pre_dims, axis):
    """the vector of host.preinlet_driving_force_vector for the pre-inlet's fluid cross-section, scaled to a magnitude of 1e-5"""
    area = int((AX.channel_mask(pre_dims, axis).take(0, axis=axis) == 0).sum())
    _, _, F = gpu.preinlet_driving_force_vector(0.5, 1.0 / 6.0, area, direction)
    return tuple(float(v) / abs(F[axis]) * 1e-5 for v in F)


class _Pair:
    """a pre-inlet (10 planes along the axis, 12 x 12 across, periodic along the axis, walled across, driven) and a domain (20
    planes along the axis, dom_n x dom_n across, walled across) coupled in `direction`, the domain's far face a pressure outlet.
    The pre-inlet's in-plane origin is global `origin`, the domain's (0, 0)."""

    def __init__(self, gpu, direction, dom_n, origin, device, pre_seed=None):
        self.axis, self.sign = DIRECTIONS[direction]
        axis = self.axis
        self.pre_dims, self.dom_dims = _dims(axis, 10, N_PRE, N_PRE), _dims(axis, 20, dom_n, dom_n)
        self.F = _driving(gpu, direction, self.pre_dims, axis)
        assert self.F[axis] * self.sign < 0 and abs(self.F[axis]) == 1e-5 and sum(v != 0.0 for v in self.F) == 1
        self.pre_per = tuple(a == axis for a in range(3))
        self.pmask, self.dmask = AX.channel_mask(self.pre_dims, axis), AX.channel_mask(self.dom_dims, axis)
        self.pre = gpu.Lattice(*self.pre_dims, self.pre_per, OMEGA_C)
        self.dom = gpu.Lattice(*self.dom_dims, NONPER, OMEGA_C)
        self.coupling = None
        try:
            self.pre.defineBounceBack(self.pmask); self.pre.setExternalVector(self.F); self.pre.latticeEquilibrium()
            if pre_seed is not None:
                self.pre.set_populations(np.random.default_rng(pre_seed).uniform(-0.003, 0.003, size=(self.pre.n, 19)))
            self.dom.defineBounceBack(self.dmask); self.dom.latticeEquilibrium()
            la, lb = np.nonzero(np.take(self.pmask, 0, axis=axis) == 0)
            self.local = (la, lb)
            self.g = np.stack([la + origin[0], lb + origin[1]], axis=1)   # global in-plane coordinates of the pre-inlet's fluid nodes
            self.n = len(self.g)
            # *neg: the pre-inlet's last plane feeds the domain's plane 0; *pos: its plane 0 feeds the domain's last plane
            self.pre_plane = self.pre_dims[axis] - 1 if self.sign < 0 else 0
            self.dom_plane = 0 if self.sign < 0 else self.dom_dims[axis] - 1
            self.out_plane = self.dom_dims[axis] - 1 if self.sign < 0 else 0
            self.coupling = gpu.PreInlet(self.pre, self.dom, self.g, self.pre_plane, self.dom_plane, direction=direction,
                                         pre_origin=origin, device=device)
            self.first = self.coupling.first
            self.pre_idx = la * N_PRE + lb
            box = [0, self.dom_dims[0] - 1, 0, self.dom_dims[1] - 1, 0, self.dom_dims[2] - 1]
            box[2 * axis] = box[2 * axis + 1] = self.out_plane
            self.fp, self.npres = self.dom._add_open_box(1, -self.sign, box, axis)
            # the declaration as the restatement wants it
            self.dom_nodes = np.empty((self.n, 3), np.int64)
            self.dom_nodes[:, axis] = self.dom_plane
            self.dom_nodes[:, _others(axis)[0]], self.dom_nodes[:, _others(axis)[1]] = self.g[:, 0], self.g[:, 1]
            self.code = -np.ones(self.dom_dims, np.int64)
            self.axes = -np.ones(self.dom_dims, np.int64)
            self.code[tuple(self.dom_nodes.T)] = (self.first + np.arange(self.n)) << 2 | (OB.VEL_0N if self.sign < 0 else OB.VEL_0P)
            out = [slice(None)] * 3; out[axis] = self.out_plane
            self.code[tuple(out)] = ((self.fp + np.arange(self.npres)) << 2 | (OB.PRES_0P if self.sign < 0 else OB.PRES_0N)).reshape(self.code[tuple(out)].shape)
            self.axes[self.code >= 0] = axis
            self.n_slots = self.first + self.n + self.npres
        except Exception:
            self.destroy()
            raise

    def pre_state(self):
        return self.pre.populations().reshape(self.pre_dims + (19,))

    def dom_state(self):
        return self.dom.populations().reshape(self.dom_dims + (19,))

    def plane_moments(self):
        return _plane_velocity_ref(self.pre_state(), self.pmask, self.axis, self.pre_plane, self.pre_idx, self.F)

    def destroy(self):
        if self.coupling is not None:
            self.coupling.destroy()
        self.pre.destroy(); self.dom.destroy()


COUPLINGS = [(d, 16, (2, 2)) for d in DIRECTIONS] + [(d, 12, (0, 0)) for d in ("Xneg", "Ypos", "Zneg")]


@pytest.mark.parametrize("direction, dom_n, origin", COUPLINGS)
def test_coupling_in_six_directions_host_path(gpu, direction, dom_n, origin):
    """test_preinlet_coupling_in_one_process of tests/test_gpu_preinlet.py with the axes permuted, and the equal cross-section
    case for one direction per axis: after every iteration the values sent are the pre-inlet's plane moments, the domain's
    slots hold them, and the domain's populations are one restated step from the state and the values BEFORE the iteration --
    the domain lags by one iteration.  The restated states stay finite with |rho - 1| < 0.1 on fluid nodes (checked beforehand
    with the restatement alone: at most 3.7e-4 over the 30 iterations of every case)."""
    p = _Pair(gpu, direction, dom_n, origin, device=False)
    try:
        axis, sign = p.axis, p.sign
        assert p.n == (N_PRE - 2) ** 2 and p.n % 256 != 0
        assert np.array_equal(p.dom.openBoundarySlots(p.dom_nodes), p.first + np.arange(p.n))
        assert np.array_equal(p.dom.openBoundaryAxes(p.dom_nodes), np.full(p.n, axis))
        assert np.all(p.dom.openBoundaryValues(p.first, p.n)[:, :3] == 0.0)   # starts at u = 0
        fluid = p.dmask == 0
        zero = (0.0, 0.0, 0.0)
        for it in range(30):
            S_dom = p.dom_state()
            val = p.dom.openBoundaryValues(0, p.n_slots)
            sent = p.coupling.iterate(1)
            assert np.array_equal(sent, p.plane_moments()), it
            assert np.array_equal(p.dom.openBoundaryValues(p.first, p.n)[:, :3], sent)
            assert np.array_equal(p.coupling.sent(), sent)
            want = AX.step(S_dom, p.dmask, NONPER, OMEGA_C, zero, p.code, p.axes, val)
            assert np.isfinite(want).all()
            rho, _, _ = AX.observe(want, p.dmask, NONPER, zero, None, p.code, p.axes, p.dom.openBoundaryValues(0, p.n_slots))
            assert float(np.abs(rho[fluid] - 1.0).max()) < 0.1, it
            got = p.dom_state()
            assert np.array_equal(got[fluid], want[fluid]), it
        assert sent[:, axis].mean() * sign < 0   # *neg drives along +axis
        _, u = p.dom.rho_u()
        two_in = p.dom_plane + 2 * (-sign)
        inflow = _plane(u.reshape(p.dom_dims + (3,)), axis, two_in)[_plane(p.dmask, axis, two_in) == 0][:, axis].mean()
        assert inflow * sign < 0   # the flow has entered the domain
        with pytest.raises(gpu.HcError, match="outside the pre-inlet"):
            gpu.PreInlet(p.pre, p.dom, p.g + 3, p.pre_plane, p.dom_plane + (1 if sign < 0 else -1), direction=direction, pre_origin=origin)
    finally:
        p.destroy()


@pytest.mark.parametrize("k", [1, 7])
@pytest.mark.parametrize("direction", ["Xneg", "Ypos", "Zneg"])
def test_device_path_equals_host_path(gpu, direction, k):
    """twin pairs from the same start (a pre-inlet with random populations, so the first exchange already carries velocities):
    k host iterations against one hcl_preinlet_iterate(k) -- populations of both lattices and every slot of the domain, rho
    included, bit for bit; applyPreInlet alone writes the pre-inlet's plane velocities"""
    host = _Pair(gpu, direction, 16, (2, 2), device=False, pre_seed=17)
    dev = None
    try:
        dev = _Pair(gpu, direction, 16, (2, 2), device=True, pre_seed=17)
        assert dev.coupling.ptr is not None and host.coupling.ptr is None
        assert np.array_equal(host.pre_state(), dev.pre_state())
        for _ in range(k):
            assert host.coupling.iterate(1) is not None
        assert dev.coupling.iterate(k) is None
        assert np.array_equal(host.pre_state(), dev.pre_state())
        assert np.array_equal(host.dom_state(), dev.dom_state())
        values = dev.dom.openBoundaryValues(0, dev.n_slots)
        assert np.array_equal(host.dom.openBoundaryValues(0, host.n_slots), values)
        assert np.any(values[dev.first:dev.first + dev.n, :3] != 0.0) and np.all(values[:, 3] == 1.0)
        assert np.array_equal(dev.coupling.sent(), dev.plane_moments())
        # apply alone: step the pre-inlet only, then hand over
        dev.pre.collideAndStream(2)
        before = dev.coupling.sent()
        assert dev.coupling.applyPreInlet() is None
        now = dev.pre.planeVelocityAxis(dev.axis, dev.pre_plane, dev.pre_idx)
        assert np.array_equal(dev.coupling.sent(), now) and not np.array_equal(now, before)
        assert np.array_equal(now, dev.plane_moments())
        after = dev.dom.openBoundaryValues(0, dev.n_slots)
        untouched = np.ones(dev.n_slots, bool); untouched[dev.first:dev.first + dev.n] = False
        assert np.array_equal(after[untouched], values[untouched]) and np.array_equal(after[:, 3], values[:, 3])
    finally:
        host.destroy()
        if dev is not None:
            dev.destroy()


# ---- 5: slot growth and clearing

def test_slot_growth_and_clearing(gpu):
    """The domain's slot storage holds exactly the n slots of its first declaration (capacity max(need, 2 * 0)), and grows to
    max(need, 2 * capacity) when a declaration does not fit: a further 16 x 16 = 256 > n pressure nodes exceed n as well as
    2 n, so the storage is reallocated after the handle was made, whatever the capacity was between those.  The handle must
    then write the new storage; after clearOpenBoundaries it must write nothing."""
    direction, axis = "Yneg", 1
    pre_dims, dom_dims = _dims(axis, 10, N_PRE, N_PRE), _dims(axis, 20, 16, 16)
    F = _driving(gpu, direction, pre_dims, axis)
    pmask, dmask = AX.channel_mask(pre_dims, axis), AX.channel_mask(dom_dims, axis)
    pre = gpu.Lattice(*pre_dims, (False, True, False), OMEGA_C)
    dom = gpu.Lattice(*dom_dims, NONPER, OMEGA_C)
    coupling = None
    try:
        pre.defineBounceBack(pmask); pre.setExternalVector(F)
        pre.set_populations(np.random.default_rng(23).uniform(-0.003, 0.003, size=(pre.n, 19)))
        dom.defineBounceBack(dmask); dom.latticeEquilibrium()
        la, lb = np.nonzero(pmask[:, 0, :] == 0)
        g = np.stack([la + 2, lb + 2], axis=1)
        coupling = gpu.PreInlet(pre, dom, g, pre_dims[axis] - 1, 0, direction=direction, pre_origin=(2, 2), device=True)
        n, idx = len(g), la * N_PRE + lb
        assert coupling.first == 0 and n == 100
        coupling.applyPreInlet()
        first_values = dom.openBoundaryValues(0, n)
        assert np.array_equal(first_values[:, :3], pre.planeVelocityAxis(axis, pre_dims[axis] - 1, idx))
        assert np.any(first_values[:, :3] != 0.0) and np.all(first_values[:, 3] == 1.0)
        fp, npres = dom.addPressureBoundary1P((0, 15, 19, 19, 0, 15))
        assert (fp, npres) == (n, 256) and npres > n
        dom.setOpenBoundaryDensitySlots(fp, np.full(npres, 1.01))
        assert np.array_equal(dom.openBoundaryValues(0, n), first_values)   # the earlier values moved with the storage
        pre.collideAndStream(3)
        coupling.applyPreInlet()
        values = dom.openBoundaryValues(0, n + npres)
        now = pre.planeVelocityAxis(axis, pre_dims[axis] - 1, idx)
        assert np.array_equal(values[:n, :3], now) and not np.array_equal(now, first_values[:, :3])
        assert np.all(values[:n, 3] == 1.0)
        assert np.all(values[n:] == np.array([0.0, 0.0, 0.0, 1.01]))
        coupling.iterate(2)   # ... and the whole iteration still runs
        assert np.array_equal(coupling.sent(), pre.planeVelocityAxis(axis, pre_dims[axis] - 1, idx))
        dom.clearOpenBoundaries()
        S_dom, S_pre = dom.populations(), pre.populations()
        with pytest.raises(gpu.HcError, match="no longer holds the coupled slots"):
            coupling.applyPreInlet()
        with pytest.raises(gpu.HcError, match="no longer holds the coupled slots"):
            coupling.iterate(3)
        assert np.array_equal(dom.populations(), S_dom) and np.array_equal(pre.populations(), S_pre)
        # nodes declared again since do not revive the handle: these slots are not the ones it was checked against
        assert dom.addPressureBoundary1P((0, 15, 19, 19, 0, 15)) == (0, 256)
        with pytest.raises(gpu.HcError, match="no longer holds the coupled slots"):
            coupling.applyPreInlet()
        assert np.all(dom.openBoundaryValues(0, 256) == np.array([0.0, 0.0, 0.0, 1.0]))
    finally:
        if coupling is not None:
            coupling.destroy()
        pre.destroy(); dom.destroy()


# ---- 6: refusals

def _create(gpu, pre, dom, axis, plane, idx, first):
    ptr = C.c_void_p()
    ii = np.ascontiguousarray(idx, dtype=np.int32)
    gpu.check(gpu.capi.lib().hcl_preinlet_create(C.byref(ptr), pre.ptr, dom.ptr, int(axis), int(plane),
                                                 ii.ctypes.data_as(C.POINTER(C.c_int)), len(ii), int(first)))
    return ptr


def test_refusals(gpu):
    L = gpu.Lattice(8, 6, 7, NONPER, 1.0)
    D = gpu.Lattice(8, 6, 7, NONPER, 1.0)
    S = gpu.Lattice(8, 6, 7, (True, True, True), 1.0, x0=0, nx_global=16, n_slabs=2)
    try:
        for axis in (3, -1):
            with pytest.raises(gpu.HcError, match="axis must be 0, 1 or 2"):
                L.planeVelocityAxis(axis, 0, [0])
        for axis, extent, size in ((0, 8, 42), (1, 6, 56), (2, 7, 48)):
            for plane in (-1, extent):
                with pytest.raises(gpu.HcError, match="plane outside the lattice"):
                    L.planeVelocityAxis(axis, plane, [0])
            with pytest.raises(gpu.HcError, match="in-plane index out of range"):
                L.planeVelocityAxis(axis, extent - 1, [0, size])
            with pytest.raises(gpu.HcError, match="in-plane index out of range"):
                L.planeVelocityAxis(axis, 0, [-1])
            assert L.planeVelocityAxis(axis, extent - 1, [size - 1]).shape == (1, 3)
        with pytest.raises(gpu.HcError, match="n_slabs = 1"):
            S.planeVelocityAxis(1, 0, [0])
        # the coupling object: velocity slots 0 .. 29 on the face y = 0 of D, pressure slots 30 .. 59 on y = 5
        fv, nv = D.addVelocityBoundary1N((1, 6, 0, 0, 1, 5))
        fp, npr = D.addPressureBoundary1P((1, 6, 5, 5, 1, 5))
        assert (fv, nv, fp, npr) == (0, 30, 30, 30)
        idx = np.arange(30)
        ok = _create(gpu, L, D, 1, 5, idx, 0)
        gpu.check(gpu.capi.lib().hcl_preinlet_destroy(ok))
        with pytest.raises(gpu.HcError, match="axis must be 0, 1 or 2"):
            _create(gpu, L, D, 3, 0, idx, 0)
        for plane in (-1, 6):
            with pytest.raises(gpu.HcError, match="plane outside the pre-inlet"):
                _create(gpu, L, D, 1, plane, idx, 0)
        with pytest.raises(gpu.HcError, match="in-plane index out of range"):
            _create(gpu, L, D, 1, 5, [0, 56], 0)
        with pytest.raises(gpu.HcError, match="n_slabs = 1"):
            _create(gpu, S, D, 1, 5, idx, 0)
        with pytest.raises(gpu.HcError, match="n_slabs = 1"):
            _create(gpu, L, S, 1, 5, [], 0)
        with pytest.raises(gpu.HcError, match="slots out of range"):
            _create(gpu, L, D, 1, 5, np.arange(31), 30)   # reaches past ob_n = 60
        with pytest.raises(gpu.HcError, match="slots out of range"):
            _create(gpu, L, D, 1, 5, idx, -1)
        with pytest.raises(gpu.HcError, match="pressure slot"):
            _create(gpu, L, D, 1, 5, idx, 1)    # slots 1 .. 30: the last one is a pressure slot
        with pytest.raises(gpu.HcError, match="pressure slot"):
            _create(gpu, L, D, 1, 5, idx, 30)
        assert np.all(D.openBoundaryValues(0, 60) == np.array([0.0, 0.0, 0.0, 1.0]))   # nothing was written
        with pytest.raises(gpu.HcError, match="unknown direction"):
            gpu.PreInlet(L, D, [[1, 1]], 0, 0, direction="Wneg")
        with pytest.raises(gpu.HcError, match="unknown direction"):
            gpu.preinlet_driving_force_vector(0.5, 0.1, 100, "xneg")
        with pytest.raises(gpu.HcError, match="n_slabs = 1"):
            gpu.PreInlet(S, D, [[1, 1]], 0, 3, direction="Zneg", device=True)
    finally:
        L.destroy(); D.destroy(); S.destroy()
