"""The pre-inlet's fluid coupling into a domain that is cut into x-slabs (tests/slab_ranks.py): a 16 x 17 x 19 pre-inlet,
periodic and driven along x, feeds a 48 x 17 x 19 walled channel with a pressure outlet at its far end.  Xneg: the pre-inlet and
the coupling live on rank 0, whose plane 0 is the inlet; Xpos: on the last rank, whose plane nx - 1 is.  The other ranks step
their slabs the same number of times.  The slabs' populations and the values sent equal the one-process host.PreInlet run, bit
for bit, lag of one iteration included."""
import ctypes as C

import numpy as np
import pytest

import open_boundary_axis_ref as AX
import open_boundary_ref as OB
import slab_ranks

pytestmark = pytest.mark.gpu

PRE_DIMS, DOM_DIMS = (16, 17, 19), (48, 17, 19)
OMEGA = 1.0
SIGN = {"Xneg": -1, "Xpos": 1}
CHECKPOINTS = (1, 2, 30, 32)     # iterations after which the state is recorded; wall-node slots are declared after 30 (slot growth)
HC_ERR_ARG, HC_ERR_STATE = 2, 3


def _masks():
    return AX.channel_mask(PRE_DIMS, 0), AX.channel_mask(DOM_DIMS, 0)


def _coupled_nodes():
    ly, lz = np.nonzero(_masks()[0][0] == 0)
    return np.stack([ly, lz], axis=1)


def _pre_lattice(host, direction):
    pre = host.Lattice(*PRE_DIMS, (True, False, False), OMEGA)
    pre.defineBounceBack(_masks()[0])
    pre.setExternalVector((-1e-5 * SIGN[direction], 0.0, 0.0))     # *neg drives along +x, *pos along -x
    pre.latticeEquilibrium()
    return pre


def _wall_box(x):
    """the bounce-back row y = 0 of plane x: declaring it changes no population (bounce-back nodes stay bounce-back), but the
    slot storage grows past its capacity and moves"""
    return (x, x, 0, 0, 0, DOM_DIMS[2] - 1)


def _single(gpu, direction, device):
    """the one-process run: {iterations: (domain populations, sent)}"""
    sign = SIGN[direction]
    nx = DOM_DIMS[0]
    pre = _pre_lattice(gpu, direction)
    dom = gpu.Lattice(*DOM_DIMS, AX.NONPER, OMEGA)
    coupling = None
    try:
        dmask = _masks()[1]
        dom.defineBounceBack(dmask); dom.latticeEquilibrium()
        g = _coupled_nodes()
        coupling = gpu.PreInlet(pre, dom, g, PRE_DIMS[0] - 1 if sign < 0 else 0, 0 if sign < 0 else nx - 1, direction=direction, device=device)
        out_plane = nx - 1 if sign < 0 else 0
        fp, npres = dom._add_open_box(1, -sign, (out_plane, out_plane, 0, DOM_DIMS[1] - 1, 0, DOM_DIMS[2] - 1), 0)
        S0 = dom.populations().reshape(DOM_DIMS + (19,))
        val0 = dom.openBoundaryValues(0, fp + npres)
        out, done = {}, 0
        for target in CHECKPOINTS:
            if done == 30:
                dom._add_open_box(0, -1, _wall_box(5 if sign < 0 else nx - 6), 0)
            coupling.iterate(target - done); done = target
            out[target] = (dom.populations().reshape(DOM_DIMS + (19,)), coupling.sent())
        # the lag: after the first iteration the slots hold the pre-inlet's velocities, and the domain has stepped with u = 0
        code = -np.ones(DOM_DIMS, np.int64)
        code[0 if sign < 0 else nx - 1, g[:, 0], g[:, 1]] = (coupling.first + np.arange(len(g))) << 2 | (OB.VEL_0N if sign < 0 else OB.VEL_0P)
        code[out_plane] = ((fp + np.arange(npres)) << 2 | (OB.PRES_0P if sign < 0 else OB.PRES_0N)).reshape(DOM_DIMS[1:])
        assert np.all(val0[:, :3] == 0.0) and np.abs(out[1][1]).max() > 0
        want = OB.step(S0, dmask, AX.NONPER, OMEGA, (0.0, 0.0, 0.0), code, val0)
        assert np.array_equal(out[1][0][dmask == 0], want[dmask == 0])
        rho, u = dom.rho_u()
        assert np.isfinite(u).all() and float(np.abs(rho.reshape(DOM_DIMS)[dmask == 0] - 1.0).max()) < 0.1
        assert (out[30][1][:, 0] * -sign).mean() > 0                      # the flow enters the domain
        return out
    finally:
        if coupling is not None:
            coupling.destroy()
        pre.destroy(); dom.destroy()


def _rank(rank, world, direction, device):
    from hemocell_amd import host
    from hemocell_amd.slab import SlabRunner
    import types
    sign = SIGN[direction]
    lib = host.capi.lib()
    nxg = DOM_DIMS[0]
    nx = nxg // world
    r = SlabRunner(nx, DOM_DIMS[1], DOM_DIMS[2], rank, world, types.SimpleNamespace(tau=1.0 / OMEGA), periodic=AX.NONPER, fluid_only=True)
    r.define_bounce_back(_masks()[1])
    r.lattice.latticeEquilibrium()
    inlet_rank = 0 if sign < 0 else world - 1
    pre = coupling = None
    out = {"refused": np.array(0)}
    if rank == inlet_rank:
        pre = _pre_lattice(host, direction)
        g = _coupled_nodes()
        # out of scope, refused with nothing changed: a y direction into a slab, a pre-inlet on slabs, the plane velocity of a slab
        for bad, kw in ((dict(direction="Ypos"), {}), (dict(direction="Ypos", device=True), {})):
            try:
                host.PreInlet(pre, r.lattice, [[1, 1]], 0, DOM_DIMS[1] - 1, **bad)
                raise AssertionError("Ypos into a slab was accepted")
            except host.HcError as e:
                assert "n_slabs = 1" in str(e), e
        try:
            host.PreInlet(r.lattice, pre, g, 0, 0, direction=direction, device=device)
            raise AssertionError("a pre-inlet on a slab was accepted")
        except host.HcError as e:
            assert "n_slabs = 1" in str(e), e
        try:
            r.lattice.planeVelocity(0, [20])
            raise AssertionError("hcl_plane_velocity on a slab was accepted")
        except host.HcError as e:
            assert "n_slabs = 1" in str(e), e
        ptr = C.c_void_p()
        idx = np.zeros(1, np.int32)
        assert lib.hcl_preinlet_create(C.byref(ptr), pre.ptr, r.lattice.ptr, 1, 0, host._iptr(idx), 0, 0) == HC_ERR_ARG and not ptr.value
        assert lib.hcl_preinlet_create(C.byref(ptr), r.lattice.ptr, pre.ptr, 0, 0, host._iptr(idx), 0, 0) == HC_ERR_ARG and not ptr.value
        assert (r.lattice.openBoundarySlots(np.argwhere(np.ones((nx,) + DOM_DIMS[1:]))) == -1).all()
        out["refused"] = np.array(4)
        coupling = host.PreInlet(pre, r.lattice, g, PRE_DIMS[0] - 1 if sign < 0 else 0, 0 if sign < 0 else nx - 1, direction=direction, device=device)
        assert coupling.first == 0
    out_plane = nxg - 1 if sign < 0 else 0
    r.add_open_boundary(1, 0, -sign, (out_plane, out_plane, 0, DOM_DIMS[1] - 1, 0, DOM_DIMS[2] - 1))
    done = 0
    for target in CHECKPOINTS:
        if done == 30:   # slot growth after create: the storage of the inlet rank's slots moves, the handle takes it at launch time
            r.add_open_boundary(0, 0, -1, _wall_box(5 if sign < 0 else nxg - 6))
        if coupling is not None:
            coupling.iterate(target - done)          # the domain's step inside is collective ...
        else:
            r.run(target - done)                     # ... the other ranks step as often
        done = target
        out["f%d" % target] = r.populations()
        out["sent%d" % target] = coupling.sent() if coupling is not None else np.zeros((0, 3))
    if coupling is not None:
        if device:   # the coupled slots go with hcl_open_boundary_clear: HC_ERR_STATE, nothing launched
            r.lattice.clearOpenBoundaries()
            assert lib.hcl_preinlet_apply(coupling.ptr) == HC_ERR_STATE
            assert lib.hcl_preinlet_iterate(coupling.ptr, 1) == HC_ERR_STATE
            out["refused"] = np.array(int(out["refused"]) + 2)
        # cells do not cross into a slab (hcp_preinlet_create): the envelope plan would go stale under an append
        P = host.base_parameters()
        plt = host.CellType.plt(P)
        pc, dc = host.Cells(pre, P), host.Cells(r.lattice, P)
        pc.addCellType(plt, 1); dc.addCellType(plt, 1)
        xp = C.c_void_p()
        sh = np.array((float(PRE_DIMS[0]), 0.0, 0.0))
        rc = lib.hcp_preinlet_create(C.byref(xp), pc.ptr, dc.ptr, 0, sign, 2.0, 11.0, host.dptr(sh), 1000)
        assert rc == HC_ERR_ARG and not xp.value and "n_slabs = 1" in lib.hc_last_error().decode()
        out["refused"] = np.array(int(out["refused"]) + 1)
        pc.destroy(); dc.destroy(); plt.destroy()
        coupling.destroy()
        pre.destroy()
    r.lattice.destroy()
    return out


@pytest.mark.parametrize("device", [True, False])
@pytest.mark.parametrize("direction,world", [("Xneg", 2), ("Xneg", 3), ("Xpos", 2), ("Xpos", 3)])
def test_preinlet_into_slabs_equals_one_process(gpu, tmp_path, direction, world, device):
    ref = _single(gpu, direction, device)
    res = slab_ranks.run(_rank, world, tmp_path, direction, device, salt=10 + 2 * (direction == "Xpos") + device)
    nx = DOM_DIMS[0] // world
    fluid = _masks()[1] == 0
    inlet = res[0 if SIGN[direction] < 0 else -1]
    for target in CHECKPOINTS:
        f = np.concatenate([r["f%d" % target].reshape((nx,) + DOM_DIMS[1:] + (19,)) for r in res], axis=0)
        assert np.array_equal(f[fluid], ref[target][0][fluid]), (target, float(np.abs(f[fluid] - ref[target][0][fluid]).max()))
        assert np.array_equal(inlet["sent%d" % target], ref[target][1]), target
    assert int(inlet["refused"]) == (7 if device else 5)
    assert not np.array_equal(ref[30][1], ref[32][1])                      # the coupling went on after the slots had moved
