"""Zou-He open boundaries on x-slabs: 2, 3 and 4 ranks (tests/slab_ranks.py) hold the single domain's bits, and the single
domain the restatement's (tests/open_boundary_ref.py, tests/open_boundary_axis_ref.py).

Scenes: a 48 x 17 x 19 channel that is open along x (velocity 0N / pressure 0P, and the mirror), so the open planes lie on the
first and the last rank; 24 x 24 x 19 and 24 x 17 x 24 channels that are periodic along x and open along y / z, so the face
planes of EVERY slab hold open nodes.  Every restated run is computed once, asserted finite with |rho - 1| < 0.1 on fluid nodes
at every step, and shared.  The face-velocity message is checked on one lattice, without ranks."""
import ctypes as C
import functools
import types

import numpy as np
import pytest

import open_boundary_axis_ref as AX
import open_boundary_ref as OB
import slab_ranks

pytestmark = pytest.mark.gpu

OMEGA, TAU, BODY = AX.OMEGA, 0.9, AX.BODY
assert 1.0 / TAU == OMEGA
VELOCITY = (OB.VEL_0N, OB.VEL_0P)
PER_X = (True, False, False)


def _plane_box(dims, axis, plane):
    box = [0, dims[0] - 1, 0, dims[1] - 1, 0, dims[2] - 1]
    box[2 * axis] = box[2 * axis + 1] = plane
    return tuple(box)


def _profile_periodic_x(box, axis, sign, dims, u_max=0.02):
    """velocity_values for a y or z face of a lattice that is periodic along x: a parabola across the walled axis, modulated (and
    nowhere zero) along x, so that the nodes on the slabs' face planes carry a velocity; tangential components 0.1 and -0.05 of it"""
    ext = [box[1] - box[0] + 1, box[3] - box[2] + 1, box[5] - box[4] + 1]
    walled = 3 - axis
    shape = [1, 1, 1]; shape[walled] = ext[walled]
    along_x = (1.0 + 0.3 * np.cos(2 * np.pi * np.arange(ext[0]) / dims[0])).reshape(ext[0], 1, 1)
    p = (u_max * along_x * AX._tent(ext[walled]).reshape(shape) * np.ones(ext)).reshape(-1)
    u = np.empty((p.size, 3))
    u[:, axis], u[:, 0], u[:, walled] = sign * p, 0.1 * p, -0.05 * p
    return u


@functools.lru_cache(maxsize=None)
def _scene(name):
    """(dims, periodic, mask, patches, code, axes, val, S0), read-only; patches in GLOBAL coordinates"""
    if name.startswith("x"):
        dims, axis, periodic = (48, 17, 19), 0, AX.NONPER
        mask = AX.channel_mask(dims, 0)                    # bounce-back shell on the y and z faces
    elif name == "y":
        dims, axis, periodic = (24, 24, 19), 1, PER_X
        mask = np.zeros(dims, np.uint8); mask[:, :, 0] = mask[:, :, -1] = 1      # walls in z
    else:
        dims, axis, periodic = (24, 17, 24), 2, PER_X
        mask = np.zeros(dims, np.uint8); mask[:, 0, :] = mask[:, -1, :] = 1      # walls in y
    n = dims[axis]
    if name == "x-mirrored":   # a P velocity face with an inward (negative) normal velocity, an N pressure face
        bv, bp = _plane_box(dims, axis, n - 1), _plane_box(dims, axis, 0)
        patches = [(OB.VEL_0P, axis, bv, AX.velocity_values(bv, axis, -1.0)), (OB.PRES_0N, axis, bp, AX.density_values(bp, 32))]
    else:                      # an N velocity face with a parabola and non-zero tangential components, a P pressure face
        bv, bp = _plane_box(dims, axis, 0), _plane_box(dims, axis, n - 1)
        values = AX.velocity_values(bv, axis, 1.0) if axis == 0 else _profile_periodic_x(bv, axis, 1.0, dims)
        patches = [(OB.VEL_0N, axis, bv, values), (OB.PRES_0P, axis, bp, AX.density_values(bp, 31))]
    code, axes, val = AX.declaration(dims, patches)
    S0 = AX.gathered(np.random.default_rng(4).uniform(-0.005, 0.005, size=dims + (19,)), periodic)
    for a in (mask, code, axes, val, S0):
        a.setflags(write=False)
    return dims, periodic, mask, patches, code, axes, val, S0


def _force_boxes(dims):
    """two body-force boxes in global coordinates: the first straddles a slab face of every decomposition into 2, 3 and 4 slabs
    (x = 24; 16; 12 of 48 planes, x = 12; 8; 6 of 24), the second overlaps it (the last box wins)"""
    s = dims[0] // 24
    first = (5 * s, 13 * s, 2, dims[1] - 3, 3, dims[2] - 3)
    second = (11 * s, 20 * s, 0, dims[1] - 1, 0, dims[2] // 2)
    for w in (2, 3, 4):
        assert any(first[0] < k * (dims[0] // w) <= first[1] for k in range(1, w))
    return [first, second], [(-3e-6, 1e-6, 2e-6), (5e-6, -2e-6, 1e-6)]


@functools.lru_cache(maxsize=None)
def _restated(name, with_boxes):
    """{1: state, 50: state} of the restatement"""
    dims, periodic, mask, patches, code, axes, val, S0 = _scene(name)
    kw = {}
    if with_boxes:
        kw["boxes"], kw["box_forces"] = _force_boxes(dims)
    S, out = S0, {}
    for n in range(1, 51):
        S = OB.step(S, mask, periodic, OMEGA, BODY, code, val, **kw) if name.startswith("x") else AX.step(S, mask, periodic, OMEGA, BODY, code, axes, val, **kw)
        assert np.isfinite(S).all()
        rho, _, _ = AX.observe(S, mask, periodic, BODY, None, code, axes, val, **kw)
        dev = float(np.abs(rho[mask == 0] - 1.0).max())
        assert dev < 0.1, (n, dev)
        if n in (1, 50):
            S.setflags(write=False)
            out[n] = S
    return out


_SINGLE = {}


def _single(gpu, name, with_boxes):
    """the single domain after 1 and 50 steps: {1: (f, rho, u, pi), 50: ..., "stats": fluid_stats(0)}; its populations are the
    restatement's, bit for bit"""
    key = (name, with_boxes)
    if key in _SINGLE:
        return _SINGLE[key]
    dims, periodic, mask, patches, code, axes, val, S0 = _scene(name)
    want = _restated(name, with_boxes)
    fluid = mask == 0
    L = gpu.Lattice(*dims, periodic, OMEGA)
    try:
        L.defineBounceBack(mask)
        L.setExternalVector(BODY)
        if with_boxes:
            L.setExternalVectorBoxes(*_force_boxes(dims))
        for kind, axis, box, values in patches:
            first, n = L._add_open_box((kind >> 1) & 1, 1 if kind & 1 else -1, box, axis)
            (L.setOpenBoundaryVelocitySlots if kind in VELOCITY else L.setOpenBoundaryDensitySlots)(first, values)
        assert np.array_equal(L.openBoundaryValues(0, len(val)), val)
        L.set_populations(S0.reshape(-1, 19))
        out, done = {}, 0
        for target in (1, 50):
            L.collideAndStream(target - done); done = target
            f = L.populations().reshape(dims + (19,))
            assert np.array_equal(f[fluid], want[target][fluid]), (name, target, float(np.abs(f[fluid] - want[target][fluid]).max()))
            rho, u = L.rho_u()
            out[target] = (f, rho.reshape(dims), u.reshape(dims + (3,)), L.pi_neq().reshape(dims + (6,)))
        out["stats"] = L.fluid_stats(0)
    finally:
        L.destroy()
    _SINGLE[key] = out
    return out


def _fluid_rank(rank, world, name, variants):
    """one rank of a fluid-only slab run of a scene: every variant in turn, the state after 1 and 50 steps"""
    from hemocell_amd import host
    from hemocell_amd.slab import SlabRunner
    dims, periodic, mask, patches, code, axes, val, S0 = _scene(name)
    nx = dims[0] // world
    out = {}
    for v in variants:
        words = v.split("-")
        host.check(host.capi.lib().hc_debug_force_plane_padding(1 if "padded" in words else -1 if "unpadded" in words else 0))
        r = SlabRunner(nx, dims[1], dims[2], rank, world, types.SimpleNamespace(tau=TAU), periodic=periodic, fluid_only=True)
        host.check(host.capi.lib().hc_debug_force_plane_padding(0))
        r.define_bounce_back(mask)
        r.lattice.setExternalVector(BODY)
        if "boxes" in words:
            r.lattice.setExternalVectorBoxes(*_force_boxes(dims))     # global coordinates on every rank
        total = 0
        for kind, axis, box, values in patches:
            first, n = r.add_open_boundary((kind >> 1) & 1, axis, 1 if kind & 1 else -1, box)
            assert first == total
            (r.set_open_velocity if kind in VELOCITY else r.set_open_density)(box, values)
            total += n
        out[v + "__vals"] = r.lattice.openBoundaryValues(0, total) if total else np.zeros((0, 4))
        plane = np.mgrid[0:1, 0:dims[1], 0:dims[2]].reshape(3, -1).T
        out[v + "__face_open"] = np.array([int((r.lattice.openBoundarySlots(plane + [x, 0, 0]) >= 0).sum()) for x in (0, nx - 1)])
        r.lattice.set_populations(S0[r.x0:r.x0 + nx].reshape(-1, 19))   # collective: the ranks exchange their face planes
        done = 0
        for target in (1, 50):
            r.run(target - done); done = target
            out["%s__f%d" % (v, target)] = r.populations()
            rho, u = r.lattice.rho_u()                                  # the face planes pull across the rank faces
            out["%s__rho%d" % (v, target)], out["%s__u%d" % (v, target)] = rho, u
            out["%s__pi%d" % (v, target)] = r.lattice.pi_neq()
        out[v + "__stats"] = np.array(r.fluid_stats(0))                 # reduced: every rank gets the global numbers
        r.lattice.destroy()
    return out


def _compare(gpu, tmp_path, name, world, variants, salt):
    from hemocell_amd.slab import open_boundary_rows
    dims, periodic, mask, patches, code, axes, val, S0 = _scene(name)
    refs = {v: _single(gpu, name, "boxes" in v.split("-")) for v in variants}     # before the ranks start: they share the GPU
    res = slab_ranks.run(_fluid_rank, world, tmp_path, name, variants, salt=salt)
    nx = dims[0] // world
    fluid = mask == 0
    for v in variants:
        ref = refs[v]
        for target in (1, 50):
            for k, (key, c) in enumerate((("f", 19), ("rho", 1), ("u", 3), ("pi", 6))):
                got = np.concatenate([r["%s__%s%d" % (v, key, target)].reshape(nx, dims[1], dims[2], c) for r in res], axis=0)
                want = ref[target][k].reshape(dims + (c,))
                assert np.array_equal(got[fluid], want[fluid]), (v, key, target, float(np.abs(got[fluid] - want[fluid]).max()))
        for r in res:   # the reduced statistics: the tolerance of tests/test_gpu_multislab.py
            got, want = r[v + "__stats"], ref["stats"]
            assert got[3] == want[3]
            assert np.allclose(got[:3], want[:3], rtol=1e-6, atol=1e-18), (got, want)
        # the values of every rank's slots are its rows of the global declaration, patch by patch
        first = 0
        want_vals = [[] for _ in res]
        for kind, axis, box, values in patches:
            n = len(values)
            for k in range(world):
                want_vals[k].append(val[first:first + n][open_boundary_rows(box, k * nx, nx)[2]])
            first += n
        for k, r in enumerate(res):
            assert np.array_equal(r[v + "__vals"], np.concatenate(want_vals[k]))
    return res


X_VARIANTS = ("plain", "boxes", "boxes-padded", "boxes-unpadded")


@pytest.mark.parametrize("world", [2, 3, 4])
@pytest.mark.parametrize("name", ["x-original", "x-mirrored"])
def test_x_faces_on_slabs_equal_the_single_domain_bit_for_bit(gpu, tmp_path, name, world):
    """a. populations, rho_u and pi_neq after 1 and 50 steps, plain and with two body-force boxes (one across a slab face: the
    <REGIONS, OPEN> collide), these also with padded and unpadded plane strides forced on the slabs; the open planes lie on the
    first and the last rank, the ranks between them run the plain instantiations"""
    dims, _, mask, _, code = _scene(name)[:5]
    assert set(int(k) for k in code[code >= 0] & 3) == ({OB.VEL_0N, OB.PRES_0P} if name == "x-original" else {OB.VEL_0P, OB.PRES_0N})
    res = _compare(gpu, tmp_path, name, world, X_VARIANTS, salt=1 + (name == "x-mirrored"))
    per_plane = dims[1] * dims[2]
    assert res[0]["plain__face_open"][0] == per_plane and res[-1]["plain__face_open"][1] == per_plane


@pytest.mark.parametrize("world", [2, 3, 4])
@pytest.mark.parametrize("name", ["y", "z"])
def test_y_and_z_faces_through_every_slab(gpu, tmp_path, name, world):
    """b. x periodic, the inlet and the outlet planes run through every slab: both face planes of every slab hold open nodes"""
    dims, _, mask, _, code = _scene(name)[:5]
    nx = dims[0] // world
    for k in range(world):
        assert (code[k * nx] >= 0).any() and (code[k * nx + nx - 1] >= 0).any()
    res = _compare(gpu, tmp_path, name, world, ("plain",), salt=5 + (name == "z"))
    for r in res:
        assert (r["plain__face_open"] == (code[0] >= 0).sum()).all() and r["plain__face_open"].min() > 0


def test_face_velocity_message_carries_completed_moments(gpu):
    """c. hcl_download_face_velocity on one lattice with open nodes on its planes 0 and nx - 1 (the y channel, a uniform body
    force and one force box, 20 steps): the u of rho_u() on those planes, bit for bit on fluid nodes -- both take hc::moments of
    the completed populations -- 0 on bounce-back nodes, and u_bc + F / 2 on the velocity nodes to 1e-14, the bound of the
    observer tests.  Plain moments (the kernel before it had an OPEN form) count the unknown populations as zeros."""
    dims, periodic, mask, patches, code, axes, val, S0 = _scene("y")
    nx, ny, nz = dims
    boxes, forces = [(0, 3, 0, 5, 2, nz - 1)], [(4e-6, -1e-6, 2e-6)]
    L = gpu.Lattice(*dims, periodic, OMEGA)
    try:
        L.defineBounceBack(mask)
        L.setExternalVector(BODY)
        L.setExternalVectorBoxes(boxes, forces)
        for kind, axis, box, values in patches:
            first, n = L._add_open_box((kind >> 1) & 1, 1 if kind & 1 else -1, box, axis)
            (L.setOpenBoundaryVelocitySlots if kind in VELOCITY else L.setOpenBoundaryDensitySlots)(first, values)
        L.set_populations(S0.reshape(-1, 19))
        L.collideAndStream(20)
        rho, u = L.rho_u()
        assert np.isfinite(u).all() and float(np.abs(rho.reshape(dims)[mask == 0] - 1.0).max()) < 0.1
        u = u.reshape(dims + (3,))
        F = OB.body_field(dims, BODY, boxes, forces)
        for side, plane in ((0, 0), (1, nx - 1)):
            fluid = (mask[plane] == 0).reshape(-1)
            c = code[plane].reshape(-1)
            vel = fluid & (c >= 0) & ((c & 2) == 0)
            pres = fluid & (c >= 0) & ((c & 2) != 0)
            assert vel.any() and pres.any()
            out = np.full((3, ny * nz), np.nan)
            gpu.check(gpu.capi.lib().hcl_download_face_velocity(L.ptr, side, out.ctypes.data_as(C.POINTER(C.c_double))))
            got = out.T
            want = u[plane].reshape(-1, 3)
            assert np.array_equal(got[fluid], want[fluid]), float(np.abs(got[fluid] - want[fluid]).max())
            assert (got[~fluid] == 0.0).all()
            expect = val[c[vel] >> 2][:, :3].astype(np.longdouble) + F[plane].reshape(-1, 3)[vel].astype(np.longdouble) / 2
            err = float(np.abs(got[vel].astype(np.longdouble) - expect).max())
            print("plane %d: largest error against u_bc + F / 2 on %d velocity nodes %.3e" % (plane, int(vel.sum()), err))
            assert err <= 1e-14
            assert np.abs(val[c[vel] >> 2][:, :3]).max() > 1e-3          # the profile is not zero on this plane
    finally:
        L.destroy()


# ---- d, e: coupled runs -- membrane cells next to open planes and across slab faces

K_P, K_M = 2, 4                                   # velocity update every 2 iterations, material model every 4
CROSS = (34, 34)
_EXTENT, _COUPLED = {}, {}


@pytest.fixture(params=[True, False], ids=["reproducible", "atomic"])
def spread(request, gpu):
    """hc_set_reproducible_spread for this process and, through the environment, for the ranks it starts"""
    import os
    on = request.param
    if on:
        os.environ["HEMOCELL_REPRODUCIBLE_SPREAD"] = "1"
    gpu.check(gpu.capi.lib().hc_set_reproducible_spread(1 if on else 0))
    yield on
    os.environ.pop("HEMOCELL_REPRODUCIBLE_SPREAD", None)
    gpu.check(gpu.capi.lib().hc_set_reproducible_spread(0))


def _celltype(host, P, what):
    return host.CellType.rbc(P) if what == "rbc" else host.CellType.plt(P)


def _extent(gpu, what, angles):
    """(lowest, highest) offsets of a placed cell's vertices from the centre it was placed at, per axis"""
    key = (what, tuple(angles))
    if key not in _EXTENT:
        P = gpu.base_parameters()
        L = gpu.Lattice(32, 32, 32, (True, True, True), 1.0 / P.tau)
        h = gpu.HemoCell(L, P)
        h.cellfields.addCellType(_celltype(gpu, P, what), 1)
        assert h.cellfields.addCell(0, (16.0, 16.0, 16.0), angles)
        p = h.cellfields.positions
        _EXTENT[key] = (p.min(axis=0) - 16.0, p.max(axis=0) - 16.0)
        L.destroy()
    return _EXTENT[key]


def _coupled_scene(kind, nxg):
    """(dims, periodic, mask, patches): d = the x channel with an N velocity inlet and a P pressure outlet, 34 x 34 across;
    e = the y channel of (b), nxg planes long"""
    if kind == "d":
        dims, periodic, axis = (nxg,) + CROSS, AX.NONPER, 0
        mask = AX.channel_mask(dims, 0)
        bv, bp = _plane_box(dims, 0, 0), _plane_box(dims, 0, nxg - 1)
        values = AX.velocity_values(bv, 0, 1.0)
    else:
        dims, periodic, axis = (nxg, 24, 19), PER_X, 1
        mask = np.zeros(dims, np.uint8); mask[:, :, 0] = mask[:, :, -1] = 1
        bv, bp = _plane_box(dims, 1, 0), _plane_box(dims, 1, 23)
        values = _profile_periodic_x(bv, 1, 1.0, dims)
    patches = [(OB.VEL_0N, axis, bv, values), (OB.PRES_0P, axis, bp, np.ones(AX._box_size(bp)))]
    return dims, periodic, mask, patches


def _coupled_build(rank, world, kind, nxg, cells):
    """cells: [(type name, centre, angles)]; the types are the distinct names in order of first appearance"""
    from hemocell_amd import host
    from hemocell_amd.slab import SlabRunner
    dims, periodic, mask, patches = _coupled_scene(kind, nxg)
    P = host.base_parameters()
    r = SlabRunner(nxg // world, dims[1], dims[2], rank, world, P, periodic=periodic, particle_timescale=K_P, material_timescale=K_M)
    r.define_bounce_back(mask)
    r.lattice.latticeEquilibrium(1.0, (0, 0, 0))
    for kind_, axis, box, values in patches:
        r.add_open_boundary((kind_ >> 1) & 1, axis, 1 if kind_ & 1 else -1, box)
        (r.set_open_velocity if kind_ in VELOCITY else r.set_open_density)(box, values)
    names = []
    for what, _, _ in cells:
        if what not in names:
            names.append(what)
            r.add_cell_type(_celltype(host, P, what))
    for t, what in enumerate(names):
        mine = [(c, a) for w, c, a in cells if w == what]
        r.load_cells(t, [np.array(c, dtype=np.float64) for c, _ in mine], [np.array(a, dtype=np.float64) for _, a in mine])
    placed = r.sync_placement()
    assert tuple(placed) == tuple(sum(w == what for w, _, _ in cells) for what in names), placed
    r.prepare()
    return r, names


def _step_pattern(r, n):
    """the same calls on every rank: single iterations first, then the rest in one call (the next spread then runs beside the collide)"""
    for _ in range(min(n, 20)):
        r.run(1)
    if n > 20:
        r.run(n - 20)


def _coupled_rank(rank, world, kind, nxg, cells, steps):
    r, names = _coupled_build(rank, world, kind, nxg, cells)
    _step_pattern(r, steps)
    out = {"f": r.populations(), "held": np.array(r.cells.counts()[1])}
    for t in range(len(names)):
        cid, vid, pos = r.owned_vertex_table(t)
        out["cid%d" % t], out["vid%d" % t], out["pos%d" % t] = cid, vid, pos
    r.lattice.destroy()
    return out


def _coupled_single(kind, nxg, cells, steps, repro):
    """the single domain: (populations, [positions of type t as [cells][nv][3]], initial positions likewise, mask)"""
    key = (kind, nxg, repr(cells), steps, repro)
    if key not in _COUPLED:
        r, names = _coupled_build(0, 1, kind, nxg, cells)
        dims, periodic, mask, patches = _coupled_scene(kind, nxg)

        def table():
            allpos, out, first = r.cells.positions, [], 0
            for t, what in enumerate(names):
                n, nv = sum(w == what for w, _, _ in cells), r.cells.types[t].nv
                out.append(allpos[first:first + n * nv].reshape(n, nv, 3).copy()); first += n * nv
            return out
        start = table()
        _step_pattern(r, steps)
        f = r.lattice.populations().reshape(dims + (19,))
        rho, u = r.lattice.rho_u()
        assert np.isfinite(f).all() and np.isfinite(u).all()
        assert float(np.abs(rho.reshape(dims)[mask == 0] - 1.0).max()) < 0.1
        _COUPLED[key] = (f, table(), start, mask)
        r.lattice.destroy()
    return _COUPLED[key]


def _compare_coupled(res, ref, dims, world, tol_f, tol_x):
    f_ref, pos_ref, _, mask = ref
    fluid = mask == 0
    f = np.concatenate([r["f"].reshape((dims[0] // world,) + dims[1:] + (19,)) for r in res], axis=0)
    err_f = float(np.abs(f - f_ref)[fluid].max())
    worst = 0.0
    for t, p_ref in enumerate(pos_ref):
        seen = np.zeros(p_ref.shape[:2], dtype=int)
        for r in res:
            d = r["pos%d" % t] - p_ref[r["cid%d" % t], r["vid%d" % t]]
            worst = max(worst, float(np.abs(d).max()) if len(d) else 0.0)
            np.add.at(seen, (r["cid%d" % t], r["vid%d" % t]), 1)
        assert (seen == 1).all()                                          # every vertex owned by exactly one rank
    print("slabs vs single domain: max |df| = %.3e, max |dx| = %.3e" % (err_f, worst))
    assert err_f <= tol_f and worst <= tol_x, (err_f, worst)


@pytest.mark.parametrize("world", [2, 3])
def test_coupled_x_channel_on_slabs(gpu, tmp_path, spread, world):
    """d. 96 x 34 x 34 as 2 slabs, 120 x 34 x 34 as 3: a parabolic 0N inlet, a 0P outlet, an RBC across the first slab face, an
    RBC whose lowest vertex lies 2.5 nodes behind the inlet plane, a platelet whose highest lies 3 nodes before the outlet plane;
    cadence (2, 4), 60 iterations.  Reproducible spread: the single domain's bits, populations and owned vertices; atomic spread:
    the bounds tests/test_gpu_multislab.py holds its runs against the oracle to (populations 1e-11, vertices 1e-9)"""
    nxg = 48 * world if world == 2 else 40 * world
    face = nxg // world
    ang = (90.0, 0.0, 0.0)
    lo_r, _ = _extent(gpu, "rbc", ang)
    _, hi_p = _extent(gpu, "plt", (0.0, 0.0, 0.0))
    cells = (("rbc", (face + 0.3, 16.5, 17.0), ang), ("rbc", (2.5 - lo_r[0], 17.0, 16.5), ang),
             ("plt", (nxg - 1 - 3.0 - hi_p[0], 15.0, 18.0), (0.0, 0.0, 0.0)))
    ref = _coupled_single("d", nxg, cells, 60, spread)
    start = ref[2]
    assert start[0][0][:, 0].min() < face - 1 and start[0][0][:, 0].max() > face       # across the slab face
    assert abs(start[0][1][:, 0].min() - 2.5) < 1e-9 and abs(start[1][0][:, 0].max() - (nxg - 4.0)) < 1e-9
    assert max(float(np.abs(a - b).max()) for a, b in zip(ref[1], start)) > 0.01       # the cells have moved
    res = slab_ranks.run(_coupled_rank, world, tmp_path, "d", nxg, cells, 60, salt=20 + spread)
    assert sum(int(r["held"]) for r in res) > len(cells)                                # the cell at the face is replicated
    _compare_coupled(res, ref, (nxg,) + CROSS, world, *((0.0, 0.0) if spread else (1e-11, 1e-9)))


@pytest.mark.parametrize("world", [2, 3])
def test_neighbours_open_face_node_in_a_stencil(gpu, tmp_path, world):
    """e. platelets only, the y channel on slabs of the least width the slab schedule takes for them (a multiple of 4): a platelet
    straddles a slab face within a node of the inlet plane y = 0, so that vertices on one slab blend the velocity of fluid
    open nodes on the NEIGHBOUR's face plane -- the value the face-velocity message carries.  Reproducible spread, 40 iterations,
    the single domain's bits."""
    import os
    ang = (0.0, 0.0, 0.0)
    lo_p, hi_p = _extent(gpu, "plt", ang)
    P = gpu.base_parameters()
    plt = gpu.CellType.plt(P)
    # make_slab: ceil(2 diameters + 2 envelope shares) planes; the diameter is twice the largest distance from the mesh's centre
    probe = gpu.Lattice(16, 16, 16, (True, True, True), 1.0 / P.tau)
    h = gpu.HemoCell(probe, P); h.cellfields.addCellType(plt, 1)
    assert h.cellfields.addCell(0, (8.0, 8.0, 8.0), ang)
    p0 = h.cellfields.positions
    diameter = 2.0 * float(np.sqrt(((p0 - 0.5 * (p0.max(axis=0) + p0.min(axis=0))) ** 2).sum(axis=1).max()))
    probe.destroy()
    need = int(np.ceil(2.0 * diameter + 2.0 * 4.0))            # 4.0: the default share (hcp_envelope)
    width = (need + 3) // 4 * 4
    assert width - 4 < need <= width
    nxg = width * world
    cells = (("plt", (width - 0.2, 0.4 - lo_p[1], 9.0), ang), ("plt", (width / 2.0, 12.0, 9.5), ang))
    os.environ["HEMOCELL_REPRODUCIBLE_SPREAD"] = "1"
    gpu.check(gpu.capi.lib().hc_set_reproducible_spread(1))
    try:
        ref = _coupled_single("e", nxg, cells, 40, True)
        dims, periodic, mask, patches = _coupled_scene("e", nxg)
        code = AX.declaration(dims, patches)[0]
        # the phi2 stencil of every vertex of the first platelet at its initial position: a vertex owned by one slab with a node
        # on the other slab's face plane that is a fluid open node
        hits = 0
        for p in ref[2][0][0]:
            c = np.floor(p + 0.5).astype(int)
            d0 = np.where(p < c, -1, 0)
            for i in range(2):
                for j in range(2):
                    for k in range(2):
                        g = c + d0 + (i, j, k)
                        if g[1] < 0 or g[1] >= dims[1] or g[2] < 0 or g[2] >= dims[2]:
                            continue
                        wt = np.prod(np.clip(1.0 - np.abs(p - g), 0.0, None))
                        gx = g[0] % nxg
                        other_slab = gx // width != (c[0] % nxg) // width
                        on_face = gx % width in (0, width - 1)
                        if wt != 0.0 and other_slab and on_face and mask[gx, g[1], g[2]] == 0 and code[gx, g[1], g[2]] >= 0:
                            hits += 1
        assert hits > 0
        res = slab_ranks.run(_coupled_rank, world, tmp_path, "e", nxg, cells, 40, salt=30)
        _compare_coupled(res, ref, dims, world, 0.0, 0.0)
    finally:
        os.environ.pop("HEMOCELL_REPRODUCIBLE_SPREAD", None)
        gpu.check(gpu.capi.lib().hc_set_reproducible_spread(0))
