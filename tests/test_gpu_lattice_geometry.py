"""The lattice kernels on geometries with inert nodes, empty planes and seams (tests/lattice_geometry_cases.py), against the
CPU oracle and the numpy restatements: the class map of hcl_set_mask, and every instantiation of the collide, the scalar
step, the observers and the slab schedule on lattices whose active-span map has rows that start late, empty rows, empty planes,
inert nodes inside spans and block seams inside rows.

Set-up of every comparison unless a test says otherwise: the random state 0.02 N(0,1) t_q, a uniform body force with three
non-zero components, 1 step and then 9 more, np.array_equal on the FLUID nodes (the oracle bounces on every solid node, the
device leaves inert ones alone: their slots are never written, by design), plain and with the padded plane stride.
tests/test_lattice_geometry_cpu.py proves that the geometries have the properties named here."""
import numpy as np
import pytest

import interior_viscosity_ref as IV
import lattice_geometry_cases as G
import lees_edwards_ref as LE
import open_boundary_ref as OB
import scalar_ref as SR
import slab_ranks
import solidify_ref
from tests import observables_ref as R

pytestmark = pytest.mark.gpu

NAMES = list(G.GEOMETRIES)
STEPS = (1, 9)


@pytest.fixture(params=[False, True], ids=["plain", "padded"])
def padded(request, gpu):
    """the padded x-plane stride, forced for the lattices the test creates; reset whatever happens"""
    lib = gpu.capi.lib()
    gpu.check(lib.hc_debug_force_plane_padding(1 if request.param else 0))
    try:
        yield request.param
    finally:
        gpu.check(lib.hc_debug_force_plane_padding(0))


def _same_on_fluid(got, want, mask, what):
    """array_equal on the fluid nodes; a failure names the first differing node"""
    fluid = np.asarray(mask).reshape(-1) == 0
    g, w = np.asarray(got).reshape(len(fluid), -1), np.asarray(want).reshape(len(fluid), -1)
    bad = fluid & (g != w).any(axis=1)
    if bad.any():
        k = int(np.flatnonzero(bad)[0])
        raise AssertionError("%s: %d of %d fluid nodes differ, the first is %s, max |diff| %.3e"
                             % (what, int(bad.sum()), int(fluid.sum()), np.unravel_index(k, np.asarray(mask).shape), np.abs(g[bad] - w[bad]).max()))
    assert np.isfinite(g[fluid]).all(), what


def _device_lattice(gpu, g, mask=None, omega=G.OMEGA, seed=G.SEED):
    L = gpu.Lattice(*g.dims, g.periodic, omega)
    L.defineBounceBack(g.mask if mask is None else mask)
    L.set_populations(G.start_state(g, seed))
    L.setExternalVector(G.BODY)
    return L


def _run_both(Lo, Lg, mask, what):
    """1 step and then 9 more on both sides, compared after each"""
    for n in STEPS:
        Lo.collide_stream(n); Lg.collideAndStream(n)
        _same_on_fluid(Lg.populations(), Lo.f, mask, "%s, %d step(s)" % (what, n))


_PLAIN = {}


def _oracle_plain(orc, name):
    """the oracle's populations of the plain collide after 1 and after 1 + 9 steps: computed once, shared, read-only"""
    if name not in _PLAIN:
        Lo = G.oracle_lattice(orc, G.GEOMETRIES[name])
        out = []
        for n in STEPS:
            Lo.collide_stream(n)
            f = Lo.f.copy(); f.setflags(write=False)
            out.append(f)
        force = Lo.force.copy(); force.setflags(write=False)
        Lo.destroy()
        _PLAIN[name] = (out, force)
    return _PLAIN[name]


# ---- 1: the class map

@pytest.mark.parametrize("name", NAMES + ["stenosis_open"])
def test_class_map(gpu, padded, name):
    """hcl_download_mask equals the restated rule node for node, and hcl_node_counts is (nodes, fluid, nodes - kept inert)"""
    g = G.STENOSIS_OPEN if name == "stenosis_open" else G.GEOMETRIES[name]
    L = gpu.Lattice(*g.dims, g.periodic, G.OMEGA)
    try:
        assert L.node_counts() == (L.n, L.n, L.n)   # before any mask: all fluid
        L.defineBounceBack(g.mask)
        want, _ = g.classes(padded)
        got = L.mask()
        assert np.array_equal(got, want), (int((got != want).sum()), tuple(np.argwhere(got != want)[0]))
        kept = int((want == 2).sum())
        assert L.node_counts() == (L.n, int((g.mask == 0).sum()), L.n - kept)
        if name == "sphere_seam":
            assert not (got == 2).any()
        else:
            assert kept > 0
    finally:
        L.destroy()


# ---- 2: the plain collide

@pytest.mark.parametrize("name", NAMES)
def test_plain_collide(orc, gpu, padded, name):
    """collide_stream_kernel<false, false>.  On all_solid (max_active forced to 1) the launch runs and writes nothing: the
    populations the upload stored come back after an even number of steps, and the other buffer still holds its zeros"""
    g = G.GEOMETRIES[name]
    want, _ = _oracle_plain(orc, name)
    L = _device_lattice(gpu, g)
    try:
        f0 = L.populations()
        _same_on_fluid(f0, G.start_state(g), g.mask, name + ", upload")
        for n, f in zip(STEPS, want):
            L.collideAndStream(n)
            got = L.populations()
            _same_on_fluid(got, f, g.mask, "%s, %d step(s)" % (name, n))
            if name == "all_solid":
                assert np.array_equal(got, f0 if n == 9 else np.zeros_like(f0))
        if name != "all_solid":
            assert not np.array_equal(want[1][g.mask.reshape(-1) == 0], want[0][g.mask.reshape(-1) == 0])
    finally:
        L.destroy()


# ---- 3: the geometry replaced on a live lattice

def test_geometry_replaced_on_a_live_lattice(orc, gpu, padded):
    """stenosis: 5 steps, then defineBounceBack with the mask shifted by 7 planes in x (the map is rebuilt, the old blocks are
    freed), fresh random populations on both sides so that stale wall slots play no part, 5 more steps; three times over"""
    g = G.GEOMETRIES["stenosis"]
    Lo = G.oracle_lattice(orc, g)
    L = _device_lattice(gpu, g)
    try:
        mask = g.mask
        for k in range(3):
            Lo.collide_stream(5); L.collideAndStream(5)
            _same_on_fluid(L.populations(), Lo.f, mask, "before change %d" % k)
            mask = np.roll(mask, 7, axis=0)
            assert not np.array_equal(mask, g.mask)
            Lo.set_mask(mask); L.defineBounceBack(mask)
            assert np.array_equal(L.mask(), G.classes(mask, g.periodic, padded)[0])
            f = G.start_state(g, 100 + k)
            Lo.f[:] = f; L.set_populations(f)
            Lo.collide_stream(5); L.collideAndStream(5)
            _same_on_fluid(L.populations(), Lo.f, mask, "after change %d" % k)
    finally:
        Lo.destroy(); L.destroy()


# ---- 4: body-force regions

@pytest.mark.parametrize("name", list(G.FORCE_BOXES))
def test_force_regions(orc, gpu, padded, name):
    """collide_stream_kernel<true, false>: three overlapping boxes, the last one holding a node wins"""
    g = G.GEOMETRIES[name]
    Lo = G.oracle_lattice(orc, g)
    L = _device_lattice(gpu, g)
    try:
        L.setExternalVectorBoxes(G.FORCE_BOXES[name], G.BOX_FORCES)
        for box, F in zip(G.FORCE_BOXES[name], G.BOX_FORCES):
            Lo.set_force_box(box, F)
        _run_both(Lo, L, g.mask, name + " with force boxes")
        plain = _oracle_plain(orc, name)[0][1]
        assert not np.array_equal(Lo.f[g.mask.reshape(-1) == 0], plain[g.mask.reshape(-1) == 0])   # the boxes act
    finally:
        Lo.destroy(); L.destroy()


# ---- 5: moving walls

def test_moving_walls(orc, gpu, padded):
    """thick_walls with the slab y < 3 as class 3 and the slab y >= 8 as class 4, both moving: only the layers that face the
    fluid keep their class, the nodes behind them are inert (or promoted to plain bounce-back nodes)"""
    g = G.GEOMETRIES["thick_walls"]
    mask = g.mask.copy()
    mask[:, :3, :] = 3
    mask[:, 8:, :] = 4
    u3, u4 = (0.01, 0.0, -0.004), (-0.006, 0.0, 0.003)
    Lo = G.oracle_lattice(orc, g, mask)
    L = _device_lattice(gpu, g, mask)
    try:
        Lo.set_wall_velocity(0, u3); L.setBoundaryVelocity(3, u3)
        Lo.set_wall_velocity(1, u4); L.setBoundaryVelocity(4, u4)
        want, before = G.classes(mask, g.periodic, padded)
        got = L.mask()
        assert np.array_equal(got, want)
        # the face y = 2 moves as a whole; on the face y = 8 the nodes behind the block see no fluid and lose their class
        hidden = before[:, 8, :] == 2
        assert np.all(got[:, 2, :] == 3) and np.all(got[:, 8, :][~hidden] == 4) and hidden.any() and np.all(np.isin(got[:, 8, :][hidden], (1, 2)))
        assert (got[:, :2, :] == 2).any() and (got[:, 9:, :] == 2).any()
        assert np.array_equal(got == 2, g.classes(padded)[0] == 2)   # the classes 3 and 4 change nothing about who is inert
        _run_both(Lo, L, mask, "thick_walls with moving walls")
        plain = _oracle_plain(orc, "thick_walls")[0][1]
        assert not np.array_equal(Lo.f[mask.reshape(-1) == 0], plain[mask.reshape(-1) == 0])   # the walls act
    finally:
        Lo.destroy(); L.destroy()


# ---- 6: open boundaries

def _inlet_profile(g, nodes):
    """0.02 at the axis of the pipe, falling to 0 at the wall of the widest section; u_y a tenth of u_x"""
    r2 = (nodes[:, 1] - 10.5) ** 2 + (nodes[:, 2] - 10.5) ** 2
    p = 0.02 * np.clip(1.0 - r2 / 9.5 ** 2, 0.0, None)
    return np.stack([p, 0.1 * p, np.zeros_like(p)], axis=1)


def test_open_boundaries(orc, gpu, padded):
    """collide_stream_kernel<*, true> on the stenosis without the periodic x: Zou-He velocity on the fluid nodes of x = 0,
    pressure on those of x = nx - 1.  The inlet plane has inert corners and rows that start at z0 > 0"""
    g = G.STENOSIS_OPEN
    nx = g.dims[0]
    Lo = G.oracle_lattice(orc, g)
    L = _device_lattice(gpu, g)
    try:
        inlet = np.argwhere(g.mask[0] == 0); inlet = np.c_[np.zeros(len(inlet), int), inlet]
        outlet = np.argwhere(g.mask[nx - 1] == 0); outlet = np.c_[np.full(len(outlet), nx - 1), outlet]
        first_v = L.addOpenBoundaryNodes(0, -1, inlet)
        L.setOpenBoundaryVelocitySlots(first_v, _inlet_profile(g, inlet))
        first_p = L.addOpenBoundaryNodes(1, 1, outlet)
        L.setOpenBoundaryDensitySlots(first_p, np.ones(len(outlet)))
        assert (first_v, first_p) == (0, len(inlet))
        code = -np.ones(g.dims, np.int64)
        code[tuple(inlet.T)] = (first_v + np.arange(len(inlet))) << 2 | OB.VEL_0N
        code[tuple(outlet.T)] = (first_p + np.arange(len(outlet))) << 2 | OB.PRES_0P
        val = L.openBoundaryValues(0, len(inlet) + len(outlet))
        assert np.array_equal(val[:len(inlet), :3], _inlet_profile(g, inlet)) and np.all(val[len(inlet):, 3] == 1.0)
        Lo.set_open_boundary(code, val)
        _run_both(Lo, L, g.mask, "stenosis with open boundaries")
    finally:
        Lo.destroy(); L.destroy()


# ---- 7: interior viscosity

def test_interior_viscosity(gpu, padded):
    """collide_stream_kernel<false, false, true> on the stenosis: two classes painted over boxes that hold fluid, bounce-back
    and inert nodes, against interior_viscosity_ref's collide"""
    g = G.GEOMETRIES["stenosis"]
    omegas = [1.0 / 2.1, 1.0 / 0.62]
    cls = np.zeros(g.dims, np.uint8)
    for k, box in enumerate(G.VISC_BOXES):
        cls[G.box_slices(box)] = k + 1
    L = _device_lattice(gpu, g)
    try:
        L.enableInteriorViscosity(omegas)
        L.setInteriorClasses(cls)
        assert np.array_equal(L.interiorClasses(), cls)
        S = G.start_state(g).reshape(g.dims + (19,))
        plain = S
        for n in STEPS:
            for _ in range(n):
                S = IV.step(S, g.mask, g.periodic, G.OMEGA, omegas, cls, G.BODY)
                plain = OB.step(plain, g.mask, g.periodic, G.OMEGA, G.BODY)
            L.collideAndStream(n)
            _same_on_fluid(L.populations(), S, g.mask, "stenosis with interior viscosity, %d step(s)" % n)
        assert not np.array_equal(S[g.mask == 0], plain[g.mask == 0])   # the classes act
    finally:
        L.destroy()


# ---- 8: the scalar step

@pytest.mark.parametrize("name", list(G.SOURCE_BOX))
def test_scalar_step(gpu, padded, name):
    """scalar_collide_stream_kernel has its own copy of the span search and of the class-2 return: 9 rounds of the flow's step
    and the scalar's, with a source box over fluid, bounce-back and inert nodes, against scalar_ref"""
    g = G.GEOMETRIES[name]
    tau = 0.8
    L = _device_lattice(gpu, g)
    try:
        S = L.createCEPACfield(tau)
        src = SR.Sources(g.dims)
        S.addSource(G.SOURCE_BOX[name], 1.75); src.add(G.SOURCE_BOX[name], 1.75)
        f = G.start_state(g).reshape(g.dims + (19,))
        s = np.random.default_rng(17).uniform(-0.01, 0.01, size=g.dims + (19,))
        S.set_populations(s.reshape(-1, 19))
        _same_on_fluid(S.populations(), s, g.mask, name + ", scalar upload")
        for it in range(9):
            L.collideAndStream(1)
            f = OB.step(f, g.mask, g.periodic, G.OMEGA, G.BODY)
            u = SR.velocity(f, g.mask, G.BODY)
            _same_on_fluid(S.velocity(), u, g.mask, "%s, advecting velocity, round %d" % (name, it))
            S.collideAndStream()
            s = SR.step(s, g.mask, g.periodic, 1.0 / tau, u, src)
            _same_on_fluid(S.populations(), s, g.mask, "%s, scalar, round %d" % (name, it))
        _same_on_fluid(S.concentration(), SR.concentration(s, g.mask, src), g.mask, name + ", concentration")
        _same_on_fluid(L.populations(), f, g.mask, name + ", flow beside the scalar")
    finally:
        L.destroy()


# ---- 9: Lees-Edwards

def test_lees_edwards(orc, gpu, padded):
    """le_block: a block whose inert core lies strictly inside the spans, between the fluid layers the pass needs; displacement
    0.37, wall velocities -+0.004, 20 steps against the oracle's step followed by the restated pass"""
    g = G.GEOMETRIES["le_block"]
    v_top, v_bottom, D = -0.004, 0.004, 0.37
    Lo = G.oracle_lattice(orc, g)
    L = _device_lattice(gpu, g)
    try:
        L.setLeesEdwards(v_top, v_bottom)
        L.setLeesEdwardsDisplacement(D)
        assert (L.mask() == 2).sum() == 64
        L.collideAndStream(20)
        for _ in range(20):
            Lo.collide_stream()
            LE.le_pass_inplace(Lo.f, g.dims, G.OMEGA, D, v_top, v_bottom)
        _same_on_fluid(L.populations(), Lo.f, g.mask, "le_block, 20 steps")
        assert L.leesEdwardsState()[0] == D
    finally:
        Lo.destroy(); L.destroy()


# ---- 10: the equilibrium start

@pytest.mark.parametrize("name", ["stenosis", "seam_slabs"])
def test_equilibrium_start(orc, gpu, padded, name):
    """latticeEquilibrium at rho = 1.02 and a velocity with three components: the slots towards solid neighbours start at 0,
    the neighbour found through the wraps; then 9 steps"""
    g = G.GEOMETRIES[name]
    rho, u = 1.02, (0.01, -0.004, 0.002)
    Lo = G.oracle_lattice(orc, g)
    L = _device_lattice(gpu, g)
    try:
        Lo.init_equilibrium(rho, u); L.latticeEquilibrium(rho, u)
        _same_on_fluid(L.populations(), Lo.f, g.mask, name + ", at equilibrium")
        Lo.collide_stream(9); L.collideAndStream(9)
        _same_on_fluid(L.populations(), Lo.f, g.mask, name + ", 9 steps from equilibrium")
    finally:
        Lo.destroy(); L.destroy()


# ---- 11: the observers

def _magnitude(v):
    return np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])    # the kernels' order of operations


def _stored_sum(S, periodic):
    """sum over q of the stored populations P(x, q) = S(x + c_q, q) per node, 0 where x + c_q lies outside a non-periodic
    axis (what the upload stores there and what a wall node parks there)"""
    total = 0
    for q in range(19):
        src = S[..., q]
        for ax, c in enumerate(R.C[q]):
            if c == 0:
                continue
            src = np.roll(src, -int(c), axis=ax)
            if not periodic[ax]:
                edge = [slice(None)] * 3
                edge[ax] = -1 if c == 1 else 0
                src[tuple(edge)] = 0
        total = total + src
    return total.reshape(-1)


@pytest.mark.parametrize("name", ["stenosis", "thick_walls"])
def test_observers(orc, gpu, padded, name):
    """after the 1 + 9 steps of the plain collide: rho_u, pi_neq and fluid_stats against observables_ref within
    16 * 2^-53 * sum|terms| (tests/test_gpu_observables.py), tresca within 1e-12 ||S||_F (tests/test_gpu_solidify.py), and a
    Statistics handle of each fluid set sampled twice equals twice the downloads exactly; on the fluid nodes"""
    g = G.GEOMETRIES[name]
    (_, f_ref), F = _oracle_plain(orc, name)
    fluid = g.mask.reshape(-1) == 0
    L = _device_lattice(gpu, g)
    try:
        L.collideAndStream(1); L.collideAndStream(9)
        fg = L.populations()
        _same_on_fluid(fg, f_ref, g.mask, name)
        rho, u = L.rho_u()
        pi = L.pi_neq()
        ru, pn = R.rho_u(f_ref[fluid], F[fluid]), R.pi_neq(f_ref[fluid])
        err = dict(rho=R.excess(rho[fluid], ru["rho"], ru["rho_abs"]), u=R.excess(u[fluid], ru["u"], ru["u_abs"]),
                   pi=R.excess(pi[fluid], pn["pi"], pn["pi_abs"]))
        assert max(err.values()) <= 1, err
        # tresca: eigvalsh on S built from the downloaded pi_neq and rho
        want, norm = solidify_ref.tresca(pi, rho, G.OMEGA, g.mask)
        got = L.tresca()
        assert np.all(np.abs(got - want)[fluid] <= 1e-12 * norm[fluid]) and np.all(got[~fluid] == 0.0) and got[fluid].max() > 0
        # FluidInfo: |u| and |F| over the fluid nodes
        for what, vec, vabs in ((0, ru["u"], ru["u_abs"]), (1, F[fluid], np.abs(F[fluid]))):
            mn, mx, avg, n = L.fluid_stats(what)
            m_ref = _magnitude(np.asarray(vec, dtype=np.float64))
            bound = 16 * 2.0 ** -53 * _magnitude(np.asarray(vabs, dtype=np.float64)) + 2.0 ** -52 * m_ref
            assert n == fluid.sum()
            if what == 1:
                assert mn == m_ref.min() and mx == m_ref.max()
            else:
                own = _magnitude(u[fluid])
                assert mn == own.min() and mx == own.max()
                assert abs(mn - m_ref.min()) <= bound.max() and abs(mx - m_ref.max()) <= bound.max()
            assert abs(avg - m_ref.mean()) <= bound.max() + 1e-14 * m_ref.mean()
        # mass: the stored populations of every bulk node, inert ones included, from the device's own post-stream rows
        S4 = R.hp(fg).reshape(g.dims + (19,))
        mass, mass_abs = R.to_double(_stored_sum(S4, g.periodic)), R.to_double(_stored_sum(np.abs(S4), g.periodic))
        mn, mx, avg, n = L.fluid_stats(2)
        b = 16 * 2.0 ** -53 * mass_abs.max()
        assert n == L.n
        assert abs(mn - mass.min()) <= b and abs(mx - mass.max()) <= b and abs(avg - mass.mean()) <= b
        # running statistics: two samples of an unchanged state
        uu = np.stack([u[:, a] * u[:, b] for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))], axis=1)
        once = {1: np.c_[rho, u], 2: uu, 4: pi}
        for what in (1, 2, 4):
            st = gpu.Statistics(L, what=what)
            try:
                st.sample(); st.sample()
                assert st.samples == 2
                got = st.sums(what)
            finally:
                st.destroy()
            assert np.array_equal(got[fluid], (once[what] + once[what])[fluid]), what
    finally:
        L.destroy()


# ---- 12: slabs

SLAB_STEPS = 12


def _slab_rank(rank, world):
    """one rank of the stenosis cut into `world` x-slabs, no cells: the class map and the populations after 12 hc_iterate
    steps, with the plain and with the padded plane stride"""
    from hemocell_amd import host
    from hemocell_amd.slab import SlabRunner
    g = G.GEOMETRIES["stenosis"]
    nx = g.dims[0] // world
    lib = host.capi.lib()
    f0 = G.start_state(g).reshape(g.dims + (19,))
    out = {}
    for tag, padded in (("plain", False), ("padded", True)):
        host.check(lib.hc_debug_force_plane_padding(1 if padded else 0))
        try:
            r = SlabRunner(nx, g.dims[1], g.dims[2], rank, world, host.base_parameters(), periodic=(True, False, False))
        finally:
            host.check(lib.hc_debug_force_plane_padding(0))
        r.define_bounce_back(g.mask)
        r.lattice.setExternalVector(G.BODY)
        r.lattice.set_populations(f0[r.x0:r.x0 + nx].reshape(-1, 19))   # collective
        out[tag + "__mask"] = r.lattice.mask()
        r.run(SLAB_STEPS)
        out[tag + "__f"] = r.populations()
        r.cells.destroy()
        r.lattice.destroy()
    return out


@pytest.mark.parametrize("world", [2, 4])
def test_slabs(tmp_path, gpu, world):
    """the stenosis, fluid only, cut into 2 and into 4 x-slabs (10 and 5 planes: the slab set-up accepts 5 planes when the
    container holds no cell type), 12 hc_iterate steps: the split launch over planes with different active counts, the halo
    planes carrying the neighbour's classes.  Every slab's class map is the rule applied to its planes, and the populations
    equal the single domain's bit for bit on fluid nodes, plain and padded"""
    g = G.GEOMETRIES["stenosis"]
    P = gpu.base_parameters()
    lib = gpu.capi.lib()
    single = {}
    for tag, padded in (("plain", False), ("padded", True)):   # before the ranks start: they share the GPU
        gpu.check(lib.hc_debug_force_plane_padding(1 if padded else 0))
        try:
            L = _device_lattice(gpu, g, omega=1.0 / P.tau)
        finally:
            gpu.check(lib.hc_debug_force_plane_padding(0))
        h = gpu.HemoCell(L, P)
        h.setParticleVelocityUpdateTimeScaleSeparation(5)
        try:
            h.iterate(SLAB_STEPS)
            single[tag] = L.populations()
        finally:
            h.cellfields.destroy(); L.destroy()
    assert np.array_equal(single["plain"][g.mask.reshape(-1) == 0], single["padded"][g.mask.reshape(-1) == 0])
    res = slab_ranks.run(_slab_rank, world, tmp_path, salt=40 + world)
    nx = g.dims[0] // world
    for tag, padded in (("plain", False), ("padded", True)):
        for k, r in enumerate(res):
            want = G.classes(g.mask, g.periodic, padded, x0=k * nx, nx=nx)[0]
            assert np.array_equal(r[tag + "__mask"], want), (tag, k)
        got = np.concatenate([r[tag + "__f"] for r in res], axis=0)
        _same_on_fluid(got, single[tag], g.mask, "stenosis on %d slabs, %s" % (world, tag))
