"""Lees-Edwards boundary on the GPU against the restatement in tests/lees_edwards_ref.py: the pass alone, fluid-only runs
and a coupled run against oracle steps with the pass inserted after the stream, the facade driver against the Python host,
the refusals, and the shear profile of the reference's 50^3 case."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import lees_edwards_ref as LE
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = os.path.join(ROOT, "tests", "golden", "lees_edwards_case")
pytestmark = pytest.mark.gpu
TOL = 1e-9   # lu, vertex positions (as tests/test_gpu_stretch.py)


def _random_state(n, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-0.01, 0.01, size=(n, 19))


@pytest.mark.parametrize("D", [0.0, 0.37, 1.0, 12.75, "nx-0.2", -0.6])
def test_pass_alone_bit_for_bit(gpu, D):
    dims = (37, 9, 11)   # odd, nx not a multiple of 64
    nx, ny, nz = dims
    D = nx - 0.2 if D == "nx-0.2" else float(D)
    omega = 1.0 / 1.37
    L = gpu.Lattice(nx, ny, nz, (True, True, True), omega)
    try:
        f0 = _random_state(L.n, 11)
        L.set_populations(f0)
        L.setLeesEdwards(-0.013, 0.011)
        assert L.leesEdwardsState() == (0.0, -0.013, 0.011, 0.0)
        L.setLeesEdwardsDisplacement(D)
        L.applyLeesEdwards()
        got = L.populations()
        want = LE.le_pass(f0, dims, omega, D, -0.013, 0.011)
        assert np.array_equal(got, want), np.abs(got - want).max()
        assert not np.array_equal(got, f0)
    finally:
        L.destroy()


def _fluid_pair(orc, gpu, dims, omega, F, seed):
    nx, ny, nz = dims
    o = O.OracleLattice(orc, nx, ny, nz, (1, 1, 1), omega)
    o.set_force_uniform(F)
    f0 = _random_state(o.n, seed) * 0.1
    o.f[...] = f0
    L = gpu.Lattice(nx, ny, nz, (True, True, True), omega)
    L.set_populations(f0)
    L.setExternalVector(F)
    return o, L


DIMS = (21, 7, 13)
OMEGA = 1.0 / 1.82
F_BODY = (1e-6, -2e-7, 3e-7)
V_TOP, V_BOTTOM = -0.004, 0.004


def test_fluid_collide_stream_fixed_displacement(orc, gpu):
    """200 hcl_collide_stream steps at D = 2.3 with a body force: oracle step + pass, bit for bit; hcl_collide_stream leaves D"""
    o, L = _fluid_pair(orc, gpu, DIMS, OMEGA, F_BODY, 5)
    try:
        L.setLeesEdwards(V_TOP, V_BOTTOM)
        L.setLeesEdwardsDisplacement(2.3, 0.013)
        for _ in range(4):
            L.collideAndStream(50)
        for _ in range(200):
            o.collide_stream()
            LE.le_pass_inplace(o.f, DIMS, OMEGA, 2.3, V_TOP, V_BOTTOM)
        assert np.array_equal(L.populations(), o.f)
        assert L.leesEdwardsState()[0] == 2.3
    finally:
        o.destroy(); L.destroy()


def test_fluid_hc_iterate_schedule(orc, gpu):
    """200 hc_iterate steps (calls of 1, 7 and 50 steps) with d = 0.013 lu per step, so that D crosses integers: the step that
    starts at iteration it uses D = fmod(d it, nx), bit for bit; the library ends with D = fmod(200 d, nx)"""
    d = 0.013
    o, L = _fluid_pair(orc, gpu, DIMS, OMEGA, F_BODY, 6)
    P = gpu.base_parameters()
    h = gpu.HemoCell(L, P)
    try:
        L.setLeesEdwards(V_TOP, V_BOTTOM)
        L.setLeesEdwardsDisplacement(0.0, d)
        for n in [1, 7, 50, 50, 50, 42]:
            h.iterate(n)
        assert h.iter == 200
        for it in range(200):
            o.collide_stream()
            LE.le_pass_inplace(o.f, DIMS, OMEGA, LE.displacement(d, it, DIMS[0]), V_TOP, V_BOTTOM)
        assert np.array_equal(L.populations(), o.f)
        assert L.leesEdwardsState()[0] == math.fmod(d * 200, float(DIMS[0]))
    finally:
        h.cellfields.destroy(); o.destroy(); L.destroy()


def test_fluid_initialize_pass(orc, gpu):
    """the pass of lattice->initialize() on the equilibrium state, then 200 steps"""
    nx, ny, nz = DIMS
    o = O.OracleLattice(orc, nx, ny, nz, (1, 1, 1), OMEGA)
    o.init_equilibrium(1.0, (0.002, 0.0, 0.0)); o.set_force_uniform(F_BODY)
    L = gpu.Lattice(nx, ny, nz, (True, True, True), OMEGA)
    try:
        L.latticeEquilibrium(1.0, (0.002, 0.0, 0.0)); L.setExternalVector(F_BODY)
        L.setLeesEdwards(V_TOP, V_BOTTOM)
        L.applyLeesEdwards()
        LE.le_pass_inplace(o.f, DIMS, OMEGA, 0.0, V_TOP, V_BOTTOM)
        assert np.array_equal(L.populations(), o.f)
        L.collideAndStream(200)
        for _ in range(200):
            o.collide_stream()
            LE.le_pass_inplace(o.f, DIMS, OMEGA, 0.0, V_TOP, V_BOTTOM)
        assert np.array_equal(L.populations(), o.f)
    finally:
        o.destroy(); L.destroy()


# ---- coupled: three RBCs, two of them across the z faces
N_BOX = 40
CELLS_LU = [(10.0, 10.0, 1.0), (30.0, 30.0, 20.0), (10.0, 30.0, 39.0)]   # examples/shear/RBC_HO.pos in lu (dx 0.5 um)
D_STEP = 0.013


def _oracle_coupled(orc, P, swaps=True, v=(-0.0195, 0.0195)):
    dims = (N_BOX,) * 3
    L = O.OracleLattice(orc, *dims, (1, 1, 1), 1.0 / P.tau)
    L.init_equilibrium(); L.set_threads(8)
    T = O.make_rbc(orc, P)
    T.contents.timescale = 20
    S = orc.orc_sim_create(L.ptr, C.byref(P)); orc.orc_sim_add_type(S, T)
    S.contents.particle_velocity_timescale = 5
    for c in CELLS_LU:
        cc = np.array(c, dtype=np.float64); a = np.zeros(3)
        assert orc.orc_sim_add_cell(S, 0, O.dptr(cc), O.dptr(a), 0.0) == 1
    orc.orc_sim_mechanics(S, 1)
    return dict(L=L, T=T, S=S, dims=dims, swaps=swaps, v=v, omega=1.0 / P.tau)


def _oracle_iterate(orc, o):
    """orc_sim_iterate with the pass after orc_collide_stream (no body force, no repulsion)"""
    S = o["S"]; it = S.contents.iter
    orc.orc_sim_spread(S)
    orc.orc_collide_stream(o["L"].ptr)
    LE.le_pass_inplace(o["L"].f, o["dims"], o["omega"], LE.displacement(D_STEP, it, N_BOX), o["v"][0], o["v"][1], o["swaps"])
    if it % 5 == 0:
        orc.orc_sim_interpolate(S)
    orc.orc_sim_advance(S)
    orc.orc_sim_mechanics(S, 0)
    o["L"].set_force_uniform((0.0, 0.0, 0.0))
    S.contents.iter = it + 1


def _oracle_positions(orc, o):
    pos = np.zeros((o["S"].contents.np, 3))
    orc.orc_sim_get(o["S"], 0, O.dptr(pos))
    return pos


@pytest.mark.parametrize("spread", ["atomic", "reproducible"])
def test_coupled_vs_oracle(orc, gpu, spread):
    """RBCs at particle cadence 5 and material cadence 20 in sheared flow (v = -+0.0195 lu, d = 0.013 lu per step): vertices
    within 1e-9 lu of the oracle over 200 iterations.  Control: the restatement without the 6 <-> 16 / 7 <-> 15 swaps is
    clearly further away."""
    lib = gpu.capi.lib()
    gpu.check(lib.hc_set_reproducible_spread(1 if spread == "reproducible" else 0))
    P = O.make_params(orc, dt=1e-7)
    o = _oracle_coupled(orc, P)
    ctl = _oracle_coupled(orc, P, swaps=False) if spread == "atomic" else None
    Pg = gpu.base_parameters(dt=1e-7)
    L = gpu.Lattice(N_BOX, N_BOX, N_BOX, (True, True, True), 1.0 / Pg.tau)
    h = None
    try:
        L.latticeEquilibrium()
        h = gpu.HemoCell(L, Pg)
        h.cellfields.addCellType(gpu.CellType.rbc(Pg), 20)
        h.setParticleVelocityUpdateTimeScaleSeparation(5)
        for c in CELLS_LU:
            assert h.cellfields.addCell(0, c, (0, 0, 0))
        h.cellfields.applyConstitutiveModel(0, True)
        L.setLeesEdwards(*o["v"])
        L.setLeesEdwardsDisplacement(0.0, D_STEP)
        assert np.abs(h.cellfields.positions - _oracle_positions(orc, o)).max() <= 1e-12
        z = h.cellfields.positions[:, 2]
        assert z.min() < 0 and z.max() > N_BOX - 1   # cells across both z faces
        worst, start = 0.0, _oracle_positions(orc, o)
        for blk in range(10):
            h.iterate(20)
            for _ in range(20):
                _oracle_iterate(orc, o)
                if ctl is not None:
                    _oracle_iterate(orc, ctl)
            d = np.abs(h.cellfields.positions - _oracle_positions(orc, o)).max()
            worst = max(worst, d)
            assert d <= TOL, (h.iter, d)
        moved = np.abs(_oracle_positions(orc, o) - start).max()
        print("\nLE coupled, %s spread: largest |dx| over 200 iterations %.3e lu (vertices moved %.3e lu)" % (spread, worst, moved))
        if ctl is not None:
            margin = np.abs(h.cellfields.positions - _oracle_positions(orc, ctl)).max()
            print("sensitivity control: without the swaps the vertices are %.3e lu away (%.0f x the tolerance)" % (margin, margin / TOL))
            assert margin >= 100 * TOL, margin
        fo, fg = o["L"].f, L.populations()
        assert np.abs(fg - fo).max() <= 1e-9 * np.abs(fo).max()
    finally:
        gpu.check(lib.hc_set_reproducible_spread(0))
        for x in (o, ctl):
            if x is not None:
                orc.orc_sim_destroy(x["S"]); x["L"].destroy(); orc.orc_celltype_destroy(x["T"])
        if h is not None:
            h.cellfields.destroy()
        L.destroy()


# ---- the facade
def _build(tmp_path):
    from hemocell_amd import capi
    out = str(tmp_path / "lees_edwards")
    libdir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wno-deprecated-declarations", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "hemocell_amd", "compat"), os.path.join(ROOT, "examples", "shear", "lees_edwards.cpp"),
                           "-o", out, "-L" + libdir, "-lhemocell_amd", "-Wl,-rpath," + libdir])
    return out


def _workdir(tmp_path, name):
    d = tmp_path / name
    d.mkdir()
    shutil.copy(os.path.join(ROOT, "examples", "shear", "config.xml"), str(d))
    shutil.copy(os.path.join(ROOT, "examples", "shear", "RBC_HO.pos"), str(d))
    shutil.copy(os.path.join(CASE, "RBC_HO.xml"), str(d))
    for f in os.listdir(str(d)):
        os.chmod(str(d / f), 0o644)
    return d


def _run(exe, d, *args, cfg="config.xml", rc=0):
    # the deterministic spread kernel: the atomic one adds in no fixed order, so two runs need not agree in the last bit
    env = dict(os.environ, HEMOCELL_REPRODUCIBLE_SPREAD="1")
    r = subprocess.run([exe, cfg] + [str(a) for a in args], cwd=str(d), capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == rc, r.stdout[-3000:] + r.stderr[-2000:]
    return r


def _state(d, n):
    raw = np.fromfile(str(d / "le_state.bin"), dtype=np.float64)
    return raw[:n * 19].reshape(n, 19), raw[n * 19:].reshape(-1, 3)


def _host_run(gpu, tmax, D_of):
    """the example's set-up on the Python host, the displacement of every step set explicitly"""
    P = gpu.base_parameters(dt=1e-7)
    L = gpu.Lattice(N_BOX, N_BOX, N_BOX, (True, True, True), 1.0 / P.tau)
    gamma = 500.0 * 1e-7
    le = gpu.LeesEdwardsBC(L, gamma, 1e-7)
    L.latticeEquilibrium()
    le.initialize(schedule=False)
    L.applyLeesEdwards()                                   # lattice->initialize()
    h = gpu.HemoCell(L, P)
    lib = gpu.capi.lib()
    gpu.check(lib.hc_set_reproducible_spread(1))
    try:
        h.cellfields.addCellType(gpu.CellType.rbc(P), 20)
        h.setParticleVelocityUpdateTimeScaleSeparation(5)
        pos = np.loadtxt(os.path.join(ROOT, "examples", "shear", "RBC_HO.pos"), skiprows=1, ndmin=2)
        for p in pos:   # readPositionsBloodCells: um * (1e-6 / dx), in the facade's storage order (these three: file order)
            assert h.cellfields.addCell(0, [v * (1e-6 / P.dx) for v in p[:3]], p[3:6])
        h.cellfields.applyConstitutiveModel(0, True)
        for it in range(tmax):
            L.setLeesEdwardsDisplacement(D_of(it, le.LEdisplacement))
            h.iterate(1)
        return L.populations(), h.cellfields.positions
    finally:
        gpu.check(lib.hc_set_reproducible_spread(0))
        h.cellfields.destroy(); L.destroy()


def test_facade_driver_update_patterns_and_checkpoint(tmp_path, gpu):
    """examples/shear/lees_edwards.cpp with updateLECurDisplacement after every iteration, every 10th and never: each equals
    a Python run with the displacements set explicitly, bit for bit; the patterns differ from each other.  A checkpoint at
    iteration 300, resumed, gives the bits of the uninterrupted 600-iteration run."""
    exe = _build(tmp_path)
    n = N_BOX ** 3
    fd = lambda d, it: math.fmod(d * it, float(N_BOX))
    patterns = {1: lambda it, d: fd(d, it), 10: lambda it, d: fd(d, it - it % 10), 0: lambda it, d: 0.0}
    results = {}
    for every, D_of in patterns.items():
        w = _workdir(tmp_path, "p%d" % every)
        r = _run(exe, w, every, 200)
        assert "DONE iteration 200 vertices" in r.stdout
        f, x = _state(w, n)
        fh, xh = _host_run(gpu, 200, D_of)
        assert np.array_equal(f, fh), (every, np.abs(f - fh).max())
        assert np.array_equal(x, xh), (every, np.abs(x - xh).max())
        results[every] = f
    assert not np.array_equal(results[1], results[0]) and not np.array_equal(results[1], results[10])
    # checkpoint and resume
    w = _workdir(tmp_path, "ck")
    _run(exe, w, 1, 600, 300)
    r = _run(exe, w, 1, 600, cfg="tmp/checkpoint/checkpoint.xml")
    assert "DONE iteration 600" in r.stdout
    f_res, x_res = _state(w, n)
    w2 = _workdir(tmp_path, "whole")
    _run(exe, w2, 1, 600)
    f_all, x_all = _state(w2, n)
    assert np.array_equal(f_res, f_all) and np.array_equal(x_res, x_all)


def test_facade_refuses_particle_shift(tmp_path, gpu):
    exe = _build(tmp_path)
    w = _workdir(tmp_path, "refuse")
    r = _run(exe, w, 1, 10, "particle-shift", rc=1)
    assert "leesEdwardsBC = true" in r.stdout + r.stderr and "is not part of this back end" in r.stdout + r.stderr


# ---- refusals and the unchanged default
def test_refusals(gpu):
    HcError = gpu.HcError
    L = gpu.Lattice(8, 6, 6, (True, True, True), 1.0, x0=0, nx_global=16, n_slabs=2)
    with pytest.raises(HcError, match="n_slabs"):
        L.setLeesEdwards(-1e-3, 1e-3)
    L.destroy()
    L = gpu.Lattice(8, 6, 6, (True, True, False), 1.0)
    with pytest.raises(HcError, match="periodic"):
        L.setLeesEdwards(-1e-3, 1e-3)
    L.destroy()
    L = gpu.Lattice(8, 6, 3, (True, True, True), 1.0)
    with pytest.raises(HcError, match="nz"):
        L.setLeesEdwards(-1e-3, 1e-3)
    L.destroy()
    for z in (0, 1, 4, 5):
        L = gpu.Lattice(8, 6, 6, (True, True, True), 1.0)
        m = np.zeros((8, 6, 6), np.uint8); m[3, 2, z] = 1
        L.defineBounceBack(m)
        with pytest.raises(HcError, match="fluid nodes only"):
            L.setLeesEdwards(-1e-3, 1e-3)
        L.destroy()
    L = gpu.Lattice(8, 6, 6, (True, True, True), 1.0)
    m = np.zeros((8, 6, 6), np.uint8); m[3, 2, 3] = 1   # a wall away from the four layers is fine
    L.defineBounceBack(m)
    L.setLeesEdwards(-1e-3, 1e-3)
    m[3, 2, 1] = 1
    with pytest.raises(HcError, match="fluid nodes only"):
        L.defineBounceBack(m)
    L.destroy()
    L = gpu.Lattice(8, 6, 6, (True, True, True), 1.0)
    with pytest.raises(HcError, match="no Lees-Edwards"):
        L.applyLeesEdwards()
    L.destroy()


def test_profile_reports_lees_edwards_only_when_enabled(gpu):
    lib = gpu.capi.lib()
    ms, n = C.c_double(), C.c_long()
    gpu.check(lib.hc_profile_enable(1))
    try:
        for le in (False, True):
            gpu.check(lib.hc_profile_reset())
            L = gpu.Lattice(16, 8, 8, (True, True, True), 1.0)
            L.latticeEquilibrium()
            if le:
                L.setLeesEdwards(-1e-3, 1e-3)
            L.collideAndStream(5)
            gpu.check(lib.hc_profile_read(b"lees_edwards", C.byref(ms), C.byref(n)))
            L.destroy()
            assert n.value == (5 if le else 0) and (ms.value > 0) == le, (le, n.value, ms.value)
    finally:
        gpu.check(lib.hc_profile_enable(0)); gpu.check(lib.hc_profile_reset())


# ---- physics: the reference's 50^3 box, fluid only, to steady state
def test_shear_profile_of_the_fixture_case(gpu):
    """cases/leesEdwards without cells: 50^3, gamma = 5e-5 per step, 60 000 steps (about 10 viscous times nz^2 / nu).
    Measured on an MI355X: u_x over z = 3..46 is linear to a residual of 1.8e-17 lu (rms), falls from bottom to top with
    slope -4.7036e-5 = 0.9407 x (-gamma), and is antisymmetric (u(0) = -u(49) = 1.2004e-3 against v_bottom = 1.225e-3):
    the literal pass loses part of the imposed velocity across the two boundary layers.  The bounds below sit around those
    numbers: the ratio within [0.93, 0.95], residual below 1e-12 lu, antisymmetry to 1e-12 lu."""
    import xml.etree.ElementTree as ET
    dom = ET.parse(os.path.join(CASE, "config.xml")).getroot().find("domain")
    rd = lambda k: float(dom.find(k).text)
    dx, dt = rd("dx"), rd("dt")
    n = int(100.0 * (1e6 * dx))
    P = gpu.base_parameters(dx=dx, dt=dt, nuP=rd("nuP"), rhoP=rd("rhoP"), kBT=rd("kBT"))
    gamma = rd("shearrate") * dt
    L = gpu.Lattice(n, n, n, (True, True, True), 1.0 / P.tau)
    try:
        le = gpu.LeesEdwardsBC(L, gamma, dt)
        L.latticeEquilibrium()
        le.initialize()
        L.applyLeesEdwards()
        prof = []
        for chunk in range(6):
            L.collideAndStream(10000)
            rho, u = L.rho_u()
            prof.append(u[:, 0].reshape(n, n, n).mean(axis=(0, 1)))
        ux = prof[-1]
        z = np.arange(n, dtype=np.float64)
        inner = slice(3, n - 3)
        slope, icpt = np.polyfit(z[inner], ux[inner], 1)
        resid = ux[inner] - (slope * z[inner] + icpt)
        change = np.abs(prof[-1] - prof[-2]).max()
        print("\nLE 50^3 fixture: slope %.6e lu/lu against -gamma %.6e (ratio %.5f), rms residual %.3e, max %.3e, "
              "last-chunk change %.3e, u(0) %.6e u(nz-1) %.6e" % (slope, -gamma, slope / -gamma, np.sqrt((resid ** 2).mean()),
                                                                   np.abs(resid).max(), change, ux[0], ux[-1]))
        print("profile:", " ".join("%.4e" % v for v in ux))
        assert slope < 0 and np.all(np.diff(ux[inner]) < 0)
        assert 0.93 <= slope / -gamma <= 0.95, slope / -gamma
        assert np.sqrt((resid ** 2).mean()) < 1e-12 and change < 1e-12
        assert np.abs(ux + ux[::-1]).max() < 1e-12
    finally:
        L.destroy()
