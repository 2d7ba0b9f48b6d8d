"""BASELINE config C4 (stretchCell: 52 x 26 x 26 box, one RBC pulled apart at 7 + 7 vertices) vertex by vertex against
the CPU oracle, and hcp_add_vertex_force -- the one entry point that edits vertex state between two hc_iterate calls --
against its definition: the entries added to the vertex forces one after another, in list order
(helper/hemoCellStretch.cpp:63-78)."""
import ctypes as C
import os
import re
import shutil
import subprocess
import xml.etree.ElementTree as ET

import numpy as np
import pytest

from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

TOL = 1e-9          # lu, vertex positions: what C1 holds over 1000 iterations (test_gpu_parity.py::test_one_cell_shear_config_c1)
N_FORCED = 1 + 6    # examples/stretchCell/stretchCell.cpp: n_forced_lsps


def _box_walls(nx, ny, nz):
    mask = np.zeros((nx, ny, nz), np.uint8)
    mask[0] = mask[-1] = 1; mask[:, 0] = mask[:, -1] = 1; mask[:, :, 0] = mask[:, :, -1] = 1
    return mask


def _oracle_c4(orc, force_pN, k_p=1, P=None, centre_um=(12.0, 6.0, 6.0), angles_deg=(90.0, 0.0, 0.0), rbc_kw=None):
    """the oracle half of C4 (tests/test_oracle_pins.py::_stretch): bounce-back walls on all six faces, one RBC, the
    N_FORCED vertices of smallest / largest x (stable order, helper/hemoCellStretch.cpp:44-60) pulled with F / N_FORCED each"""
    P = O.make_params(orc, dt=1e-7) if P is None else P
    um = 1e-6 / P.dx
    nz = int(13 * um); nx, ny = 2 * nz, nz                     # examples/stretchCell/stretchCell.cpp:55-59
    mask = _box_walls(nx, ny, nz)
    L = O.OracleLattice(orc, nx, ny, nz, (0, 0, 0), 1.0 / P.tau)
    L.set_mask(mask); L.init_equilibrium(); L.set_threads(8)
    T = O.make_rbc(orc, P, **(rbc_kw or {}))
    T.contents.timescale = 1
    S = orc.orc_sim_create(L.ptr, C.byref(P)); orc.orc_sim_add_type(S, T)
    S.contents.particle_velocity_timescale = k_p
    c = np.array(centre_um, dtype=np.float64) * um
    a = np.array(angles_deg, dtype=np.float64) * (3.14159265358979323846 / 180.0) * -1.0
    assert orc.orc_sim_add_cell(S, 0, O.dptr(c), O.dptr(a), 0.0) == 1
    o = dict(orc=orc, P=P, L=L, T=T, S=S, mask=mask, um=um, nv=T.contents.nv, tri=T.contents.arr("triangles").reshape(-1, 3),
             V0=T.contents.volume_eq)
    pos = _orc_positions(o)
    order = np.argsort(pos[:, 0], kind="stable")
    o["lower"], o["upper"] = order[:N_FORCED], order[-N_FORCED:][::-1]
    f = force_pN * 1e-12 / P.df / N_FORCED
    o["fm"], o["fp"] = np.array([-f, 0.0, 0.0]), np.array([f, 0.0, 0.0])
    orc.orc_sim_mechanics(S, 1)                                # the forces of the initial shape
    return o


def _orc_add(o):
    """HemoCellStretch::applyForce: lower list, then upper list"""
    for v in o["lower"]:
        o["orc"].orc_sim_add_vertex_force(o["S"], int(v), O.dptr(o["fm"]))
    for v in o["upper"]:
        o["orc"].orc_sim_add_vertex_force(o["S"], int(v), O.dptr(o["fp"]))


def _orc_positions(o):
    pos = np.zeros((o["S"].contents.np, 3))
    o["orc"].orc_sim_get(o["S"], 0, O.dptr(pos))
    return pos


def _orc_shape(o):
    """(axial, transverse) bounding-box diameters in um and the volume ratio, from the oracle's vertex positions"""
    pos = _orc_positions(o)
    a, b, c = pos[o["tri"][:, 0]], pos[o["tri"][:, 1]], pos[o["tri"][:, 2]]
    V = np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0
    bb = (pos.max(0) - pos.min(0)) / o["um"]
    return bb[0], bb[1], V / o["V0"]


def _orc_destroy(o):
    o["orc"].orc_sim_destroy(o["S"]); o["L"].destroy(); o["orc"].orc_celltype_destroy(o["T"])


def _gpu_c4(gpu, o, k_p=1):
    """the HIP half of C4 on the same box, cell and forced vertices (tests/test_gpu_parity.py::test_stretch_cell_validation_band)"""
    P = gpu.base_parameters(dt=1e-7)
    nx, ny, nz = o["mask"].shape
    L = gpu.Lattice(nx, ny, nz, (0, 0, 0), 1.0 / P.tau)
    L.defineBounceBack(o["mask"]); L.latticeEquilibrium()
    h = gpu.HemoCell(L, P)
    h.cellfields.addCellType(gpu.CellType.rbc(P), 1)
    h.setParticleVelocityUpdateTimeScaleSeparation(k_p)
    assert h.cellfields.addCell(0, np.array([12.0, 6.0, 6.0]) * o["um"], (90, 0, 0))
    pos = h.cellfields.positions
    assert np.abs(pos - _orc_positions(o)).max() <= 1e-12
    order = np.argsort(pos[:, 0], kind="stable")
    assert np.array_equal(order[:N_FORCED], o["lower"]) and np.array_equal(order[-N_FORCED:][::-1], o["upper"])
    idx = np.concatenate([o["lower"], o["upper"]])
    ff = np.concatenate([np.tile(o["fm"], (N_FORCED, 1)), np.tile(o["fp"], (N_FORCED, 1))])
    h.cellfields.applyConstitutiveModel(0, True)
    return dict(L=L, h=h, idx=idx, ff=ff)


def _gpu_shape(g, o):
    info = g["h"].cellfields.cell_info(0)
    bb = info["bbox"][0] / o["um"]
    return bb[1] - bb[0], bb[3] - bb[2], info["volume"][0] / o["V0"]


def _gpu_destroy(g):
    g["h"].cellfields.destroy(); g["L"].destroy()


@pytest.mark.parametrize("spread", ["atomic", "reproducible"])
@pytest.mark.parametrize("force", [25, 75, 125])
def test_stretch_vs_oracle(orc, gpu, force, spread):
    """C4 at 25 / 75 / 125 pN, 2000 iterations at dt 1e-7, both spread kernels: every 100 iterations all vertex positions
    within 1e-9 lu of the oracle's and the axial / transverse diameters within 1e-9 um; at the end the fluid populations
    within 1e-6 relative, the volume ratio within 1e-9 relative, one cell.
    At 25 pN a second oracle adds the forces one iteration late (after orc_sim_iterate instead of before): after 200
    iterations it is at least 100 x the tolerance away from the HIP run, so the comparison sees a mis-scheduled force."""
    lib = gpu.capi.lib()
    gpu.check(lib.hc_set_reproducible_spread(1 if spread == "reproducible" else 0))
    o = g = late = None
    try:
        o = _oracle_c4(orc, float(force))
        g = _gpu_c4(gpu, o)
        late = _oracle_c4(orc, float(force)) if force == 25 else None
        cf = g["h"].cellfields
        drift = []
        for it in range(1, 2001):
            _orc_add(o); orc.orc_sim_iterate(o["S"])
            cf.addVertexForce(g["idx"], g["ff"]); g["h"].iterate(1)   # cellStretch.applyForce(); hemocell.iterate()
            if late is not None and it <= 200:
                orc.orc_sim_iterate(late["S"]); _orc_add(late)
            if it % 100 == 0:
                pg = cf.positions
                d = np.abs(pg - _orc_positions(o)).max()
                drift.append((it, d))
                assert d <= TOL, (it, d)
                ax_o, tr_o, _ = _orc_shape(o)
                ax_g, tr_g, _ = _gpu_shape(g, o)
                assert abs(ax_g - ax_o) <= 1e-9 and abs(tr_g - tr_o) <= 1e-9, (it, ax_g - ax_o, tr_g - tr_o)
                if late is not None and it == 200:
                    margin = np.abs(pg - _orc_positions(late)).max()
                    print("\nsensitivity control: a force one iteration late moves the vertices by %.3e lu (%.0f x the tolerance)"
                          % (margin, margin / TOL))
                    assert margin >= 100 * TOL, margin
        assert g["h"].iter == o["S"].contents.iter == 2000
        fluid = o["mask"].reshape(-1) == 0
        fo, fg = o["L"].f[fluid], g["L"].populations()[fluid]
        assert np.abs(fg - fo).max() <= 1e-6 * np.abs(fo).max()
        ax_o, tr_o, vr_o = _orc_shape(o)
        ax_g, tr_g, vr_g = _gpu_shape(g, o)
        assert abs(vr_g - vr_o) <= 1e-9 * abs(vr_o), (vr_g, vr_o)
        assert cf.counts()[1] == 1
        assert ax_o > 8.5   # the cell is stretched (7.82 um undeformed)
        print("\nC4 %d pN, %s spread: largest |dx| over 2000 iterations %.3e lu; every 100: %s"
              % (force, spread, max(d for _, d in drift), " ".join("%.1e" % d for _, d in drift)))
    finally:
        gpu.check(lib.hc_set_reproducible_spread(0))
        for x in (o, late):
            if x is not None:
                _orc_destroy(x)
        if g is not None:
            _gpu_destroy(g)


def test_vertex_forces_inside_multi_step_calls(orc, gpu):
    """C4 at 25 pN with particle velocity updates every 3 iterations and calls of 3 iterations: hc_iterate then runs the
    middle iteration's advance, mechanics and next spread on the side stream beside the collide, so forces added before a
    call travel through that schedule.  The oracle gets the forces before the first of every three iterations."""
    lib = gpu.capi.lib()
    o = _oracle_c4(orc, 25.0, k_p=3)
    g = _gpu_c4(gpu, o, k_p=3)
    h, cf = g["h"], g["h"].cellfields
    h.deletion_check_every = 10 ** 6
    gpu.check(lib.hc_profile_reset()); gpu.check(lib.hc_profile_enable(1))
    try:
        worst = 0.0
        for it in range(0, 600, 3):
            _orc_add(o)
            for _ in range(3):
                orc.orc_sim_iterate(o["S"])
            cf.addVertexForce(g["idx"], g["ff"]); h.iterate(3)
            if (it + 3) % 60 == 0:
                d = np.abs(cf.positions - _orc_positions(o)).max()
                worst = max(worst, d)
                assert d <= TOL, (it + 3, d)
    finally:
        gpu.check(lib.hc_profile_enable(0))
    ms, n = C.c_double(), C.c_long()
    gpu.check(lib.hc_profile_read(b"collide_stream_beside", C.byref(ms), C.byref(n)))
    assert n.value == 600 // 3, n.value   # the middle iteration of every call
    assert h.iter == o["S"].contents.iter == 600
    assert _orc_shape(o)[0] > 8.0   # stretched (7.82 um undeformed): the added forces did act
    print("\nC4 25 pN, calls of 3 iterations: largest |dx| %.3e lu" % worst)
    _orc_destroy(o); _gpu_destroy(g)


# ---------------------------------------------------------------------------------------------------------------------
# hcp_add_vertex_force against the sequential loop it stands for
def _four_cells(gpu):
    """RBC + PLT, two cells each, in the pipe of test_gpu_parity.py::test_cell_removed_when_it_reaches_the_wall (cell mode):
    velocities are held (updated every 1000 iterations), the second RBC moves towards the wall at 0.05 lu per iteration"""
    nx, ny, nz = 40, 34, 34
    mask, _ = gpu.pipe_mask(nx, ny, nz)
    P = gpu.base_parameters()
    L = gpu.Lattice(nx, ny, nz, (1, 0, 0), 1.0 / P.tau)
    L.defineBounceBack(mask); L.latticeEquilibrium()
    h = gpu.HemoCell(L, P); cf = h.cellfields
    cf.addCellType(gpu.CellType.rbc(P), 3); cf.addCellType(gpu.CellType.plt(P), 3)
    h.setParticleVelocityUpdateTimeScaleSeparation(1000)
    cf.setDeletionMode("cell")
    assert cf.addCell(0, (12.0, 16.5, 16.5), (90, 0, 0)) and cf.addCell(0, (30.0, 16.5, 25.0), (90, 0, 0))
    assert cf.addCell(1, (21.0, 10.0, 16.5), (10, 20, 30)) and cf.addCell(1, (21.0, 23.0, 16.5), (0, 0, 0))
    cf.applyConstitutiveModel(0, True)
    h.iterate(1)                                                       # iteration 0 interpolates
    nv, nvp = cf.types[0].nv, cf.types[1].nv
    vel = np.zeros((2 * nv + 2 * nvp, 3)); vel[nv:2 * nv, 2] = 0.05
    cf.velocities = vel
    return L, h


def _sequential(before, idx, f):
    out = before.copy()
    for i, v in enumerate(idx):
        out[v] += f[i]
    return out


def _add_and_check(cf, idx, f):
    idx = np.asarray(idx, dtype=np.int64)
    f = np.asarray(f, dtype=np.float64).reshape(len(idx), 3)
    before = cf.forces
    cf.addVertexForce(idx, f)
    after = cf.forces
    expect = _sequential(before, idx, f)
    bad = np.argwhere(after != expect)
    assert len(bad) == 0, "%d components differ, first at vertex %d: got %r, sequential sum %r" % (
        len(bad), bad[0][0], after[bad[0][0]], expect[bad[0][0]])
    return after


def _forces(rng, n):
    """magnitudes over four decades, so that a different order of the adds gives different bits"""
    return rng.standard_normal((n, 3)) * 10.0 ** rng.uniform(-7, -3, (n, 1))


def test_add_vertex_force_is_sequential_addition(gpu):
    """every call leaves exactly the forces of `F[idx[i]] += f[i]` for i in list order (the reference's loops over its
    lower / upper lists, helper/hemoCellStretch.cpp:63-78): repeated vertices within one wave and across blocks, the first
    and last vertex of each type and the two on each side of the type boundary (indices count vertices in download order,
    types back to back), a list that outgrows the staging block and one that reuses it, two calls without an iterate in
    between, an empty list, and indices into the download order right after a call in which a cell was deleted at the wall
    (the device knew, the host had not looked yet).  Out-of-range indices are refused and change nothing."""
    lib = gpu.capi.lib()
    rng = np.random.default_rng(11)
    L, h = _four_cells(gpu)
    cf = h.cellfields
    h.iterate(4)
    nv, nvp = cf.types[0].nv, cf.types[1].nv
    total, n0 = cf.counts()[0], 2 * nv
    assert total == 2 * nv + 2 * nvp
    # a vertex repeated within one 64-lane wave
    idx = [5, 17, 5, 900, 5, 17, n0 + 3, 5, n0 + 3] + list(range(100, 140))
    _add_and_check(cf, idx, _forces(rng, len(idx)))
    # one vertex 300 times among 700 entries (three blocks of 256)
    idx = rng.integers(0, total, 700)
    idx[np.sort(rng.choice(700, 300, replace=False))] = 321
    _add_and_check(cf, idx, _forces(rng, len(idx)))
    # first and last vertex of each type, the two indices on each side of the type boundary
    idx = [0, n0 - 1, n0, total - 1, n0 - 2, n0 - 1, n0, n0 + 1]
    _add_and_check(cf, idx, _forces(rng, len(idx)))
    # larger than any list so far (the staging block grows), then a smaller one (it is reused)
    idx = rng.integers(0, total, 5000)
    _add_and_check(cf, idx, _forces(rng, len(idx)))
    idx = rng.integers(0, total, 100)
    _add_and_check(cf, idx, _forces(rng, len(idx)))
    # two calls back to back, no iterate in between
    i1, i2 = rng.integers(0, total, 300), rng.integers(0, total, 40)
    f1, f2 = _forces(rng, 300), _forces(rng, 40)
    before = cf.forces
    cf.addVertexForce(i1, f1); cf.addVertexForce(i2, f2)
    assert np.array_equal(cf.forces, _sequential(_sequential(before, i1, f1), i2, f2))
    # nothing
    _add_and_check(cf, [], np.zeros((0, 3)))
    # refused: index -1 and index == number of vertices; a valid entry in front of the bad one is not applied either
    before = cf.forces
    for bad in (-1, total):
        i = np.array([3, bad], dtype=np.int64); f = np.ones((2, 3))
        assert lib.hcp_add_vertex_force(cf.ptr, gpu.lptr(i), 2, gpu.dptr(f)) != 0
        assert "hcp_add_vertex_force" in lib.hc_last_error().decode()
    assert np.array_equal(cf.forces, before)
    # and the path still works after a refusal
    h.iterate(2)
    idx = [1, n0 + 1, 1]
    _add_and_check(cf, idx, _forces(rng, len(idx)))
    L.destroy()


def test_add_vertex_force_right_after_a_cell_was_deleted(gpu):
    """cell mode: the second RBC reaches the wall and is deleted inside hc_iterate, on the device; the host compacts its
    view only when somebody asks.  Indices given to hcp_add_vertex_force right after that call are positions in the
    download that follows (the deleted cell is not in it, the platelets moved down by one RBC).  Two runs of the same
    calls with the reproducible spread give the same bits: run A downloads the forces before the call, run B calls
    hcp_add_vertex_force straight after hc_iterate; B must end where A's sequential sum does."""
    lib = gpu.capi.lib()
    gpu.check(lib.hc_set_reproducible_spread(1))
    try:
        # find the call in which the cell goes
        L, h = _four_cells(gpu)
        calls = 0
        while h.cellfields.deletion_counts()[0] == 0:
            h.iterate(1); calls += 1
            assert calls < 400
        assert calls > 10 and h.cellfields.counts()[1] == 3
        L.destroy()

        def run(download_first):
            L, h = _four_cells(gpu)
            for _ in range(calls):
                h.iterate(1)
            cf = h.cellfields
            before = cf.forces if download_first else None
            nv, nvp = cf.types[0].nv, cf.types[1].nv
            idx = np.array([0, nv - 1, nv, nv + 1, nv + nvp, nv + 2 * nvp - 1, 7], dtype=np.int64)   # no vertex twice
            f = _forces(np.random.default_rng(5), len(idx))
            cf.addVertexForce(idx, f)
            after = cf.forces
            assert cf.counts() == (nv + 2 * nvp, 3, 1)
            L.destroy()
            return before, after, idx, f

        before, after_a, idx, f = run(True)
        assert np.array_equal(after_a, _sequential(before, idx, f))
        _, after_b, _, _ = run(False)
        bad = np.argwhere(after_b != after_a)
        assert len(bad) == 0, "%d components differ, first at vertex %d" % (len(bad), bad[0][0])
    finally:
        gpu.check(lib.hc_set_reproducible_spread(0))


# ---------------------------------------------------------------------------------------------------------------------
# C4 through the C++ facade and through the reference's own driver, against the oracle
HDF5_INC, HDF5_LIB = "/opt/conda/include", "/opt/conda/lib"
HAVE_HDF5 = os.path.exists(os.path.join(HDF5_INC, "hdf5.h")) and os.path.exists(os.path.join(HDF5_LIB, "libhdf5_hl.so.100"))


def _build(tmp_path, example):
    """the recipe of tests/test_gpu_compat_driver.py::_build"""
    from hemocell_amd import capi
    out = str(tmp_path / "drv")
    libdir = os.path.dirname(capi.LIB_PATH)
    cmd = ["g++", "-std=c++14", "-O2", "-Wno-deprecated-declarations", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "hemocell_amd", "compat"), os.path.join(ROOT, example), "-o", out,
           "-L" + libdir, "-lhemocell_amd", "-Wl,-rpath," + libdir]
    if HAVE_HDF5:
        priv = tmp_path / "hdf5lib"
        priv.mkdir(exist_ok=True)
        for lib in ("libhdf5.so.103", "libhdf5_hl.so.100", "libz.so.1"):
            if not (priv / lib).exists():
                os.symlink(os.path.join(HDF5_LIB, lib), str(priv / lib))
        cmd += ["-DHEMOCELL_WITH_HDF5", "-I" + HDF5_INC, str(priv / "libhdf5_hl.so.100"), str(priv / "libhdf5.so.103"), "-Wl,-rpath," + str(priv)]
    subprocess.check_call(cmd)
    return out


def _oracle_rows(o, iters):
    """run the oracle C4 to max(iters); (axial, transverse, volume ratio) at each of iters"""
    rows = {}
    for it in range(1, max(iters) + 1):
        _orc_add(o); o["orc"].orc_sim_iterate(o["S"])
        if it in iters:
            rows[it] = _orc_shape(o)
    return rows


def test_stretch_facade_driver_vs_oracle(tmp_path, orc, gpu):
    """examples/stretch/stretch_cell.cpp (HemoCellStretch + HemoCell::iterate of the facade), 25 pN, 2000 iterations: its
    RESULT rows at iterations 1, 1000 and 2000 against the oracle -- diameters within 2e-9 um (printed with %.10f), volume
    ratio within 1e-9"""
    exe = _build(tmp_path, "examples/stretch/stretch_cell.cpp")
    work = tmp_path / "run"
    shutil.copytree(os.path.join(ROOT, "examples", "stretch"), str(work))
    r = subprocess.run([exe, "config.xml", "25", "2000"], cwd=str(work), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "CELLS 1" in r.stdout
    rows = {int(float(l.split()[1])): list(map(float, l.split()[2:])) for l in r.stdout.splitlines() if l.startswith("RESULT")}
    assert sorted(rows) == [1, 1000, 2000], sorted(rows)
    o = _oracle_c4(orc, 25.0)
    ref = _oracle_rows(o, (1, 1000, 2000))
    _orc_destroy(o)
    for it in (1, 1000, 2000):
        ax, tr, vr = rows[it]
        ax_o, tr_o, vr_o = ref[it]
        assert abs(ax - ax_o) <= 2e-9 and abs(tr - tr_o) <= 2e-9 and abs(vr - vr_o) <= 1e-9, (it, ax - ax_o, tr - tr_o, vr - vr_o)


def _ref_driver(name):
    exe = os.path.join(ROOT, "oracle", "_ref", name)
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/%s not built (needs the reference tree at build time)" % name)
    return exe


def test_reference_stretchcell_driver_vs_oracle(tmp_path, orc, gpu):
    """the reference's own stretchCell driver (examples/stretchCell/stretchCell.cpp against the facade) on
    tests/golden/stretch_validation at 25 pN, tmax 2000, tmeas 500: every row of stretch-25.log equals the oracle's
    axial / transverse diameters at that iteration to the log's six significant digits (BASELINE C4, vs reference).
    The oracle mirrors the driver's set-up: domain 26 x 13 x 13 um at the config's dx, walls on every face, parameters
    from <domain>, the material from RBC.xml, the cell from RBC.pos, stretch force / 7 on the 7 + 7 extreme-x vertices,
    the initial forces before the first iteration (loadParticles).  The driver runs no fluid warm-up (it never reads
    <warmup>)."""
    exe = _ref_driver("stretchCell")
    src = os.path.join(ROOT, "tests", "golden", "stretch_validation")
    work = tmp_path / "c4"
    shutil.copytree(src, str(work))
    cfg = open(str(work / "config.xml")).read()
    cfg = re.sub(r"<stretchForce>[^<]*</stretchForce>", "<stretchForce> 25 </stretchForce>", cfg)
    cfg = re.sub(r"<tmax>[^<]*</tmax>", "<tmax> 2000 </tmax>", cfg)
    cfg = re.sub(r"<tmeas>[^<]*</tmeas>", "<tmeas> 500 </tmeas>", cfg)
    os.chmod(str(work / "config.xml"), 0o644)                  # fixtures may be checked out read-only
    open(str(work / "config.xml"), "w").write(cfg)
    r = subprocess.run([exe, "config.xml"], cwd=str(work), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    log = np.loadtxt(str(work / "stretch-25.log"), skiprows=1, ndmin=2)
    assert log[:, 0].tolist() == [1, 500, 1000, 1500, 2000], log[:, 0]

    dom = ET.parse(str(work / "config.xml")).getroot().find("domain")
    num = lambda e, k: float(e.find(k).text)
    P = O.make_params(orc, dx=num(dom, "dx"), dt=num(dom, "dt"), nu_p=num(dom, "nuP"), rho_p=num(dom, "rhoP"), kBT=num(dom, "kBT"))
    mat = ET.parse(os.path.join(src, "RBC.xml")).getroot().find("MaterialModel")
    rbc_kw = dict(radius=num(mat, "radius"), min_tri=int(num(mat, "minNumTriangles")), kLink=num(mat, "kLink"), kArea=num(mat, "kArea"),
                  kVolume=num(mat, "kVolume"), kBend=num(mat, "kBend"), eta_m=num(mat, "eta_m"))
    lines = open(os.path.join(src, "RBC.pos")).read().split("\n")
    assert int(lines[0]) == 1
    p = [float(x) for x in lines[1].split()]
    o = _oracle_c4(orc, 25.0, P=P, centre_um=p[:3], angles_deg=p[3:6], rbc_kw=rbc_kw)
    ref = _oracle_rows(o, set(int(i) for i in log[:, 0]))
    _orc_destroy(o)
    for it, ax, tr in log:
        ax_o, tr_o, _ = ref[int(it)]
        assert abs(ax - ax_o) <= 5e-6 * ax_o and abs(tr - tr_o) <= 5e-6 * tr_o, (it, ax, ax_o, tr, tr_o)
