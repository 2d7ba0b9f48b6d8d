"""Interior viscosity through the C++ facade: examples/interior/couette_interior.cpp on tests/golden/interior_viscosity_case
(the inputs of the reference's examples/cellCollision_interior_viscosity).  The facade reads <enableInteriorViscosity> and
<viscosityRatio>, pushes the cadences, runs the passes inside iterate(), writes InteriorPoints and Omega and carries the class
field through saveCheckPoint / loadCheckPoint.  A 35-iteration run of the example equals the same case set up on the Python host
bit for bit: populations, vertices and class field."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import interior_viscosity_ref as IV

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = os.path.join(ROOT, "tests", "golden", "interior_viscosity_case")
DIMS, PERIODIC = (50, 50, 30), (True, True, False)
N = DIMS[0] * DIMS[1] * DIMS[2]
TMAX, EVERY, GRID = 35, 10, 20   # iterations 0 .. 34; membrane pass every 10, entire grid every 20 (velocity update every 5)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from tests.test_gpu_stretch import _build
    return _build(tmp_path_factory.mktemp("couette_interior"), "examples/interior/couette_interior.cpp")


def _run(exe, d, *args, cfg="config.xml"):
    if not os.path.isdir(str(d)):
        shutil.copytree(CASE, str(d))
        for f in os.listdir(str(d)):
            os.chmod(os.path.join(str(d), f), 0o644)
    env = dict(os.environ, HEMOCELL_REPRODUCIBLE_SPREAD="1")
    r = subprocess.run([exe, cfg] + [str(a) for a in args], cwd=str(d), capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    return r.stdout


def _state(d):
    raw = open(os.path.join(str(d), "interior_state.bin"), "rb").read()
    f = np.frombuffer(raw[:N * 19 * 8], dtype=np.float64).reshape(N, 19)
    pos = np.frombuffer(raw[N * 19 * 8:len(raw) - N], dtype=np.float64).reshape(-1, 3)
    cls = np.frombuffer(raw[len(raw) - N:], dtype=np.uint8).reshape(DIMS)
    return f, pos, cls


@pytest.fixture(scope="module")
def whole(exe, tmp_path_factory):
    """the uninterrupted run of TMAX iterations: its directory, output and state"""
    d = tmp_path_factory.mktemp("whole") / "run"
    out = _run(exe, d, TMAX, 0, EVERY, GRID)
    assert "DONE iteration %d" % TMAX in out
    return d, out, _state(d)


def _xml(path, *tags):
    import xml.etree.ElementTree as ET
    el = ET.parse(path).getroot()
    for t in tags:
        el = el.find(t)
    return float(el.text)


def _host_run(gpu, tmax, every, grid, ratio=None, particle_timescale=5):
    """the example's case on the Python host, from the same three files: config.xml (dx, dt, shear rate), RBC.xml (ratio) and
    RBC.pos.  The Couette walls as helper/hemocellInit.hh's iniLatticeSquareCouette sets them in the facade: the top layer
    z = nz - 1 moves with -vWall, the bottom layer z = 0 with +vWall, vWall = vHalf (nz - 2) / (nz - 1), vHalf = (nz - 1) shear / 2."""
    cfg = os.path.join(CASE, "config.xml")
    dx, dt = _xml(cfg, "domain", "dx"), _xml(cfg, "domain", "dt")
    P = gpu.base_parameters(dx=dx, dt=dt, nuP=_xml(cfg, "domain", "nuP"), rhoP=_xml(cfg, "domain", "rhoP"), kBT=_xml(cfg, "domain", "kBT"))
    nx, ny, nz = DIMS
    shear = _xml(cfg, "domain", "shearrate") * dt
    v_half = (nz - 1) * shear * 0.5
    v_wall = v_half * float(nz - 2) / float(nz - 1)
    L = gpu.Lattice(nx, ny, nz, PERIODIC, 1.0 / P.tau)
    lib = gpu.capi.lib()
    gpu.check(lib.hc_set_reproducible_spread(1))
    try:
        mask = np.zeros(DIMS, np.uint8)
        mask[:, :, nz - 1], mask[:, :, 0] = 3, 4
        L.defineBounceBack(mask)
        L.setBoundaryVelocity(3, (-v_wall, 0.0, 0.0)); L.setBoundaryVelocity(4, (v_wall, 0.0, 0.0))
        L.latticeEquilibrium(1.0, (0.0, 0.0, 0.0))
        h = gpu.HemoCell(L, P)
        h.setParticleVelocityUpdateTimeScaleSeparation(particle_timescale)
        m = gpu.read_material(os.path.join(CASE, "RBC.xml"))
        assert m["enableInteriorViscosity"] == 1.0
        rbc = gpu.CellType.rbc(P, radius=m["radius"], min_triangles=int(m["minNumTriangles"]), kLink=m["kLink"], kArea=m["kArea"],
                               kVolume=m["kVolume"], kBend=m["kBend"], eta_m=m["eta_m"], interior_viscosity=True,
                               viscosity_ratio=m["viscosityRatio"] if ratio is None else ratio)
        h.cellfields.addCellType(rbc, 1)
        h.cellfields.setInteriorViscosityTimeScaleSeparation(every, grid)
        pos = np.loadtxt(os.path.join(CASE, "RBC.pos"), skiprows=1, ndmin=2)
        for k, p in enumerate(pos):
            assert h.cellfields.addCell(0, [v * (1e-6 / P.dx) for v in p[:3]], p[3:6], cell_id=k)
        h.cellfields.applyConstitutiveModel(0, True)
        gpu.check(lib.hc_profile_enable(1)); gpu.check(lib.hc_profile_reset())
        h.iterate(tmax)
        return L.populations(), h.cellfields.positions, L.interiorClasses(), (_passes(lib, "interior_find"), _passes(lib, "interior_membrane"))
    finally:
        gpu.check(lib.hc_set_reproducible_spread(0)); gpu.check(lib.hc_profile_enable(0))
        L.destroy()


def _passes(lib, name):
    import ctypes as C
    ms, n = C.c_double(), C.c_long()
    assert lib.hc_profile_read(name.encode(), C.byref(ms), C.byref(n)) == 0
    return n.value


def test_example_equals_python_host_bit_for_bit(whole, gpu):
    """populations, vertex positions and class field of the example after 35 iterations (0 .. 34) are those of the Python host
    on the same fixture with the same cadences, and both ran the entire-grid pass twice (iterations 0, 20) and the membrane
    pass four times (0, 10, 20, 30) -- a cadence counted from 1 would give one and three.  The comparison can tell a facade
    error from none: a host run with another viscosity ratio or another velocity-update timescale differs.  (In 35
    iterations the cell hardly moves, so other cadences alone leave the state as it is: hence the counts.)"""
    out, (f, pos, cls) = whole[1], whole[2]
    assert "PASSES entire-grid 2 membrane 4" in out
    fh, ph, ch, passes = _host_run(gpu, TMAX, EVERY, GRID)
    assert passes == (2, 4)
    assert int((ch != 0).sum()) > 300 and np.abs(fh).max() > 0
    assert np.array_equal(cls, ch), int((cls != ch).sum())
    assert np.array_equal(pos, ph), float(np.abs(pos - ph).max())
    assert np.array_equal(f, fh), float(np.abs(f - fh).max())
    for kw in (dict(ratio=4.0), dict(particle_timescale=10)):
        fo, po, co, _ = _host_run(gpu, TMAX, EVERY, GRID, **kw)
        assert not (np.array_equal(fo, f) and np.array_equal(po, pos) and np.array_equal(co, cls)), kw


def test_first_iteration_tags_what_the_restatement_tags(exe, tmp_path, gpu):
    """one iteration: both passes run at iteration 0 on the positions the iteration leaves, so the class field is the
    restatement's ray cast followed by its membrane rule on the downloaded positions; tau_int is that of the XML's ratio 5"""
    out = _run(exe, tmp_path / "one", 1, 0, EVERY, GRID)
    assert "Enabling interior viscosity" in out and "is not part of this back end" not in out
    done = [l for l in out.splitlines() if l.startswith("DONE")][0].split()
    P = gpu.base_parameters(dt=1e-7)
    assert float(done[-1]) == IV.tau_interior(5.0, P.tau)
    f, pos, cls = _state(tmp_path / "one")
    assert int(done[2]) == 1 and int(done[4]) == len(pos) == 642 and int(done[6]) == int((cls != 0).sum()) > 300
    t = gpu.CellType.rbc(P)
    try:
        tab = t.tables()
    finally:
        t.destroy()
    mask = np.zeros(DIMS, np.uint8)
    mask[:, :, 0] = mask[:, :, -1] = 1
    cells = [dict(id=0, type=0, pos=pos, tri=tab["triangles"], klass=1, area_mean_eq=tab["area_mean_eq"], edge_mean_eq=tab["edge_mean_eq"])]
    want = IV.membrane(IV.find(cells, mask, PERIODIC), cells, mask, PERIODIC)
    assert np.array_equal(cls, want), int((cls != want).sum())


def test_output_fields(whole, gpu):
    """InteriorPoints holds tau_int on the tagged nodes and 0 elsewhere, Omega 1 / tau_int on the same nodes and the lattice's
    omega on the other fluid nodes"""
    from tests.test_gpu_stretch import HAVE_HDF5
    from tests.test_gpu_compat_driver import _h5_array
    if not HAVE_HDF5:
        pytest.skip("no HDF5 headers and libraries on this machine: the example was built without its HDF5 writer")
    d, _, (f, pos, cls) = whole
    P = gpu.base_parameters(dt=1e-7)
    tau_int = IV.tau_interior(5.0, P.tau)
    h5 = os.path.join(str(d), "tmp", "hdf5", "%012d" % TMAX, "Fluid.%012d.p.0.h5" % TMAX)
    assert os.path.exists(h5), os.listdir(os.path.join(str(d), "tmp"))
    shape = (DIMS[2] + 2, DIMS[1] + 2, DIMS[0] + 2)
    ip = _h5_array(h5, "InteriorPoints").reshape(shape)[1:-1, 1:-1, 1:-1].transpose(2, 1, 0)
    om = _h5_array(h5, "Omega").reshape(shape)[1:-1, 1:-1, 1:-1].transpose(2, 1, 0)
    tagged = cls != 0
    assert tagged.sum() > 300
    # the datasets are float32 and h5dump prints nine digits: compared as float32
    assert np.array_equal(ip.astype(np.float32), np.where(tagged, np.float32(tau_int), np.float32(0.0)))
    wall = np.zeros(DIMS, bool)
    wall[:, :, 0] = wall[:, :, -1] = True
    want = np.where(tagged, np.float32(1.0 / tau_int), np.float32(1.0 / P.tau))
    assert np.array_equal(om.astype(np.float32)[~wall], want[~wall])


def test_checkpoint_and_resume(exe, whole, tmp_path):
    """a run saved at iteration 20 (the resumed run starts with an entire-grid pass) and resumed ends in the bytes of the uninterrupted run: populations, vertices and class field"""
    cut = tmp_path / "cut"
    _run(exe, cut, TMAX, 20, EVERY, GRID)
    out = _run(exe, cut, TMAX, 0, EVERY, GRID, cfg="tmp/checkpoint/checkpoint.xml")
    assert "DONE iteration %d" % TMAX in out
    for got, want, name in zip(_state(cut), whole[2], ("populations", "positions", "classes")):
        assert np.array_equal(got, want), name


def test_sanity_check_of_the_cadences(exe, tmp_path):
    """core/hemoCell.cpp:614-620: a cadence the velocity-update timescale (5) does not divide ends the run with the reference's line"""
    d = tmp_path / "bad"
    shutil.copytree(CASE, str(d))
    r = subprocess.run([exe, "config.xml", "5", "0", "7", "20"], cwd=str(d), capture_output=True, text=True, timeout=300)
    assert r.returncode == 1
    assert "Velocity timescale separation cannot divide this interior viscosity timescale separation" in r.stdout + r.stderr + _logs(d)


def _logs(d):
    out = ""
    for root, _, files in os.walk(str(d)):
        for f in files:
            if "log" in f.lower():
                out += open(os.path.join(root, f), errors="replace").read()
    return out
