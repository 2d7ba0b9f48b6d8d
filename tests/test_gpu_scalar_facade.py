"""The CEPAC field through the C++ facade: examples/cepac/cepac_channel.cpp on tests/golden/cepac_case.  The facade reads
<enableCEPACfield>, builds HemoCellFields::CEPACfield with omega = 1 / param::tau_CEPAC, takes the Palabos names of the
reference's cases/CEPAC driver, steps the field inside iterate(), writes CEPAC.<iter>.p.<block>.h5 and carries the field
through saveCheckPoint / loadCheckPoint.  A run of the example equals the same case set up on the Python host bit for bit."""
import os
import shutil
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = os.path.join(ROOT, "tests", "golden", "cepac_case")
DIMS, PERIODIC = (40, 30, 30), (True, True, False)
N = DIMS[0] * DIMS[1] * DIMS[2]
SOURCE, SOURCE_C = (18, 22, 12, 16, 1, 2), 2.0
TMAX = 20


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from tests.test_gpu_stretch import _build
    return _build(tmp_path_factory.mktemp("cepac_channel"), "examples/cepac/cepac_channel.cpp")


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
    """(scalar populations, flow populations, vertex positions) as the example dumped them"""
    raw = np.fromfile(os.path.join(str(d), "cepac_state.bin"), dtype=np.float64)
    return raw[:N * 19].reshape(N, 19), raw[N * 19:2 * N * 19].reshape(N, 19), raw[2 * N * 19:].reshape(-1, 3)


@pytest.fixture(scope="module")
def whole(exe, tmp_path_factory):
    """the uninterrupted run of TMAX iterations: its directory, output and state"""
    d = tmp_path_factory.mktemp("whole") / "run"
    out = _run(exe, d, TMAX)
    assert "DONE iteration %d" % TMAX in out and "is not part of this back end" not in out
    return d, out, _state(d)


def _xml(path, *tags):
    import xml.etree.ElementTree as ET
    el = ET.parse(path).getroot()
    for t in tags:
        el = el.find(t)
    return float(el.text)


def _host_run(gpu, tmax, source_c=SOURCE_C):
    """the example's case on the Python host, from the same files.  The Couette walls as iniLatticeSquareCouette sets them in
    the facade (tests/test_gpu_interior_viscosity_facade.py); tau_CEPAC in the example's operation order."""
    cfg = os.path.join(CASE, "config.xml")
    dx, dt = _xml(cfg, "domain", "dx"), _xml(cfg, "domain", "dt")
    P = gpu.base_parameters(dx=dx, dt=dt, nuP=_xml(cfg, "domain", "nuP"), rhoP=_xml(cfg, "domain", "rhoP"), kBT=_xml(cfg, "domain", "kBT"))
    nx, ny, nz = DIMS
    shear = _xml(cfg, "domain", "shearrate") * dt
    v_half = (nz - 1) * shear * 0.5
    v_wall = v_half * float(nz - 2) / float(nz - 1)
    D = _xml(cfg, "domain", "CEPACdiffusivity") * P.dt / (P.dx * P.dx)
    tau_cepac = 3.0 * D + 0.5
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
        h.setParticleVelocityUpdateTimeScaleSeparation(5)
        m = gpu.read_material(os.path.join(CASE, "RBC.xml"))
        rbc = gpu.CellType.rbc(P, radius=m["radius"], min_triangles=int(m["minNumTriangles"]), kLink=m["kLink"], kArea=m["kArea"],
                               kVolume=m["kVolume"], kBend=m["kBend"], eta_m=m["eta_m"])
        m = gpu.read_material(os.path.join(CASE, "PLT.xml"))
        plt = gpu.CellType.plt(P, radius=m["radius"], min_triangles=int(m["minNumTriangles"]), kLink=m["kLink"], kArea=m["kArea"],
                               kVolume=m["kVolume"], kBend=m["kBend"], eta_m=m["eta_m"], aspect_ratio=m["aspectRatio"])
        h.cellfields.addCellType(rbc, 1); h.cellfields.addCellType(plt, 1)
        cid = 0
        for t, name in enumerate(("RBC", "PLT")):
            for p in np.loadtxt(os.path.join(CASE, name + ".pos"), skiprows=1, ndmin=2):
                assert h.cellfields.addCell(t, [v * (1e-6 / P.dx) for v in p[:3]], p[3:6], cell_id=cid)
                cid += 1
        S = L.createCEPACfield(tau_cepac)
        S.initializeAtEquilibrium(1.0)
        S.addSource(SOURCE, source_c)
        h.cellfields.applyConstitutiveModel(0, True)
        h.iterate(tmax)
        return S.populations(), L.populations(), h.cellfields.positions, S.concentration(), tau_cepac
    finally:
        gpu.check(lib.hc_set_reproducible_spread(0))
        L.destroy()


def test_example_equals_python_host_bit_for_bit(whole, gpu):
    """scalar populations, flow populations and vertex positions after 20 iterations; a host run with another source value
    differs, so the comparison can tell"""
    out, (g, f, pos) = whole[1], whole[2]
    gh, fh, ph, Ch, tau = _host_run(gpu, TMAX)
    done = [l for l in out.splitlines() if l.startswith("DONE")][0].split()
    assert float(done[6]) == tau and abs(tau - 0.8) < 1e-12
    assert len(pos) == len(ph) > 642   # the red cell and the platelet
    assert Ch.max() == SOURCE_C and 1.0 < Ch.reshape(DIMS)[24, 14, 2] < SOURCE_C   # the source feeds the field
    assert np.array_equal(pos, ph), float(np.abs(pos - ph).max())
    assert np.array_equal(f, fh), float(np.abs(f - fh).max())
    assert np.array_equal(g, gh), float(np.abs(g - gh).max())
    go = _host_run(gpu, TMAX, source_c=1.5)[0]
    assert not np.array_equal(go, g)


def test_density_in_the_cepac_file_is_the_concentration(whole, gpu):
    from tests.test_gpu_stretch import HAVE_HDF5
    from tests.test_gpu_compat_driver import _h5_array
    if not HAVE_HDF5:
        pytest.skip("no HDF5 headers and libraries on this machine: the example was built without its HDF5 writer")
    d = whole[0]
    h5dir = os.path.join(str(d), "tmp", "hdf5", "%012d" % TMAX)
    h5 = os.path.join(h5dir, "CEPAC.%012d.p.0.h5" % TMAX)
    assert os.path.exists(h5) and os.path.exists(os.path.join(h5dir, "Fluid.%012d.p.0.h5" % TMAX)), os.listdir(h5dir)
    shape = (DIMS[2] + 2, DIMS[1] + 2, DIMS[0] + 2)
    dens = _h5_array(h5, "Density").reshape(shape)[1:-1, 1:-1, 1:-1].transpose(2, 1, 0)
    Ch = _host_run(gpu, TMAX)[3].reshape(DIMS)
    # the dataset is float32 and h5dump prints nine digits: compared as float32
    assert np.array_equal(dens.astype(np.float32), Ch.astype(np.float32))
    assert dens[20, 14, 1] == np.float32(SOURCE_C)


def test_checkpoint_and_resume(exe, whole, tmp_path):
    """20 iterations equal 10, then checkpoint, then resume, then 10: scalar and flow populations and vertices"""
    cut = tmp_path / "cut"
    _run(exe, cut, TMAX, 10)
    out = _run(exe, cut, TMAX, 0, cfg="tmp/checkpoint/checkpoint.xml")
    assert "DONE iteration %d" % TMAX in out
    for got, want, name in zip(_state(cut), whole[2], ("scalar populations", "flow populations", "positions")):
        assert np.array_equal(got, want), name


def test_tau_cepac_at_or_below_one_half_is_refused(exe, tmp_path):
    """a diffusivity of 0 gives tau_CEPAC = 0.5: the run ends with a line that names the parameter"""
    d = tmp_path / "bad"
    shutil.copytree(CASE, str(d))
    cfg = os.path.join(str(d), "config.xml")
    os.chmod(cfg, 0o644)
    txt = open(cfg).read().replace("<CEPACdiffusivity> 2.5e-7 </CEPACdiffusivity>", "<CEPACdiffusivity> 0.0 </CEPACdiffusivity>")
    open(cfg, "w").write(txt)
    r = subprocess.run([exe, "config.xml", "2"], cwd=str(d), capture_output=True, text=True, timeout=300)
    log = r.stdout + r.stderr
    for root, _, files in os.walk(str(d)):
        for f in files:
            if "log" in f.lower():
                log += open(os.path.join(root, f), errors="replace").read()
    assert r.returncode == 1 and "param::tau_CEPAC is 0.5" in log
