"""Running statistics through the C++ facade: examples/statistics/pipe_profile.cpp on tests/golden/statistics_case.
hemo::FlowStatistics (compat/flowStatistics.h) attaches an hc_stats to the facade's lattice and container, HemoCell::iterate()
samples it every <statistics><every> iterations, and write() puts the means into Statistics.<iter>.p.0.h5 beside the fluid file.
The example's raw sums equal a Python-host run of the same fixture bit for bit, and the file holds those sums divided by the
sample count, narrowed to float32."""
import os
import shutil
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = os.path.join(ROOT, "tests", "golden", "statistics_case")
DIMS, PERIODIC = (40, 30, 30), (True, True, False)
N = DIMS[0] * DIMS[1] * DIMS[2]
TMAX, EVERY = 60, 5


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """the example's run: its directory and output"""
    from tests.test_gpu_stretch import _build
    exe = _build(tmp_path_factory.mktemp("pipe_profile"), "examples/statistics/pipe_profile.cpp")
    d = str(tmp_path_factory.mktemp("run") / "case")
    shutil.copytree(CASE, d)
    for f in os.listdir(d):
        os.chmod(os.path.join(d, f), 0o644)
    env = dict(os.environ, HEMOCELL_REPRODUCIBLE_SPREAD="1")
    r = subprocess.run([exe, "config.xml"], cwd=d, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "DONE iteration %d samples %d" % (TMAX, TMAX // EVERY) in r.stdout
    return d, r.stdout


def _state(d):
    raw = np.fromfile(os.path.join(d, "statistics_state.bin"), dtype=np.int64)
    ns, o = int(raw[0]), 1
    out = {"samples": ns}
    for name, k in (("rho_u", 4), ("uu", 6), ("pi", 6)):
        out[name] = raw[o:o + N * k].view(np.float64).reshape(N, k); o += N * k
    for name in ("density_RBC", "inside_RBC", "density_PLT", "inside_PLT"):
        out[name] = raw[o:o + N].copy(); o += N
    assert o == len(raw)
    return out


def _xml(path, *tags):
    import xml.etree.ElementTree as ET
    el = ET.parse(path).getroot()
    for t in tags:
        el = el.find(t)
    return float(el.text)


@pytest.fixture(scope="module")
def host(gpu):
    """the example's case on the Python host, from the same files: the sums, the sample count and omega"""
    cfg = os.path.join(CASE, "config.xml")
    P = gpu.base_parameters(dx=_xml(cfg, "domain", "dx"), dt=_xml(cfg, "domain", "dt"), nuP=_xml(cfg, "domain", "nuP"),
                            rhoP=_xml(cfg, "domain", "rhoP"), kBT=_xml(cfg, "domain", "kBT"))
    k_m, k_p = int(_xml(cfg, "ibm", "stepMaterialEvery")), int(_xml(cfg, "ibm", "stepParticleEvery"))
    lib = gpu.capi.lib()
    gpu.check(lib.hc_set_reproducible_spread(1))
    made = []
    try:
        L = gpu.Lattice(*DIMS, PERIODIC, 1.0 / P.tau); made.append(L)
        mask = np.zeros(DIMS, np.uint8); mask[:, :, 0] = 1; mask[:, :, -1] = 1
        L.defineBounceBack(mask); L.latticeEquilibrium(1.0, (0.0, 0.0, 0.0))
        L.setExternalVector((_xml(cfg, "domain", "drivingForce"), 0.0, 0.0))
        h = gpu.HemoCell(L, P); made.insert(0, h.cellfields)
        h.setParticleVelocityUpdateTimeScaleSeparation(k_p)
        m = gpu.read_material(os.path.join(CASE, "RBC.xml"))
        rbc = gpu.CellType.rbc(P, radius=m["radius"], min_triangles=int(m["minNumTriangles"]), kLink=m["kLink"], kArea=m["kArea"],
                               kVolume=m["kVolume"], kBend=m["kBend"], eta_m=m["eta_m"])
        m = gpu.read_material(os.path.join(CASE, "PLT.xml"))
        plt = gpu.CellType.plt(P, radius=m["radius"], min_triangles=int(m["minNumTriangles"]), kLink=m["kLink"], kArea=m["kArea"],
                               kVolume=m["kVolume"], kBend=m["kBend"], eta_m=m["eta_m"], aspect_ratio=m["aspectRatio"])
        made += [rbc, plt]
        h.cellfields.addCellType(rbc, k_m); h.cellfields.addCellType(plt, k_m)
        cid = 0
        for t, name in enumerate(("RBC", "PLT")):
            for p in np.loadtxt(os.path.join(CASE, name + ".pos"), skiprows=1, ndmin=2):
                assert h.cellfields.addCell(t, [v * (1e-6 / P.dx) for v in p[:3]], p[3:6], cell_id=cid)
                cid += 1
        st = gpu.Statistics(L, h.cellfields, what=31, every=EVERY); made.insert(0, st)
        h.cellfields.applyConstitutiveModel(0, True)
        h.iterate(TMAX)
        out = {"samples": st.samples, "rho_u": st.sums(1), "uu": st.sums(2), "pi": st.sums(4), "omega": 1.0 / P.tau, "mask": mask}
        for t, name in enumerate(("RBC", "PLT")):
            out["density_" + name], out["inside_" + name] = st.counts(8, t), st.counts(16, t)
        return out
    finally:
        for x in made:
            x.destroy()
        gpu.check(lib.hc_set_reproducible_spread(0))


def test_example_sums_equal_python_host_bit_for_bit(run, host):
    got = _state(run[0])
    assert got["samples"] == host["samples"] == TMAX // EVERY
    for name in ("rho_u", "uu", "pi", "density_RBC", "inside_RBC", "density_PLT", "inside_PLT"):
        assert np.array_equal(got[name], host[name]), name
    assert got["inside_RBC"].max() == got["samples"] and got["density_PLT"].sum() > 0 and got["inside_PLT"].sum() > 0
    assert np.abs(got["rho_u"][:, 1]).max() > 0


def test_printed_profiles(run):
    """the samples and one profile line per plane; <u_x> is zero on the two wall planes and positive between them, and no red
    cell reaches the planes next to the walls"""
    rows = [l.split() for l in run[1].splitlines() if l.startswith("PROFILE")]
    assert "SAMPLES %d iteration %d" % (TMAX // EVERY, TMAX) in run[1] and len(rows) == DIMS[2]
    u = np.array([float(r[4]) for r in rows]); hct = np.array([float(r[6]) for r in rows])
    assert u[0] == 0.0 and u[-1] == 0.0 and (u[1:-1] > 0).all() and u[DIMS[2] // 2] > u[1]
    assert hct[:3].max() == 0.0 and hct[-2:].max() == 0.0 and hct.max() > 0.02


def test_statistics_file(run, host):
    """dataset names and shapes through h5dump, and every dataset against the host's sums after the same float32 narrowing"""
    from tests.test_gpu_stretch import HAVE_HDF5
    from tests.test_gpu_compat_driver import _h5_array
    if not HAVE_HDF5:
        pytest.skip("no HDF5 headers and libraries on this machine: the example was built without its HDF5 writer")
    h5dir = os.path.join(run[0], "tmp", "hdf5", "%012d" % TMAX)
    h5 = os.path.join(h5dir, "Statistics.%012d.p.0.h5" % TMAX)
    assert os.path.exists(h5) and os.path.exists(os.path.join(h5dir, "Fluid.%012d.p.0.h5" % TMAX)), os.listdir(h5dir)
    hdr = subprocess.run(["/opt/conda/bin/h5dump", "-H", h5], capture_output=True, text=True).stdout
    ext = "( %d, %d, %d, " % (DIMS[2] + 2, DIMS[1] + 2, DIMS[0] + 2)
    comps = {"MeanVelocity": 3, "MeanDensity": 1, "VelocityCovariance": 6, "MeanShearStress": 6, "CellDensity_RBC": 1,
             "Hematocrit_RBC": 1, "CellDensity_PLT": 1, "Hematocrit_PLT": 1}
    for name, c in comps.items():
        assert 'DATASET "%s"' % name in hdr and ext + "%d )" % c in hdr, name
    assert hdr.count("DATASET ") == len(comps) and "H5T_IEEE_F32LE" in hdr and 'ATTRIBUTE "numberOfSamples"' in hdr

    def interior(name):   # [n][c] in the lattice's node order, the envelope taken off
        a = _h5_array(h5, name).reshape(DIMS[2] + 2, DIMS[1] + 2, DIMS[0] + 2, comps[name])
        return a[1:-1, 1:-1, 1:-1].transpose(2, 1, 0, 3).reshape(N, comps[name]).astype(np.float32)

    n = float(host["samples"])
    wall = host["mask"].reshape(-1) != 0
    u = host["rho_u"][:, 1:] / n
    want = {"MeanVelocity": np.where(wall[:, None], 0.0, u), "MeanDensity": np.where(wall, 1.0, host["rho_u"][:, 0] / n)[:, None]}
    pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    cov = host["uu"] / n - np.stack([u[:, a] * u[:, b] for a, b in pairs], axis=1)
    want["VelocityCovariance"] = np.where(wall[:, None], 0.0, cov)
    want["MeanShearStress"] = np.where(wall[:, None], 0.0, (0.5 * host["omega"] - 1.0) * (host["pi"] / n))
    for name in ("RBC", "PLT"):
        want["CellDensity_" + name] = (host["density_" + name].astype(np.float64) / n)[:, None]
        want["Hematocrit_" + name] = (host["inside_" + name].astype(np.float64) / n)[:, None]
    for name in comps:
        assert np.array_equal(interior(name), want[name].astype(np.float32)), name
    assert np.abs(want["MeanShearStress"]).max() > 0 and want["Hematocrit_RBC"].max() == 1.0
