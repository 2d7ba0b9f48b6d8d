"""Solidify mechanics through the C++ facade: examples/solidify/solidify_channel.cpp on tests/golden/solidify_case with a
position file of the test's own (the fixture's first platelet is rejected at placement, its others stay out of reach of the
floor within a short run).  The example equals a Python-host run bit for bit, writes BindingSites and Boundary from the live
fields, and resumes from a checkpoint written after the first solidification to the same bits."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import solidify_ref as SR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = os.path.join(ROOT, "tests", "golden", "solidify_case")
DIMS, PERIODIC = (15, 15, 15), (True, True, False)
N = 15 ** 3
TMAX, MID = 400, 300
# micrometres and degrees: one platelet turned so that its thin axis is z, lying 0.95 um above the floor (its lowest vertices keep
# a wall-free nearest node),
# one in mid-channel
POS = "2\n3.5 2.6 0.95 90 0 0\n3.0 5.5 4.0 20 0 0\n"


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from tests.test_gpu_stretch import _build
    return _build(tmp_path_factory.mktemp("solidify_channel"), "examples/solidify/solidify_channel.cpp")


def _run(exe, d, *args, cfg="config.xml"):
    if not os.path.isdir(str(d)):
        shutil.copytree(CASE, str(d))
        for f in os.listdir(str(d)):
            os.chmod(os.path.join(str(d), f), 0o644)
        open(os.path.join(str(d), "PLT.pos"), "w").write(POS)
    env = dict(os.environ, HEMOCELL_REPRODUCIBLE_SPREAD="1")
    r = subprocess.run([exe, cfg] + [str(a) for a in args], cwd=str(d), capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    return r.stdout


def _state(d):
    """(populations, mask, binding field, vertex positions, vertex flags) as the example dumped them"""
    raw = open(os.path.join(str(d), "solidify_state.bin"), "rb").read()
    f = np.frombuffer(raw[:N * 19 * 8], dtype=np.float64).reshape(N, 19)
    o = N * 19 * 8
    mask = np.frombuffer(raw[o:o + N], dtype=np.uint8).reshape(DIMS); o += N
    sites = np.frombuffer(raw[o:o + N], dtype=np.uint8).reshape(DIMS); o += N
    nv = (len(raw) - o) // 25
    pos = np.frombuffer(raw[o:o + nv * 24], dtype=np.float64).reshape(nv, 3); o += nv * 24
    return f, mask, sites, pos, np.frombuffer(raw[o:], dtype=np.uint8)


@pytest.fixture(scope="module")
def whole(exe, tmp_path_factory):
    d = tmp_path_factory.mktemp("whole") / "run"
    out = _run(exe, d, TMAX, 0, MID)
    assert "DONE iteration %d" % TMAX in out and "is not part of this back end" not in out
    return d, out, _state(d)


def _xml(path, *tags):
    import xml.etree.ElementTree as ET
    el = ET.parse(path).getroot()
    for t in tags:
        el = el.find(t)
    return float(el.text)


def _host_run(gpu, tmax):
    cfg = os.path.join(CASE, "config.xml")
    dx, dt = _xml(cfg, "domain", "dx"), _xml(cfg, "domain", "dt")
    P = gpu.base_parameters(dx=dx, dt=dt, nuP=_xml(cfg, "domain", "nuP"), rhoP=_xml(cfg, "domain", "rhoP"), kBT=_xml(cfg, "domain", "kBT"))
    u_top = _xml(cfg, "parameters", "shearRate") * 15.0 * P.dx * (P.dt / P.dx)
    every = int(_xml(cfg, "ibm", "stepParticleEvery"))
    L = gpu.Lattice(*DIMS, PERIODIC, 1.0 / P.tau)
    lib = gpu.capi.lib()
    gpu.check(lib.hc_set_reproducible_spread(1))
    try:
        mask = np.zeros(DIMS, np.uint8)
        mask[:, :, 0], mask[:, :, -1] = 1, 3
        L.defineBounceBack(mask)
        L.setBoundaryVelocity(3, (u_top, 0.0, 0.0))
        L.latticeEquilibrium(1.0, (0.0, 0.0, 0.0))
        L.populateBindingSites((0, 14, 0, 14, 0, 0))
        h = gpu.HemoCell(L, P)
        h.setParticleVelocityUpdateTimeScaleSeparation(every)
        m = gpu.read_material(os.path.join(CASE, "PLT.xml"))
        plt = gpu.CellType.plt(P, radius=m["radius"], min_triangles=int(m["minNumTriangles"]), kLink=m["kLink"], kArea=m["kArea"],
                               kVolume=m["kVolume"], kBend=m["kBend"], eta_m=m["eta_m"], aspect_ratio=m["aspectRatio"],
                               inner_edges=m["inner_edges"], solidify=(m["distanceThreshold"], m["shearThreshold"]))
        h.cellfields.addCellType(plt, int(_xml(cfg, "ibm", "stepMaterialEvery")))
        h.cellfields.setSolidifyTimeScaleSeparation(every)
        for cid, row in enumerate(POS.splitlines()[1:]):
            p = [float(v) for v in row.split()]
            assert h.cellfields.addCell(0, [v * (1e-6 / P.dx) for v in p[:3]], p[3:6], cell_id=cid)
        h.cellfields.applyConstitutiveModel(0, True)
        h.iterate(tmax)
        return L.populations(), L.mask(), L.bindingSites(), h.cellfields.positions, h.cellfields.solidifyFlags(), h.cellfields.solidify_counts()
    finally:
        gpu.check(lib.hc_set_reproducible_spread(0))
        L.destroy()


def test_example_equals_python_host_bit_for_bit(whole, gpu):
    """positions, populations, mask, binding field and flags after 400 iterations; a platelet has solidified by then"""
    out, (f, mask, sites, pos, flags) = whole[1], whole[2]
    fh, mh, sh, ph, flh, counts = _host_run(gpu, TMAX)
    done = [l for l in out.splitlines() if l.startswith("DONE")][0].split()
    assert int(done[done.index("solidified_cells") + 1]) == counts[0] >= 1 and int(done[done.index("solidified_nodes") + 1]) == counts[1] > 3
    assert np.array_equal(mask != 0, mh != 0) and np.array_equal(sites, sh) and int(sites.sum()) == 15 * 15 + counts[1]
    assert len(pos) == len(ph) and np.array_equal(pos, ph)
    assert np.array_equal(flags.astype(bool), flh)
    assert np.array_equal(f, fh), float(np.abs(f - fh).max())


def test_binding_sites_and_boundary_outputs_follow_the_fields(whole):
    """BindingSites and Boundary of the fluid file equal the downloaded fields at the end and differ from the first output;
    the first output's BindingSites are the site rule on the floor box the driver handed to cellfields->populateBindingSites"""
    from tests.test_gpu_stretch import HAVE_HDF5
    from tests.test_gpu_compat_driver import _h5_array
    if not HAVE_HDF5:
        pytest.skip("no HDF5 headers and libraries on this machine: the example was built without its HDF5 writer")
    d, _, (_, mask, sites, _, _) = whole

    def fields(it):
        h5 = os.path.join(str(d), "tmp", "hdf5", "%012d" % it, "Fluid.%012d.p.0.h5" % it)
        assert os.path.exists(h5), h5
        shape = (DIMS[2] + 2, DIMS[1] + 2, DIMS[0] + 2)
        return [_h5_array(h5, n).reshape(shape)[1:-1, 1:-1, 1:-1].transpose(2, 1, 0) for n in ("BindingSites", "Boundary")]
    b0, w0 = fields(0)
    b1, w1 = fields(MID)
    b2, w2 = fields(TMAX)
    start = np.zeros(DIMS, np.uint8)
    start[:, :, 0] = 1
    start[:, :, -1] = 1
    assert np.array_equal(b0, SR.populate(np.zeros(DIMS, np.uint8), start, PERIODIC, (0, 14, 0, 14, 0, 0)))
    assert np.array_equal(w0, start)
    assert np.array_equal(b2, sites) and np.array_equal(w2, (mask != 0).astype(np.uint8))
    assert not np.array_equal(b1, b0) and not np.array_equal(w1, w0)        # the first solidification lies before MID


def test_checkpoint_after_the_first_solidification_resumes_to_the_same_bits(exe, whole, tmp_path):
    cut = tmp_path / "cut"
    _run(exe, cut, TMAX, MID)
    out = _run(exe, cut, TMAX, 0, cfg="tmp/tmp/checkpoint.xml")   # <checkpointDirectory> tmp below <outputDirectory> tmp
    assert "DONE iteration %d" % TMAX in out
    for got, want, name in zip(_state(cut), whole[2], ("populations", "mask", "binding field", "positions", "flags")):
        assert np.array_equal(got, want), name
