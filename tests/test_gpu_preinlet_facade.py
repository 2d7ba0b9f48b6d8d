"""The pre-inlet through the C++ facade on the GPU: examples/preinlet/pipe_with_preinlet.cpp (hemo::PreInlet, the Zou-He names)
against the same scene built with host.Lattice, host.Cells and host.PreInlet(device=True, cells=..., cells_every=1) -- the
populations of both lattices and the particle records of both containers bit for bit after iterations 1 and N, with the
deterministic spread -- plus the pulsatile force, another direction, and the facade's refusals."""
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = os.path.join(ROOT, "tests", "golden", "preinlet_facade_case")
pytestmark = pytest.mark.gpu

HDF5_INC, HDF5_LIB, H5DUMP = "/opt/conda/include", "/opt/conda/lib", "/opt/conda/bin/h5dump"
HAVE_HDF5 = os.path.exists(os.path.join(HDF5_INC, "hdf5.h")) and os.path.exists(os.path.join(HDF5_LIB, "libhdf5_hl.so.100"))

N_ITER = 300
LENGTH_N, ENVELOPE, RE = 40, 25, 7.0   # <preInlet><parameters><lengthN>, <domain><particleEnvelope>, <preInlet><parameters><Re>
PULSE_T = [0.0, 0.25, 0.5, 0.75, 1.0]
PULSE_V = [0.6, 1.4, 1.0, 0.7, 0.6]
PULSE_FREQUENCY = 50000.0


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from hemocell_amd import capi
    out = str(tmp_path_factory.mktemp("build") / "pipe_with_preinlet")
    libdir = os.path.dirname(capi.LIB_PATH)
    cmd = ["g++", "-std=c++14", "-O2", "-Wno-deprecated-declarations", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "hemocell_amd", "compat"), os.path.join(ROOT, "examples", "preinlet", "pipe_with_preinlet.cpp"),
           "-o", out, "-L" + libdir, "-lhemocell_amd", "-Wl,-rpath," + libdir]
    if HAVE_HDF5:   # as tests/test_gpu_compat_driver.py: the two libraries by path, loaded from a private directory of links
        priv = os.path.join(os.path.dirname(out), "hdf5lib")
        os.makedirs(priv, exist_ok=True)
        for lib in ("libhdf5.so.103", "libhdf5_hl.so.100", "libz.so.1"):
            os.symlink(os.path.join(HDF5_LIB, lib), os.path.join(priv, lib))
        cmd += ["-DHEMOCELL_WITH_HDF5", "-I" + HDF5_INC, os.path.join(priv, "libhdf5_hl.so.100"), os.path.join(priv, "libhdf5.so.103"), "-Wl,-rpath," + priv]
    subprocess.check_call(cmd)
    return out


def _workdir(tmp_path, name):
    d = tmp_path / name
    shutil.copytree(CASE, str(d))
    for f in os.listdir(str(d)):
        os.chmod(str(d / f), 0o644)
    return d


def _run(exe, d, *args, rc=0, env=None):
    # the deterministic spread kernel: the atomic one adds in no fixed order, so two runs need not agree in the last bit
    e = dict(os.environ, HEMOCELL_REPRODUCIBLE_SPREAD="1")
    e.update(env or {})
    r = subprocess.run([exe, "config.xml"] + [str(a) for a in args], cwd=str(d), capture_output=True, text=True, timeout=600, env=e)
    assert r.returncode == rc, r.stdout[-3000:] + r.stderr[-2000:]
    return r.stdout + r.stderr


def _dump(d, it, sv):
    raw = open(str(d / ("preinlet_dump.%d.bin" % it)), "rb").read()
    nd, npre, rd, rp = (int(v) for v in np.frombuffer(raw, np.int64, 4))
    o = 32
    fd = np.frombuffer(raw, np.float64, nd * 19, o).reshape(nd, 19); o += nd * 19 * 8
    fp = np.frombuffer(raw, np.float64, npre * 19, o).reshape(npre, 19); o += npre * 19 * 8
    recd = np.frombuffer(raw, sv, rd, o); o += rd * 120
    recp = np.frombuffer(raw, sv, rp, o)
    return fd, fp, recd, recp


def _same_records(a, b):
    return len(a) == len(b) and a.tobytes() == b.tobytes()


def _interpolate(x):   # PreInlet::interpolate without extrapolation (helper/preInlet.cpp:841-870)
    n = len(PULSE_T)
    if x >= PULSE_T[n - 2]:
        i = n - 2
    else:
        i = 0
        while x > PULSE_T[i + 1]:
            i += 1
    xL, yL, xR, yR = PULSE_T[i], PULSE_V[i], PULSE_T[i + 1], PULSE_V[i + 1]
    if x < xL:
        yR = yL
    if x > xR:
        yL = yR
    return yL + (yR - yL) / (xR - xL) * (x - xL)


def _pulse_factor(t):   # setDrivingForceTimeDependent (:874-886)
    end = PULSE_T[-1]
    t *= PULSE_FREQUENCY * end
    t = math.fmod(t, end)
    return _interpolate(t) / (sum(PULSE_V) / len(PULSE_V))


class Scene:
    """the driver's scene on the Python host: a cylinder along the direction's axis, the pre-inlet's box by
    helper/preInlet.cpp's rules (written out here, not taken from the code under test), both containers, the coupling"""

    def __init__(self, gpu, dims, direction, with_cells):
        self.gpu, self.lib = gpu, gpu.capi.lib()
        axis, sign = "XYZ".index(direction[0]), (-1 if direction.endswith("neg") else 1)
        self.axis, self.sign = axis, sign
        P = self.P = gpu.base_parameters(dt=1e-7)
        omega = 1.0 / P.tau
        others = [d for d in range(3) if d != axis]
        na, nb = dims[others[0]], dims[others[1]]
        a, b = np.meshgrid(np.arange(na), np.arange(nb), indexing="ij")
        R = (min(na, nb) - 2) / 2.0
        wall2d = ((a - (na - 1) / 2.0) ** 2 + (b - (nb - 1) / 2.0) ** 2 > R * R).astype(np.uint8)
        fl = np.nonzero(wall2d == 0)
        # the slice's fluid box enlarged by 1 and clipped to the lattice; lengthN away from the domain on the axis
        lo = [0, 0, 0]; hi = [0, 0, 0]
        for k, d in enumerate(others):
            lo[d] = max(int(fl[k].min()) - 1, 0); hi[d] = min(int(fl[k].max()) + 1, dims[d] - 1)
        face = 0 if sign < 0 else dims[axis] - 1
        lo[axis], hi[axis] = (face - 1 - LENGTH_N, face + 1) if sign < 0 else (face - 1, face + 1 + LENGTH_N)
        self.lo = lo
        pdims = tuple(hi[d] - lo[d] + 1 for d in range(3))
        inlet = min(hi[axis], dims[axis] - 1) if sign < 0 else max(lo[axis], 0)   # fluidInlet's plane
        send_lo = inlet - LENGTH_N if sign < 0 else inlet + LENGTH_N - ENVELOPE
        window = (send_lo - lo[axis] - 0.5, send_lo + ENVELOPE - lo[axis] + 0.5)
        shift = [float(v) for v in lo]
        shift[axis] += LENGTH_N if sign < 0 else -LENGTH_N

        def extrude(n, w2):
            shape = [1, 1, 1]; shape[others[0]], shape[others[1]] = w2.shape
            reps = [1, 1, 1]; reps[axis] = n
            return np.ascontiguousarray(np.tile(w2.reshape(shape), reps))
        dmask = extrude(dims[axis], wall2d)
        pmask = extrude(pdims[axis], wall2d[lo[others[0]]:hi[others[0]] + 1, lo[others[1]]:hi[others[1]] + 1])
        periodic = [False] * 3; periodic[axis] = True
        self.dom = gpu.Lattice(*dims, (False, False, False), omega)
        self.pre = gpu.Lattice(*pdims, tuple(periodic), omega)
        self.dom.defineBounceBack(dmask); self.dom.latticeEquilibrium(1.0, (0.0, 0.0, 0.0))
        self.pre.defineBounceBack(pmask); self.pre.latticeEquilibrium(1.0, (0.0, 0.0, 0.0))
        # calculateDrivingForce: the fluid nodes of the pre-inlet's plane two inside its end
        area = int((pmask.take(2 if sign < 0 else pdims[axis] - 3, axis=axis) == 0).sum())
        _, _, self.F = gpu.preinlet_driving_force_vector(RE, P.nu_lbm, area, direction)
        self.types, self.cells = [], None
        kw = {}
        if with_cells:
            self.types = [gpu.CellType.rbc(P), gpu.CellType.plt(P)]
            pc, dc = gpu.Cells(self.pre, P), gpu.Cells(self.dom, P)
            self.cells = (pc, dc)
            for t in self.types:
                pc.addCellType(t, 4); dc.addCellType(t, 4)
            cid, total = 0, 0
            for ti, name in enumerate(("RBC", "PLT")):   # loadParticles: the file's running counter; the domain wins a tie
                rows = np.loadtxt(os.path.join(CASE, name + ".pos"), skiprows=1, ndmin=2)
                total += len(rows)
                for row in rows:
                    p = np.array([v * (1e-6 / P.dx) for v in row[:3]])
                    if all(p[d] > -0.5 and p[d] <= dims[d] - 0.5 for d in range(3)):
                        assert dc.addCell(ti, p, row[3:6], cell_id=cid)
                    else:
                        assert all(p[d] > lo[d] - 0.5 and p[d] <= hi[d] + 0.5 for d in range(3)), row
                        assert pc.addCell(ti, p - np.array(lo, dtype=np.float64), row[3:6], cell_id=cid)
                    cid += 1
            dc.applyConstitutiveModel(0, True); pc.applyConstitutiveModel(0, True)
            kw = dict(cells=(pc, dc), window=window, shift=shift, id_stride=total, sink=(float(dims[axis] - 1) if sign < 0 else 0.0),
                      cells_every=1, particle_timescale=2)
        g = np.stack(fl, axis=1)   # global in-plane coordinates of the inlet plane's fluid flags, first axis outermost
        self.coupling = gpu.PreInlet(self.pre, self.dom, g, inlet - lo[axis], inlet, direction=direction,
                                     pre_origin=(lo[others[0]], lo[others[1]]), device=True, **kw)
        outlet = [0, dims[0] - 1, 0, dims[1] - 1, 0, dims[2] - 1]
        outlet[2 * axis] = outlet[2 * axis + 1] = dims[axis] - 1 if sign < 0 else 0
        getattr(self.dom, "addPressureBoundary%d%s" % (axis, "P" if sign < 0 else "N"))(tuple(outlet))

    def step(self, n, force):
        self.pre.setExternalVector(force)
        self.coupling.iterate(n)

    def state(self):
        rec = [c.records() for c in reversed(self.cells)] if self.cells else [None, None]
        return self.dom.populations(), self.pre.populations(), rec[0], rec[1]

    def destroy(self):
        self.coupling.destroy()
        for c in self.cells or ():
            c.destroy()
        self.pre.destroy(); self.dom.destroy()
        for t in self.types:
            t.destroy()


def _compare(d, it, scene, sv):
    fd, fp, recd, recp = _dump(d, it, sv)
    hd, hp, hrd, hrp = scene.state()
    assert np.array_equal(fd, hd), (it, "domain populations", np.abs(fd - hd).max())
    assert np.array_equal(fp, hp), (it, "pre-inlet populations", np.abs(fp - hp).max())
    if hrd is not None:
        assert _same_records(recd, hrd), (it, "domain records", len(recd), len(hrd))
        assert _same_records(recp, hrp), (it, "pre-inlet records", len(recp), len(hrp))


def _logged_counts(out):
    m = re.search(r"cells injected (\d+) rejected (\d+) removed by the sink (\d+) checks (\d+)", out)
    assert m, out[-2000:]
    return tuple(int(v) for v in m.groups())


@pytest.mark.parametrize("pulse", [False, True])
def test_driver_equals_python_host_bit_for_bit(tmp_path, gpu, exe, pulse):
    """Xneg on the 64 x 34 x 34 cylinder with cells.  The Python run alone shows an injection at iteration 1 (the RBC and the PLT
    that start in the send box), one after iteration 10 (the PLT that starts just upstream) and a removal by the sink (the PLT
    near the outlet); then both dumps and the counts are the driver's.  pulse: readNormalizedVelocities(), the force of
    iteration k is setDrivingForceTimeDependent(k * dt); the Python run sets it per iteration"""
    gpu.check(gpu.capi.lib().hc_set_reproducible_spread(1))
    scene = None
    try:
        scene = Scene(gpu, (64, 34, 34), "Xneg", True)
        sv = gpu.Cells.SV_DTYPE
        force = lambda k: (0.0, 0.0, 0.0) if k == 0 else tuple(f * (_pulse_factor(k * scene.P.dt) if pulse else 1.0) for f in scene.F)
        w = _workdir(tmp_path, "run")
        out = _run(exe, w, "tmax=%d" % N_ITER, "dump=1", "pulse=%d" % int(pulse))
        scene.step(1, force(0))   # the first iteration runs unforced
        at1 = scene.coupling.cell_counts()
        print("after iteration 1:", at1)
        assert at1[0] >= 1
        _compare(w, 1, scene, sv)
        if pulse:
            for k in range(1, N_ITER):
                scene.step(1, force(k))
        else:
            scene.step(9, force(1))
            at10 = scene.coupling.cell_counts()
            scene.step(N_ITER - 10, force(1))
        counts = scene.coupling.cell_counts()
        print("after iteration %d:" % N_ITER, counts)
        if not pulse:
            assert counts[0] > at10[0], (at10, counts)   # an injection after iteration 10
        assert counts[2] >= 1 and counts[3] == N_ITER
        _compare(w, N_ITER, scene, sv)
        assert _logged_counts(out) == counts
        n_rbc = sum(c.type_range(0)[1] for c in scene.cells); n_plt = sum(c.type_range(1)[1] for c in scene.cells)
        assert "# of cells: %d | # of RBC: %d, PLT: %d" % (n_rbc + n_plt, n_rbc, n_plt) in out
    finally:
        gpu.check(gpu.capi.lib().hc_set_reproducible_spread(0))
        if scene:
            scene.destroy()


def test_ypos_fluid_only(tmp_path, gpu, exe):
    """Direction::Ypos on a 34 x 48 x 34 cylinder without cells: the pre-inlet lies above the domain and drives along -y"""
    scene = Scene(gpu, (34, 48, 34), "Ypos", False)
    try:
        w = _workdir(tmp_path, "ypos")
        out = _run(exe, w, "direction=Ypos", "nx=34", "ny=48", "nz=34", "cells=0", "tmax=120", "dump=1")
        assert "location 0 33 46 88 0 33" in out
        scene.step(1, (0.0, 0.0, 0.0))
        _compare(w, 1, scene, None)
        scene.step(119, scene.F)
        _compare(w, 120, scene, None)
        u = scene.coupling.sent()
        assert u[:, 1].min() < -1e-4   # the domain is fed along -y
    finally:
        scene.destroy()


def test_output_has_the_preinlet_as_one_more_block(tmp_path, exe):
    """writeOutput(): beside the domain's block 0 every field has a block 1, the pre-inlet, 43 x 34 x 34 nodes plus the envelope,
    whose relativePosition {z, y, x} is location's corner (-41, 0, 0) - 1.5 in SI units; its cell files hold the three cells
    that start there, in global coordinates; the CSV lists the cells of both containers"""
    assert HAVE_HDF5, "the HDF5 headers and libraries the other facade tests use are missing"
    w = _workdir(tmp_path, "out")
    _run(exe, w, "tmax=4", "output=1")
    d = str(w / "tmp" / "hdf5" / "000000000004")
    hdr = lambda f, *a: subprocess.run([H5DUMP] + list(a) + [os.path.join(d, f)], capture_output=True, text=True).stdout
    assert "( 36, 36, 66, 3 )" in hdr("Fluid.000000000004.p.0.h5", "-H")
    assert "( 36, 36, 45, 3 )" in hdr("Fluid.000000000004.p.1.h5", "-H")
    rel = [float(v) for v in re.findall(r"\(0\): ([-0-9.e, ]+)", hdr("Fluid.000000000004.p.1.h5", "-a", "/relativePosition"))[0].split(",")]
    assert np.allclose(rel, [-1.5 * 5e-7, -1.5 * 5e-7, (-41 - 1.5) * 5e-7], rtol=1e-6, atol=0)
    pid = hdr("Fluid.000000000004.p.1.h5", "-a", "/processorId")
    assert re.search(r"\(0\): 1\b", pid), pid
    count = lambda f: int(re.search(r"\(0\): (\d+)", hdr(f, "-a", "/numberOfParticles")).group(1))
    for name, n_pre, n_dom in (("RBC", 1, 1), ("PLT", 2, 2)):   # the domain: what arrived at iteration 1, and its resident PLT
        nv = count("%s.000000000004.p.0.h5" % name) // n_dom
        assert nv > 0 and count("%s.000000000004.p.0.h5" % name) == n_dom * nv and count("%s.000000000004.p.1.h5" % name) == n_pre * nv
        x = hdr("%s.000000000004.p.1.h5" % name, "-d", "/Position", "-y", "-w", "0")
        xs = [float(l.split(",")[0]) for l in x.splitlines() if re.match(r"^\s*-?[0-9.]+(e-?[0-9]+)?,", l)]
        # inside location's box, x = -41 .. 1 (a vertex across the periodic seam is written at its wrapped place, as the domain's are)
        assert len(xs) == n_pre * nv and max(xs) <= 1.5 * 5e-7 and min(xs) > -41.5 * 5e-7
        assert name != "RBC" or max(xs) < 0.0   # the RBC lies in the middle of the pre-inlet
    rows = open(str(w / "tmp" / "csv" / "PLT.000000000004.csv")).read().strip().splitlines()[1:]
    assert len(rows) == 4 and sorted(int(r.split(",")[5]) for r in rows) == [0, 0, 1, 1]   # atomic_block: two in each


def test_refusals_and_checkpoint_warning(tmp_path, exe):
    small = ["cells=0", "tmax=2"]
    out = _run(exe, _workdir(tmp_path, "twice"), "twice=1", *small, rc=1)
    assert "declared twice" in out
    out = _run(exe, _workdir(tmp_path, "load"), "checkpoint=load", *small, rc=1)
    assert "loadCheckPoint" in out and "is not part of this back end" in out
    w = _workdir(tmp_path, "save")
    out = _run(exe, w, "checkpoint=save", *small)
    assert out.count("the pre-inlet's state is not checkpointed") == 1 and "DONE iteration 2" in out
    assert not os.path.exists(str(w / "tmp" / "checkpoint"))


def test_two_ranks_are_refused(tmp_path, exe):
    w = _workdir(tmp_path, "ranks")
    port = str(36000 + os.getpid() % 20000)
    procs = []
    for rk in range(2):
        env = dict(os.environ, OMPI_COMM_WORLD_RANK=str(rk), OMPI_COMM_WORLD_SIZE="2", OMPI_COMM_WORLD_LOCAL_RANK=str(rk), HEMOCELL_PORT=port,
                   HEMOCELL_TRANSPORT="tcp", HEMOCELL_COMM_TIMEOUT="60")
        for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
            env.pop(k, None)
        procs.append(subprocess.Popen([exe, "config.xml", "cells=0", "tmax=2"], cwd=str(w), env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=300)[0] for p in procs]
    assert [p.returncode for p in procs] == [1, 1], outs
    assert "a run of 2 ranks is not part of this back end" in outs[0]
