"""GPU runs of the example drivers written against the C++ facade; the assertions are the reference's own
validation bounds, so these read like tests/validation/* of the reference."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


HDF5_INC, HDF5_LIB = "/opt/conda/include", "/opt/conda/lib"
HAVE_HDF5 = os.path.exists(os.path.join(HDF5_INC, "hdf5.h")) and os.path.exists(os.path.join(HDF5_LIB, "libhdf5_hl.so.100"))


def _build(tmp_path, example):
    from hemocell_amd import capi
    out = str(tmp_path / "drv")
    libdir = os.path.dirname(capi.LIB_PATH)
    cmd = ["g++", "-std=c++14", "-O2", "-Wno-deprecated-declarations", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "hemocell_amd", "compat"), os.path.join(ROOT, example), "-o", out,
           "-L" + libdir, "-lhemocell_amd", "-Wl,-rpath," + libdir]
    if HAVE_HDF5:
        # link the two HDF5 libraries by path and load them from a private directory of symlinks: putting
        # /opt/conda/lib itself on the search path would also pull in conda's older libstdc++
        priv = tmp_path / "hdf5lib"
        priv.mkdir(exist_ok=True)
        for lib in ("libhdf5.so.103", "libhdf5_hl.so.100", "libz.so.1"):
            if not (priv / lib).exists():
                os.symlink(os.path.join(HDF5_LIB, lib), str(priv / lib))
        cmd += ["-DHEMOCELL_WITH_HDF5", "-I" + HDF5_INC, str(priv / "libhdf5_hl.so.100"), str(priv / "libhdf5.so.103"), "-Wl,-rpath," + str(priv)]
    subprocess.check_call(cmd)
    return out


def test_stretch_driver_matches_python_host_and_band(tmp_path, gpu):
    """tests/validation/stretch_cell/test_stretch_cell.cpp:158: 25 pN -> transverse 7.3-7.9 um, axial 9.2-9.7 um;
    the C++ facade and the Python host drive the same library, so their trajectories are identical"""
    exe = _build(tmp_path, "examples/stretch/stretch_cell.cpp")
    r = subprocess.run([exe, "config.xml", "25", "10000"], cwd=os.path.join(ROOT, "examples", "stretch"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rows = [list(map(float, l.split()[1:])) for l in r.stdout.splitlines() if l.startswith("RESULT")]
    assert "CELLS 1" in r.stdout
    it, axial, transverse, vratio = rows[-1]
    assert it == 10000 and 7.3 <= transverse <= 7.9 and 9.2 <= axial <= 9.7 and 0.98 < vratio <= 1.02, rows[-1]
    # same case through the Python host layer
    P = gpu.base_parameters(dt=1e-7)
    nx, ny, nz = 52, 26, 26
    mask = np.zeros((nx, ny, nz), np.uint8)
    mask[0] = mask[-1] = 1; mask[:, 0] = mask[:, -1] = 1; mask[:, :, 0] = mask[:, :, -1] = 1
    L = gpu.Lattice(nx, ny, nz, (0, 0, 0), 1.0 / P.tau); L.defineBounceBack(mask); L.latticeEquilibrium()
    h = gpu.HemoCell(L, P); h.cellfields.addCellType(gpu.CellType.rbc(P), 1)
    assert h.cellfields.addCell(0, (24.0, 12.0, 12.0), (90, 0, 0))
    pos = h.cellfields.positions
    order = np.argsort(pos[:, 0], kind="stable")
    idx = np.concatenate([order[:7], order[-7:]])
    f = 25.0 * 1e-12 / P.df / 7
    ff = np.zeros((14, 3)); ff[:7, 0] = -f; ff[7:, 0] = f
    h.cellfields.applyConstitutiveModel(0, True)
    for _ in range(1000):
        h.cellfields.addVertexForce(idx, ff); h.iterate(1)
    bb = h.cellfields.cell_info(0)["bbox"][0] / 2.0
    row1000 = [x for x in rows if x[0] == 1000][0]
    assert abs((bb[1] - bb[0]) - row1000[1]) < 1e-9 and abs((bb[3] - bb[2]) - row1000[2]) < 1e-9
    L.destroy()


def _h5_array(path, name):
    """one dataset of an HDF5 file as a flat float array (through h5dump: no h5py in the image)"""
    dump = subprocess.run(["/opt/conda/bin/h5dump", "-d", "/" + name, "-y", "-w", "0", "-m", "%.9g", path], capture_output=True, text=True).stdout
    body = dump[dump.index("DATA {") + 6:dump.rindex("}")]
    return np.array([float(t) for t in body.replace("}", " ").replace(",", " ").split()])


def test_pipe_driver_validation_bounds(tmp_path, gpu):
    """tests/validation/pipeflow/test_pipeflow.cpp:87-106 on the synthetic pipe: the cell count stays constant,
    relative apparent viscosity in (1.03, 3.0), mean vertex force below 4 pN"""
    exe = _build(tmp_path, "examples/pipe/pipe_synthetic.cpp")
    case = str(tmp_path / "pipe"); os.makedirs(case)
    for f in ("config.xml", "RBC.xml", "PLT.xml", "RBC.pos", "PLT.pos"):
        shutil.copy(os.path.join(ROOT, "examples", "pipe", f), case)
    r = subprocess.run([exe, "config.xml"], cwd=case, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    stats = [l.split()[1:] for l in r.stdout.splitlines() if l.startswith("STAT")]
    assert len(stats) == 4
    counts = {int(s[1]) for s in stats}
    assert len(counts) == 1 and counts.pop() == 30          # 25 RBC + 5 PLT, none lost
    for s in stats:
        visc, force = float(s[4]), float(s[5])
        assert 1.03 < visc < 3.0, s
        assert force < 4.0, s
    # ---- checkpoint / resume (core/hemoCellFields.cpp:240-319): restart from the dump written at iteration 200 with
    # checkpoint.xml as the configuration, like the reference; the continuation reproduces the remaining lines exactly
    ck = os.path.join(case, "tmp_pipe", "checkpoint")
    assert os.path.exists(os.path.join(ck, "checkpoint.bin.old")) and os.path.exists(os.path.join(ck, "checkpoint.xml.old"))
    os.replace(os.path.join(ck, "checkpoint.bin.old"), os.path.join(ck, "checkpoint.bin"))     # the iteration-200 dump
    os.replace(os.path.join(ck, "checkpoint.xml.old"), os.path.join(ck, "checkpoint.xml"))
    r2 = subprocess.run([exe, "tmp_pipe/checkpoint/checkpoint.xml"], cwd=case, capture_output=True, text=True, timeout=600)
    assert r2.returncode == 0, r2.stdout[-2000:] + r2.stderr[-2000:]
    # config/config.cpp:88-174: the constructor opens a fresh directory when the configured one exists (tmp_pipe_0), loading the
    # checkpoint goes back to the one it names, and the log of the continuation does not overwrite the first (logfile.0)
    assert os.path.isdir(os.path.join(case, "tmp_pipe_0")) and os.path.exists(os.path.join(case, "tmp_pipe", "log", "logfile.0"))
    assert "resumed at iteration 200" in open(os.path.join(case, "tmp_pipe", "log", "logfile.0")).read()
    stats2 = [l for l in r2.stdout.splitlines() if l.startswith("STAT")]
    assert stats2 == [l for l in r.stdout.splitlines() if l.startswith("STAT")][2:], (stats2, stats)
    # ---- output layout (io/ParticleHdf5IO.cpp, io/FluidHdf5IO.hh, io/writeCellInfoCSV.cpp:52)
    out = os.path.join(case, "tmp_pipe")
    csv = open(os.path.join(out, "csv", "RBC.000000000400.csv")).read().splitlines()
    assert csv[0] == "X,Y,Z,area,volume,atomic_block,cellId,baseCellId,velocity_x,velocity_y,velocity_z" and len(csv) == 26
    if not HAVE_HDF5:
        return
    d = os.path.join(out, "hdf5", "000000000400")
    assert sorted(os.listdir(d)) == ["Fluid.000000000400.p.0.h5", "PLT.000000000400.p.0.h5", "RBC.000000000400.p.0.h5"]
    hdr = subprocess.run(["/opt/conda/bin/h5dump", "-H", os.path.join(d, "RBC.000000000400.p.0.h5")], capture_output=True, text=True).stdout
    for name, shape in (("Position", "( 16050, 3 )"), ("Total force", "( 16050, 3 )"), ("Volume force", "( 16050, 3 )"), ("Area force", "( 16050, 3 )"),
                        ("Bending force", "( 16050, 3 )"), ("Link force", "( 16050, 3 )"), ("Viscous force", "( 16050, 3 )"),
                        ("Cell Id", "( 16050, 1 )"), ("Vertex Id", "( 16050, 1 )"), ("Triangles", "( 32000, 3 )")):
        assert 'DATASET "%s"' % name in hdr, name
        seg = hdr[hdr.index('DATASET "%s"' % name):][:300]
        assert shape in seg, (name, seg)
    assert "H5T_IEEE_F32LE" in hdr and "H5T_STD_I32LE" in hdr
    for attr in ("dx", "dt", "iteration", "processorId", "numberOfProcessors", "numberOfParticles", "numberOfTriangles"):
        assert 'ATTRIBUTE "%s"' % attr in hdr, attr
    hp = subprocess.run(["/opt/conda/bin/h5dump", "-H", os.path.join(d, "PLT.000000000400.p.0.h5")], capture_output=True, text=True).stdout
    assert 'DATASET "InnerLinks"' in hp and "( 105, 2 )" in hp and 'DATASET "Inner link force"' in hp
    hf = subprocess.run(["/opt/conda/bin/h5dump", "-H", os.path.join(d, "Fluid.000000000400.p.0.h5")], capture_output=True, text=True).stdout
    for name, c in (("Velocity", 3), ("Force", 3), ("Density", 1), ("Boundary", 1)):
        seg = hf[hf.index('DATASET "%s"' % name):][:300]
        assert "( 54, 54, 102, %d )" % c in seg, (name, seg)      # [Nz+2][Ny+2][Nx+2][C]
    for attr in ("numberOfCells", "subdomainSize", "relativePosition", "dxdydz"):
        assert 'ATTRIBUTE "%s"' % attr in hf, attr
    # ---- values and units, checked against each other and against the CSV summary (all SI: outputInSiUnits is the default,
    # core/hemoCell.cpp:221-287): positions in m, forces in N, the separate force vectors add up to the total force
    rbc = os.path.join(d, "RBC.000000000400.p.0.h5")
    pos = _h5_array(rbc, "Position").reshape(25, 642, 3)
    cid = _h5_array(rbc, "Cell Id").reshape(25, 642)[:, 0].astype(int)
    vid = _h5_array(rbc, "Vertex Id").reshape(25, 642)
    assert (vid == np.arange(642)[None, :]).all()
    rows = {int(l.split(",")[6]): [float(x) for x in l.split(",")[:5]] for l in csv[1:]}
    cellv = np.array([[float(x) for x in l.split(",")[8:11]] for l in csv[1:]])            # mean vertex velocity of every cell [m/s] (helper/cellInfo.cpp:216-217)
    assert (cellv[:, 0] > 0).all() and cellv[:, 0].max() < 0.05 and np.abs(cellv[:, 1:]).max() < 0.2 * cellv[:, 0].max()   # carried along +x
    assert sorted(rows) == sorted(cid.tolist())
    Lx = 100 * 0.5e-6                                                                     # the pipe is periodic along x: the writer wraps vertex by vertex
    for k, c in enumerate(cid):
        q = pos[k].copy(); q[:, 0] = q[0, 0] + ((q[:, 0] - q[0, 0] + Lx / 2) % Lx - Lx / 2)   # one contiguous image of the cell
        dmean = q.mean(axis=0) - np.array(rows[c][:3]); dmean[0] = (dmean[0] + Lx / 2) % Lx - Lx / 2
        assert np.abs(dmean).max() < 3e-6 * Lx, (c, dmean)                               # cell centre [m] of the CSV = mean of its vertices (float32 datasets)
        assert 120e-12 < rows[c][3] < 140e-12 and 75e-18 < rows[c][4] < 90e-18            # RBC surface ~ 130 um^2, volume ~ 81 um^3
    assert 0 < pos[:, :, 0].min() and pos[:, :, 0].max() < 100 * 0.5e-6 and pos[:, :, 1:].min() > 0 and pos[:, :, 1:].max() < 52 * 0.5e-6   # inside the 100 x 52 x 52 box of 0.5 um nodes
    total = _h5_array(rbc, "Total force")
    parts = sum(_h5_array(rbc, n) for n in ("Volume force", "Area force", "Bending force", "Link force", "Viscous force"))
    assert np.abs(total).max() > 0 and np.abs(total - parts).max() <= 1e-5 * np.abs(total).max()   # float32 datasets, printed with 6 digits; iteration 400 is a material step
    assert np.abs(total).max() < 50e-12                                                   # N: below the 50 pN force limit
    fl = os.path.join(d, "Fluid.000000000400.p.0.h5")
    bnd = _h5_array(fl, "Boundary").reshape(54, 54, 102)
    assert set(np.unique(bnd)) == {0.0, 1.0} and 0.15 < bnd.mean() < 0.35                 # the pipe wall, one-node envelope included
    vel = _h5_array(fl, "Velocity").reshape(54, 54, 102, 3)
    assert np.abs(vel[bnd == 1]).max() == 0.0 and 0 < vel[..., 0].max() < 0.1            # m/s: no flow in the wall nodes, mm/s to cm/s along x in the lumen
    ux = vel[1:-1, 1:-1, 1:-1, 0].mean(axis=2)                                            # [z][y], averaged along the axis
    assert ux[26, 26] > 0.5 * ux.max() and ux[26, 26] > 3 * ux[26, 4]                     # fastest near the axis, slow next to the wall
    rho = _h5_array(fl, "Density").reshape(54, 54, 102)
    assert (rho[bnd == 1] == rho[bnd == 1][0]).all() and abs(rho[bnd == 0].mean() / rho[bnd == 1][0] - 1) < 1e-2   # BounceBack(1.) nodes answer rho = 1 (in SI here)


@pytest.mark.skipif(not HAVE_HDF5, reason="no HDF5 in this image")
def test_every_fluid_output_variable(tmp_path, gpu):
    """io/FluidHdf5IO.hh:139-199: Velocity, Density, Force, Boundary, Omega, ShearStress, ShearRate, StrainRate,
    CellDensity_<type>, BindingSites, InteriorPoints of a settled pipe flow with one RBC, checked against each other.
    Palabos' prefactors of computeShearStress / computeStrainRateFromStress cannot be read here (parity unpinned); the
    physics pins them: strain rate = symmetric velocity gradient, stress = 2 mu strain rate."""
    exe = _build(tmp_path, "tests/drivers/fluid_outputs.cpp")
    d = str(tmp_path / "case"); shutil.copytree(os.path.join(ROOT, "tests", "golden", "shear_case"), d)
    for f in os.listdir(d):
        os.chmod(os.path.join(d, f), 0o644)
    open(os.path.join(d, "RBC.pos"), "w").write("1\n8.0 8.25 8.25 0 0 0\n")          # x = 16 lu, on the axis
    r = subprocess.run([exe, "config.xml"], cwd=d, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "OUTPUT_BINDING_SITES requested, but binding sites not used" in r.stdout and "OUTPUT_INTERIOR_POINTS requested" in r.stdout
    par = [l.split() for l in r.stdout.splitlines() if l.startswith("PARAMS")][0]
    tau, dx, dt, df, frac = (float(par[k]) for k in (2, 4, 6, 8, 10))
    f = os.path.join(d, "tmp", "hdf5", "000000000010", "Fluid.000000000010.p.0.h5")
    hdr = subprocess.run(["/opt/conda/bin/h5dump", "-H", f], capture_output=True, text=True).stdout
    for name, c in (("Velocity", 3), ("Density", 1), ("Force", 3), ("Boundary", 1), ("Omega", 1), ("ShearStress", 6), ("ShearRate", 9), ("StrainRate", 6),
                    ("CellDensity_RBC", 1), ("BindingSites", 1), ("InteriorPoints", 1)):
        seg = hdr[hdr.index('DATASET "%s"' % name):][:300]
        assert "( 36, 36, 98, %d )" % c in seg, (name, seg)
    N = (36, 36, 98)
    vel = _h5_array(f, "Velocity").reshape(N + (3,))
    bnd = _h5_array(f, "Boundary").reshape(N)
    umax = vel[..., 0].max() * dt / dx
    assert 0.017 < umax < 0.023                                                       # lattice units: the parabola the driving force was chosen for
    # ---- ShearRate[3a+b] = d u_a / d x_b, central differences of the Velocity dataset itself (float32 both)
    sr = _h5_array(f, "ShearRate").reshape(N + (3, 3))
    inner = (slice(1, -1),) * 3
    for b, axis in ((0, 2), (1, 1), (2, 0)):                                          # x is the fastest index of the file
        grad = (np.roll(vel, -1, axis=axis) - np.roll(vel, 1, axis=axis)) / (2 * dx)
        err = np.abs(sr[..., :, b] - grad)[inner]
        assert err.max() <= 2e-6 * np.abs(sr).max(), (b, err.max(), np.abs(sr).max())
    # ---- StrainRate (xx, xy, xz, yy, yz, zz) against the symmetric part of that gradient: bulk nodes three nodes off the
    # wall, half the pipe away from the cell
    st = _h5_array(f, "StrainRate").reshape(N + (6,))
    sym = 0.5 * (sr + np.swapaxes(sr, -1, -2))
    zz, yy = np.meshgrid(np.arange(36) - 1 - 16.5, np.arange(36) - 1 - 16.5, indexing="ij")
    bulk = (np.sqrt(zz ** 2 + yy ** 2) < 12.5)[:, :, None] & (np.arange(98)[None, None, :] > 56) & (np.arange(98)[None, None, :] < 90)
    scale = np.abs(sym[bulk]).max()
    for k, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        assert np.abs(st[..., k] - sym[..., a, b])[bulk].max() < 0.03 * scale, (k, np.abs(st[..., k] - sym[..., a, b])[bulk].max(), scale)
    assert scale > 1e3                                                                 # 1/s: a real gradient (u_max / R ~ 0.02 / 16 / dt)
    # ---- ShearStress = 2 rho nu StrainRate: [Pa] = 2 * (rho_l * 1025 kg/m3) * 1.1e-6 m2/s * [1/s]
    ss = _h5_array(f, "ShearStress").reshape(N + (6,))
    rho = _h5_array(f, "Density").reshape(N) / (df / dx ** 2)
    fluid = bnd == 0
    want = 2 * 1025.0 * 1.1e-6 * rho[..., None] * st
    assert np.abs(ss - want)[fluid].max() < 1e-5 * np.abs(ss).max() and np.abs(ss).max() > 0
    assert np.abs(ss[bnd == 1]).max() == 0 and np.abs(st[bnd == 1]).max() == 0
    # ---- Omega: 1 / tau on bulk nodes (scaled like a stress, as the reference scales it), none on BounceBack nodes
    om = _h5_array(f, "Omega").reshape(N)
    assert np.allclose(om[fluid], (1.0 / tau) * df / dx ** 2, rtol=1e-6) and (om[bnd == 1] == 0).all()
    # ---- CellDensity: every vertex counted once at its nearest node (times the volume fraction per vertex in SI)
    cd = _h5_array(f, "CellDensity_RBC").reshape(N)
    assert abs(cd.sum() / frac - 642) < 1e-2 and abs(frac - 90.0 / 642 / 0.125) < 1e-6
    zs, ys, xs = np.nonzero(cd)
    assert 4 < xs.min() and xs.max() < 30 and 5 < ys.min() and ys.max() < 30            # around x = 16 (+ the few steps it drifted), on the axis
    assert (_h5_array(f, "BindingSites") == 0).all() and (_h5_array(f, "InteriorPoints") == 0).all()
    # ---- the same driver as two ranks (two x-slabs of 48 planes): every block's file carries its neighbour's face plane in the
    # one-node envelope, so the two files put side by side are the one-rank file, gradients across the slab face included
    d2 = str(tmp_path / "case2"); shutil.copytree(os.path.join(ROOT, "tests", "golden", "shear_case"), d2)
    for fn in os.listdir(d2):
        os.chmod(os.path.join(d2, fn), 0o644)
    open(os.path.join(d2, "RBC.pos"), "w").write("1\n8.0 8.25 8.25 0 0 0\n")
    port = str(34000 + os.getpid() % 20000)
    procs = []
    for rk in range(2):
        env = dict(os.environ, OMPI_COMM_WORLD_RANK=str(rk), OMPI_COMM_WORLD_SIZE="2", OMPI_COMM_WORLD_LOCAL_RANK=str(rk), HEMOCELL_PORT=port, HEMOCELL_TRANSPORT="tcp",
                   HEMOCELL_COMM_TIMEOUT="120")
        for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
            env.pop(k, None)
        procs.append(subprocess.Popen([exe, "config.xml"], cwd=d2, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=600)[0] for p in procs]
    assert [p.returncode for p in procs] == [0, 0], outs[0][-2000:] + outs[1][-2000:]
    halves = [os.path.join(d2, "tmp", "hdf5", "000000000010", "Fluid.000000000010.p.%d.h5" % rk) for rk in range(2)]
    for name, c in (("Velocity", 3), ("Density", 1), ("ShearRate", 9), ("StrainRate", 6), ("ShearStress", 6), ("Boundary", 1)):
        one = _h5_array(f, name).reshape(N + (c,))
        two = [_h5_array(hf, name).reshape((36, 36, 50, c)) for hf in halves]
        scale = np.abs(one).max()
        for rk in range(2):   # all 50 planes of a block's file, envelope planes included, against planes 48 rk .. 48 rk + 49 of the whole
            assert np.abs(two[rk] - one[:, :, 48 * rk:48 * rk + 50]).max() <= 2e-5 * scale, (name, rk)


def _launch_ranks(exe, args, cwd, world, salt=0, expect_ok=True):
    """a driver binary started as `world` processes the way mpirun would start them (rank and size in the environment); the
    ranks share the one GPU of the test box, so the data plane is the host-staged one"""
    port = str(30000 + (os.getpid() * 7 + salt * 131) % 20000)
    procs = []
    for rk in range(world):
        env = dict(os.environ, OMPI_COMM_WORLD_RANK=str(rk), OMPI_COMM_WORLD_SIZE=str(world), OMPI_COMM_WORLD_LOCAL_RANK=str(rk), HEMOCELL_PORT=port,
                   HEMOCELL_TRANSPORT="tcp", HEMOCELL_COMM_TIMEOUT="120")
        for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
            env.pop(k, None)
        procs.append(subprocess.Popen([exe] + args, cwd=cwd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=900)[0] for p in procs]
    if not expect_ok:
        return outs, [p.returncode for p in procs]
    assert [p.returncode for p in procs] == [0] * world, "".join(o[-1500:] for o in outs)
    return outs


def test_checkpoint_with_an_incomplete_cell_and_a_truncated_dump(tmp_path, gpu):
    """ADVICE round 2 (hemocell.h saveCheckPoint / loadCheckPoint): a dump written while a cell has lost particles at a wall
    loads again and the remnant is removed as the reference's load path does (core/hemoCellFields.cpp:272-274:
    load, syncEnvelopes, deleteIncompleteCells); a truncated dump is refused with a log line and exit(1)"""
    exe = _build(tmp_path, "tests/drivers/checkpoint_incomplete.cpp")
    d = str(tmp_path / "case"); shutil.copytree(os.path.join(ROOT, "tests", "golden", "shear_case"), d)
    for f in os.listdir(d):
        os.chmod(os.path.join(d, f), 0o644)
    open(os.path.join(d, "RBC.pos"), "w").write("2\n15.0 8.25 8.25 90 0 0\n34.5 8.25 12.5 90 0 0\n")     # lu: (30, 16.5, 16.5) and (69, 16.5, 25)
    r = subprocess.run([exe, "config.xml", "save"], cwd=d, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    before = [l.split() for l in r.stdout.splitlines() if l.startswith("BEFORE")][0]
    assert int(before[2]) == 2 and int(before[4]) == 1 and int(before[6]) > 0          # two cells, one incomplete, particles missing
    resumed = [l.split() for l in r.stdout.splitlines() if l.startswith("RESUMED")][0]
    assert int(resumed[2]) == 56 and int(resumed[4]) == 1 and int(resumed[6]) == 0 and int(resumed[8]) == 0
    assert "CONTINUED iteration 64 cells 1" in r.stdout
    ck = os.path.join(d, "tmp", "checkpoint", "checkpoint.bin")
    assert os.path.exists(ck) and not os.path.exists(ck + ".tmp")
    size = os.path.getsize(ck)
    for cut in (size - 1000, size // 2, 40):                                            # inside the records, the populations, the header
        with open(ck, "rb") as fh:
            blob = fh.read()
        with open(ck, "wb") as fh:
            fh.write(blob[:cut])
        # checkpoint.xml as the configuration, as the reference resumes: the run goes back to the directory the dump names
        r2 = subprocess.run([exe, "tmp/checkpoint/checkpoint.xml", "load"], cwd=d, capture_output=True, text=True, timeout=600)
        assert r2.returncode == 1 and "truncated or damaged" in r2.stdout + r2.stderr, (cut, r2.returncode, r2.stdout[-1500:])
        assert "RESUMED" not in r2.stdout
        with open(ck, "wb") as fh:
            fh.write(blob)
    r3 = subprocess.run([exe, "tmp/checkpoint/checkpoint.xml", "load"], cwd=d, capture_output=True, text=True, timeout=600)     # the intact dump still loads
    assert r3.returncode == 0 and "RESUMED iteration 56 cells 1" in r3.stdout, r3.stdout[-1500:]


def test_two_rank_checkpoint_and_resume(tmp_path, gpu):
    """core/hemoCellFields.cpp:240-319 with two ranks: every rank dumps its block (checkpoint.<rank>.bin), a restart of two ranks
    from the iteration-200 dump prints the remaining statistics of the uninterrupted two-rank run, digit for digit"""
    exe = _build(tmp_path, "examples/pipe/pipe_synthetic.cpp")
    case = str(tmp_path / "pipe2"); os.makedirs(case)
    for f in ("config.xml", "RBC.xml", "PLT.xml", "RBC.pos", "PLT.pos"):
        shutil.copy(os.path.join(ROOT, "examples", "pipe", f), case)
    full = _launch_ranks(exe, ["config.xml"], case, 2, salt=1)
    stat_full = [l for l in full[0].splitlines() if l.startswith("STAT")]
    assert len(stat_full) == 4
    assert [l for l in full[1].splitlines() if l.startswith("STAT")] == stat_full      # the statistics are reduced over the ranks: both print the same
    ck = os.path.join(case, "tmp_pipe", "checkpoint")
    for f in ("checkpoint.0.bin", "checkpoint.1.bin", "checkpoint.xml"):
        assert os.path.exists(os.path.join(ck, f + ".old")), f
        os.replace(os.path.join(ck, f + ".old"), os.path.join(ck, f))        # the iteration-200 dump
    again = _launch_ranks(exe, ["tmp_pipe/checkpoint/checkpoint.xml"], case, 2, salt=2)
    stat_again = [l for l in again[0].splitlines() if l.startswith("STAT")]
    assert stat_again == stat_full[2:], (stat_again, stat_full)
    assert "resumed at iteration 200" in open(os.path.join(case, "tmp_pipe", "log", "logfile.0")).read()
    # ranks that hold dumps of different iterations are refused: rank 1 gets its previous dump back
    assert os.path.exists(os.path.join(ck, "checkpoint.1.bin.old"))
    shutil.copy(os.path.join(ck, "checkpoint.1.bin.old"), os.path.join(ck, "checkpoint.1.bin"))
    outs, rcs = _launch_ranks(exe, ["tmp_pipe/checkpoint/checkpoint.xml"], case, 2, salt=3, expect_ok=False)
    assert rcs == [1, 1], (rcs, outs[0][-800:], outs[1][-800:])
    assert "different iterations" in outs[0]


def test_moving_wall_couette_vs_oracle(orc, gpu):
    """helper/hemocellInit.hh:71-86 (oneCellShear): top/bottom walls moving in +-x, x and y periodic.  GPU vs
    oracle bit for bit, and the steady profile is linear with the imposed shear rate."""
    from oracle import oracle as O
    nx, ny, nz = 8, 6, 22
    mask = np.zeros((nx, ny, nz), np.uint8); mask[:, :, 0] = 3; mask[:, :, -1] = 4
    shear = 1e-4; vhalf = (nz - 1) * shear * 0.5
    Lo = O.OracleLattice(orc, nx, ny, nz, (1, 1, 0), 1.0); Lg = gpu.Lattice(nx, ny, nz, (1, 1, 0), 1.0)
    Lo.set_mask(mask); Lg.defineBounceBack(mask)
    Lo.set_wall_velocity(0, (vhalf, 0, 0)); Lo.set_wall_velocity(1, (-vhalf, 0, 0))
    Lg.setBoundaryVelocity(3, (vhalf, 0, 0)); Lg.setBoundaryVelocity(4, (-vhalf, 0, 0))
    Lo.init_equilibrium(); Lg.latticeEquilibrium()
    Lo.collide_stream(3000); Lg.collideAndStream(3000)
    fluid = mask.reshape(-1) == 0
    assert np.array_equal(Lg.populations()[fluid], Lo.f[fluid])
    rho, u = Lg.rho_u()
    ux = u[:, 0].reshape(nx, ny, nz)[0, 0, 1:-1]
    z = np.arange(1, nz - 1)
    expect = vhalf - (z - 0.5) * (2 * vhalf) / (nz - 2)      # walls sit half a node outside the first/last fluid node
    assert np.abs(ux - expect).max() < 0.02 * vhalf
    # the facade's iniLatticeSquareCouette gives the walls vhalf (nz-2)/(nz-1): the fluid then has the profile of the
    # reference's on-node walls, u(z) = vhalf (1 - 2 z / (nz-1)), i.e. exactly the requested shear rate
    w = vhalf * (nz - 2) / (nz - 1)
    Lg.setBoundaryVelocity(3, (w, 0, 0)); Lg.setBoundaryVelocity(4, (-w, 0, 0))
    Lg.collideAndStream(3000)
    ux = Lg.rho_u()[1][:, 0].reshape(nx, ny, nz)[0, 0, 1:-1]
    assert np.abs(ux - vhalf * (1 - 2 * z / (nz - 1))).max() < 2e-3 * vhalf
    assert abs(np.polyfit(z, ux, 1)[0] + shear) < 2e-3 * shear
    Lo.destroy(); Lg.destroy()


# ---------------------------------------------------------------------------------------------------------------------
# The reference's OWN drivers (examples/pipeflow/pipeflow.cpp, examples/stretchCell/stretchCell.cpp), compiled unchanged
# against the facade by __graft_entry__.build() into oracle/_ref/ where the reference tree is present (it does not
# travel), run here on its own CI inputs (tests/golden/*_case: the config of scripts/ci, the XML / .pos / .stl files of
# the example) and judged by its own CI scripts, restated line by line.
def _ref_driver(name):
    exe = os.path.join(ROOT, "oracle", "_ref", name)
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/%s not built (needs the reference tree at build time)" % name)
    return exe


def _run_case(tmp_path, exe, case):
    import shutil
    work = tmp_path / case
    shutil.copytree(os.path.join(ROOT, "tests", "golden", case), str(work))
    r = subprocess.run([exe, "config.xml"], cwd=str(work), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    log = open(str(work / "tmp" / "log" / "logfile")).read().splitlines()
    return work, log


def _run_short(tmp_path, name, tmax, tmeas):
    """a reference driver on its own inputs (tests/golden/<name>_case = the data files of its directory) with tmax / tmeas cut down"""
    import re
    work = tmp_path / name
    shutil.copytree(os.path.join(ROOT, "tests", "golden", name + "_case"), str(work))
    for f in os.listdir(str(work)):
        os.chmod(str(work / f), 0o644)
    cfg = open(str(work / "config.xml")).read()
    cfg = re.sub(r"<tmax>[^<]*</tmax>", "<tmax> %d </tmax>" % tmax, cfg); cfg = re.sub(r"<tmeas>[^<]*</tmeas>", "<tmeas> %d </tmeas>" % tmeas, cfg)
    open(str(work / "config.xml"), "w").write(cfg)
    r = subprocess.run([_ref_driver(name), "config.xml"], cwd=str(work), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return work, r.stdout.splitlines()


def _csv(path):
    rows = open(path).read().splitlines()
    return rows[0].split(","), np.array([[float(v) for v in l.split(",")] for l in rows[1:]]).reshape(-1, 11)


def test_reference_simple_driver(tmp_path, gpu):
    """examples/simple/simple.cpp: initializeLattice, a square duct of BounceBack planes, a cell type without cells, every
    derived fluid field in the output list (:71-74)"""
    work, out = _run_short(tmp_path, "simple", 1000, 500)
    assert sum("writing output at timestep" in l for l in out) == 2
    if not HAVE_HDF5:
        return
    f = str(work / "tmp" / "hdf5" / "000000001000" / "Fluid.000000001000.p.0.h5")
    hdr = subprocess.run(["/opt/conda/bin/h5dump", "-H", f], capture_output=True, text=True).stdout
    for name, c in (("Velocity", 3), ("Density", 1), ("Force", 3), ("ShearRate", 9), ("StrainRate", 6), ("ShearStress", 6), ("Boundary", 1), ("Omega", 1), ("CellDensity_RBC_HO", 1)):
        seg = hdr[hdr.index('DATASET "%s"' % name):][:300]
        assert "( 52, 52, 52, %d )" % c in seg, (name, seg)
    vel = _h5_array(f, "Velocity").reshape(52, 52, 52, 3)
    bnd = _h5_array(f, "Boundary").reshape(52, 52, 52)
    assert vel[26, 26, 26, 0] > 0 and vel[26, 26, 26, 0] == pytest.approx(vel[..., 0].max(), rel=1e-3) and np.abs(vel[bnd == 1]).max() == 0   # duct flow along +x, fastest on the axis
    frc = _h5_array(f, "Force").reshape(52, 52, 52, 3)
    assert frc[..., 0].min() == frc[..., 0].max() > 0 and np.abs(frc[..., 1:]).max() == 0     # the driving force the driver wrote after the iteration
    assert (_h5_array(f, "CellDensity_RBC_HO") == 0).all()


def test_reference_cell_collision_driver(tmp_path, gpu):
    """cases/cellCollision/cellCollision.cpp: iniLatticeSquareCouette shear box with one RBC and one platelet"""
    work, out = _run_short(tmp_path, "cellCollision", 2000, 1000)
    assert "(readPositionsBloodCells) 1 complete RBC cells placed." in out and "(readPositionsBloodCells) 1 complete PLT cells placed." in out
    assert out[-1] == "(CellCollision) Simulation finished :)"
    for t in ("RBC", "PLT"):
        h0, c0 = _csv(str(work / "tmp" / "csv" / (t + ".000000000000.csv")))
        h1, c1 = _csv(str(work / "tmp" / "csv" / (t + ".000000002000.csv")))
        assert len(c0) == len(c1) == 1
        assert abs(c1[0, 4] / c0[0, 4] - 1) < 0.02                   # volume kept
        assert abs(c1[0, 0] - c0[0, 0]) > 1e-9                       # carried along x by the shear flow [m]


def test_reference_kolmogorov_driver(tmp_path, gpu):
    """cases/kolmogorovFlow/kolmogorovFlow.cpp: fully periodic box, +F on one half and -F on the other, written with
    setExternalVector on two sub-domains before every iteration (:136-140)"""
    work, out = _run_short(tmp_path, "kolmogorovFlow", 2000, 1000)
    cells = [l for l in out if "# of cells" in l]
    assert len(cells) == 2 and len(set(cells)) == 1 and "# of RBC: 10" in cells[0]                 # 105 in the file; none lost on the way
    vel = [l for l in out if "Velocity  -" in l]
    vmax, vmean = float(vel[-1].split("max.:")[1].split()[0]), float(vel[-1].split("mean:")[1].split()[0])
    assert vmax > 1.3 * vmean > 0                                                               # a shear flow, not a uniformly accelerated box
    if HAVE_HDF5:
        f = str(work / "tmp" / "hdf5" / "000000002000" / "Fluid.000000002000.p.0.h5")
        ux = _h5_array(f, "Velocity").reshape(62, 62, 62, 3)[1:-1, 1:-1, 1:-1, 0]                   # [z][y][x]
        top, bottom = ux[:, :30, :].mean(), ux[:, 30:, :].mean()
        assert top > 0 > bottom and abs(top + bottom) < 0.05 * top                                 # the two halves stream against each other
        frc = _h5_array(f, "Force").reshape(62, 62, 62, 3)[1:-1, 1:-1, 1:-1, 0]
        assert (frc[:, :30, :] > 0).all() and (frc[:, 30:, :] < 0).all() and np.allclose(frc[:, :30, :], -frc[:, 30:, :][:, ::-1, :])


def test_reference_parachuting_driver(tmp_path, gpu):
    """examples/parachuting/parachuting.cpp: one RBC in a narrow voxelised tube (tube.stl), driven flow"""
    work, out = _run_short(tmp_path, "parachuting", 2000, 500)
    cells = [l for l in out if "# of cells" in l]
    assert len(cells) == 4 and all("# of cells: 1 | # of RBC: 1" in l for l in cells)
    visc = [float(l.split("viscosity:")[1]) for l in out if "viscosity" in l]
    assert all(0.9 < v < 1.5 for v in visc), visc
    x = [_csv(str(work / "tmp" / "csv" / ("RBC.%012d.csv" % it)))[1][0, 0] for it in (500, 1000, 1500, 2000)]
    assert x[0] < x[1] < x[2] < x[3]                                                             # carried downstream


def test_reference_parallel_planes_driver(tmp_path, gpu):
    """examples/parallelplanes/parallelplanes.cpp: channel between two BounceBack planes, periodic in x and y, RBC + PLT
    suspension from its own .pos files (written for a larger box: what falls outside is not placed)"""
    work, out = _run_short(tmp_path, "parallelplanes", 1000, 500)
    log = out                                                                                     # hlog goes to the terminal too
    cells = [l for l in log if "# of cells" in l]
    assert len(cells) == 2 and len(set(cells)) == 1                                               # nothing lost between the measurements
    n = int(cells[0].split("# of cells:")[1].split()[0])
    assert 300 < n < 1189
    fmax = [float(l.split("max.:")[1].split()[0]) for l in log if "Force  -" in l]
    assert all(f < 5.0 for f in fmax), fmax                                                       # pN: a relaxed suspension


def test_reference_flow_around_sphere_driver(tmp_path, gpu):
    """examples/flowaroundsphere/flowaroundsphere.cpp: a sphere of BounceBack nodes from the driver's own plb::DomainFunctional3D,
    a moving top wall (velocity condition), periodic in x and y, RBC + PLT suspension with the cell-cell repulsion switched on"""
    work, out = _run_short(tmp_path, "flowaroundsphere", 400, 200)
    cells = [l for l in out if "# of cells" in l]
    assert len(cells) == 2 and len(set(cells)) == 1 and int(cells[0].split("# of cells:")[1].split()[0]) > 500
    vmax = [float(l.split("max.:")[1].split()[0]) for l in out if "Velocity  -" in l]
    assert all(0.02 < v <= 0.0338 for v in vmax), vmax        # the wall moves at 0.75 * 1800 1/s * 100 um / 4 = 33.75 mm/s; nothing is faster
    if HAVE_HDF5:
        f = str(work / "tmp" / "hdf5" / "000000000400" / "Fluid.000000000400.p.0.h5")
        ux = _h5_array(f, "Velocity").reshape(102, 102, 202, 3)[..., 0]
        assert np.abs(ux[1 + 15, 1 + 50, 1 + 50]) == 0 and ux[100, 51, 101] == pytest.approx(0.03375, rel=1e-5)   # inside the sphere; on the moving wall


def test_reference_bent_microvessel_driver(tmp_path, gpu):
    """cases/microvessel_bended/microvessel_bended.cpp: a sinusoidally bent vessel from a DomainFunctional3D, fully periodic
    box, 20 000 warm-up steps of the fluid alone, then the suspension"""
    work, out = _run_short(tmp_path, "microvessel_bended", 400, 200)
    cells = [l for l in out if "# of cells" in l]
    assert len(cells) == 2 and len(set(cells)) == 1 and int(cells[0].split("# of cells:")[1].split()[0]) > 200
    visc = [float(l.split("viscosity:")[1]) for l in out if "viscosity:" in l]
    assert len(visc) == 2 and all(0.9 < v < 1.3 for v in visc), visc


def test_reference_vasoconstriction_driver(tmp_path, gpu):
    """cases/vasoconstriction_pipe/vasoconstriction_pipe.cpp: a pipe with a narrowed stretch from a DomainFunctional3D, RBC + PLT"""
    work, out = _run_short(tmp_path, "vasoconstriction_pipe", 400, 200)
    cells = [l for l in out if "# of cells" in l]
    assert len(cells) == 2 and len(set(cells)) == 1 and int(cells[0].split("# of cells:")[1].split()[0]) > 300
    visc = [float(l.split("viscosity:")[1]) for l in out if "viscosity:" in l]
    assert len(visc) >= 2 and all(0.9 < v < 1.3 for v in visc[-2:]), visc


def test_reference_stentflow_driver(tmp_path, gpu):
    """cases/stentflow/stentflow.cpp ships no .pos files: the driver warns and runs the fluid alone through its stented pipe"""
    work, out = _run_short(tmp_path, "stentflow", 400, 200)
    assert any("does not exist" in l for l in out)                       # "*** WARNING! particle positions input file ... does not exist!"
    cells = [l for l in out if "# of cells" in l]
    assert len(cells) == 2 and all("# of cells: 0 " in l for l in cells)
    visc = [float(l.split("viscosity:")[1]) for l in out if "viscosity:" in l]
    assert all(0.9 < v < 1.1 for v in visc[-2:]), visc


def test_reference_atherosclerosis_driver(tmp_path, gpu):
    """cases/atherosclerosis/atherosclerosis.cpp: a channel with a plaque from a DomainFunctional3D.  The .pos files the case ships
    announce 0 cells (its suspensions live under initial_states/); the fixtures keep that first line only"""
    work, out = _run_short(tmp_path, "atherosclerosis", 200, 100)
    assert "(readPositionsBloodCells) Particle count in file (RBC): 0." in out
    vmax = [float(l.split("max.:")[1].split()[0]) for l in out if "Velocity  -" in l]
    assert len(vmax) == 2 and 0 < vmax[0] < vmax[1] < 0.1                    # the driven flow is still accelerating
    assert out[-1].strip() == "(main) Simulation finished :)"


def _cut(line, *spec):
    """cut -d<delim> -f<n> chains of the CI scripts"""
    for delim, n in spec:
        line = line.split(delim)[n - 1]
    return line


def test_reference_pipeflow_driver_passes_its_ci_sanity(tmp_path, gpu):
    """scripts/ci/pipeflow_sanity.sh:7-22 on the log of the reference's pipeflow driver: 42 cells at every
    measurement, relative apparent viscosity in (1.03, 3.0), maximum vertex force below 4 pN"""
    work, log = _run_case(tmp_path, _ref_driver("pipeflow"), "pipeflow_case")
    cells = [_cut(l, (":", 2), (" ", 2)) for l in log if "# of cells" in l]
    assert len(cells) == 10 and all(c == "42" for c in cells), cells
    visc = [float(_cut(l, (":", 4), (" ", 2))) for l in log if "viscosity" in l]
    assert len(visc) == 10 and all(1.03 < v < 3.0 for v in visc), visc
    fmax = [float(_cut(l, (":", 3), (" ", 2))) for l in log if "Force  -" in l]
    assert len(fmax) == 10 and all(f < 4.0 for f in fmax), fmax
    # :38-50 "Checking checkpointing": a current and a previous dump exist and are not empty (this back end keeps one
    # file, checkpoint.bin, where the reference has lattice.dat + particleField.dat + checkpoint.xml)
    for f in ("checkpoint.bin", "checkpoint.bin.old"):
        assert os.path.getsize(str(work / "tmp" / "checkpoint" / f)) > 0
    if HAVE_HDF5:   # hemocell.writeOutput(): one directory per measurement with fluid and cell files
        out = sorted(os.listdir(str(work / "tmp" / "hdf5")))
        assert len(out) >= 10
        # particles are written where a block holds them: inside the periodic domain (cells that straddle x = 0 from
        # the start would otherwise show up at negative x)
        rbc = str(work / "tmp" / "hdf5" / out[-1] / ("RBC." + out[-1] + ".p.0.h5"))
        dump = subprocess.run(["/opt/conda/bin/h5dump", "-d", "/Position", "-y", "-w", "0", rbc], capture_output=True, text=True).stdout
        body = dump[dump.index("DATA {") + 6:dump.rindex("}")]
        vals = np.array([float(t) for t in body.replace("}", " ").replace(",", " ").split()]).reshape(-1, 3)
        assert len(vals) == 35 * 642
        assert vals[:, 0].min() >= -0.5 and vals[:, 0].max() < 102.5


def test_reference_pipeflow_driver_two_ranks_reproduce_the_one_rank_log(tmp_path, gpu):
    """scripts/ci/pipeflow_sanity.sh:23-33 "Checking for similar output, differing CPU's": the reference's pipeflow driver run
    as 2 ranks must print the logfile of the 1-rank run (lines that name the atomic-block layout or the voxelizer excepted).
    Here: the reference's own binary, started as two processes the way mpirun would start them (rank and world size in the
    environment), becomes two x-slabs of 51 and 52 planes with the native slab schedule in between; both processes share
    the one GPU of the test box, so the data plane is HC_TRANSPORT_TCP (RCCL refuses two ranks on one device)."""
    import shutil
    exe = _ref_driver("pipeflow")
    one, log1 = _run_case(tmp_path, exe, "pipeflow_case")
    work = tmp_path / "two"
    shutil.copytree(os.path.join(ROOT, "tests", "golden", "pipeflow_case"), str(work))
    port = str(33000 + os.getpid() % 20000)
    procs = []
    for r in range(2):
        env = dict(os.environ, OMPI_COMM_WORLD_RANK=str(r), OMPI_COMM_WORLD_SIZE="2", OMPI_COMM_WORLD_LOCAL_RANK=str(r), HEMOCELL_PORT=port,
                   HEMOCELL_TRANSPORT="tcp", HEMOCELL_COMM_TIMEOUT="120")
        for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
            env.pop(k, None)
        procs.append(subprocess.Popen([exe, "config.xml"], cwd=str(work), env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=900)[0] for p in procs]
    assert [p.returncode for p in procs] == [0, 0], outs[0][-2000:] + outs[1][-2000:]
    assert outs[1].strip() == "", outs[1][-500:]                     # rank 1 is silent: the log is rank 0's
    log2 = open(str(work / "tmp" / "log" / "logfile")).read().splitlines()
    keep = lambda lines: [l for l in lines if "atomic-block" not in l and "Voxelizer" not in l]
    a, b = keep(log1), keep(log2)
    assert len(a) == len(b) and len(a) > 40
    diff = [(x, y) for x, y in zip(a, b) if x != y]
    assert not diff, diff[:5]
    assert sum("# of cells: 42" in l for l in b) == 10
    for r in range(2):   # every rank wrote its block and its checkpoint
        assert os.path.getsize(str(work / "tmp" / "checkpoint" / ("checkpoint.%d.bin" % r))) > 0
    if HAVE_HDF5:
        last = sorted(os.listdir(str(work / "tmp" / "hdf5")))[-1]
        n = 0
        for r in range(2):
            rbc = str(work / "tmp" / "hdf5" / last / ("RBC.%s.p.%d.h5" % (last, r)))
            dump = subprocess.run(["/opt/conda/bin/h5dump", "-a", "/numberOfParticles", rbc], capture_output=True, text=True).stdout
            n += int(dump[dump.index("(0):") + 4:].split()[0])
        assert n == 35 * 642                                           # every RBC is written by exactly one rank
    # the CSV summaries are gathered on rank 0 (io/writeCellInfoCSV.cpp:45): same cells, same numbers as the one-rank run
    for name in sorted(os.listdir(str(one / "tmp" / "csv"))):
        h1, c1 = _csv(str(one / "tmp" / "csv" / name)); h2, c2 = _csv(str(work / "tmp" / "csv" / name))
        assert h1 == h2 and c1.shape == c2.shape
        c1, c2 = c1[np.argsort(c1[:, 6])], c2[np.argsort(c2[:, 6])]
        cols = [0, 1, 2, 3, 4, 6, 7, 8, 9, 10]                         # all but atomic_block
        Lx = 103 * 0.5e-6
        dxp = (c2[:, 0] - c1[:, 0] + Lx / 2) % Lx - Lx / 2              # a centre next to the periodic seam may be reported on either side of it
        assert np.abs(dxp).max() < 1e-9
        assert np.allclose(c1[:, cols[1:]], c2[:, cols[1:]], rtol=1e-4, atol=1e-12), name


def test_reference_stretchcell_driver_passes_its_ci_sanity(tmp_path, gpu):
    """scripts/ci/stretchCell_sanity.sh:7-33 on the log of the reference's stretchCell driver (137 pN, 1000
    iterations): largest diameter <= 9.6 um, volume in [81.12, 81.19] um^3 and [100, 100.1] %, surface in
    [129.34, 133.04] um^2"""
    work, log = _run_case(tmp_path, _ref_driver("stretchCell"), "stretch_case")
    diam = [float(_cut(l, (":", 2), (" ", 2))) for l in log if "diameter" in l]
    assert len(diam) >= 10 and all(d < 9.6 for d in diam), diam
    # The script cuts field 3 of the "Volume:" line, which has only two ':'-separated fields, so its four volume checks
    # never see a number; the intended quantities are checked here.  The driver also reports at iteration 1, when
    # volume and surface are still the undeformed ones (81.117 um^3, 129.21 um^2 here); the bands' lower edges are
    # the values of the report at iteration 100 (129.342 um^2 here against the edge 129.34), so they are applied from
    # that report on, as in tests/test_oracle_pins.py::test_stretch_ci_bands.
    vol = [l for l in log if "Volume:" in l]
    pct = [float(_cut(l, (":", 2), ("(", 2), ("%", 1))) for l in vol]
    um3 = [float(_cut(l, (":", 2), (" ", 2))) for l in vol]
    assert len(vol) == 11 and all(100.0 <= p < 100.1 for p in pct), pct
    assert all(81.12 < v < 81.19 for v in um3[1:]), um3
    surf = [float(_cut(l, (":", 2), (" ", 2))) for l in log if "Surface:" in l]
    assert len(surf) == 11 and all(129.34 < s < 133.04 for s in surf[1:]), surf


def test_reference_stretchcell_validation_sweep(tmp_path, gpu):
    """examples/stretchCell/validation.sh through the reference's own stretchCell binary on the HIP path: forces 0, 25, 50, 75,
    125, 150, 173, 175 pN with the example's own config.xml (40 000 iterations each, dt 1e-7), the axial / transverse
    diameters the driver writes to stretch-<force>.log.
    Known answers the reference holds for it:
      * tests/validation/stretch_cell/test_stretch_cell.cpp:158-162 -- bands for 25 / 75 / 125 pN at iteration 10 000;
      * examples/stretchCell/validation/reference-{axial,transverse}.dat -- the published steady-state curves
        (doi 10.3389/fphys.2017.00563, Fig. 4) and reference-bounds.dat, the experimental error bars, which validation.sh
        only PLOTS next to the run.  After 40 000 iterations the cell is still creeping towards that steady state (25 pN:
        9.56 -> 9.84 -> 9.99 um at 10 / 20 / 40 thousand iterations), so the curves are approached from the unstretched side and
        not reached: the gap is asserted to shrink and bounded, not to vanish (tests/golden/stretch_validation, fixtures)."""
    import shutil
    exe = _ref_driver("stretchCell")
    src = os.path.join(ROOT, "tests", "golden", "stretch_validation")
    work = tmp_path / "sweep"
    shutil.copytree(src, str(work))
    ref_ax = np.loadtxt(os.path.join(src, "reference-axial.dat"), delimiter=",", comments="#")
    ref_tr = np.loadtxt(os.path.join(src, "reference-transverse.dat"), delimiter=",", comments="#")
    cfg0 = open(str(work / "config.xml")).read()
    forces = [0, 25, 50, 75, 125, 150, 173, 175]                      # validation.sh:11
    rows = {}
    import re
    for F in forces:
        os.chmod(str(work / "config.xml"), 0o644)                      # fixtures may be checked out read-only
        open(str(work / "config.xml"), "w").write(re.sub(r"<stretchForce>[^<]*</stretchForce>", "<stretchForce>%d</stretchForce>" % F, cfg0))
        r = subprocess.run([exe, "config.xml"], cwd=str(work), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        rows[F] = np.loadtxt(str(work / ("stretch-%d.log" % F)), skiprows=1)
        assert rows[F][-1, 0] == 40000
    at = lambda F, it: rows[F][rows[F][:, 0] == it][0, 1:]
    # (1) the reference's own test bands at its test's iteration count
    for F, t_lo, t_hi, a_lo, a_hi in ((25, 7.3, 7.9, 9.2, 9.7), (75, 7.0, 7.5, 11, 12), (125, 6.5, 7.0, 12.25, 12.75)):
        a, t = at(F, 10000)
        assert a_lo <= a <= a_hi and t_lo <= t <= t_hi, (F, a, t)
    # (2) no force, no deformation: 2 x 3.91 um both ways
    assert np.abs(at(0, 40000) - 7.82).max() < 0.01
    # (3) the force-displacement curves are monotone
    fin = np.array([at(F, 40000) for F in forces])
    assert (np.diff(fin[:, 0]) > 0).all() and (np.diff(fin[:, 1]) < 0).all(), fin
    # (4) approach to the published steady state: closer at 40 000 than at 10 000 iterations, from the unstretched side, gap bounded
    for F in forces[1:]:
        ra, rt = np.interp(F, ref_ax[:, 0], ref_ax[:, 1]), np.interp(F, ref_tr[:, 0], ref_tr[:, 1])
        a1, t1 = at(F, 10000); a4, t4 = at(F, 40000)
        assert a1 < a4 < ra and rt < t4 < t1, (F, a1, a4, ra, t1, t4, rt)
        assert (ra - a4) / ra < 0.11 and (t4 - rt) < 1.05, (F, a4, ra, t4, rt)
    print("\nforce axial transverse published_axial published_transverse")
    for F, (a, t) in zip(forces, fin):
        print("%5d %7.3f %7.3f %7.3f %7.3f" % (F, a, t, np.interp(F, ref_ax[:, 0], ref_ax[:, 1]), np.interp(F, ref_tr[:, 0], ref_tr[:, 1])))


def test_reference_onecellshear_driver_runs_config_c1(tmp_path, gpu):
    """BASELINE config 1 through the reference's own driver and config (examples/oneCellShear: 40 x 40 x 20 box, shear
    rate 111 1/s, one RBC, 100 000 iterations, report every 2000).  The reference holds no known-answer for this case,
    so the checks are physical: the membrane keeps its volume and area, the cell stays between the walls, it is
    stretched by the shear (positive deformation index that settles), and the run reaches the end."""
    import shutil
    work = tmp_path / "shear_case"
    shutil.copytree(os.path.join(ROOT, "tests", "golden", "shear_case"), str(work))
    r = subprocess.run([_ref_driver("oneCellShear"), "config.xml"], cwd=str(work), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "Simulation finished" in r.stdout
    rows = np.array([[float(x) for x in l.split()] for l in open(str(work / "stretch.log")).read().splitlines()])
    assert rows.shape == (50, 8) and rows[-1, 0] == 100000
    vol, surf, diam, di = rows[:, 4], rows[:, 5], rows[:, 6], rows[:, 7]
    assert np.abs(vol - 100).max() < 0.5 and np.abs(surf - 100).max() < 2.0
    assert (di > 0).all() and di.max() < 20 and abs(di[-1] - di[-10:].mean()) < 1.0      # deformed and settled
    assert diam.min() > 7.5 and diam.max() < 9.5
    centre = [l for l in r.stdout.splitlines() if "Cell center at" in l][-1]
    z = float(centre.split("{")[1].split("}")[0].split(",")[2])
    assert 3.0 < z < 7.0                                                                # stays between the walls (box height 10 um)


def test_reference_performance_testing_driver_runs_its_1_rank_case(tmp_path, gpu):
    """cases/performance_testing/performance_testing.cpp (compiled unchanged) on the reference's own inputs for the 1-rank
    case of its strong-scaling series (tests/golden/performance_case: 256^3 fully periodic, hematocrit_33/RBC.pos,
    velocities interpolated every step).  The reference holds no known answer for this case: the checks are that every
    cell of the .pos file that lies in the 128 um domain is placed and none is lost, and that the flow responds to the
    body force (statistics printed by the driver itself)."""
    drv = os.path.join(ROOT, "oracle", "_ref", "performance_testing_nohdf5")
    if not os.path.exists(drv):
        pytest.skip("oracle/_ref/performance_testing_nohdf5 is built by __graft_entry__.build() where the reference tree is present")
    import re
    import shutil
    case = os.path.join(ROOT, "tests", "golden", "performance_case")
    for name in ("RBC.xml", "RBC.pos"):
        shutil.copy(os.path.join(case, name), str(tmp_path / name))
    cfg = open(os.path.join(case, "config.xml")).read()
    cfg = re.sub(r"<tmax>[^<]*</tmax>", "<tmax> 100 </tmax>", cfg)
    cfg = re.sub(r"<tmeas>[^<]*</tmeas>", "<tmeas> 50 </tmeas>", cfg)
    (tmp_path / "config.xml").write_text(cfg)
    r = subprocess.run([drv, "config.xml"], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    pos = np.loadtxt(os.path.join(case, "RBC.pos"), skiprows=1)[:, :3] * 2.0          # lattice units (dx = 0.5 um)
    expected = int(((pos > -0.5) & (pos <= 255.5)).all(axis=1).sum())                # nearest node inside the 256^3 domain
    assert int(re.search(r"nCells \(global\) = (\d+)", r.stdout).group(1)) == expected == 9358
    counts = [int(m) for m in re.findall(r"# of cells: (\d+)", r.stdout)]
    assert counts == [expected, expected], counts
    means = [float(m) for m in re.findall(r"mean: ([0-9.eE+-]+) m/s", r.stdout)]
    assert len(means) == 2 and 0 < means[0] < means[1] < 1e-3, means                  # accelerating from rest, far below lattice speed
    assert "Simulation finished" in r.stdout
