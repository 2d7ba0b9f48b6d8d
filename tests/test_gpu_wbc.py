"""White blood cells on the GPU (WbcHighOrderModel, WBC_SPHERE), through the C ABI: mesh pins, membrane forces against
the CPU oracle plus a restatement of the inner-link law, coupled runs, slabs and the facade driver."""
import ctypes as C
import math
import multiprocessing as mp
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = os.path.join(ROOT, "tests", "golden", "wbc_case")
WBC_XML, ELL_XML = os.path.join(CASE, "WBC_HO.xml"), os.path.join(CASE, "ELL.xml")
pytestmark = pytest.mark.gpu

# (fixture, construct type, vertices, inner edges): examples/cell_shapes/WBC_HO.xml on WBC_SPHERE and
# cases/cellCollision_sphere/ELL.xml on ELLIPSOID_FROM_SPHERE (aspect ratio 1: an octasphere)
MESHES = {"wbc_sphere": (WBC_XML, 0, 642, 321), "ell": (ELL_XML, 6, 1026, 1026)}


def _wbc(gpu, P, mesh, **kw):
    xml, shape, _, _ = MESHES[mesh]
    return gpu.CellType.wbc(P, xml=xml, shape=shape, **kw)


class _OracleType:
    """an orc_celltype filled from the product's own tables (hcp_celltype_tables / _tables2): the oracle's force routine
    and simulation work on whatever mesh they are given.  model RBC_HO: the WBC model is that model plus the inner links"""

    def __init__(self, Tg, timescale=1):
        t = Tg.tables()
        ebt, ebo = np.empty((Tg.ne, 2), np.int64), np.empty((Tg.ne, 2), np.int64)
        ie, iel, nring = np.empty((max(Tg.nie, 1), 2), np.int64), np.empty(max(Tg.nie, 1)), np.empty(Tg.nv, np.int32)
        Tg.lib.hcp_celltype_tables2(Tg.ptr, O.lptr(ebt), O.lptr(ebo), O.lptr(ie), O.dptr(iel), nring.ctypes.data_as(O.c_int_p))
        self.keep = dict(vertices=np.ascontiguousarray(t["vertices"]), triangles=np.ascontiguousarray(t["triangles"]),
                         edges=np.ascontiguousarray(t["edges"]), edge_length_eq=t["edge_length_eq"], edge_angle_eq=t["edge_angle_eq"],
                         edge_bending_triangles=ebt, edge_bending_outer=ebo, triangle_area_eq=t["triangle_area_eq"],
                         vertex_vertexes=np.ascontiguousarray(t["vertex_vertexes"]), vertex_n_vertexes=nring,
                         patch_dist_eq=t["patch_dist_eq"], inner_edges=ie, inner_edge_length_eq=iel)
        s = O.CellType()
        s.model, s.nv, s.nt, s.ne, s.nie = 0, Tg.nv, Tg.nt, Tg.ne, 0    # the oracle's inner links are the platelet law: none here
        for name, a in self.keep.items():
            ptype = dict(O.CellType._fields_)[name]
            setattr(s, name, a.ctypes.data_as(ptype))
        for name in ("volume_eq", "area_mean_eq", "edge_mean_eq", "angle_mean_eq", "k_volume", "k_area", "k_link", "k_bend", "eta_m"):
            setattr(s, name, t[name])
        s.timescale = timescale
        self.s = s
        self.ptr = C.pointer(s)
        self.inner = ie[:Tg.nie].copy()
        self.inner_len_eq = iel[:Tg.nie].copy()


def _inner_links(inner, pos, k):
    """mechanics/wbcHighOrderModel.cpp:199-223 restated in scalar Python: per inner edge in list order, the cytoskeleton term
    then the rigid-core term, each subtracted from edge[0] and added to edge[1].  Returns the [nv][3] contribution
    (force_inner_link) and how many times each term fired"""
    f = np.zeros_like(pos)
    fired = [0, 0]
    for a, b in inner:
        ev = [pos[b][d] - pos[a][d] for d in range(3)]
        el = 0.0
        for d in range(3):
            el += ev[d] * ev[d]
        el = math.sqrt(el)
        uv = [ev[d] / el for d in range(3)]
        for term, (thr, kk) in enumerate(((2 * k["radius"], k["k_cytoskeleton"]), (2 * k["core_radius"], k["k_inner_rigid"]))):
            if el < thr:
                s = 1.0 - (el / thr)
                fr = [(uv[d] * s) * kk for d in range(3)]
                for d in range(3):
                    f[a][d] -= fr[d]
                    f[b][d] += fr[d]
                fired[term] += 1
    return f, fired


def _add_inner_links_in_order(inner, pos, k, force):
    """the unified force of the reference: the same inner-link additions continued on the accumulated force"""
    f = force.copy()
    for a, b in inner:
        ev = [pos[b][d] - pos[a][d] for d in range(3)]
        el = math.sqrt(ev[0] * ev[0] + ev[1] * ev[1] + ev[2] * ev[2])
        uv = [ev[d] / el for d in range(3)]
        for thr, kk in ((2 * k["radius"], k["k_cytoskeleton"]), (2 * k["core_radius"], k["k_inner_rigid"])):
            if el < thr:
                s = 1.0 - (el / thr)
                for d in range(3):
                    fr = (uv[d] * s) * kk
                    f[a][d] -= fr
                    f[b][d] += fr
    return f


@pytest.mark.parametrize("mesh", list(MESHES))
def test_wbc_mesh_pins(gpu, mesh):
    """WBC_SPHERE (constructSphereIcosahedron, helper/meshGeneratingFunctions.h:73-74) and the octasphere of ELL.xml: the
    vertex numbering of the product's welding makes every inner edge of the reference's XML join two antipodes"""
    xml, shape, nv, nie = MESHES[mesh]
    P = gpu.base_parameters()
    T = _wbc(gpu, P, mesh)
    assert (T.nv, T.nie) == (nv, nie)
    if mesh == "wbc_sphere":
        assert T.nt == 1280
    t = T.tables()
    V = t["vertices"]
    c = V.mean(0)
    ot = _OracleType(T)
    mid = 0.5 * (V[ot.inner[:, 0]] + V[ot.inner[:, 1]])
    assert np.abs(mid - c).max() <= 1e-9
    R = 4e-6 / P.dx
    # rest length 2R + 2e-3 (inflate() moves every vertex 1e-3 lu out along its vertex normal); the vertex normals of these
    # meshes lean off the radius by up to ~1e-2 rad, which shortens a few diameters by up to 3e-7 lu
    assert np.abs(ot.inner_len_eq - (2 * R + 2e-3)).max() <= 1e-6
    d = V[ot.inner[:, 1]] - V[ot.inner[:, 0]]
    assert np.array_equal(ot.inner_len_eq, np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]))
    # moduli: the RBC model's, plus the four WBC constants (mechanics/wbcHighOrderModel.cpp:242-262)
    m = gpu.read_material(xml)
    k = T.wbc_constants()
    assert k == dict(k_inner_rigid=m["kInnerRigid"] / P.df, k_cytoskeleton=m["kCytoskeleton"] / P.df,
                     core_radius=m["coreRadius"] / P.dx, radius=m["radius"] / P.dx)
    Tr = gpu.CellType(P, gpu.MODEL_RBC_HO, shape, m["radius"], int(m["minNumTriangles"]), m["kLink"], m["kArea"], m["kVolume"],
                      m["kBend"], m["eta_m"], aspect_ratio=m.get("aspectRatio", 0.3))
    tr = Tr.tables()
    for name in ("vertices", "triangles", "edges", "edge_length_eq", "patch_dist_eq", "scalars"):
        assert np.array_equal(tr[name], t[name]), name
    assert Tr.wbc_constants() == dict(k_inner_rigid=0.0, k_cytoskeleton=0.0, core_radius=0.0, radius=0.0)
    Tr.destroy(); T.destroy()


def test_wbc_model_needs_its_own_entry_point(gpu):
    P = gpu.base_parameters()
    M = gpu.capi.Material(kLink=60.0, kArea=20.0, kVolume=20.0, kBend=200.0, radius=4e-6, min_triangles=600, aspect_ratio=0.3)
    ptr = C.c_void_p()
    lib = gpu.capi.lib()
    assert lib.hcp_celltype_create(C.byref(ptr), gpu.MODEL_WBC_HO, gpu.WBC_SPHERE, C.byref(P), C.byref(M)) != 0
    assert b"hcp_celltype_create_wbc" in lib.hc_last_error()
    assert lib.hcp_celltype_create_wbc(C.byref(ptr), gpu.WBC_SPHERE, C.byref(P), C.byref(M), None) != 0


@pytest.mark.parametrize("state", ["rest", "compressed_0.8", "compressed_0.55", "random"])
@pytest.mark.parametrize("mesh", list(MESHES))
def test_wbc_forces_vs_oracle(orc, gpu, mesh, state):
    """components 0-4 bit-identical to the oracle's RBC_HO forces on the same tables (the WBC evaluates its membrane
    viscosity without the eta_m test; with eta_m = 0 that only adds zeros), component 5 bit-identical to the restatement
    of :199-223, the unified force equal to the reference's accumulation order"""
    rng = np.random.default_rng(23)
    P = gpu.base_parameters()
    kw = dict(eta_m=5e-10) if (state == "random" and mesh == "ell") else {}   # ELL.xml has eta_m = 0
    T = _wbc(gpu, P, mesh, **kw)
    k = T.wbc_constants()
    ot = _OracleType(T)
    L = gpu.Lattice(64, 48, 48, (1, 1, 1), 1.0)
    cells = gpu.Cells(L, P)
    t = cells.addCellType(T, 1)
    for c, a in (((16.3, 24.1, 23.7), (0, 0, 0)), ((45.0, 22.4, 25.2), (35.0, 10.0, -70.0))):
        assert cells.addCell(t, c, a)
    pos = cells.positions.reshape(2, T.nv, 3)
    vel = np.zeros_like(pos)
    if state.startswith("compressed"):
        s = float(state.split("_")[1])
        cen = pos.mean(1, keepdims=True)
        pos = cen + s * (pos - cen)
    elif state == "random":
        pos = pos + 0.05 * rng.standard_normal(pos.shape)
        vel = 1e-3 * rng.standard_normal(pos.shape)
    cells.positions = pos.reshape(-1, 3); cells.velocities = vel.reshape(-1, 3)
    cells.applyConstitutiveModel(0, True)
    fg = cells.forces.reshape(2, T.nv, 3)
    comp = cells.force_components(t).reshape(6, 2, T.nv, 3)
    fired = [0, 0]
    for c in range(2):
        p, v = np.ascontiguousarray(pos[c]), np.ascontiguousarray(vel[c])
        co, fo = np.zeros((6, T.nv, 3)), np.zeros((T.nv, 3))
        orc.orc_cell_forces(ot.ptr, O.dptr(p), O.dptr(v), O.dptr(np.zeros((T.nv, 3))), O.dptr(co), 0x0f)
        orc.orc_cell_forces(ot.ptr, O.dptr(p), O.dptr(v), O.dptr(fo), None, 0x0f)
        for j in range(5):
            assert np.array_equal(comp[j, c], co[j]), (j, np.abs(comp[j, c] - co[j]).max())
        fi, n = _inner_links(ot.inner, p, k)
        fired = [fired[0] + n[0], fired[1] + n[1]]
        assert np.array_equal(comp[5, c], fi), np.abs(comp[5, c] - fi).max()
        fu = _add_inner_links_in_order(ot.inner, p, k, fo)
        assert np.abs(fg[c] - fu).max() <= 1e-14 * np.abs(fu).max()
    nie = 2 * T.nie
    if state == "rest":
        assert fired == [0, 0]
    elif state == "compressed_0.8":
        assert fired == ([nie, 0] if mesh == "wbc_sphere" else [nie, nie])   # 6.4 um: cytoskeleton only for WBC_HO.xml
        assert np.abs(comp[5]).max() > 0
    elif state == "compressed_0.55":
        assert fired == [nie, nie]
    cells.destroy(); L.destroy(); T.destroy()


def test_wbc_and_rbc_coupled_without_inner_links_match_the_oracle(orc, gpu):
    """with kInnerRigid = kCytoskeleton = 0 a WBC is the RBC_HO model on its own mesh, with the viscosity term always on:
    one WBC and one RBC in a bounce-back pipe, 200 iterations at stepMaterialEvery 4, stepParticleEvery 2, against
    orc_sim_iterate with an RBC_HO type built from the WBC tables"""
    nx, ny, nz = 64, 30, 30
    k_m, k_p = 4, 2
    mask, _ = gpu.pipe_mask(nx, ny, nz)
    Po, Pg = O.make_params(orc), gpu.base_parameters()
    Lo = O.OracleLattice(orc, nx, ny, nz, (1, 0, 0), 1.0 / Po.tau)
    Lg = gpu.Lattice(nx, ny, nz, (1, 0, 0), 1.0 / Pg.tau)
    Lo.set_mask(mask); Lg.defineBounceBack(mask)
    Lo.init_equilibrium(); Lg.latticeEquilibrium()
    Tw = _wbc(gpu, Pg, "wbc_sphere", kInnerRigid=0.0, kCytoskeleton=0.0)
    ow = _OracleType(Tw, timescale=k_m)
    assert ow.s.eta_m != 0.0        # WBC_HO.xml: eta_m = 1e-9, so the oracle's RBC path evaluates the viscosity as well
    To = O.make_rbc(orc, Po); To.contents.timescale = k_m
    So = orc.orc_sim_create(Lo.ptr, C.byref(Po))
    orc.orc_sim_add_type(So, ow.ptr); orc.orc_sim_add_type(So, To)
    hg = gpu.HemoCell(Lg, Pg)
    hg.cellfields.addCellType(Tw, k_m); hg.cellfields.addCellType(gpu.CellType.rbc(Pg), k_m)
    So.contents.particle_velocity_timescale = k_p
    hg.setParticleVelocityUpdateTimeScaleSeparation(k_p)
    for t, c, a in ((0, (16.0, 14.5, 14.5), (0.0, 0.0, 0.0)), (1, (46.0, 14.5, 14.5), (90.0, 0.0, 0.0))):
        cc = np.array(c)
        a_ref = np.array(a) * (3.14159265358979323846 / 180.0) * -1.0
        assert orc.orc_sim_add_cell(So, t, O.dptr(cc), O.dptr(a_ref), 0.0) == 1
        assert hg.cellfields.addCell(t, c, a)
    F = (5e-6, 0.0, 0.0)
    Lo.set_force_uniform(F); Lg.setExternalVector(F)
    for d in range(3):
        So.contents.body_force[d] = F[d]
    Lo.set_threads(8)
    orc.orc_sim_mechanics(So, 1); hg.cellfields.applyConstitutiveModel(0, True)
    steps = 200
    for _ in range(steps):
        orc.orc_sim_iterate(So)
    hg.iterate(steps)
    po = np.zeros((So.contents.np, 3)); orc.orc_sim_get(So, 0, O.dptr(po))
    pg = hg.cellfields.positions
    assert np.abs(pg - po).max() <= 1e-9, np.abs(pg - po).max()
    assert np.abs(pg[:Tw.nv, 0].mean() - po[:Tw.nv, 0].mean()) < 1e-9 and pg[:Tw.nv, 0].mean() > 16.0 + 1e-3   # it moved
    fluid = mask.reshape(-1) == 0
    fo, fg = Lo.f[fluid], Lg.populations()[fluid]
    assert np.abs(fg - fo).max() <= 1e-6 * np.abs(fo).max()
    orc.orc_sim_destroy(So); Lo.destroy(); Lg.destroy()


def _squeeze_run(gpu, kInnerRigid, steps, per_vertex_pn):
    """one WBC_HO.xml cell in a periodic box, its two z caps pushed towards each other before every iteration (the
    HemoCellStretch pattern, helper/hemoCellStretch.cpp); returns the minimum inner-edge length seen, volumes, NaN flag"""
    P = gpu.base_parameters()
    n = 48
    L = gpu.Lattice(n, n, n, (1, 1, 1), 1.0 / P.tau)
    L.latticeEquilibrium()
    h = gpu.HemoCell(L, P)
    kw = {} if kInnerRigid is None else dict(kInnerRigid=kInnerRigid)
    T = gpu.CellType.wbc(P, **kw)
    t = h.cellfields.addCellType(T, 1)
    assert h.cellfields.addCell(t, (24.0, 24.0, 24.0))
    ot = _OracleType(T)
    pos = h.cellfields.positions
    dz = pos[:, 2] - pos[:, 2].mean()
    top, bottom = np.nonzero(dz > 6.5)[0], np.nonzero(dz < -6.5)[0]
    idx = np.concatenate([top, bottom])
    f = per_vertex_pn * 1e-12 / P.df
    frc = np.zeros((len(idx), 3)); frc[:len(top), 2] = -f; frc[len(top):, 2] = f
    v0 = h.cellfields.cell_info(t)["volume"][0]
    lmin, vols = np.inf, []
    for it in range(steps):
        h.cellfields.addVertexForce(idx, frc)
        h.iterate(1)
        if (it + 1) % 100 == 0:
            p = h.cellfields.positions
            d = p[ot.inner[:, 1]] - p[ot.inner[:, 0]]
            lmin = min(lmin, np.sqrt((d * d).sum(1)).min())
            vols.append(h.cellfields.cell_info(t)["volume"][0] / v0)
    nan = bool(np.isnan(h.cellfields.positions).any())
    h.cellfields.destroy(); L.destroy(); T.destroy()
    return lmin, np.array(vols), nan, ot.inner_len_eq.min()


def test_wbc_rigid_core_resists_a_squeeze(gpu):
    """the inner links act in a coupled run: squeezed between its two z caps, the cell with the fixture's rigid core keeps
    its diameters longer than the same cell without it, and both keep their volume"""
    steps, f_pn = 1200, 20.0   # without the core the closest antipodes come to ~7 lu, inside 2 core_radius = 10 lu
    on = _squeeze_run(gpu, None, steps, f_pn)
    off = _squeeze_run(gpu, 0.0, steps, f_pn)
    print("squeeze: min inner-edge length with core %.4f, without %.4f (rest %.4f)" % (on[0], off[0], on[3]))
    assert not on[2] and not off[2]
    assert off[0] < on[0] < on[3]
    for r in (on, off):
        assert np.abs(r[1] - 1).max() < 0.02, r[1]


# ----------------------------------------------------------------------------------------------- slabs
NXG, NY, NZ, STEPS = 96, 34, 34, 200
WBCS = [((47.0, 16.5, 16.5), (0, 0, 0)), ((12.0, 17.0, 16.0), (20, 10, 0))]     # the first one across the face at x = 48


def _slab_build(rank, world):
    from hemocell_amd import host
    from hemocell_amd.slab import SlabRunner
    P = host.base_parameters()
    r = SlabRunner(NXG // world, NY, NZ, rank, world, P, periodic=(True, False, False), particle_timescale=2,
                   material_timescale=2, deletion_check_every=1)
    mask, _ = host.pipe_mask(NXG, NY, NZ)
    r.define_bounce_back(mask)
    r.lattice.latticeEquilibrium(1.0, (0, 0, 0))
    r.lattice.setExternalVector((1e-4, 0.0, 0.0))
    r.add_cell_type(host.CellType.wbc(P, kInnerRigid=6.40625e-10))   # a core that acts in this flow
    r.load_cells(0, [np.array(c) for c, _ in WBCS], [np.array(a) for _, a in WBCS])
    assert tuple(r.sync_placement()) == (len(WBCS),)
    r.prepare()
    return r, mask


def _slab_worker(rank, world, port, out, q):
    try:
        sys.path.insert(0, ROOT)
        from hemocell_amd import host, slab
        slab.comm_init(rank, world, local_rank=0, port=port, transport="tcp")
        r, _ = _slab_build(rank, world)
        r.run(STEPS)
        cid, vid, pos = r.owned_vertex_table(0)
        np.savez(os.path.join(out, "w%d.npz" % rank), f=r.populations(), cid=cid, vid=vid, pos=pos,
                 stats=np.array(list(r.slab_stats().values())))
        slab.barrier()
        slab.comm_finalize()
        q.put((rank, "ok"))
    except BaseException as e:   # noqa: BLE001 -- reported by the parent
        import traceback
        q.put((rank, "FAILED: %r\n%s" % (e, traceback.format_exc())))


def test_wbc_slabs_equal_single_domain_bit_for_bit(tmp_path, gpu):
    """2 host-staged ranks on one GPU with a WBC across the face, reproducible spread: populations and vertex positions
    are the bits of the single domain, so the envelope and the cell records carry the new type unchanged"""
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 32000 + (os.getpid() * 7 + 977) % 20000
    os.environ["HEMOCELL_COMM_TIMEOUT"] = "90"
    os.environ["HEMOCELL_REPRODUCIBLE_SPREAD"] = "1"     # the ranks choose the spread at its first use
    ps = [ctx.Process(target=_slab_worker, args=(r, world, port, str(tmp_path), q)) for r in range(world)]
    for p in ps:
        p.start()
    del os.environ["HEMOCELL_REPRODUCIBLE_SPREAD"]
    res = [q.get(timeout=600) for _ in ps]
    for p in ps:
        p.join(60)
    assert all(r[1] == "ok" for r in res), res
    lib = gpu.capi.lib()
    gpu.check(lib.hc_set_reproducible_spread(1))
    try:
        ref, mask = _slab_build(0, 1)
        ref.run(STEPS)
        f_ref = ref.lattice.populations().reshape(NXG, NY * NZ, 19)
        p_ref = ref.cells.positions.reshape(len(WBCS), -1, 3)
    finally:
        gpu.check(lib.hc_set_reproducible_spread(0))
    out = [dict(np.load(os.path.join(str(tmp_path), "w%d.npz" % k))) for k in range(world)]
    f_all = np.concatenate([o["f"].reshape(NXG // world, NY * NZ, 19) for o in out], axis=0)
    fluid = mask.reshape(NXG, NY * NZ) == 0
    assert np.abs(f_all - f_ref)[fluid].max() == 0.0
    for o in out:
        assert np.array_equal(o["pos"], p_ref[o["cid"], o["vid"]])
    assert all((o["cid"] == 0).any() for o in out)   # the crossing cell has vertices on both slabs


# ----------------------------------------------------------------------------------------------- facade driver
def test_wbc_collision_driver(tmp_path, gpu):
    """examples/wbc/wbc_collision.cpp on tests/golden/wbc_case: both cells placed, the WBC statistics logged, volumes
    kept, the two cells carried in opposite x directions by the shear"""
    from hemocell_amd import capi
    exe = str(tmp_path / "wbc_collision")
    libdir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wno-deprecated-declarations", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "hemocell_amd", "compat"), os.path.join(ROOT, "examples", "wbc", "wbc_collision.cpp"),
                           "-o", exe, "-L" + libdir, "-lhemocell_amd", "-Wl,-rpath," + libdir])
    work = tmp_path / "case"
    shutil.copytree(CASE, str(work))
    for f in os.listdir(str(work)):
        os.chmod(str(work / f), 0o644)
    cfg = open(str(work / "config.xml")).read()
    cfg = re.sub(r"<tmax>[^<]*</tmax>", "<tmax> 2000 </tmax>", cfg)
    open(str(work / "config.xml"), "w").write(cfg)
    r = subprocess.run([exe, "config.xml"], cwd=str(work), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    out = r.stdout
    assert "(readPositionsBloodCells) 2 complete WBC_HO cells placed." in out
    for tag in ("k_cytoskeleton:", "k_inner_rigid:", "wbc_radius:", "core_radius:"):
        assert "\t " + tag in out, tag
    assert out.rstrip().splitlines()[-1] == "(WbcCollision) Simulation finished :)"

    def csv(it):
        rows = open(str(work / "tmp" / "csv" / ("WBC_HO.%012d.csv" % it))).read().splitlines()[1:]
        a = np.array([[float(v) for v in l.split(",")] for l in rows])
        return a[np.argsort(a[:, 6])]
    c0, c1 = csv(0), csv(2000)
    assert len(c0) == len(c1) == 2
    assert np.abs(c1[:, 4] / c0[:, 4] - 1).max() < 0.02
    dx = c1[:, 0] - c0[:, 0]
    lower = np.argmin(c0[:, 2])   # below the mid-plane the flow goes to +x, above it to -x
    assert dx[lower] > 1e-8 and dx[1 - lower] < -1e-8, dx
