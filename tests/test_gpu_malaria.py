"""Malaria-infected cells (RbcMalariaModel) and cell meshes from STL files (MESH_FROM_STL) on the GPU, through the C ABI:
mesh construction against a numpy restatement, the reference's numbering pin, the truncated neighbour rings, the ASCII
reader, membrane forces against the CPU oracle plus a restatement of the inner-link law (the wide per-vertex tables
included), the old model / shape pairs through the general entry point, coupled runs, slabs and the facade driver.
Inputs: tests/golden/malaria_case only."""
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
CASE = os.path.join(ROOT, "tests", "golden", "malaria_case")
XML = os.path.join(CASE, "RBC_MALARIA.xml")
STLS = {"stretch": os.path.join(CASE, "vRBC_uniform.stl"), "pipeflow": os.path.join(CASE, "vRBC_uniform_pipeflowMalaria.stl")}
COUNTS = {"stretch": (1507, 3010, 4515), "pipeflow": (1509, 3014, 4521)}
pytestmark = pytest.mark.gpu


class _OracleType:
    """an orc_celltype filled from the product's own tables (hcp_celltype_tables / _tables2), model RBC_HO: the malaria
    model is that model plus the linear inner links, which the oracle does not have (its inner links are the platelet's)"""

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
        s.model, s.nv, s.nt, s.ne, s.nie = 0, Tg.nv, Tg.nt, Tg.ne, 0
        for name, a in self.keep.items():
            setattr(s, name, a.ctypes.data_as(dict(O.CellType._fields_)[name]))
        for name in ("volume_eq", "area_mean_eq", "edge_mean_eq", "angle_mean_eq", "k_volume", "k_area", "k_link", "k_bend", "eta_m"):
            setattr(s, name, t[name])
        s.timescale = timescale
        self.s = s
        self.ptr = C.pointer(s)
        self.tables = t
        self.nring = nring
        self.inner = ie[:Tg.nie].copy()
        self.inner_len_eq = iel[:Tg.nie].copy()


def _inner_links(inner, leq, pos, k, force=None):
    """mechanics/rbcMalariaModel.cpp:198-217 in scalar Python: per inner edge in list order, f = uv * (k_inner_link * 5.0 *
    (l - l0) / l0) added to edge[0] and subtracted from edge[1]; continued on `force` when given"""
    f = np.zeros_like(pos) if force is None else force.copy()
    for n, (a, b) in enumerate(inner):
        ev = [pos[b][d] - pos[a][d] for d in range(3)]
        el = math.sqrt(ev[0] * ev[0] + ev[1] * ev[1] + ev[2] * ev[2])
        uv = [ev[d] / el for d in range(3)]
        ef = (el - leq[n]) / leq[n]
        fs = k * 5.0 * ef
        for d in range(3):
            f[a][d] += uv[d] * fs
            f[b][d] -= uv[d] * fs
    return f


def _read_binary_stl(path):
    raw = open(path, "rb").read()
    n = int(np.frombuffer(raw[80:84], np.uint32)[0])
    rec = np.frombuffer(raw[84:], np.dtype([("n", "<f4", 3), ("v", "<f4", (3, 3)), ("a", "<u2")]), count=n)
    return rec["v"]   # [n][3 corners][3] float32


def _restated_mesh(path, radius_lu):
    """constructCell (helper/meshGeneratingFunctions.hh:275-288) restated: scale the largest extent to 2 radius, rotate
    zxz(pi/2, pi/2, 0), weld by first occurrence on exact coordinates, inflate 1e-3 lu along the vertex normals"""
    v = _read_binary_stl(path)
    ids, verts, tris = {}, [], []
    for tr in v:
        row = []
        for p in tr:
            key = tuple(float(x) for x in p)
            if key not in ids:
                ids[key] = len(verts)
                verts.append(key)
            row.append(ids[key])
        tris.append(row)
    p = np.array(verts)
    allp = v.reshape(-1, 3).astype(np.float64)
    sf = (allp.max(0) - allp.min(0)).max()
    p = p * (radius_lu * 2.0 / sf)
    th, ph = math.pi / 2.0, math.pi / 2.0
    a = np.array([[1, 0, 0], [0, math.cos(th), -math.sin(th)], [0, math.sin(th), math.cos(th)]])
    b = np.array([[math.cos(ph), -math.sin(ph), 0], [math.sin(ph), math.cos(ph), 0], [0, 0, 1]])
    m = np.eye(3) @ (a @ b)
    p = p @ m.T
    tris = np.array(tris)
    vn = np.zeros_like(p)
    for t in tris:
        n = np.cross(p[t[1]] - p[t[0]], p[t[2]] - p[t[0]])
        n /= np.linalg.norm(n)
        vn[t] += n
    p = p + 1e-3 * (vn / np.linalg.norm(vn, axis=1)[:, None])
    return p, tris


def _restated_rings(tris, edges):
    """mechanics/commonCellConstants.cpp:213-271: the first six neighbours in edge-list order, then the fan walk"""
    nv = tris.max() + 1
    ring = [[] for _ in range(nv)]
    for a, b in edges:
        if len(ring[a]) < 6:
            ring[a].append(b)
        if len(ring[b]) < 6:
            ring[b].append(a)
    half = {}
    for t, tr in enumerate(tris):
        for k in range(3):
            half[(tr[k], tr[(k + 1) % 3])] = t
    for v in range(nv):
        cur = ring[v][0]
        for n in range(1, len(ring[v])):
            tr = list(tris[half[(v, cur)]])
            cur = tr[(tr.index(v) + 2) % 3]
            ring[v][n] = cur
    out = -np.ones((nv, 6), np.int64)
    for v in range(nv):
        out[v, :len(ring[v])] = ring[v]
    return out, np.array([len(r) for r in ring])


@pytest.mark.parametrize("stl", list(STLS))
def test_stl_mesh_construction(gpu, stl):
    """counts, vertex positions against the restatement, triangles and the truncated rings; k_inner_link in lattice units"""
    P = gpu.base_parameters()
    T = gpu.CellType.malaria(P, stl=STLS[stl])
    assert (T.nv, T.nt, T.ne) == COUNTS[stl]
    assert T.nie == 525
    ot = _OracleType(T)
    t = ot.tables
    p, tris = _restated_mesh(STLS[stl], 5.4e-6 / P.dx)
    assert np.array_equal(t["triangles"], tris)
    assert np.abs(t["vertices"] - p).max() <= 1e-12, np.abs(t["vertices"] - p).max()
    ext = t["vertices"].max(0) - t["vertices"].min(0)
    assert abs(ext.max() - 2 * 5.4e-6 / P.dx) < 1e-2   # 2 radius, plus the inflate
    edges = []
    for tr in tris:
        for k in range(3):
            if tr[k] < tr[(k + 1) % 3]:
                edges.append((tr[k], tr[(k + 1) % 3]))
    assert np.array_equal(t["edges"], np.array(edges))
    ring, nring = _restated_rings(tris, edges)
    assert np.array_equal(t["vertex_vertexes"], ring) and np.array_equal(ot.nring, nring)
    valence = np.bincount(np.array(edges).reshape(-1), minlength=T.nv)
    assert valence.max() == (8 if stl == "stretch" else 10)
    assert (ot.nring[valence > 6] == 6).all() and (ot.nring[valence <= 6] == valence[valence <= 6]).all()
    assert t["volume_eq"] > 0
    m = gpu.read_material(XML)
    assert T.malaria_constants() == dict(k_inner_link=m["kInnerLink"] * (P.kBT_lbm / (7.5e-9 / P.dx)))
    T.destroy()


def test_inner_edge_numbering_pin(gpu):
    """the 525 inner edges of RBC_MALARIA.xml were made for the first-occurrence numbering of the stretchMalaria STL: all
    are shorter than 0.3 of the cell's length, which random vertex pairs are not.  On the pipeflowMalaria STL the reference
    applies the same list to another numbering; that is reproduced as it is"""
    P = gpu.base_parameters()
    lens = {}
    for stl in STLS:
        T = gpu.CellType.malaria(P, stl=STLS[stl])
        ot = _OracleType(T)
        V = ot.tables["vertices"]
        L = (V.max(0) - V.min(0)).max()
        d = V[ot.inner[:, 1]] - V[ot.inner[:, 0]]
        assert np.array_equal(ot.inner_len_eq, np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]))
        lens[stl] = ot.inner_len_eq / L
        if stl == "stretch":
            rng = np.random.default_rng(5)
            pairs = rng.integers(0, T.nv, size=(525, 2))
            r = np.linalg.norm(V[pairs[:, 1]] - V[pairs[:, 0]], axis=1) / L
            assert (r > 0.3).sum() > 100
        T.destroy()
    assert lens["stretch"].max() <= 0.3
    assert lens["pipeflow"].max() > 0.5


def test_ascii_stl_gives_identical_tables(gpu, tmp_path):
    """an ASCII copy of the stretch STL written with %.17g is read as double and gives the same tables bit for bit"""
    v = _read_binary_stl(STLS["stretch"])
    path = str(tmp_path / "cell_ascii.stl")
    with open(path, "w") as f:
        f.write("solid cell\n")
        for tr in v:
            f.write("  facet normal 0 0 0\n    outer loop\n")
            for p in tr:
                f.write("      vertex %.17g %.17g %.17g\n" % tuple(float(x) for x in p))
            f.write("    endloop\n  endfacet\n")
        f.write("endsolid cell\n")
    P = gpu.base_parameters()
    Tb, Ta = gpu.CellType.malaria(P, stl=STLS["stretch"]), gpu.CellType.malaria(P, stl=path)
    tb, ta = Tb.tables(), Ta.tables()
    for name in ("vertices", "triangles", "edges", "edge_length_eq", "edge_angle_eq", "triangle_area_eq", "vertex_vertexes",
                 "patch_dist_eq", "scalars"):
        assert np.array_equal(ta[name], tb[name]), name
    Ta.destroy(); Tb.destroy()


def test_bad_stl_inputs_are_refused(gpu, tmp_path):
    P = gpu.base_parameters()
    lib = gpu.capi.lib()
    with pytest.raises(gpu.HcError, match="cannot open STL file"):
        gpu.CellType.malaria(P, stl=str(tmp_path / "missing.stl"))
    v = _read_binary_stl(STLS["stretch"]).astype(np.float64)

    def write(name, tris):
        path = str(tmp_path / name)
        with open(path, "w") as f:
            f.write("solid x\n")
            for tr in tris:
                f.write("facet normal 0 0 0\nouter loop\n")
                for p in tr:
                    f.write("vertex %.17g %.17g %.17g\n" % tuple(p))
                f.write("endloop\nendfacet\n")
            f.write("endsolid x\n")
        return path
    with pytest.raises(gpu.HcError, match="open mesh"):
        gpu.CellType.malaria(P, stl=write("open.stl", v[:-1]))
    deg = v.copy(); deg[7, 2] = deg[7, 1]
    with pytest.raises(gpu.HcError, match="degenerate triangle 7"):
        gpu.CellType.malaria(P, stl=write("degenerate.stl", deg))
    with pytest.raises(gpu.HcError, match="oriented manifold"):
        gpu.CellType.malaria(P, stl=write("twice.stl", np.concatenate([v, v])))   # the same surface twice
    # a second copy reflected through the vertex of largest x (corner order reversed to keep it outward): two closed
    # surfaces that share one vertex, whose triangles then form two fans
    c = v.reshape(-1, 3)[np.argmax(v.reshape(-1, 3)[:, 0])]
    refl = (2.0 * c - v)[:, ::-1, :]
    with pytest.raises(gpu.HcError, match="non-manifold mesh"):
        gpu.CellType.malaria(P, stl=write("touching.stl", np.concatenate([v, refl])))
    M = gpu.capi.Material(kLink=15.0, kArea=3.0, kVolume=-0.5, kBend=60.0, radius=5.4e-6, min_triangles=1)
    ptr = C.c_void_p()
    assert lib.hcp_celltype_create(C.byref(ptr), gpu.MODEL_RBC_MALARIA, gpu.MESH_FROM_STL, C.byref(P), C.byref(M)) != 0
    assert b"hcp_celltype_create_ex" in lib.hc_last_error()
    assert lib.hcp_celltype_create(C.byref(ptr), gpu.MODEL_RBC_HO, gpu.MESH_FROM_STL, C.byref(P), C.byref(M)) != 0
    assert b"hcp_celltype_create_ex" in lib.hc_last_error()
    assert lib.hcp_celltype_create_wbc(C.byref(ptr), gpu.MESH_FROM_STL, C.byref(P), C.byref(M),
                                       C.byref(gpu.capi.WbcMaterial(1.0, 1.0, 1e-6, 4e-6))) != 0
    assert b"hcp_celltype_create_ex" in lib.hc_last_error()


def _place_two(gpu, P, T, seed, state, scale_vel=1e-3):
    L = gpu.Lattice(72, 48, 48, (1, 1, 1), 1.0)
    cells = gpu.Cells(L, P)
    t = cells.addCellType(T, 1)
    for c, a in (((18.3, 24.1, 23.7), (90, 0, 0)), ((54.0, 22.4, 25.2), (35.0, 10.0, -70.0))):
        assert cells.addCell(t, c, a)
    rng = np.random.default_rng(seed)
    pos = cells.positions.reshape(2, T.nv, 3)
    cen = pos.mean(1, keepdims=True)
    if state == "perturbed":
        pos = pos + 0.05 * rng.standard_normal(pos.shape)
    elif state == "stretched":
        pos = cen + (pos - cen) * np.array([1.15, 0.93, 0.93])
    vel = scale_vel * rng.standard_normal(pos.shape)
    cells.positions = pos.reshape(-1, 3); cells.velocities = vel.reshape(-1, 3)
    return L, cells, t, pos, vel


@pytest.mark.parametrize("eta_m", [0.0, 5e-10])
@pytest.mark.parametrize("state", ["rest", "perturbed", "stretched"])
@pytest.mark.parametrize("stl", list(STLS))
def test_malaria_forces_vs_oracle(orc, gpu, stl, state, eta_m):
    """components 0-4 bit-identical to the oracle's RBC_HO forces on the same tables (the malaria model evaluates its
    membrane viscosity without the eta_m test; with eta_m = 0 that adds only zeros), component 5 bit-identical to the
    restatement of :198-217, the unified force equal to the reference's accumulation order"""
    P = gpu.base_parameters()
    T = gpu.CellType.malaria(P, stl=STLS[stl], eta_m=eta_m)
    k = T.malaria_constants()["k_inner_link"]
    ot = _OracleType(T)
    assert ot.s.eta_m == eta_m * P.dx / P.dt / P.df
    L, cells, t, pos, vel = _place_two(gpu, P, T, 11, state)
    cells.applyConstitutiveModel(0, True)
    fg = cells.forces.reshape(2, T.nv, 3)
    comp = cells.force_components(t).reshape(6, 2, T.nv, 3)
    for c in range(2):
        p, v = np.ascontiguousarray(pos[c]), np.ascontiguousarray(vel[c])
        co, fo = np.zeros((6, T.nv, 3)), np.zeros((T.nv, 3))
        orc.orc_cell_forces(ot.ptr, O.dptr(p), O.dptr(v), O.dptr(np.zeros((T.nv, 3))), O.dptr(co), 0x0f)
        orc.orc_cell_forces(ot.ptr, O.dptr(p), O.dptr(v), O.dptr(fo), None, 0x0f)
        for j in range(5):
            assert np.array_equal(comp[j, c], co[j]), (j, np.abs(comp[j, c] - co[j]).max())
        fi = _inner_links(ot.inner, ot.inner_len_eq, p, k)
        assert np.array_equal(comp[5, c], fi), np.abs(comp[5, c] - fi).max()
        if state == "rest":
            assert np.abs(fi).max() <= 1e-12 * abs(k)
        else:
            assert np.abs(fi).max() > 0
        if eta_m:
            assert np.abs(comp[4, c]).max() > 0
        fu = _inner_links(ot.inner, ot.inner_len_eq, p, k, fo)
        assert np.abs(fg[c] - fu).max() <= 1e-14 * np.abs(fu).max()
    cells.destroy(); L.destroy(); T.destroy()


@pytest.mark.parametrize("stl", list(STLS))
def test_rbc_high_order_on_stl_vs_oracle(orc, gpu, stl):
    """examples/cell_shapes' RBC_FROM_STL: RbcHighOrderModel on an STL mesh, every component bit-identical to the oracle"""
    P = gpu.base_parameters()
    m = gpu.read_material(XML)
    T = gpu.CellType.rbc(P, stl=STLS[stl], radius=m["radius"], kLink=m["kLink"], kArea=m["kArea"], kVolume=m["kVolume"],
                         kBend=m["kBend"], eta_m=5e-10)
    assert T.nv == COUNTS[stl][0] and T.malaria_constants() == dict(k_inner_link=0.0)
    ot = _OracleType(T)
    L, cells, t, pos, vel = _place_two(gpu, P, T, 3, "perturbed")
    cells.applyConstitutiveModel(0, True)
    fg = cells.forces.reshape(2, T.nv, 3)
    comp = cells.force_components(t).reshape(6, 2, T.nv, 3)
    for c in range(2):
        p, v = np.ascontiguousarray(pos[c]), np.ascontiguousarray(vel[c])
        co, fo = np.zeros((6, T.nv, 3)), np.zeros((T.nv, 3))
        orc.orc_cell_forces(ot.ptr, O.dptr(p), O.dptr(v), O.dptr(np.zeros((T.nv, 3))), O.dptr(co), 0x0f)
        orc.orc_cell_forces(ot.ptr, O.dptr(p), O.dptr(v), O.dptr(fo), None, 0x0f)
        for j in range(6):
            assert np.array_equal(comp[j, c], co[j]), (j, np.abs(comp[j, c] - co[j]).max())
        assert np.abs(fg[c] - fo).max() <= 1e-14 * np.abs(fo).max()
    cells.destroy(); L.destroy(); T.destroy()


@pytest.mark.parametrize("kind", ["rbc", "plt", "wbc"])
def test_old_pairs_through_create_ex(gpu, kind):
    """hcp_celltype_create_ex on RBC_HO / PLT_SIMPLE / WBC_HO with their own shapes: the tables and forces of the old
    entry points"""
    P = gpu.base_parameters()
    make = getattr(gpu.CellType, kind)
    Ta, Tb = make(P), make(P, ex=True)
    ta, tb = Ta.tables(), Tb.tables()
    for name in ("vertices", "triangles", "edges", "edge_length_eq", "edge_angle_eq", "triangle_area_eq", "vertex_vertexes",
                 "patch_dist_eq", "scalars"):
        assert np.array_equal(ta[name], tb[name]), name
    if kind == "wbc":
        assert Ta.wbc_constants() == Tb.wbc_constants()
    out = []
    for T in (Ta, Tb):
        L, cells, t, pos, vel = _place_two(gpu, P, T, 7, "perturbed")
        cells.applyConstitutiveModel(0, True)
        out.append((cells.forces.copy(), cells.force_components(t).copy()))
        cells.destroy(); L.destroy()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    Ta.destroy(); Tb.destroy()


def test_malaria_and_rbc_coupled_without_inner_links_match_the_oracle(orc, gpu):
    """with kInnerLink = 0 and eta_m = 0 the malaria model is RBC_HO on its STL mesh (the oracle has no linear inner-link
    law): one gametocyte and one RBC in a bounce-back pipe, 200 iterations at stepMaterialEvery 4, stepParticleEvery 2,
    against orc_sim_iterate with an RBC_HO type built from the malaria tables"""
    nx, ny, nz = 80, 34, 34
    k_m, k_p = 4, 2
    mask, _ = gpu.pipe_mask(nx, ny, nz)
    Po, Pg = O.make_params(orc), gpu.base_parameters()
    Lo = O.OracleLattice(orc, nx, ny, nz, (1, 0, 0), 1.0 / Po.tau)
    Lg = gpu.Lattice(nx, ny, nz, (1, 0, 0), 1.0 / Pg.tau)
    Lo.set_mask(mask); Lg.defineBounceBack(mask)
    Lo.init_equilibrium(); Lg.latticeEquilibrium()
    Tm = gpu.CellType.malaria(Pg, kInnerLink=0.0)
    assert Tm.malaria_constants()["k_inner_link"] == 0.0
    om = _OracleType(Tm, timescale=k_m)
    To = O.make_rbc(orc, Po); To.contents.timescale = k_m
    So = orc.orc_sim_create(Lo.ptr, C.byref(Po))
    orc.orc_sim_add_type(So, om.ptr); orc.orc_sim_add_type(So, To)
    hg = gpu.HemoCell(Lg, Pg)
    hg.cellfields.addCellType(Tm, k_m); hg.cellfields.addCellType(gpu.CellType.rbc(Pg), k_m)
    So.contents.particle_velocity_timescale = k_p
    hg.setParticleVelocityUpdateTimeScaleSeparation(k_p)
    for t, c, a in ((0, (22.0, 16.5, 16.5), (0.0, 0.0, 0.0)), (1, (58.0, 16.5, 16.5), (90.0, 0.0, 0.0))):
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
    assert pg[:Tm.nv, 0].mean() > 22.0 + 1e-3   # it moved
    fluid = mask.reshape(-1) == 0
    fo, fg = Lo.f[fluid], Lg.populations()[fluid]
    assert np.abs(fg - fo).max() <= 1e-6 * np.abs(fo).max()
    orc.orc_sim_destroy(So); Lo.destroy(); Lg.destroy()


# ----------------------------------------------------------------------------------------------- slabs
NXG, NY, NZ, STEPS = 112, 34, 34, 200
CELLS = [((55.0, 16.5, 16.5), (0, 0, 0)), ((14.0, 17.0, 16.0), (20, 10, 0))]     # the first one across the face at x = 56


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
    r.add_cell_type(host.CellType.malaria(P, eta_m=5e-10))
    r.load_cells(0, [np.array(c) for c, _ in CELLS], [np.array(a) for _, a in CELLS])
    assert tuple(r.sync_placement()) == (len(CELLS),)
    r.prepare()
    return r, mask


def _slab_worker(rank, world, port, out, q):
    try:
        sys.path.insert(0, ROOT)
        from hemocell_amd import slab
        slab.comm_init(rank, world, local_rank=0, port=port, transport="tcp")
        r, _ = _slab_build(rank, world)
        r.run(STEPS)
        cid, vid, pos = r.owned_vertex_table(0)
        np.savez(os.path.join(out, "w%d.npz" % rank), f=r.populations(), cid=cid, vid=vid, pos=pos)
        slab.barrier()
        slab.comm_finalize()
        q.put((rank, "ok"))
    except BaseException as e:   # noqa: BLE001 -- reported by the parent
        import traceback
        q.put((rank, "FAILED: %r\n%s" % (e, traceback.format_exc())))


def test_malaria_slabs_equal_single_domain_bit_for_bit(tmp_path, gpu):
    """2 host-staged ranks on one GPU with a gametocyte (wide tables, inner links) across the face, reproducible spread:
    populations and vertex positions are the bits of the single domain"""
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 32000 + (os.getpid() * 7 + 1291) % 20000
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
        p_ref = ref.cells.positions.reshape(len(CELLS), -1, 3)
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
def test_stretch_malaria_driver(tmp_path, gpu):
    """examples/malaria/stretch_malaria.cpp on tests/golden/malaria_case: the cell read from the STL file named by
    <StlFile> relative to the working directory, the malaria statistics logged, the volume kept within 2 % and the axial
    diameter grown under the pull"""
    from hemocell_amd import capi
    exe = str(tmp_path / "stretch_malaria")
    libdir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wno-deprecated-declarations", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "hemocell_amd", "compat"), os.path.join(ROOT, "examples", "malaria", "stretch_malaria.cpp"),
                           "-o", exe, "-L" + libdir, "-lhemocell_amd", "-Wl,-rpath," + libdir])
    work = tmp_path / "case"
    shutil.copytree(CASE, str(work))
    for f in os.listdir(str(work)):
        os.chmod(str(work / f), 0o644)
    cfg = open(str(work / "config.xml")).read()
    cfg = re.sub(r"<tmax>[^<]*</tmax>", "<tmax> 4000 </tmax>", cfg)
    open(str(work / "config.xml"), "w").write(cfg)
    r = subprocess.run([exe, "config.xml"], cwd=str(work), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    out = r.stdout
    assert "(Cell-mechanics model) Malaria model parameters for RBC_MALARIA cellfield" in out
    assert "\t k_inner_link:   " in out
    assert "Nvertex: 1507" in out
    assert out.rstrip().splitlines()[-1] == "(MalariaStretch) Simulation finished :)"
    log = np.loadtxt(str(work / "stretch.log"))
    assert log.shape == (5, 7) and log[0, 0] == 0 and log[-1, 0] == 4000
    assert np.abs(log[:, 4] - 100.0).max() < 2.0, log[:, 4]
    assert log[-1, 1] > log[0, 1] + 0.1, log[:, 1]
