"""Restatement of the membrane forces in extended precision -- test infrastructure only.

ParticleMechanics of the four models, written from the reference's model files (mechanics/rbcHighOrderModel.cpp:38-207,
pltSimpleModel.cpp:44-208, wbcHighOrderModel.cpp:42-225, rbcMalariaModel.cpp:40-218), its helpers (helper/array.h:270-304,
helper/geometryUtils.h:49-52) and config/constant_defaults.h, as whole-array numpy: one pass per law over all triangles, all
vertices of one ring size, all edges.  Nothing here follows the order or the form of the kernel or of the C oracle.

forces(tab, pos, vel, model) takes the tables of a cell type (TABLE_KEYS: what CellType.tables() / hcp_celltype_tables2 give
and what the oracle's orc_celltype holds, plus the WBC / malaria constants), positions and velocities [nv][3] of ONE cell,
and returns comp [6][nv][3] (volume, area, bending, link, viscosity, inner link), force (their sum), comp_abs / force_abs
(per vertex component the sum of the magnitudes of the terms that were added into it) and info: the intermediate scalars
of every law (volume fraction, area ratios, dDev, edge fractions, dihedral angles and their atan2 arguments, viscous
magnitudes and which were capped, inner-edge lengths and which thresholds fired) that the state checkers of
tests/membrane_states.py assert from.

Every value is computed in the extended type tests/observables_ref.py selects (np.longdouble with a 64-bit significand, or
mpmath at 113 bits) from the double inputs and the double constants of the reference, and rounded to double at the end.

wrong=<name> (WRONG) gives a restatement with one transcription slip: the mutation controls of the tests.
"""
import numpy as np

from tests.observables_ref import HP, hp, to_double, _sqrt

MODELS = ("rbc", "plt", "wbc", "malaria")
COMPONENTS = ("volume", "area", "bending", "link", "viscosity", "inner_link")
TABLE_KEYS = ("triangles", "edges", "edge_length_eq", "edge_angle_eq", "edge_bending_triangles", "edge_bending_outer",
              "triangle_area_eq", "vertex_vertexes", "vertex_n_vertexes", "patch_dist_eq", "inner_edges", "inner_edge_length_eq",
              "volume_eq", "area_mean_eq", "edge_mean_eq", "k_volume", "k_area", "k_link", "k_bend", "eta_m")
# config/constant_defaults.h:73-74, 157-173: c of every law x + x / fabs(c - x*x), and the limit of the viscous force
MAX_VOLUME, MAX_AREA, MAX_BENDING, MAX_PLT_BENDING, MAX_LINK = 0.01, 0.09, 0.0555, 2.467, 9.0
POLES = dict(volume=MAX_VOLUME, area=MAX_AREA, bending=MAX_BENDING, link=MAX_LINK, dihedral=MAX_PLT_BENDING)
VISC_CAP = 50.0 / 4.0

WRONG = ("no_fabs_volume", "no_fabs_area", "no_fabs_bending", "no_fabs_link", "no_fabs_dihedral",   # the fabs dropped from one law
         "no_visc_cap",              # the viscous force never limited
         "cap_per_component",        # each component limited to FORCE_LIMIT / 4 instead of the norm
         "wbc_le_radius", "wbc_le_core",   # <= for < at a WBC threshold
         "ring_share_over_6",        # a ring neighbour's share of the bending force divided by 6, not by the ring size
         "atan2_swapped",            # atan2(dot(n1, n2), dot(cross, edge))
         "plt_outer_plus",           # the outer points of the platelet bending given + instead of -
         "malaria_inner_k_link")     # the malaria inner link with the platelet's k_link instead of k_inner_link

if HP is np.longdouble:
    def _atan2(y, x):
        return np.arctan2(y, x)
else:
    import mpmath
    _matan2 = np.vectorize(mpmath.atan2, otypes=[object])

    def _atan2(y, x):
        return _matan2(y, x)


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _dot(a, b):
    return (a * b).sum(axis=-1)


def _norm(a):
    return _sqrt(_dot(a, a))


def _law(x, c, fabs=True):
    d = hp(c) - x * x
    return x + x / (np.abs(d) if fabs else d)


def _bool(a):
    return np.asarray(a).astype(bool)


def forces(tab, pos, vel, model, wrong=None):
    assert model in MODELS and (wrong is None or wrong in WRONG)
    pos = np.asarray(pos, dtype=np.float64)
    nv = pos.shape[0]
    p, v = hp(pos), hp(np.asarray(vel, dtype=np.float64))
    comp, cabs = np.zeros((6, nv, 3), dtype=HP), np.zeros((6, nv, 3), dtype=HP)
    info = {}

    def add(c, idx, vec):
        np.add.at(comp[c], idx, vec)
        np.add.at(cabs[c], idx, np.abs(vec))

    # ---- triangles: area force, then the volume force scaled with the face area
    tri = np.asarray(tab["triangles"], dtype=np.int64)
    v0, v1, v2 = p[tri[:, 0]], p[tri[:, 1]], p[tri[:, 2]]
    n = _cross(v1 - v0, v2 - v0)
    nn = _norm(n)
    area, unit = nn / 2, n / nn[:, None]
    aeq = hp(tab["triangle_area_eq"])
    ratio = (area - aeq) / aeq
    afm = hp(tab["k_area"]) * _law(ratio, MAX_AREA, wrong != "no_fabs_area")
    centroid = (v0 + v1 + v2) / 3
    for k, vk in enumerate((v0, v1, v2)):
        add(1, tri[:, k], afm[:, None] * (centroid - vk))
    six = (-v2[:, 0] * v1[:, 1] * v0[:, 2] + v1[:, 0] * v2[:, 1] * v0[:, 2] + v2[:, 0] * v0[:, 1] * v1[:, 2]
           - v0[:, 0] * v2[:, 1] * v1[:, 2] - v1[:, 0] * v0[:, 1] * v2[:, 2] + v0[:, 0] * v1[:, 1] * v2[:, 2])
    volume = six.sum() * hp(1.0 / 6.0)
    veq = hp(tab["volume_eq"])
    vf = (volume - veq) / veq
    dv = hp(MAX_VOLUME) - vf * vf
    volume_force = -hp(tab["k_volume"]) * vf / (np.abs(dv) if wrong != "no_fabs_volume" else dv)
    lvf = (volume_force * unit) * (area / hp(tab["area_mean_eq"]))[:, None]
    for k in range(3):
        add(0, tri[:, k], lvf)
    info.update(vf=to_double(vf), area_ratio=to_double(ratio), area=to_double(area))

    # ---- per-vertex bending of the high-order models: deviation from the ring's mean along the ring's normal
    if model != "plt":
        ring, nring = np.asarray(tab["vertex_vertexes"], dtype=np.int64), np.asarray(tab["vertex_n_vertexes"], dtype=np.int64)
        dDev, ring_min = np.zeros(nv), np.inf
        for m in np.unique(nring):
            idx = np.nonzero(nring == m)[0]
            R = ring[idx, :m]
            x, q = p[idx], p[R]                                  # [k][3], [k][m][3]
            dev = q.sum(axis=1) / int(m) - x
            a = q - x[:, None]
            tn = _cross(a, np.roll(a, -1, axis=1))               # (ring j, ring j+1), the last one with the first
            l = _norm(tn)
            pn = (tn / l[..., None]).sum(axis=1)
            L = _norm(pn)
            pn = pn / L[:, None]
            d = (_dot(pn, dev) - hp(tab["patch_dist_eq"])[idx]) / hp(tab["edge_mean_eq"])
            bf = (hp(tab["k_bend"]) * _law(d, MAX_BENDING, wrong != "no_fabs_bending"))[:, None] * pn
            add(2, idx, bf)
            share = -bf / (6 if wrong == "ring_share_over_6" else int(m))
            for j in range(m):
                add(2, R[:, j], share)
            dDev[idx] = to_double(d)
            ring_min = min(ring_min, float(to_double(l).min()), float(to_double(L).min()))
        info.update(dDev=dDev, ring_normal_min=ring_min)

    # ---- edges: link, membrane viscosity, and the platelet's dihedral bending
    edge = np.asarray(tab["edges"], dtype=np.int64)
    e0, e1 = edge[:, 0], edge[:, 1]
    ev = p[e1] - p[e0]
    el = _norm(ev)
    uv = ev / el[:, None]
    leq = hp(tab["edge_length_eq"])
    ef = (el - leq) / leq
    f = uv * (hp(tab["k_link"]) * _law(ef, MAX_LINK, wrong != "no_fabs_link"))[:, None]
    add(3, e0, f); add(3, e1, -f)
    info.update(ef=to_double(ef), el=to_double(el))
    eta = float(tab["eta_m"])
    cap = hp(VISC_CAP)
    info.update(visc_mag=np.zeros(len(edge)), capped=np.zeros(len(edge), bool))
    if model != "rbc" or eta != 0.0:         # only RbcHighOrderModel tests eta_m
        fv = hp(eta) * (_dot(v[e1] - v[e0], uv)[:, None] * uv)
        mag = _norm(fv)
        over = _bool(mag > cap)
        if wrong == "cap_per_component":
            fv = np.where(_bool(fv > cap), cap, np.where(_bool(fv < -cap), -cap, fv))
        elif wrong != "no_visc_cap" and over.any():
            s = np.ones(len(edge), dtype=HP)
            s[over] = cap / mag[over]
            fv = fv * s[:, None]
        add(4, e0, fv); add(4, e1, -fv)
        info.update(visc_mag=to_double(mag), capped=over)
    if model == "plt":
        ebt, ebo = np.asarray(tab["edge_bending_triangles"], dtype=np.int64), np.asarray(tab["edge_bending_outer"], dtype=np.int64)
        n1, n2 = unit[ebt[:, 0]], unit[ebt[:, 1]]
        y, x = _dot(_cross(n1, n2), uv), _dot(n1, n2)
        angle = _atan2(x, y) if wrong == "atan2_swapped" else _atan2(y, x)
        af = angle - hp(tab["edge_angle_eq"])
        bf = (hp(tab["k_bend"]) * _law(af, MAX_PLT_BENDING, wrong != "no_fabs_dihedral"))[:, None] * (n1 + n2) * hp(0.5)
        add(2, e0, bf); add(2, e1, bf)
        outer = bf if wrong == "plt_outer_plus" else -bf
        add(2, ebo[:, 0], outer); add(2, ebo[:, 1], outer)
        info.update(af=to_double(af), angle=to_double(angle), atan_y=to_double(y), atan_x=to_double(x))

    # ---- inner links
    ie = np.asarray(tab["inner_edges"], dtype=np.int64).reshape(-1, 2)
    if len(ie):
        i0, i1 = ie[:, 0], ie[:, 1]
        iv = p[i1] - p[i0]
        il = _norm(iv)
        iu = iv / il[:, None]
        info.update(inner_el=to_double(il))
        if model == "wbc":
            fired = []
            for name, d, kk in (("radius", 2 * hp(tab["radius"]), tab["k_cytoskeleton"]), ("core", 2 * hp(tab["core_radius"]), tab["k_inner_rigid"])):
                on = _bool(il <= d) if wrong == "wbc_le_" + name else _bool(il < d)
                fi = iu[on] * (1 - il[on] / d)[:, None] * hp(kk)
                add(5, i0[on], -fi); add(5, i1[on], fi)
                fired.append(on)
            info.update(fired_radius=fired[0], fired_core=fired[1])
        else:                                  # the platelet's linear law, the malaria model's with its own modulus
            k = tab["k_link"] if (model == "plt" or wrong == "malaria_inner_k_link") else tab["k_inner_link"]
            ileq = hp(tab["inner_edge_length_eq"])
            fi = iu * (hp(k) * 5 * ((il - ileq) / ileq))[:, None]
            add(5, i0, fi); add(5, i1, -fi)
    return dict(comp=to_double(comp), comp_abs=to_double(cabs), force=to_double(comp.sum(axis=0)),
                force_abs=to_double(cabs.sum(axis=0)), info=info)


def ratio(got, ref, ref_abs):
    """largest |got - ref| / (2^-53 ref_abs); where the bound is zero (every term zero) a difference gives inf"""
    got, ref, ref_abs = (np.asarray(a, dtype=np.float64) for a in (got, ref, ref_abs))
    err, tol = np.abs(got - ref), 2.0 ** -53 * ref_abs
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(r.max()) if r.size else 0.0
