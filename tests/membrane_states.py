"""Deformed states for the membrane-force tests -- test infrastructure only, pure numpy, shared by the CPU and the GPU tests.

build(tab, model, rest) makes, from the rest positions of two cells of a type (rest [2][nv][3]; rest_pair() places and
rotates them for the CPU tests, the GPU tests take what addCell placed), one state per regime of the laws of
tests/membrane_ref.py, named for what it reaches:

  moderate        rest + 0.05 standard_normal: the noise state of the older force tests, the anchor
  large_strain    an anisotropic stretch with a shear (the largest of 1.3 x 0.88 x 0.88 with shear 0.15, and two smaller
                  ones, that keeps every law on the near side of its pole: the area pole at 0.3 is what bounds it), of the
                  rest shape with noise of 1 % of the shortest edge at each vertex
  volume_plus/minus   cell 0 scaled until its volume fraction is beyond +-0.1, cell 1 left on the near side (one cell has
                  one volume fraction: "both sides" are the two cells)
  area_plus/minus     a few triangles per cell scaled about their centroids until their area ratio is beyond +-0.3
  bending_plus/minus  a few vertices per cell moved along their ring normal until dDev is beyond +-sqrt(0.0555) (not PLT)
  link_plus       a few vertices per cell pulled out until every edge at them is more than four times its rest length
                  (ef > 3; there is no link_minus: ef = l / l0 - 1 > -1 can not reach -3)
  dihedral_plus/minus, fold   PLT: the outer vertex of a few edges turned about the edge, until the angle deviation is
                  beyond +-sqrt(2.467), and until the atan2 has been taken in all four quadrants and within 1e-3 of +-pi
  visc_cap        velocities scaled until about half of the edges have their viscous force limited
  wbc_radius, wbc_core   WBC: four diameters per cell pulled to 2 radius (1 -+ 1e-2), (1 -+ 1e-5); both cells scaled until
                  2 core_radius lies between their middle inner-edge lengths; in each, one inner edge of cell 0 laid along
                  x with both ends on one coordinate line, exactly the threshold apart

The pole states start from the rest shape with noise of 2.5 % of the shortest edge at each vertex, made 1.2 % larger
(volume fraction +0.036), so that no element and no cell sits at x = 0, where the forces vanish and a bound relative to
their magnitude means nothing, and so that only the elements meant to cross a pole do.

Every state is then settled: while an element of any law lies within MARGIN_BUILD of a pole (|c - x^2| < 0.06 c), one
vertex of it that the state did not place on purpose is moved by a small random step; while a cell's volume fraction is
in the margin of its pole or within 0.012 of zero, the cell grows by 0.4 %.  (The volume force is one scalar per cell, made of a
signed-volume sum whose terms, taken where the cell lies in the lattice, are ~1e4 times the volume: at vf = 0 nothing but
the rounding of that sum is left of it.  The noise state of the older tests has vf = 0.001.)  check() asserts, from the
restatement's intermediate scalars alone, the condition |c - x^2| >= 0.05 c for every element of every law, |vf| >= 0.01,
that no edge, triangle or ring normal is degenerate, and what the state's name claims.
"""
import numpy as np

from tests import membrane_ref as M

MARGIN, MARGIN_BUILD = 0.05, 0.06
MIN_VF = 0.01   # a cell's volume fraction stays this far from zero
CENTRES = ((16.3, 24.1, 23.7), (45.0, 22.4, 25.2))


def tables_from_oracle(T, **extra):
    """T: POINTER(orc_celltype) of oracle/oracle.py"""
    t = T.contents
    tab = {k: t.arr(k) for k in ("triangles", "edges", "edge_length_eq", "edge_angle_eq", "edge_bending_triangles", "edge_bending_outer",
                                 "triangle_area_eq", "vertex_vertexes", "vertex_n_vertexes", "patch_dist_eq", "vertices")}
    tab["inner_edges"] = t.arr("inner_edges").astype(np.int64).reshape(-1, 2)[:t.nie]
    tab["inner_edge_length_eq"] = t.arr("inner_edge_length_eq")[:t.nie]
    for k in ("volume_eq", "area_mean_eq", "edge_mean_eq", "k_volume", "k_area", "k_link", "k_bend", "eta_m"):
        tab[k] = float(getattr(t, k))
    tab.update(extra)
    return tab


def rest_pair(vertices):
    """two cells at CENTRES, the second one turned so that nothing in it is parallel to an axis"""
    a, b, c = 0.61, -0.23, 1.17
    rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    v = vertices - vertices.mean(0)
    return np.stack([v + np.array(CENTRES[0]), v @ (rz @ ry @ rx).T + np.array(CENTRES[1])])


class State:
    def __init__(self, name, pos, vel, **claim):
        self.name, self.pos, self.vel, self.claim = name, np.ascontiguousarray(pos), np.ascontiguousarray(vel), claim


def evaluate(tab, model, st, wrong=None):
    return [M.forces(tab, st.pos[c], st.vel[c], model, wrong=wrong) for c in range(len(st.pos))]


def _law_values(info, model):
    """law -> (x per element, c)"""
    out = dict(volume=(np.atleast_1d(info["vf"]), M.MAX_VOLUME), area=(info["area_ratio"], M.MAX_AREA), link=(info["ef"], M.MAX_LINK))
    if model == "plt":
        out["dihedral"] = (info["af"], M.MAX_PLT_BENDING)
    else:
        out["bending"] = (info["dDev"], M.MAX_BENDING)
    return out


def _near_pole(info, model, margin):
    """law -> indices of the elements with |c - x^2| < margin c"""
    return {law: np.nonzero(np.abs(c - x * x) < margin * c)[0] for law, (x, c) in _law_values(info, model).items()}


def _adjacency(tab, nv):
    adj = [set() for _ in range(nv)]
    for a, b in np.asarray(tab["edges"]):
        adj[a].add(int(b)); adj[b].add(int(a))
    return adj


def _grow(adj, verts, depth):
    s = set(int(v) for v in verts)
    for _ in range(depth):
        s |= set(w for v in s for w in adj[v])
    return s


def _sites(adj, candidates, count, depth=2):
    """the first `count` candidates (vertex tuples) whose neighbourhoods of `depth` rings do not meet"""
    used, out = set(), []
    for k, verts in candidates:
        g = _grow(adj, verts, depth)
        if not (g & used):
            out.append(k); used |= g
            if len(out) == count:
                break
    assert len(out) == count, "mesh too small for %d separate sites" % count
    return out


def _local_size(tab, nv):
    """per vertex the rest length of the shortest edge at it"""
    local = np.full(nv, np.inf)
    for k in range(2):
        np.minimum.at(local, np.asarray(tab["edges"])[:, k], np.asarray(tab["edge_length_eq"]))
    return local


def _settle(tab, model, pos, vel, rng, protect):
    """move unprotected vertices of elements that lie within MARGIN_BUILD of a pole until none does"""
    local = _local_size(tab, pos.shape[1])
    tri, edge = np.asarray(tab["triangles"]), np.asarray(tab["edges"])
    ring, ebo = np.asarray(tab["vertex_vertexes"]), np.asarray(tab["edge_bending_outer"])
    for c in range(len(pos)):
        free = np.array([i not in protect[c] for i in range(pos.shape[1])])
        for _ in range(60):
            info = M.forces(tab, pos[c], vel[c], model)["info"]
            near = _near_pole(info, model, MARGIN_BUILD)
            if abs(info["vf"]) < 1.2 * MIN_VF:
                near["volume"] = [0]
            if not any(len(v) for v in near.values()):
                break
            move = set()
            for law, cand in (("area", lambda t: tri[t]), ("link", lambda e: edge[e]), ("dihedral", lambda e: list(ebo[e]) + list(edge[e])),
                              ("bending", lambda i: [i] + [r for r in ring[i] if r >= 0])):
                for k in near.get(law, ()):
                    ok = [int(i) for i in cand(k) if free[i]]
                    assert ok, "an element placed on purpose lies in the margin of the %s pole" % law
                    move.add(ok[0])
            if len(near["volume"]):
                cen = pos[c].mean(0)
                pos[c][free] = cen + 1.004 * (pos[c][free] - cen)
            for i in sorted(move):
                pos[c][i] += 0.03 * local[i] * rng.standard_normal(3)
        else:
            raise AssertionError("state does not settle away from the poles")
    return pos


def _unit(v):
    return v / np.sqrt((v * v).sum(-1))[..., None]


def _ring_normal(tab, p, i):
    r = [k for k in np.asarray(tab["vertex_vertexes"])[i] if k >= 0]
    a = p[r] - p[i]
    return _unit(_unit(np.cross(a, np.roll(a, -1, axis=0))).sum(0))


def _turn(q, p0, u, theta):
    """q turned about the axis through p0 along the unit vector u"""
    w = q - p0
    return p0 + w * np.cos(theta) + np.cross(u, w) * np.sin(theta) + u * (u @ w) * (1 - np.cos(theta))


def _set_dihedral(tab, pos, vel, e, target, of):
    """turn the first outer vertex of edge e of a PLT cell about the edge until info[of][e] == target"""
    edge, ebo = np.asarray(tab["edges"]), np.asarray(tab["edge_bending_outer"])
    now = M.forces(tab, pos, vel, "plt")["info"][of][e]
    p0, u, q = pos[edge[e, 0]], _unit(pos[edge[e, 1]] - pos[edge[e, 0]]), pos[ebo[e, 0]].copy()
    for sign in (1.0, -1.0):
        pos[ebo[e, 0]] = _turn(q, p0, u, sign * (target - now))
        if abs(M.forces(tab, pos, vel, "plt")["info"][of][e] - target) < 1e-9:
            return
    raise AssertionError("the dihedral of edge %d does not follow the turn" % e)


def _exact_offset(d, near):
    """c, a multiple of 1/4 close to `near`, with (c + d) - c == d in double and c + d exact"""
    for k in sorted(range(1, 4 * 60), key=lambda k: abs(k / 4.0 - near)):
        c = k / 4.0
        if (c + d) - c == d and M.hp(c) + M.hp(d) == M.hp(c + d):
            return c
    raise AssertionError("no exact offset for d = %r" % d)


def build(tab, model, rest, seed=11):
    """-> dict name -> State (positions and velocities [2][nv][3])"""
    rng = np.random.default_rng(seed)
    rest = np.asarray(rest, dtype=np.float64)
    nc, nv, _ = rest.shape
    assert nc == 2
    tri, edge = np.asarray(tab["triangles"]), np.asarray(tab["edges"])
    adj = _adjacency(tab, nv)
    vel = 1e-3 * rng.standard_normal(rest.shape)
    local = _local_size(tab, nv)
    cen = rest.mean(1, keepdims=True)
    base = cen + 1.012 * (rest + 0.025 * local[None, :, None] * rng.standard_normal(rest.shape) - cen)
    none = [set(), set()]
    out = {}

    def done(name, pos, v=vel, protect=none, **claim):
        out[name] = State(name, _settle(tab, model, pos, v, rng, protect), v, **claim)

    done("moderate", rest + 0.05 * rng.standard_normal(rest.shape))

    calm = rest + 0.01 * local[None, :, None] * rng.standard_normal(rest.shape)
    for a, b, g in ((1.3, 0.88, 0.15), (1.25, 0.9, 0.12), (1.2, 0.92, 0.1)):
        F = np.array([[a, g, 0.0], [0.0, b, 0.0], [0.0, 0.0, b]])
        pos = cen + (calm - cen) @ F.T
        infos = [M.forces(tab, pos[c], vel[c], model)["info"] for c in range(2)]
        if all((np.abs(x) < np.sqrt(c_) * (1 - MARGIN_BUILD)).all() for i in infos for x, c_ in _law_values(i, model).values()):
            done("large_strain", pos, stretch=(a, b, g))
            break
    else:
        raise AssertionError("no large strain keeps every law on the near side of its pole")

    for name, target in (("volume_plus", 0.16), ("volume_minus", -0.16)):
        pos = base.copy()
        vf0 = float(M.forces(tab, pos[0], vel[0], model)["info"]["vf"])
        pos[0] = cen[0] + ((1 + target) / (1 + vf0)) ** (1.0 / 3.0) * (pos[0] - cen[0])
        done(name, pos, law="volume", sign=np.sign(target))

    n_sites = 2 if nv < 200 else 3
    tri_sites = _sites(adj, [(t, tri[t]) for t in rng.permutation(len(tri))], n_sites)
    for name, target in (("area_plus", 0.45), ("area_minus", -0.45)):
        pos, protect = base.copy(), [set(), set()]
        for c in range(2):
            x0 = M.forces(tab, pos[c], vel[c], model)["info"]["area_ratio"]
            for t in tri_sites:
                m = pos[c][tri[t]].mean(0)
                pos[c][tri[t]] = m + np.sqrt((1 + target) / (1 + x0[t])) * (pos[c][tri[t]] - m)
                protect[c] |= set(int(i) for i in tri[t])
        done(name, pos, protect=protect, law="area", sign=np.sign(target), elements=tri_sites)

    vert_sites = _sites(adj, [(i, [i]) for i in rng.permutation(nv)], n_sites)
    if model != "plt":
        for name, target in (("bending_plus", 0.35), ("bending_minus", -0.35)):
            pos, protect = base.copy(), [set(), set()]
            for c in range(2):
                for _ in range(6):     # dDev falls by delta / edge_mean_eq when the vertex moves by delta along its ring normal
                    d = M.forces(tab, pos[c], vel[c], model)["info"]["dDev"]
                    for i in vert_sites:
                        pos[c][i] += (d[i] - target) * tab["edge_mean_eq"] * _ring_normal(tab, pos[c], i)
                protect[c] |= set(int(i) for i in vert_sites)   # a settling step of a ring vertex moves dDev by less than 0.01
            done(name, pos, protect=protect, law="bending", sign=np.sign(target), elements=vert_sites)

    pos, protect = base.copy(), [set(), set()]
    for c in range(2):
        for i in vert_sites:
            nrm = _ring_normal(tab, pos[c], i) if model != "plt" else _unit(pos[c][i] - pos[c].mean(0))
            mine = np.nonzero((edge == i).any(1))[0]
            for _ in range(8):         # until the shortest edge at the vertex has ef = 3.3
                ef = np.sqrt(((pos[c][edge[mine, 1]] - pos[c][edge[mine, 0]]) ** 2).sum(1)) / tab["edge_length_eq"][mine] - 1
                pos[c][i] += nrm * (3.3 - ef.min()) * tab["edge_length_eq"][mine].mean()
            protect[c] |= {int(i)}
    done("link_plus", pos, protect=protect, law="link", sign=1.0, elements=vert_sites)

    if model == "plt":
        ebo = np.asarray(tab["edge_bending_outer"])
        edge_sites = _sites(adj, [(e, list(edge[e]) + list(ebo[e])) for e in rng.permutation(len(edge))], 2, depth=1)
        for name, target in (("dihedral_plus", 1.9), ("dihedral_minus", -1.9)):
            pos, protect = base.copy(), [set(), set()]
            for c in range(2):
                for e in edge_sites:
                    _set_dihedral(tab, pos[c], vel[c], e, target, "af")
                    protect[c] |= set(int(i) for i in list(edge[e]) + list(ebo[e]))
            done(name, pos, protect=protect, law="dihedral", sign=np.sign(target), elements=edge_sites)
        pos, protect = base.copy(), [set(), set()]
        for c, targets in enumerate(((2.4, -np.pi + 5e-4), (-2.4, np.pi - 5e-4))):
            for e, target in zip(edge_sites, targets):
                _set_dihedral(tab, pos[c], vel[c], e, target, "angle")
                protect[c] |= set(int(i) for i in list(edge[e]) + list(ebo[e]))
        done("fold", pos, protect=protect, elements=edge_sites)

    if tab["eta_m"] != 0.0:
        pos = out["moderate"].pos
        unit_vel = rng.standard_normal(rest.shape)
        mag = np.concatenate([M.forces(tab, pos[c], unit_vel[c], model, wrong="no_visc_cap")["info"]["visc_mag"] for c in range(2)])
        out["visc_cap"] = State("visc_cap", pos, unit_vel * (M.VISC_CAP / np.median(mag)))

    if model == "wbc":
        ie = np.asarray(tab["inner_edges"])
        for name, d in (("wbc_radius", 2 * tab["radius"]), ("wbc_core", 2 * tab["core_radius"])):
            pos, protect = base.copy(), [set(), set()]
            dv = pos[0][ie[:, 1]] - pos[0][ie[:, 0]]
            e = int(np.argmax(np.abs(dv[:, 0]) / np.sqrt((dv * dv).sum(1))))       # the diameter of cell 0 closest to the x axis
            if name == "wbc_core":     # the cell scaled until 2 core_radius lies between its two middle inner-edge lengths
                for c in range(2):
                    l = np.sort(np.sqrt(((pos[c][ie[:, 1]] - pos[c][ie[:, 0]]) ** 2).sum(1)))
                    pos[c] = cen[c] + d / (0.5 * (l[len(l) // 2 - 1] + l[len(l) // 2])) * (pos[c] - cen[c])
            else:                      # the rest length is 2 radius + 2e-3: a few diameters pulled to just below and just above
                pairs = _sites(adj, [(e, ie[e])] + [(k, ie[k]) for k in rng.permutation(len(ie))], 5, depth=1)[1:]
                for c in range(2):
                    for k, rel in zip(pairs, (-1e-2, -1e-5, 1e-5, 1e-2)):
                        a, b = pos[c][ie[k, 0]].copy(), pos[c][ie[k, 1]].copy()
                        m, h = 0.5 * (a + b), 0.5 * (b - a)
                        h *= d * (1 + rel) / (2 * np.sqrt((h * h).sum()))
                        pos[c][ie[k, 0]], pos[c][ie[k, 1]] = m - h, m + h
                        protect[c] |= {int(ie[k, 0]), int(ie[k, 1])}
            dv = pos[0][ie[:, 1]] - pos[0][ie[:, 0]]
            lo, hi = (ie[e, 0], ie[e, 1]) if dv[e, 0] > 0 else (ie[e, 1], ie[e, 0])
            c0 = _exact_offset(d, pos[0][lo, 0])
            pos[0] += np.array([c0 - pos[0][lo, 0], 0.0, 0.0])
            y, z = 0.5 * (pos[0][lo, 1:] + pos[0][hi, 1:])
            pos[0][lo], pos[0][hi] = (c0, y, z), (c0 + d, y, z)
            protect[0] |= {int(lo), int(hi)}
            done(name, pos, protect=protect, threshold=d, which=name[4:], exact_edge=e)
    return out


def check(tab, model, st):
    """assert, from the restatement alone, the margin to every pole, that nothing is degenerate and what the state's name
    claims; -> the restatement's results per cell (the tests compare against them)"""
    res = evaluate(tab, model, st)
    infos = [r["info"] for r in res]
    for c, info in enumerate(infos):
        for law, idx in _near_pole(info, model, MARGIN).items():
            assert len(idx) == 0, (st.name, c, law, idx[:5])
        assert abs(info["vf"]) >= MIN_VF, (st.name, c, info["vf"])
        assert info["el"].min() > 1e-3 * tab["edge_mean_eq"] and info["area"].min() > 1e-4 * tab["area_mean_eq"], st.name
        assert model == "plt" or info["ring_normal_min"] > 1e-3, st.name
        assert np.isfinite(res[c]["force"]).all()
    name, claim = st.name, st.claim

    def beyond(info, law):
        x, c = _law_values(info, model)[law]
        return claim["sign"] * x > np.sqrt(c)

    if name == "large_strain":
        for info in infos:
            for x, c in _law_values(info, model).values():
                assert (np.abs(x) < np.sqrt(c)).all()
        # the older tests' 1.15 x 0.93 x 0.93 has area ratios within 0.07 and edge strains within 0.15.  The area pole at
        # 0.3 bounds a stretch that keeps the volume: this one goes more than half of the way there
        assert min(np.abs(i["area_ratio"]).max() for i in infos) > 0.15 and min(np.abs(i["ef"]).max() for i in infos) > 0.2
    elif name.startswith("volume"):
        assert beyond(infos[0], "volume").all() and not beyond(infos[1], "volume").any()
    elif "law" in claim:
        for info in infos:       # both sides of the pole in the same cell, the elements placed there among those beyond it
            b = beyond(info, claim["law"])
            assert b.any() and not b.all()
            if claim["law"] == "link":
                assert all(b[(np.asarray(tab["edges"]) == i).any(1)].all() for i in claim["elements"])
            else:
                assert b[claim["elements"]].all()
    elif name == "fold":
        y, x, ang = (np.concatenate([i[k] for i in infos]) for k in ("atan_y", "atan_x", "angle"))
        for sy in (1, -1):
            for sx in (1, -1):
                assert ((sy * y > 0) & (sx * x > 0)).any(), (sy, sx)
        assert (np.abs(ang - np.pi) < 1e-3).any() and (np.abs(ang + np.pi) < 1e-3).any()
    elif name == "visc_cap":
        capped = np.concatenate([i["capped"] for i in infos])
        mag = np.concatenate([i["visc_mag"] for i in infos])
        assert 0.25 <= capped.mean() <= 0.75, capped.mean()
        assert np.abs(mag - M.VISC_CAP).min() > 1e-9
        assert (mag.max() > 2 * M.VISC_CAP)
    elif name.startswith("wbc_"):
        d, e, ie = claim["threshold"], claim["exact_edge"], np.asarray(tab["inner_edges"])
        dv = st.pos[0][ie[e, 1]] - st.pos[0][ie[e, 0]]
        assert abs(dv[0]) == d and dv[1] == 0.0 and dv[2] == 0.0 and np.sqrt(dv[0] * dv[0] + dv[1] * dv[1] + dv[2] * dv[2]) == d
        assert infos[0]["inner_el"][e] == d and not infos[0]["fired_" + claim["which"]][e]      # the law does not fire at el == d
        for c, info in enumerate(infos):
            el, fired = info["inner_el"], info["fired_" + claim["which"]]
            other = np.ones(len(el), bool)
            if c == 0:
                other[e] = False
            just = other & (np.abs(el - d) < 1e-4 * d)
            assert (fired & just).any() and (~fired & just).any()                  # just below and just above
            assert np.abs(el[other] - d).min() > 1e-9 and np.abs(el - d).max() < 0.05 * d
            assert np.array_equal(fired[other], el[other] < d)
    return res
