"""Restatement of the interior-viscosity passes and of the collide with a per-node omega, in numpy -- test infrastructure only.

What the reference does (INTERIOR_VISCOSITY builds; file:line in the HemoCell tree):

* findInternalParticleGridPoints (core/hemoCellParticleField.cpp:777-807, helper/octree.h:107-147): all tags are cleared;
  then, cell after cell, every integer node of the truncated bounding box of the cell's vertices, (int)min .. (int)max on
  every axis, is interior when the number of triangles hit by hemo::MollerTrumbore (helper/mollerTrumbore.h) is odd.  The ray
  starts at the node and runs along (-40, -40, -40); EPSILON = 1e-7, u and v bounds inclusive, t narrowed to float before
  t > EPSILON.  The octree only culls, so the result is the parity over all triangles.
* internalGridPointsMembrane (:746-773): particle after particle, every node of the particle's phi2 stencil (non-zero weight,
  not a boundary node) with d = node - position no longer than edge_mean_eq is tagged when d . n < 0 and cleared otherwise;
  n is the particle's normalDirection (mechanics/rbcHighOrderModel.cpp:115-121): starting from 0, for every triangle in list
  order, unit normal * (area / area_mean_eq) added to its three vertices.
* nodes inside relax with omega = 1 / tau_int, tau_int = viscosityRatio (tau - 0.5) + 0.5 (core/hemoCellField.cpp:100-112).

Here a node carries a class: 0 = the lattice's omega, k >= 1 = omegas[k - 1].  Cells and vertices are visited in ascending
(cell id, type, vertex) order and a later writer overrules an earlier one.  Positions are unwrapped; a node is brought onto
the lattice by wrapping periodic axes and dropped outside a non-periodic one, and only fluid nodes (mask == 0) are tagged.
Every operation is an IEEE double operation in the order of helper/array.h (dot: ret = 0; ret += a_i b_i), so the GPU (built
with -ffp-contract=off) must agree decision for decision.
"""
import numpy as np

import open_boundary_ref as OB

EPSILON = 0.0000001
RAY = (-40.0, -40.0, -40.0)


def _dot(a, b):
    r = 0.0
    for d in range(3):
        r = r + a[d] * b[d]
    return r


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def moller_trumbore(v0, v1, v2, origin):
    """hits [m][nt] (bool) of the rays from the integer nodes origin [m][3] with the triangles v0, v1, v2 [nt][3]"""
    o = [np.asarray(origin, dtype=np.float64)[:, d][:, None] for d in range(3)]
    a0 = [v0[:, d][None, :] for d in range(3)]
    e1 = [(v1[:, d] - v0[:, d])[None, :] for d in range(3)]
    e2 = [(v2[:, d] - v0[:, d])[None, :] for d in range(3)]
    p = _cross(RAY, e2)
    det = _dot(e1, p)
    ok = ~((det > -EPSILON) & (det < EPSILON))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv = 1 / det
        s = [o[d] - a0[d] for d in range(3)]
        u = inv * _dot(s, p)
        ok = ok & ~((u < 0.0) | (u > 1.0))
        q = _cross(s, e1)
        v = inv * _dot(RAY, q)
        ok = ok & ~((v < 0.0) | (u + v > 1.0))
        t = (inv * _dot(e2, q)).astype(np.float32).astype(np.float64)
    return ok & (t > EPSILON)


def box_nodes(pos):
    """the integer nodes [m][3] of the truncated bounding box of pos [nv][3] (octree.h:119-121), x outermost"""
    lo = [int(v) for v in pos.min(axis=0)]
    hi = [int(v) for v in pos.max(axis=0)]
    g = np.mgrid[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1]
    return g.reshape(3, -1).T.astype(np.int64)


def interior_nodes(pos, tri, chunk=512):
    """the unwrapped integer nodes inside the closed surface (pos [nv][3], tri [nt][3]): odd number of crossings"""
    nodes = box_nodes(pos)
    v0, v1, v2 = pos[tri[:, 0]], pos[tri[:, 1]], pos[tri[:, 2]]
    inside = np.zeros(len(nodes), bool)
    for a in range(0, len(nodes), chunk):
        hits = moller_trumbore(v0, v1, v2, nodes[a:a + chunk])
        inside[a:a + chunk] = hits.sum(axis=1) % 2 == 1
    return nodes[inside]


def wrap(nodes, dims, periodic):
    """nodes [m][3] unwrapped -> (kept [m] bool, wrapped [m][3]): periodic axes wrap, other axes drop what lies outside"""
    nodes = np.asarray(nodes, dtype=np.int64).reshape(-1, 3)
    w = nodes.copy()
    keep = np.ones(len(nodes), bool)
    for d in range(3):
        if periodic[d]:
            w[:, d] = np.mod(nodes[:, d], dims[d])
        else:
            keep &= (nodes[:, d] >= 0) & (nodes[:, d] < dims[d])
    return keep, w


def _ordered(cells):
    return sorted(cells, key=lambda c: (c["id"], c["type"]))


def find(cells, mask, periodic):
    """findInternalParticleGridPoints.  cells: dicts with id, type, pos [nv][3], tri [nt][3], klass; mask [nx][ny][nz].
    Returns the class field uint8 [nx][ny][nz]."""
    cls = np.zeros(mask.shape, np.uint8)
    for c in _ordered(cells):
        keep, w = wrap(interior_nodes(c["pos"], c["tri"]), mask.shape, periodic)
        w = w[keep]
        fluid = mask[w[:, 0], w[:, 1], w[:, 2]] == 0
        w = w[fluid]
        cls[w[:, 0], w[:, 1], w[:, 2]] = c["klass"]
    return cls


def normals(pos, tri, area_mean_eq):
    """normalDirection of every vertex [nv][3]: the reference's scatter loop over the triangle list"""
    v0 = pos[tri[:, 0]]
    e1, e2 = pos[tri[:, 1]] - v0, pos[tri[:, 2]] - v0
    c = np.stack(_cross([e1[:, d] for d in range(3)], [e2[:, d] for d in range(3)]), axis=1)
    nn = np.zeros(len(tri))
    for d in range(3):
        nn = nn + c[:, d] * c[:, d]
    nn = np.sqrt(nn)
    nz = nn != 0.0
    area = np.where(nz, 0.5 * nn, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        unit = np.where(nz[:, None], c / nn[:, None], 0.0)
    local = unit * (area / area_mean_eq)[:, None]
    n = np.zeros_like(pos)
    for t in range(len(tri)):
        for k in range(3):
            n[tri[t, k]] = n[tri[t, k]] + local[t]
    return n


def _phi2(x):
    x = 1.0 - abs(x)
    return x if x > 0.0 else 0.0


def stencil_nodes(p, mask, periodic):
    """the admitted nodes of the phi2 stencil of the position p, in stencil order: [(unwrapped node, wrapped node)]"""
    c = [int(np.floor(v + 0.5)) for v in p]
    d0 = [-1 if p[a] < float(c[a]) else 0 for a in range(3)]
    out = []
    for i in range(2):
        for j in range(2):
            for k in range(2):
                g = (c[0] + d0[0] + i, c[1] + d0[1] + j, c[2] + d0[2] + k)
                keep, w = wrap([g], mask.shape, periodic)
                if not keep[0]:
                    continue
                if _phi2(p[0] - float(g[0])) * _phi2(p[1] - float(g[1])) * _phi2(p[2] - float(g[2])) == 0.0:
                    continue
                w = tuple(int(v) for v in w[0])
                if mask[w] != 0:
                    continue
                out.append((g, w))
    return out


def membrane(cls, cells, mask, periodic, log=None):
    """internalGridPointsMembrane on the class field cls (changed in place and returned).  cells as for find(), plus
    area_mean_eq and edge_mean_eq; an optional normal [nv][3] overrides the one formed from pos.  log: a list that
    receives (wrapped node, cell id, vertex, verdict) for every decision, in order."""
    for c in _ordered(cells):
        pos = c["pos"]
        n = c["normal"] if c.get("normal") is not None else normals(pos, c["tri"], c["area_mean_eq"])
        for i in range(len(pos)):
            p = [float(v) for v in pos[i]]
            for g, w in stencil_nodes(p, mask, periodic):
                d = [float(g[a]) - p[a] for a in range(3)]
                if np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) > c["edge_mean_eq"]:
                    continue
                inside = _dot(d, [float(v) for v in n[i]]) < 0.0
                cls[w] = c["klass"] if inside else 0
                if log is not None:
                    log.append((w, c["id"], i, bool(inside)))
    return cls


def tau_interior(ratio, tau):
    """core/hemoCellField.cpp:100"""
    return ratio * (tau - 0.5) + 0.5


def step(S, mask, periodic, omega, omegas, cls, body, **kw):
    """one collide-stream with the omega of every node's class: open_boundary_ref.step with an array over the fluid nodes"""
    table = np.r_[float(omega), np.asarray(omegas, dtype=np.float64)]
    per_node = table[np.asarray(cls).reshape(-1)][mask.reshape(-1) == 0]
    return OB.step(S, mask, periodic, per_node, body, **kw)
