"""Restatement of the solidify mechanics in numpy -- test infrastructure only.

What the reference does (SOLIDIFY_MECHANICS builds; file:line in the HemoCell tree):

* populateBindingSites (core/hemoCellParticleField.cpp:920-948): every boundary node of the box with a non-boundary node
  among its 26 neighbours becomes a binding site; calls add up.
* prepareSolidification -> PltSimpleModel::solidifyMechanics (mechanics/pltSimpleModel.cpp:211-252): every complete cell of
  an enabled type with a flagged vertex turns the inner nodes (helper/octree.h:107-147: the ray cast of
  interior_viscosity_ref.interior_nodes) that are not boundary nodes yet into bounce-back nodes and binding sites, and is
  removed.
* solidifyCells (core/hemoCellParticleField.cpp:1018-1065): for every binding site b, every node n of the 3 x 3 x 3 block
  around it and every particle whose nearest node is n: the particle is flagged when |pos - b| <= distanceThreshold and
  |tresca(n) / 1e-7| > shearThreshold, tresca = (lambda_max - lambda_min) / 2 of S = -omega 3 / (2 rho) PiNeq(n)
  (eigenValueFromCell, :951-1000).  Seen from the particle: the binding sites among its nearest node and the 26 around it.

Here: positions are unwrapped; a node is brought onto the lattice by wrapping periodic axes and dropped outside a
non-periodic one (interior_viscosity_ref.wrap), the distance is taken to the unwrapped site; the nearest node is
floor(pos + 0.5); the Tresca value of a node that is not fluid is 0; only vertices of enabled types are flagged.
mask, binding: [nx][ny][nz]; non-zero mask = boundary.
"""
import numpy as np

import interior_viscosity_ref as IV

OFFSETS27 = np.array([(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)], dtype=np.int64)


def populate(binding, mask, periodic, box):
    """populateBindingSites on the inclusive box (x0, x1, y0, y1, z0, z1), clipped to the lattice; binding is changed in
    place and returned"""
    dims = mask.shape
    lo = [max(int(box[2 * d]), 0) for d in range(3)]
    hi = [min(int(box[2 * d + 1]), dims[d] - 1) for d in range(3)]
    for x in range(lo[0], hi[0] + 1):
        for y in range(lo[1], hi[1] + 1):
            for z in range(lo[2], hi[2] + 1):
                if mask[x, y, z] == 0:
                    continue
                keep, w = IV.wrap(OFFSETS27 + (x, y, z), dims, periodic)
                w = w[keep]
                if (mask[w[:, 0], w[:, 1], w[:, 2]] == 0).any():
                    binding[x, y, z] = 1
    return binding


def strain_rate(pi_neq, rho, omega):
    """S [n][3][3] of eigenValueFromCell from PiNeq [n][6] (xx, xy, xz, yy, yz, zz) and rho [n]"""
    pre = (-omega * 3.0) / (2.0 * np.asarray(rho, dtype=np.float64))
    e = np.asarray(pi_neq, dtype=np.float64) * pre[:, None]
    S = np.empty((len(e), 3, 3))
    S[:, 0, 0], S[:, 0, 1], S[:, 0, 2] = e[:, 0], e[:, 1], e[:, 2]
    S[:, 1, 0], S[:, 1, 1], S[:, 1, 2] = e[:, 1], e[:, 3], e[:, 4]
    S[:, 2, 0], S[:, 2, 1], S[:, 2, 2] = e[:, 2], e[:, 4], e[:, 5]
    return S


def tresca(pi_neq, rho, omega, mask):
    """(lambda_max - lambda_min) / 2 per node, 0 where the node is not fluid; and the Frobenius norm of S per node"""
    S = strain_rate(pi_neq, rho, omega)
    lam = np.linalg.eigvalsh(S)
    t = (lam[:, 2] - lam[:, 0]) / 2.0
    fluid = np.asarray(mask).reshape(-1) == 0
    return np.where(fluid, t, 0.0), np.sqrt((S * S).sum(axis=(1, 2)))


def nearest(pos):
    return np.floor(np.asarray(pos, dtype=np.float64) + 0.5).astype(np.int64)


def flag(flags, pos, live, binding, mask, periodic, tresca_node, dist_max, shear_min, margin=1e-9):
    """solidifyCells for the vertices pos [n][3] of one enabled type (live [n] bool: not removed): flags [n] is changed in
    place and returned.  tresca_node [nx*ny*nz].  A candidate -- a vertex with a site in reach -- whose |tresca / 1e-7| lies
    within `margin` (relative) of the threshold would make the verdict depend on the last bits of the eigenvalues: that is
    asserted not to happen, for every candidate (margin 0: no such condition, for listing the candidates).  Returns (flags, candidates [n] bool)."""
    dims = mask.shape
    T = np.asarray(tresca_node).reshape(dims)
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    n = len(pos)
    c = nearest(pos)
    in_grid, cw = IV.wrap(c, dims, periodic)
    g = c[:, None, :] + OFFSETS27[None, :, :]                      # the unwrapped candidates b
    keep, w = IV.wrap(g.reshape(-1, 3), dims, periodic)
    w[~keep] = 0
    site = (keep & (binding[w[:, 0], w[:, 1], w[:, 2]] != 0)).reshape(n, 27)
    d = pos[:, None, :] - g.astype(np.float64)
    dist = np.sqrt(d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1] + d[:, :, 2] * d[:, :, 2])
    cand = np.asarray(live, bool) & in_grid & (site & (dist <= dist_max)).any(axis=1)
    for i in np.flatnonzero(cand):
        node = tuple(cw[i])
        value = abs((float(T[node]) if mask[node] == 0 else 0.0) / 1e-7)
        assert not margin or abs(value - shear_min) > margin * max(value, shear_min), (i, value, shear_min)
        if value > shear_min:
            flags[i] = True
    return flags, cand


def prepare(cells, mask, binding, periodic):
    """prepareSolidification.  cells: dicts with pos [nv][3], tri [nt][3], flags [nv] bool, complete (bool), enabled (bool).
    mask and binding are changed in place.  Returns (solidified [cells] bool, number of nodes turned to wall)."""
    gone = np.zeros(len(cells), bool)
    start = mask.copy()   # the nodes that were fluid when the pass began: the order of the cells does not matter
    nodes = 0
    for k, c in enumerate(cells):
        if not (c["enabled"] and c["complete"] and np.any(c["flags"])):
            continue
        keep, w = IV.wrap(IV.interior_nodes(c["pos"], c["tri"]), mask.shape, periodic)
        w = w[keep]
        w = w[start[w[:, 0], w[:, 1], w[:, 2]] == 0]
        fresh = mask[w[:, 0], w[:, 1], w[:, 2]] == 0
        nodes += int(len(np.unique(w[fresh], axis=0))) if fresh.any() else 0
        mask[w[:, 0], w[:, 1], w[:, 2]] = 1
        binding[w[:, 0], w[:, 1], w[:, 2]] = 1
        gone[k] = True
    return gone, nodes
