"""Restatement of the running statistics (hemocell_amd/csrc/stats.hip) in numpy -- test infrastructure only.

* Fluid sets: running sums of what the observers download, acc = acc + value in sample order starting from +0.0; the second
  moments are the rounded products u_a * u_b of the downloaded u, in the order xx, xy, xz, yy, yz, zz.
* cell_density: +1 per live vertex at its nearest node floor(p + 0.5) (the reference's CellDensity, io/FluidHdf5IO.hh:374-402),
  wrapped on periodic axes and dropped outside the block on the others.
* inside: +1 per complete cell on every FLUID node its surface encloses, by the ray cast of interior_viscosity_ref (truncated
  bounding box, odd number of crossings); overlapping cells both count.
"""
import numpy as np

import interior_viscosity_ref as IV

UU_PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


class FluidSums:
    """the three fluid sets as a host loop over observer downloads"""

    def __init__(self, n):
        self.rho_u = np.zeros((n, 4))
        self.uu = np.zeros((n, 6))
        self.pi = np.zeros((n, 6))
        self.samples = 0

    def add(self, rho, u, pi):
        self.rho_u[:, 0] = self.rho_u[:, 0] + rho
        self.rho_u[:, 1:4] = self.rho_u[:, 1:4] + u
        for k, (a, b) in enumerate(UU_PAIRS):
            prod = u[:, a] * u[:, b]          # rounded, then added
            self.uu[:, k] = self.uu[:, k] + prod
        self.pi = self.pi + pi
        self.samples += 1

    def add_lattice(self, lattice):
        rho, u = lattice.rho_u()
        self.add(rho, u, lattice.pi_neq())


def cell_density(pos, alive, dims, periodic):
    """int64 [nx][ny][nz]: vertices pos [m][3] with alive [m] counted at their nearest node"""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    alive = np.asarray(alive, dtype=bool).reshape(-1)
    nodes = np.floor(pos + 0.5).astype(np.int64)
    keep, w = IV.wrap(nodes, dims, periodic)
    keep &= alive
    out = np.zeros(tuple(dims), np.int64)
    w = w[keep]
    np.add.at(out, (w[:, 0], w[:, 1], w[:, 2]), 1)
    return out


def inside(cells, mask, periodic):
    """int64 [nx][ny][nz]: for every cell (dict with pos [nv][3], tri [nt][3] and optionally complete, default True) +1 on the
    fluid nodes it encloses"""
    out = np.zeros(mask.shape, np.int64)
    for c in cells:
        if not c.get("complete", True):
            continue
        pos = np.asarray(c["pos"], dtype=np.float64)
        span = pos.max(axis=0).astype(np.int64) - pos.min(axis=0).astype(np.int64)
        # a cell that blew up tags nothing (on the other axes the box is cut to the lattice first)
        if np.any((span >= 4 * np.asarray(mask.shape)) & np.asarray(periodic, dtype=bool)):
            continue
        keep, w = IV.wrap(IV.interior_nodes(pos, np.asarray(c["tri"])), mask.shape, periodic)
        w = w[keep]
        w = w[mask[w[:, 0], w[:, 1], w[:, 2]] == 0]
        np.add.at(out, (w[:, 0], w[:, 1], w[:, 2]), 1)
    return out


def cells_of(positions, alive, tri, nv):
    """split the packed positions [ncells * nv][3] of one type into the dicts inside() takes; a cell with a removed vertex is
    incomplete"""
    positions = np.asarray(positions, dtype=np.float64).reshape(-1, nv, 3)
    alive = np.asarray(alive, dtype=bool).reshape(-1, nv)
    return [dict(pos=positions[c], tri=tri, complete=bool(alive[c].all())) for c in range(len(positions))]
