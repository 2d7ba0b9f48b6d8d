"""Shared pieces of the interior-viscosity tests: an icosphere, the sphere property the restatement must have, and the
scene of the GPU tests -- test infrastructure only."""
import numpy as np

import interior_viscosity_ref as IV


def icosphere(radius, subdivisions=2):
    """a closed, outward-oriented triangulation of the sphere: vertices [nv][3] on the sphere, triangles [nt][3]"""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(subdivisions):
        mid, g = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            g += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = g
    return radius * np.array(v), np.array(f, dtype=np.int64)


def check_sphere(verts, tri, centres, dims=(24, 24, 24)):
    """verts: a closed mesh around the origin that holds the ball of its inscribed radius (the least distance of a triangle's
    plane from the origin) and lies in the ball of its largest vertex radius.  For the mesh moved to every centre: every node
    closer to the centre than the inscribed radius is interior, no node farther than the largest vertex radius is, also
    with the cell wrapped over the periodic faces of a lattice `dims`.  Returns the number of interior nodes per centre."""
    v0, v1, v2 = verts[tri[:, 0]], verts[tri[:, 1]], verts[tri[:, 2]]
    n = np.cross(v1 - v0, v2 - v0)
    n /= np.linalg.norm(n, axis=1)[:, None]
    r_in = float(np.abs((n * v0).sum(axis=1)).min())
    r_out = float(np.linalg.norm(verts, axis=1).max())
    assert 0.5 * r_out < r_in < r_out
    counts = []
    for c in centres:
        c = np.asarray(c, dtype=np.float64)
        pos = verts + c
        inside = IV.interior_nodes(pos, tri)
        dist = np.linalg.norm(inside - c, axis=1)
        assert dist.max() <= r_out, (c, dist.max(), r_out)
        box = IV.box_nodes(pos)
        must = box[np.linalg.norm(box - c, axis=1) < r_in]
        got = {tuple(p) for p in inside.tolist()}
        missing = [tuple(p) for p in must.tolist() if tuple(p) not in got]
        assert not missing, (c, missing[:5])
        assert len(must) > 100
        # the same cell on a periodic lattice: the class field holds exactly the wrapped interior nodes
        mask = np.zeros(dims, np.uint8)
        cls = IV.find([dict(id=0, type=0, pos=pos, tri=tri, klass=1)], mask, (True, True, True))
        want = np.zeros(dims, np.uint8)
        w = np.mod(inside, np.array(dims))
        want[w[:, 0], w[:, 1], w[:, 2]] = 1
        assert np.array_equal(cls, want)
        assert int(cls.sum()) == len(inside)   # the cell is narrower than the lattice: no two nodes fold onto one
        counts.append(len(inside))
    return counts


SPHERE_CENTRES = [(11.3, 12.7, 10.2), (12.05, 11.45, 12.8), (10.62, 10.91, 13.37), (1.3, 12.4, 22.6), (-2.2, 25.1, 0.4)]


# ---- the scene of the GPU tests: a 32 x 24 x 24 lattice, periodic along x and z, a wall layer on both y faces (moving-wall
# classes 3 and 4: shear), and four RBCs of two types with different viscosity ratios
DIMS = (32, 24, 24)
PERIODIC = (True, False, True)
WALL_U = {3: (0.02, 0.0, 0.0), 4: (-0.02, 0.0, 0.0)}
RATIOS = (5.0, 3.0)


def scene_mask():
    m = np.zeros(DIMS, np.uint8)
    m[:, 0, :] = 3
    m[:, -1, :] = 4
    return m


def _rotation(deg):
    a, b, c = (np.deg2rad(v) for v in deg)
    rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    return rz @ ry @ rx


def scene_cells(mesh, wall_overlap):
    """[(cell id, type, positions)]: one RBC rotated off-axis mid-box; one across the periodic x face and the periodic z face;
    one at the lower wall -- with wall_overlap its surface reaches through the wall layer y = 0 and below the lattice, else
    it stays 0.8 above the wall nodes; and one of the second type that intersects the first.  Ids are neither in append order
    nor grouped by type."""
    v = mesh - 0.5 * (mesh.max(axis=0) + mesh.min(axis=0))
    thin = int(np.argmin(v.max(axis=0) - v.min(axis=0)))   # the disc's axis
    # a rotation (not a reflection: the surface keeps its orientation) that brings the thin axis onto y
    flat = v @ _rotation({0: (0.0, 0.0, 90.0), 1: (0.0, 0.0, 0.0), 2: (90.0, 0.0, 0.0)}[thin]).T
    assert int(np.argmin(flat.max(axis=0) - flat.min(axis=0))) == 1
    half = float(-flat[:, 1].min())
    cells = [(7, 0, v @ _rotation((30.0, 20.0, 10.0)).T + np.array([15.3, 12.2, 11.6])),
             (2, 0, v @ _rotation((0.0, 75.0, 40.0)).T + np.array([0.7, 11.4, 23.2])),
             (5, 0, (flat @ _rotation((0.0, 0.0, 90.0)).T + np.array([22.4, 1.3, 6.6])) if wall_overlap
              else flat + np.array([22.4, 0.8 + half, 6.6])),
             (3, 1, v @ _rotation((30.0, 20.0, 10.0)).T + np.array([17.9, 12.9, 13.1]))]
    return cells


def restatement_cells(cells, tables, klass_of_type):
    return [dict(id=i, type=t, pos=p, tri=tables["triangles"], klass=klass_of_type[t], area_mean_eq=tables["area_mean_eq"],
                 edge_mean_eq=tables["edge_mean_eq"]) for i, t, p in cells]
