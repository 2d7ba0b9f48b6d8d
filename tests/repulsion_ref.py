"""Restatement of the three vertex kernels that bin a vertex at its nearest lattice node -- test infrastructure only.

- repulsion(): vertex-vertex repulsion (core/hemoCellParticleField.cpp:677-743 with the particle grid of update_pg,
  :137-168), as a brute-force loop over all pairs.
- boundary_repulsion(): wall-node repulsion (:865-918), per vertex over the 27 nodes around its bin in ascending
  (x, y, z) order; the float64 result is computed operation for operation in that order, so it can be compared bit
  for bit, and a np.longdouble twin comes with it.
- tagged(): which vertices advanceParticles tags (:566-588): the nearest node is solid after wrapping.

The rules, stated once.  The bin of a vertex is floor(x + 0.5) per axis, wrapped on periodic axes; a vertex whose
nearest node lies outside a non-periodic axis, or that is not alive (a removed particle, a vertex of a gone cell), is
in no bin.  Two vertices interact when they belong to different cells, both are binned, their bins are equal or
adjacent after wrapping and their minimum-image distance is < cutoff (strict).  Storage is unwrapped: a cell that
crossed a periodic face n times is stored n domain lengths away.

Precision.  A pair's separation dv (a difference of two stored doubles, taken to its minimum image) and its term
r_const * (1 / (d / cutoff)) * (dv / d) are formed in float64 by the one expression the device and the oracle both
use, so all three hold the same term bit for bit (the product is built without contraction); the sums -- where the
implementations differ, in order -- are taken in np.longdouble.  That is what makes the bound
|gpu - ref| <= 4 * k * 2^-53 * sum|t| (bound()) a statement about summation only.  repulsion(..., full=True) forms the
separation and the term in np.longdouble as well; the two agree to the rounding of the terms (see
tests/test_repulsion_edges_cpu.py).

wrong=<name> gives a deliberately wrong restatement (the mutation controls of the tests), as
observables_ref.cell_info(..., wrong=) does: a comparison against it has to fail by far.

The input builders are shared by the CPU and the GPU tests, so both see the same bits.
"""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 1e-18, "np.longdouble has no more precision than double on this platform"

DIMS = (12, 10, 11)
CUTOFF = 1.25          # lattice units, exactly representable
NV_RBC, NV_PLT = 642, 66
WRONG = ("single_same_bin", "no_min_image", "bin_outside", "dead_push")
U = 2.0 ** -53


def nearest_node(pos):
    return np.floor(np.asarray(pos, dtype=np.float64) + 0.5).astype(np.int64)


def in_grid(node, dims, periodic, outside=0):
    """the nearest node lies on the lattice, or anywhere along a periodic axis"""
    ok = np.ones(len(node), dtype=bool)
    for a in range(3):
        if not periodic[a]:
            ok &= (node[:, a] >= -outside) & (node[:, a] < dims[a] + outside)
    return ok


def bound(res):
    """|device - restatement| <= 4 k 2^-53 sum|t| per vertex and component: recursive summation in two different
    orders ((k - 1) u sum|t| each) plus one unit per term"""
    return 4.0 * res["k"][:, None] * U * res["abs"]


def repulsion(pos, cell_of, alive, dims, periodic, r_const, cutoff, wrong=None, full=False):
    """-> dict(sum [n][3] float64, abs [n][3] float64 (sum of |term|), k [n] (terms; a same-bin pair counts twice),
    pairs [m][2] (i < j), same [m] (equal bins), through [m][3] (the bins sit on either side of that periodic seam))"""
    assert wrong is None or wrong in WRONG
    pos = np.ascontiguousarray(pos, dtype=np.float64)
    cell_of = np.asarray(cell_of)
    alive = np.asarray(alive, dtype=bool)
    n = len(pos)
    node = nearest_node(pos)
    inside = in_grid(node, dims, periodic, 2 if wrong == "bin_outside" else 0)
    pushed = alive & inside                                        # gets a force
    pushes = inside if wrong == "dead_push" else pushed            # exerts one
    out = dict(sum=np.zeros((n, 3)), abs=np.zeros((n, 3)), k=np.zeros(n, dtype=np.int64))
    sub = np.nonzero(pushes | pushed)[0]                           # nothing else takes part
    p, c, b = pos[sub], cell_of[sub], node[sub].copy()
    for a in range(3):
        if periodic[a]:
            b[:, a] = np.mod(b[:, a], dims[a])
    p_hp = p.astype(LD)
    pairs, same_l, through_l = [], [], []
    for s in np.nonzero(pushed[sub])[0]:
        db = b[s] - b
        adj = pushes[sub] & (c != c[s])
        seam = np.zeros((len(b), 3), dtype=bool)
        for a in range(3):
            if periodic[a]:
                m = np.mod(db[:, a], dims[a])
                adj &= (m == 0) | (m == 1) | (m == dims[a] - 1)
                seam[:, a] = np.abs(db[:, a]) == dims[a] - 1
            else:
                adj &= np.abs(db[:, a]) <= 1
        j = np.nonzero(adj)[0]
        if len(j) == 0:
            continue
        same = np.all(db[j] == 0, axis=1)            # the bins are wrapped already
        if full:
            dv = p_hp[s] - p_hp[j]
            for a in range(3):
                if periodic[a] and wrong != "no_min_image":
                    dv[:, a] = dv[:, a] - LD(dims[a]) * np.rint(dv[:, a] / LD(dims[a]))
            cut, one = LD(cutoff), LD(1)
        else:
            dv = p[s] - p[j]
            for a in range(3):
                if periodic[a] and wrong != "no_min_image":
                    dv[:, a] = dv[:, a] - float(dims[a]) * np.rint(dv[:, a] / float(dims[a]))
            cut, one = float(cutoff), 1.0
        dist = np.sqrt(dv[:, 0] * dv[:, 0] + dv[:, 1] * dv[:, 1] + dv[:, 2] * dv[:, 2])
        hit = dist < cut
        if not hit.any():
            continue
        j, dv, dist, same = j[hit], dv[hit], dist[hit], same[hit]
        t = (r_const * (one / (dist / cut)))[:, None] * (dv / dist[:, None])
        fac = np.where(same, 1 if wrong == "single_same_bin" else 2, 1)
        t = t.astype(LD) * fac[:, None]
        i = sub[s]
        out["sum"][i] = t.sum(axis=0).astype(np.float64)
        out["abs"][i] = np.abs(t).sum(axis=0).astype(np.float64)
        out["k"][i] = fac.sum()
        up = sub[j] > i
        pairs += [(i, q) for q in sub[j][up]]
        same_l += list(same[up])
        through_l += list(seam[j][up])
    out["pairs"] = np.array(pairs, dtype=np.int64).reshape(-1, 2)
    out["same"] = np.array(same_l, dtype=bool)
    out["through"] = np.array(through_l, dtype=bool).reshape(-1, 3)
    return out


def boundary_flags(mask, periodic):
    """a wall node with a known non-wall node among its 26 neighbours; neighbours wrap on periodic axes and are
    unknown beyond non-periodic faces"""
    solid = np.asarray(mask) != 0
    fluid = ~solid
    for a in range(3):
        pad = [(0, 0)] * 3
        pad[a] = (1, 1)
        fluid = np.pad(fluid, pad, mode="wrap") if periodic[a] else np.pad(fluid, pad, mode="constant", constant_values=False)
    nx, ny, nz = solid.shape
    near = np.zeros_like(solid)
    for a in range(3):
        for b in range(3):
            for c in range(3):
                near |= fluid[a:a + nx, b:b + ny, c:c + nz]
    return solid & near


def boundary_repulsion(pos, alive, mask, periodic, k, cutoff, r0):
    """force_repulsion after one applyBoundaryRepulsionForce on top of r0 -> (float64 in the kernel's order of
    operations, np.longdouble twin rounded to double)"""
    pos = np.ascontiguousarray(pos, dtype=np.float64)
    dims = np.asarray(mask).shape
    flag = boundary_flags(mask, periodic)
    node = nearest_node(pos)
    act = np.asarray(alive, dtype=bool) & in_grid(node, dims, periodic)
    r = np.array(r0, dtype=np.float64)
    r_hp = r.astype(LD)
    p, c = pos[act], node[act]
    acc, acc_hp = r[act].copy(), r_hp[act].copy()
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                g = c + np.array([dx, dy, dz])
                w, ok = g.copy(), np.ones(len(g), dtype=bool)
                for a in range(3):
                    if periodic[a]:
                        w[:, a] = np.mod(w[:, a], dims[a])
                    else:
                        ok &= (w[:, a] >= 0) & (w[:, a] < dims[a])
                        w[:, a] = np.clip(w[:, a], 0, dims[a] - 1)
                ok &= flag[w[:, 0], w[:, 1], w[:, 2]]
                dv = p - g.astype(np.float64)
                dist = np.sqrt(dv[:, 0] * dv[:, 0] + dv[:, 1] * dv[:, 1] + dv[:, 2] * dv[:, 2])
                hit = ok & (dist < cutoff)
                with np.errstate(divide="ignore", invalid="ignore"):
                    t = (k * (1 / (dist / cutoff)))[:, None] * (dv / dist[:, None])
                acc[hit] = acc[hit] + t[hit]
                dh = p.astype(LD) - g.astype(LD)
                dist_h = np.sqrt(dh[:, 0] * dh[:, 0] + dh[:, 1] * dh[:, 1] + dh[:, 2] * dh[:, 2])
                with np.errstate(divide="ignore", invalid="ignore"):
                    th = (LD(k) * (LD(1) / (dist_h / LD(cutoff))))[:, None] * (dh / dist_h[:, None])
                acc_hp[hit] = acc_hp[hit] + th[hit]
    r[act] = acc
    r_hp[act] = acc_hp
    return r, r_hp.astype(np.float64)


def tagged(pos, mask, periodic):
    """the nearest node is solid after wrapping; a node outside a non-periodic axis tags nothing"""
    mask = np.asarray(mask)
    dims = mask.shape
    node = nearest_node(pos)
    ok = in_grid(node, dims, periodic)
    w = np.mod(node, dims)
    return ok & (mask[w[:, 0], w[:, 1], w[:, 2]] != 0)


# ------------------------------------------------------------------------------------------------ inputs
def block_mask(dims=DIMS):
    """Solid blocks that touch the faces.  Block A (x 0..1, y 0..4, every z) holds wall nodes whose only fluid
    neighbours lie across the x seam (0, 2, z) or across the y seam; block B (x nx-2..nx-1, y 4..6, z nz-1) touches the
    high x and z faces.  On a non-periodic axis the same nodes are wall nodes on a face."""
    nx, ny, nz = dims
    m = np.zeros(dims, dtype=np.uint8)
    m[0:2, 0:min(5, ny), :] = 1
    m[nx - 2:nx, min(4, ny - 1):min(7, ny), nz - 1] = 1
    return m


def slab_mask(dims=DIMS):
    """the two lowest z layers are solid"""
    m = np.zeros(dims, dtype=np.uint8)
    m[:, :, 0:2] = 1
    return m


class _Placer:
    """puts vertices one by one, refusing one that would be the 11th of its bin, that comes closer than 0.05 lu to
    another (minimum image) or that comes near a protected vertex"""

    def __init__(self, dims, periodic, sizes, lap):
        self.n = np.array(dims, dtype=np.float64)
        self.dims, self.per = dims, np.array(periodic, dtype=bool)
        self.left = list(sizes)
        self.lap = np.asarray(lap, dtype=np.float64)
        self.pts, self.owner, self.count, self.protected = [], [], {}, []

    def _sep(self, q, others):
        d = q - np.asarray(others)
        d[:, self.per] -= self.n[self.per] * np.rint(d[:, self.per] / self.n[self.per])
        return np.sqrt((d * d).sum(axis=1))

    def add(self, p, cell, protect=False):
        if self.left[cell] == 0:
            return False
        q = np.asarray(p, dtype=np.float64) + self.lap[cell] * self.n      # stored unwrapped
        node = nearest_node(q)
        key = tuple(np.where(self.per, np.mod(node, self.dims), node))
        if self.count.get(key, 0) >= 10:
            return False
        if self.pts and self._sep(q, self.pts).min() < 0.05:
            return False
        if not protect and self.protected and self._sep(q, self.protected).min() < 2.0:
            return False
        self.pts.append(q); self.owner.append(cell); self.left[cell] -= 1
        self.count[key] = self.count.get(key, 0) + 1
        if protect:
            self.protected.append(q)
        return True


def build_case(periodic, dims=DIMS, seed=1, n_plt=6, big=True):
    """One 642-vertex bag (cell 0; none with big=False) and n_plt 66-vertex bags, in storage order (the big type first).  Cell 1 is stored
    +2 domain lengths away on every periodic axis and cell 2 one domain length back.  Vertices of different cells lie
    0.2 .. 2 lu apart: in the interior, across the low and the high face of every axis, at two corners, along ladders
    that leave the lattice through every face (nearest nodes -3 .. 0 and n-1 .. n+2) and all over a box 1.5 lu larger
    than the lattice.  One vertex per cloud (on -0.5 and n - 0.5 at the faces) and every tenth of the rest sit on a
    half-integer coordinate.  Cells
    3 and 4 hold a pair along x exactly one cut-off apart, cells 5 and 6 a pair along z one ulp of the cut-off closer; nothing else comes
    within 2 lu of these four.
    -> dict(pos [n][3], cell_of [n], sizes, cut (i, j), twin (i, j))"""
    assert n_plt >= 7 - big
    rng = np.random.default_rng(seed)
    nx, ny, nz = dims
    n = np.array(dims, dtype=np.float64)
    per = np.array(periodic, dtype=np.float64)
    sizes = [NV_RBC] * big + [NV_PLT] * n_plt
    lap = np.zeros((len(sizes), 3)); lap[1] = 2 * per; lap[2] = -1 * per
    P = _Placer(dims, periodic, sizes, lap)
    ya, yb = np.floor(0.7 * ny) + 0.25, np.floor(0.2 * ny) + 0.25
    special = [((2.0, ya, 8.0), 3), ((2.0 + CUTOFF, ya, 8.0), 4), ((8.0, yb, 0.5), 5), ((8.0, yb, np.nextafter(0.5 + CUTOFF, 0.0)), 6)]
    for p, cell in special:
        assert P.add(p, cell, protect=True)
    mid = np.array([0.45 * nx, 0.66 * ny, 0.5 * nz])
    sites = [(mid, None, None)]
    others = [np.array([0.0, 0.66 * ny, 5.4]), np.array([6.3, 0.0, 5.4]), np.array([4.3, 0.64 * ny, 0.0])]
    others_hi = [np.array([0.0, 0.68 * ny, 3.4]), np.array([5.8, 0.0, 2.4]), np.array([8.3, 0.74 * ny, 0.0])]
    for a in range(3):
        lo, hi = others[a].copy(), others_hi[a].copy()
        lo[a], hi[a] = -0.3, n[a] - 0.6
        sites += [(lo, a, -0.5), (hi, a, n[a] - 0.5)]
    sites += [(np.array([-0.3, -0.3, -0.3]), None, None), (n - 0.6, None, None)]
    cells = len(sizes)
    for s, (centre, axis, tie) in enumerate(sites):
        placed = 0
        while placed < 12:
            p = centre + rng.uniform(-0.75, 0.75, 3)
            if placed == 0:                          # a tie of floor(x + 0.5)
                if axis is None:
                    p[s % 3] = np.floor(p[s % 3]) + 0.5
                else:
                    p[axis] = tie
            placed += P.add(p, (s + placed) % cells)
    low = [-2.9, -2.6, -2.1, -1.7, -1.3, -0.8, -0.4, 0.2]
    high = [-0.7, -0.2, 0.3, 0.8, 1.2, 1.8]
    base = [np.array([0.0, 0.85 * ny, 2.5]), np.array([5.5, 0.0, 3.5]), np.array([5.0, 0.35 * ny, 0.0])]
    for a in range(3):
        for r, v in enumerate(low + [n[a] + h for h in high]):
            for _ in range(100):
                p = base[a] + rng.uniform(-0.3, 0.3, 3)
                p[a] = v
                if P.add(p, 3 + (r + a) % 4):          # cells without laps: outside means outside
                    break
            else:
                raise AssertionError("ladder vertex not placed")
    tries = 0
    while sum(P.left):
        tries += 1
        assert tries < 200000, "the filler does not fit"
        w = np.array(P.left, dtype=np.float64)
        p = rng.uniform(-1.5, n + 1.5)
        if tries % 10 == 0:
            p[tries % 3] = np.floor(p[tries % 3]) + 0.5
        P.add(p, int(rng.choice(cells, p=w / w.sum())))
    owner = np.array(P.owner)
    pts = np.array(P.pts)
    order = np.argsort(owner, kind="stable")
    where = np.empty(len(order), dtype=np.int64); where[order] = np.arange(len(order))
    pos = np.ascontiguousarray(pts[order])
    return dict(pos=pos, cell_of=owner[order], sizes=sizes, cut=(where[0], where[1]), twin=(where[2], where[3]))


def build_gone_case(dims=DIMS, seed=3):
    """Three 66-vertex cells over slab_mask(): cell 0 is given velocities that put its low vertices (z < 2.3) on the
    wall layer z = 1 in one advance; cell 1 stays just above the wall, within the cut-off of those; cell 2 lies among
    the survivors of cell 0.  -> dict(pos, vel, cell_of, sizes, mask)"""
    rng = np.random.default_rng(seed)
    sizes = [NV_PLT] * 3
    P = _Placer(dims, (0, 0, 0), sizes, np.zeros((3, 3)))
    zr = [(1.6, 3.2), (1.55, 2.4), (2.5, 3.5)]
    start, vel = [], []
    for cell in range(3):
        while P.left[cell]:
            p = np.array([rng.uniform(2.0, 8.0), rng.uniform(2.0, 8.0), rng.uniform(*zr[cell])])
            v = -0.9 if (cell == 0 and p[2] < 2.3) else 0.0
            q = p + np.array([0.0, 0.0, v])
            if P.add(q, cell):                       # the spacing and the bin limit hold where the vertices end up
                start.append(p); vel.append((0.0, 0.0, v))
    pos, vel = np.array(start), np.array(vel)
    return dict(pos=pos, vel=vel, cell_of=np.array(P.owner), sizes=sizes, mask=slab_mask(dims))


def conditions(ref, ref_outside, pos, alive, dims, periodic, case=None):
    """What keeps a comparison from passing on nothing, from the restatement alone -> dict of counts"""
    out = dict(pairs=len(ref["pairs"]), same_bin=int(ref["same"].sum()),
               through=[int(ref["through"][:, a].sum()) for a in range(3)])
    outside = np.asarray(alive, dtype=bool) & ~in_grid(nearest_node(pos), dims, periodic)
    out["outside_would_interact"] = int((outside & (ref_outside["k"] > 0)).sum())
    out["outside_silent"] = bool((ref["k"][outside] == 0).all())
    if case is not None:
        out["cut_is_zero"] = all(ref["k"][i] == 0 for i in case["cut"])
        out["twin_is_not"] = all(ref["k"][i] == 1 for i in case["twin"])
    return out


def check_conditions(c, periodic):
    assert c["pairs"] >= 50 and c["same_bin"] >= 5, c
    for a in range(3):
        assert c["through"][a] >= 5 if periodic[a] else c["through"][a] == 0, c
    if not all(periodic):
        assert c["outside_would_interact"] >= 5, c
    assert c["outside_silent"] and c.get("cut_is_zero", True) and c.get("twin_is_not", True), c
