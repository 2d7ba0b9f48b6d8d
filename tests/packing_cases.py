"""Starts for the packing kernels past their first wave, block and grid cell (tests/test_gpu_packing_shapes.py on the device,
tests/test_packing_cpu.py for the conditions each start rests on).

build(name) returns a Case: grid, sizes_scaled [ns][3], counts, nominal_fraction (the attributes DevicePacking of
tests/test_gpu_packing.py reads from a plan), names, pos [N][3], quat [N][4] or None, all from
numpy.random.Generator(PCG64(seed)).  The sizes are the scaled ones of the other packing tests (1.2 / 8.4 per um).

  uneven288   grid (5, 6, 8), 260 RBC + 25 PLT + 3 WBC, given orientations: every species on the cell list, N above one
              block and no multiple of a wave (pk_list runs five chunks, the last one partial)
  uneven134   grid (3, 6, 8), 120 + 12 + 2: RBC and WBC on all pairs, the platelet on the cell list
  uneven70    grid (3, 6, 8), 60 + 8 + 2: N just past one wave
  cluster     grid 8^3, 190 RBC + 10 PLT inside a cube of edge 0.9: every particle is every other's partner, so the
              create-time list length (161) is short and hc_packing_create has to grow the lists
  faces       grid 4^3, 43 + 3 with four rows on the faces and the origin (deviation 8)
  coincident  faces with row 45 moved onto row 1 modulo the box: rij = 0, the pair's force is 0/0
  thrown      grid 8^3, 310 + 10 inside half a cell: the first steps are longer than the box and leave it (deviation 11)

list_capacity, modes and partner_counts restate the rules of hc_packing_create, pk_bin and partner() in numpy, apart from
tests/packing_ref.cpp, so that a test can say what a start reaches before anything runs."""
import numpy as np

SCALE = 1.2 / 8.4
RBC = np.array([8.4, 4.4, 8.4]) * SCALE
PLT = np.array([2.4, 1.05, 2.4]) * SCALE
WBC = np.array([8.4, 8.4, 8.4]) * SCALE
SIZES = dict(RBC=RBC, PLT=PLT, WBC=WBC)


class Case:
    def __init__(self, name, grid, names, counts, nominal, pos, quat=None):
        self.name, self.grid, self.names, self.counts = name, tuple(grid), list(names), list(counts)
        self.sizes_scaled = np.ascontiguousarray([SIZES[n] for n in names])
        self.nominal_fraction = nominal
        self.n = sum(counts)
        self.pos = np.ascontiguousarray(pos, dtype=np.float64)
        self.quat = None if quat is None else np.ascontiguousarray(quat, dtype=np.float64)
        assert self.pos.shape == (self.n, 3)
        self.spec = np.repeat(np.arange(len(counts)), counts)

    def rows(self, name):
        return self.spec == self.names.index(name)


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _uneven(name, grid, counts, seed=5):
    rng = _rng(seed)
    n = sum(counts)
    pos = rng.random((n, 3)) * np.array(grid, dtype=np.float64)
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1)[:, None]
    return Case(name, grid, ("RBC", "PLT", "WBC"), counts, 0.5, pos, q)


def _faces(name, last):
    pos = _rng(5).random((46, 3)) * 4.0
    pos[0] = (4.0, 1.3, 2.2)
    pos[1] = (0.0, 0.0, 0.0)
    pos[2] = (2.0, 4.0, 4.0)
    pos[45] = last
    return Case(name, (4, 4, 4), ("RBC", "PLT"), (43, 3), 0.506331, pos)


def build(name):
    if name == "uneven288":
        return _uneven(name, (5, 6, 8), (260, 25, 3))
    if name == "uneven134":
        return _uneven(name, (3, 6, 8), (120, 12, 2))
    if name == "uneven70":
        return _uneven(name, (3, 6, 8), (60, 8, 2))
    if name == "cluster":
        return Case(name, (8, 8, 8), ("RBC", "PLT"), (190, 10), 0.3, _rng(7).random((200, 3)) * 0.9 + 3.0)
    if name == "faces":
        return _faces(name, (4.0, 4.0, 1.7))
    if name == "coincident":
        return _faces(name, (4.0, 4.0, 4.0))
    if name == "thrown":
        return Case(name, (8, 8, 8), ("RBC", "PLT"), (310, 10), 0.3, _rng(11).random((320, 3)) * 0.5 + 0.5)
    raise KeyError(name)


UNEVEN = ("uneven288", "uneven134", "uneven70")
# per species of (RBC, PLT, WBC): the cell list ("part") or all pairs ("all") at the first diameter
UNEVEN_MODES = dict(uneven288=["part", "part", "part"], uneven134=["all", "part", "all"], uneven70=["all", "all", "all"])


def first_diameter(case):
    """Douter of Packing::init (packing.h:268-289)"""
    cells = case.grid[0] * case.grid[1] * case.grid[2]
    diam_dens = cells / (3.141592653589793 / 6.) / float(sum(case.counts))
    return (diam_dens * case.nominal_fraction) ** (1. / 3.)


def modes(case, Douter):
    """which path a species takes as A (packing.h:390-393): the cell list while (int)(2 Rcut) < smallest grid axis - 1"""
    rc_max = case.sizes_scaled[:, 0].max()
    return ["part" if int(2.0 * (0.55 * Douter * (s + rc_max))) < min(case.grid) - 1 else "all" for s in case.sizes_scaled[:, 0]]


def list_capacity(case):
    """the list length hc_packing_create starts with: twice the mean number of particles in the largest cell range at the first
    diameter plus 64, and N - 1 where that range is the whole grid"""
    n, grid = case.n, case.grid
    rcut0 = 0.55 * first_diameter(case) * 2 * case.sizes_scaled[:, 0].max()
    if not int(2.0 * rcut0) < min(grid) - 1:
        return max(n - 1, 1)
    cells = 1.0
    for g in grid:
        cells *= min(2 * rcut0 + 2, g)
    return max(min(int(2 * (cells * n / (grid[0] * grid[1] * grid[2]))) + 64, n - 1), 1)


def grown_capacity(case, largest):
    """pk_grow: the largest partner count seen plus a quarter plus 16, at most N - 1"""
    return max(min(largest + largest // 4 + 16, case.n - 1), 1)


def partner_matrix(case, pos, Douter):
    """[A][B] for B < A: B is a partner of A (deviations 8 and 11 of DESIGN section 6): A on all pairs, or on every axis
    (int)x_B in 0..grid-1 and within A's range (int)(x_A + grid - Rcut) .. (int)(x_A + grid + Rcut) taken modulo the grid"""
    n = case.n
    rc_max = case.sizes_scaled[:, 0].max()
    rcut = 0.55 * Douter * (case.sizes_scaled[case.spec, 0] + rc_max)
    part = np.array([int(2.0 * r) < min(case.grid) - 1 for r in rcut])
    act = np.ones((n, n), dtype=bool)
    for k, g in enumerate(case.grid):
        c = np.trunc(pos[:, k]).astype(np.int64)
        lo = np.trunc(pos[:, k] + g - rcut).astype(np.int64)
        hi = np.trunc(pos[:, k] + g + rcut).astype(np.int64)
        span = np.clip(hi - lo, 0, g - 1)
        d = (c[None, :] - lo[:, None]) % g                  # numpy's % is the floor modulo
        act &= (d <= span[:, None]) & ((c >= 0) & (c < g))[None, :]
    act |= ~part[:, None]
    return np.tril(act, -1)


def partner_counts(case, pos, Douter):
    """partners per particle, as A and as B together: what pk_list counts"""
    m = partner_matrix(case, pos, Douter)
    return m.sum(axis=1) + m.sum(axis=0)
