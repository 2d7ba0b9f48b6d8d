"""Deterministic synthetic cell packing for benchmark / test domains (replaces tools/packCells for the
synthetic pipeflow inputs of SURVEY.md §8d: a jittered grid, seed fixed, cells kept only when they lie
inside the lumen).  Pure host-side input generation; positions are in lattice units."""
import numpy as np


def pack_pipe_rbc(nx, ny, nz, hematocrit, seed=12345, rbc_volume_lu=649.0, x0=0, nx_global=None):
    """RBC centres + Euler angles (degrees, .pos convention) for a pipe along x of radius (ny-2)/2.

    RBCs are discs ~16 lu across and ~5 lu thick; they are laid flat (thin axis along z after the
    (90,0,0) rotation of the reference's .pos files) on a grid whose pitch is chosen to hit the requested
    hematocrit, with +-1 lu jitter and +-8 degree tilt.  Only cells whose centre lies in
    [x0, x0+nx) are returned so that slabs of a larger domain get disjoint, consistent subsets."""
    nxg = nx_global if nx_global is not None else nx
    R = (ny - 2) / 2.0
    cy, cz = (ny - 1) / 2.0, (nz - 1) / 2.0
    lumen = np.pi * R * R * nxg
    target = hematocrit * lumen / rbc_volume_lu
    # in-plane pitch fixed by the disc size, axial pitch from the target count
    px = py = 19.0
    pz_min = 7.0
    # count of usable (y,z,x) sites for a given pz; choose pz to meet the target
    best = None
    for pz in np.arange(pz_min, 40.0, 0.25):
        ys = np.arange(cy - np.floor((R - 9) / py) * py, cy + R, py)
        zs = np.arange(cz - np.floor((R - 4) / pz) * pz, cz + R, pz)
        xs = np.arange(px / 2, nxg - px / 2 + 1e-9, px)
        n = 0
        for y in ys:
            for z in zs:
                # the whole disc (radius 8.5 in x-y, half thickness 3 in z) must stay inside R-2
                if np.hypot(abs(y - cy) + 8.5, abs(z - cz) + 3.0) < R - 2.0:
                    n += 1
        n *= len(xs)
        if best is None or abs(n - target) < abs(best[0] - target):
            best = (n, pz, ys, zs, xs)
    n, pz, ys, zs, xs = best
    rng = np.random.default_rng(seed)
    centres, angles = [], []
    for ix, x in enumerate(xs):
        for y in ys:
            for z in zs:
                if not np.hypot(abs(y - cy) + 8.5, abs(z - cz) + 3.0) < R - 2.0:
                    continue
                j = rng.uniform(-0.75, 0.75, 3)
                j[2] = rng.uniform(-0.4, 0.4)
                a = rng.uniform(-8.0, 8.0, 3)
                c = np.array([x, y, z]) + j
                if x0 <= c[0] < x0 + nx:
                    centres.append(c)
                    angles.append(np.array([90.0, 0.0, 0.0]) + a)
    return np.array(centres).reshape(-1, 3), np.array(angles).reshape(-1, 3)


# ---------------------------------------------------------------------------------------------------------------------------
# tools/packCells: cells to a target hematocrit in a periodic box.  packing_plan is the host arithmetic of packCells.cpp and
# Packing::initBlood; pack_cells runs the force-bias packing on the GPU (csrc/packing.hip, hc_packing_*).

# full axes of the enclosing ellipsoids in um (packCells.cpp:88-96)
CELL_SIZES_UM = {
    "RBC": (8.4, 4.4, 8.4),
    "PLT": (2.4, 1.05, 2.4),
    "WBC": (8.4, 8.4, 8.4),
    "vRBC": (3.5, 6.0, 11.0),
    "RBC_m": (5.8, 3.4, 5.8),
    "PLT_m": (1.84, 1.05, 1.84),
    "PLT_mko": (1.71, 1.71, 1.71),
}
RBC_VOLUME_NOMINAL_UM3 = 97.0   # packCells.cpp:203
MAX_ITER_DEFAULT = 2147483647 - 100   # packCells.cpp:106


class PackingPlan:
    """what packCells decides before it packs: the cell types with their counts and sizes, the sizing factor, the grid of the
    collision check, the nominal volume fraction of the enclosing ellipsoids and the box that is really packed"""

    def __init__(self, size_um, names, counts, sizes_um, scale, grid, nominal_fraction, hematocrit, plt_ratio):
        self.size_um = tuple(float(s) for s in size_um)
        self.names = list(names)
        self.counts = [int(c) for c in counts]
        self.sizes_um = np.array(sizes_um, dtype=np.float64).reshape(-1, 3)
        self.scale = float(scale)
        self.sizes_scaled = self.sizes_um * self.scale
        self.grid = tuple(int(g) for g in grid)
        self.nominal_fraction = float(nominal_fraction)
        self.hematocrit = hematocrit
        self.plt_ratio = plt_ratio
        self.box_um = tuple(g * (1.0 / self.scale) for g in self.grid)
        self.warning = None
        if self.nominal_fraction > 0.7:   # packing.h:249-253
            self.warning = ("the enclosing ellipsoids yield a nominal volume ratio of %.6f; the densest possible packing is "
                            "around 0.77" % self.nominal_fraction)

    def count(self, name):
        return sum(c for n, c in zip(self.names, self.counts) if n == name)


def _c_round(x):
    """C's round(): halves away from zero"""
    return int(np.floor(x + 0.5)) if x >= 0 else -int(np.floor(-x + 0.5))


def packing_plan(size_um, hematocrit=None, plt_ratio=0.07, cells=None, scale=None, volume_um3=None):
    """packCells.cpp:197-241 and Packing::initBlood (packing.h:198-262), pure host code.

    size_um: the requested box; cells: a list of (name, count) with a name of CELL_SIZES_UM, or (name, count, (dx, dy, dz))
    for a custom ellipsoid, in the order of the command line; hematocrit adds round(Hct V / 97) RBC and round(nRBC ratio)
    PLT after them.  As in the reference, hematocrit excludes explicit RBC and PLT counts, and one of the two is needed.
    scale=None is 1.2 / (largest axis of the most numerous type).  Reference quirks that stay: the grid is ceil(size * scale)
    cells per axis, so the packed box (box_um) is larger than requested (24 um: 4 cells = 28 um) while the nominal fraction
    is computed from the requested size; the reference carries the hematocrit and the scaled box sizes in single precision,
    which decides the rounding of a borderline count or grid and is kept.  volume_um3 (this back end's own, for a vessel inside
    the box): the hematocrit's cell counts come from this volume, the lumen, and not from the box; nothing else changes."""
    size = [float(s) for s in size_um]
    if len(size) != 3 or not all(np.isfinite(s) and s > 0 for s in size):
        raise ValueError("size_um must be three positive lengths")
    types = []
    for c in (cells or []):
        name, n = c[0], int(c[1])
        if len(c) > 2:
            dims = tuple(float(v) for v in c[2])
        elif name in CELL_SIZES_UM:
            dims = CELL_SIZES_UM[name]
        else:
            raise ValueError("unknown cell type %r: give (name, count, (dx, dy, dz))" % (name,))
        if n < 0 or len(dims) != 3 or not all(np.isfinite(v) and v > 0 for v in dims):
            raise ValueError("cell type %r needs a count >= 0 and three positive sizes" % (name,))
        types.append((name, n, dims))
    if hematocrit is not None and any(len(c) == 2 and c[0] in ("RBC", "PLT") for c in (cells or [])):
        raise ValueError("hematocrit is mutually exclusive with explicit RBC and PLT counts")   # packCells.cpp:120-146
    if hematocrit is None and not types:
        raise ValueError("specify at least a cell type or the hematocrit")                     # packCells.cpp:197-200
    if hematocrit is not None:
        h = float(np.float32(hematocrit))
        if not (np.isfinite(h) and h >= 0):
            raise ValueError("hematocrit must be a non-negative number")
        volume = size[0] * size[1] * size[2]
        if volume_um3 is not None:
            volume = float(volume_um3)
            if not (np.isfinite(volume) and volume > 0):
                raise ValueError("volume_um3 must be a positive volume")
        n_rbc = _c_round(h * volume / RBC_VOLUME_NOMINAL_UM3)
        types.append(("RBC", n_rbc, CELL_SIZES_UM["RBC"]))
        n_plt = _c_round(n_rbc * float(plt_ratio))
        if n_plt > 0:
            types.append(("PLT", n_plt, CELL_SIZES_UM["PLT"]))
    if scale is None or scale <= 0.0:   # packCells.cpp:216-241: the first of the most numerous types
        most, largest = 0, 0.0
        for _, n, dims in types:
            if most < n:
                most, largest = n, max(dims)
        if most == 0:
            raise ValueError("no cells to pack")
        scale = (1. / largest) * 1.2
    scale = float(scale)
    # initBlood: float sizeX *= Sizing; ceil; the volume is the product of the three floats
    fs = [np.float32(np.float64(np.float32(s)) * scale) for s in size]
    grid = [int(np.ceil(v)) for v in fs]
    domain = float(np.float32(np.float32(fs[0] * fs[1]) * fs[2]))
    cell_volume = 0.0
    for _, n, dims in types:
        dx, dy, dz = (v * scale for v in dims)
        cell_volume += ((4. / 3. * 3.141592653589793 * dx / 2. * dy / 2. * dz / 2.) * n)
    return PackingPlan(size, [t[0] for t in types], [t[1] for t in types], [t[2] for t in types], scale, grid, cell_volume / domain,
                       hematocrit, plt_ratio if hematocrit is not None else None)


def quaternion_matrix(q):
    """Quaternion::countQ (geometry.h:424-428) of (s, p): 2 (p p^T - s skew(p) + (s^2 - 1/2) I); [..., 3, 3]"""
    q = np.asarray(q, dtype=np.float64)
    s, p = q[..., 0], q[..., 1:]
    skew = np.zeros(q.shape[:-1] + (3, 3))
    skew[..., 0, 1], skew[..., 0, 2] = -p[..., 2], p[..., 1]
    skew[..., 1, 0], skew[..., 1, 2] = p[..., 2], -p[..., 0]
    skew[..., 2, 0], skew[..., 2, 1] = -p[..., 1], p[..., 0]
    return 2.0 * (p[..., :, None] * p[..., None, :] - s[..., None, None] * skew + (s * s - 0.5)[..., None, None] * np.eye(3))


def euler_angles_deg(q):
    """the angles packCells writes (saveBloodCellPositions, packing.h:634-636): (atan2(Q12, Q22), -asin(Q02), atan2(Q01, Q00))
    of countQ(), in degrees.  A .pos reader (io/readPositionsBloodCells.cpp:40-109, 228-229; host.Cells.addCell) turns them
    into the body-to-world rotation Rz(c) Ry(b) Rx(a), which is the transpose of countQ()."""
    Q = quaternion_matrix(q)
    a = np.arctan2(Q[..., 1, 2], Q[..., 2, 2])
    b = -np.arcsin(np.clip(Q[..., 0, 2], -1.0, 1.0))
    c = np.arctan2(Q[..., 0, 1], Q[..., 0, 0])
    return np.stack([a, b, c], axis=-1) * (180 / 3.141592653589793)


class PackResult:
    """a finished (or interrupted) packing: per type the centres in um and the Euler angles in degrees of a .pos file"""

    def __init__(self, plan, positions_um, quaternions, status, seed):
        self.plan = plan
        self.names, self.counts = plan.names, plan.counts
        self.box_um = plan.box_um   # the box that was packed: grid cells / scale, not the requested size
        self.seed = seed
        self.positions, self.angles, self.quaternions = {}, {}, {}
        at = 0
        for name, n in zip(plan.names, plan.counts):
            self.positions[name] = positions_um[at:at + n].copy()
            self.quaternions[name] = quaternions[at:at + n].copy()
            self.angles[name] = euler_angles_deg(quaternions[at:at + n]).reshape(n, 3)
            at += n
        self.steps, self.finished = int(status[0]), bool(status[1])
        self.outer_diameter, self.inner_diameter = float(status[2]), float(status[3])
        self.density, self.nominal_density = float(status[4]), float(status[5])   # Pactual, DensityNominal
        self.force_per_particle = float(status[6])
        self.max_root_evaluations = int(status[10])

    def write_pos(self, directory="."):
        """<name>.pos per type as saveBloodCellPositions writes them (packing.h:617-648): the count, then x y z ax ay az per
        cell, um and degrees.  Returns the paths."""
        import os
        os.makedirs(directory, exist_ok=True)
        paths = []
        for name in self.names:
            path = os.path.join(directory, name + ".pos")
            with open(path, "w") as f:
                f.write("%d\n" % len(self.positions[name]))
                for p, a in zip(self.positions[name], self.angles[name]):
                    f.write(" ".join("%.10g" % v for v in (*p, *a)) + "\n")
            paths.append(path)
        return paths


def read_pos(path):
    """a .pos file: (centres [n][3] in um, angles [n][3] in degrees)"""
    with open(path) as f:
        n = int(f.readline().split()[0])
        rows = np.array([[float(v) for v in f.readline().split()[:6]] for _ in range(n)], dtype=np.float64).reshape(n, 6)
    return rows[:, :3].copy(), rows[:, 3:].copy()


PROGRESS_HEADER = ("\n     Steps     Actual       Nominal        Inner         Outer             Force\n"
                   "              density       density       diameter      diameter       per particle\n")


def progress_line(status):
    """the reference's progress columns (Packing::output, packing.h:516-527)"""
    return "%9d%14.10f%14.10f%14.10f%14.10f%19.15f" % (int(status[0]), status[4], status[5], status[3], status[2], status[6])


def wall_distance_field(mask, periodic, truncation):
    """The packing's wall field on the host, as hc_packing_set_walls builds it on the device: sqrt(min(d^2, R^2)) - 1/2 per
    node, d the exact Euclidean distance in node spacings to the nearest wall node (periodic axes wrap), R = truncation;
    three separable passes min over k of g[k] + (k - j)^2 on integers, along z, y and x in turn.  uint8 mask [nx][ny][nz],
    1 = wall; returns float64 of the same shape, -1/2 on wall nodes."""
    m = np.asarray(mask)
    R = int(truncation)
    far = 1 << 40
    g = np.where(m != 0, 0, far).astype(np.int64)
    for axis in (2, 1, 0):
        n = m.shape[axis]
        best = np.full(m.shape, far, dtype=np.int64)
        for o in range(-R, R + 1):
            if periodic[axis]:
                cand = np.roll(g, -o, axis=axis)   # cand[j] = g[(j + o) mod n]
            else:
                if abs(o) >= n:
                    continue
                cand = np.full(m.shape, far, dtype=np.int64)
                dst = [slice(None)] * 3
                src = [slice(None)] * 3
                dst[axis] = slice(max(0, -o), n - max(0, o))
                src[axis] = slice(max(0, o), n - max(0, -o))
                cand[tuple(dst)] = g[tuple(src)]
            best = np.minimum(best, np.where(cand < far, cand + o * o, far))
        g = best
    return np.sqrt(np.minimum(g, R * R).astype(np.float64)) - 0.5


def _check_walls(mask, mask_dx_um, periodic, size_um):
    """the refusals of a wall mask that need no device, with the messages of hc_packing_set_walls"""
    m = np.asarray(mask)
    if m.ndim != 3 or min(m.shape) < 2:
        raise ValueError("wall_mask must be a three-dimensional array with at least 2 nodes per axis")
    if mask_dx_um is None or not (np.isfinite(mask_dx_um) and mask_dx_um > 0):
        raise ValueError("a wall mask needs its node spacing mask_dx_um")
    periodic = tuple(bool(p) for p in periodic)
    if len(periodic) != 3:
        raise ValueError("periodic must hold one flag per axis")
    for k in range(3):
        if periodic[k]:
            if abs(m.shape[k] * mask_dx_um - size_um[k]) > 1e-9 * size_um[k]:
                raise ValueError("the mask and the box disagree: axis %s is periodic, so its %d nodes x %g um must equal the box's %g um"
                                 % ("xyz"[k], m.shape[k], mask_dx_um, size_um[k]))
            continue
        if (m.shape[k] - 1) * mask_dx_um > size_um[k] * (1 + 1e-9):
            raise ValueError("the mask and the box disagree: the mask is longer than the box along %s" % "xyz"[k])
        faces = np.take(m, [0, m.shape[k] - 1], axis=k)
        if not (faces != 0).all():
            raise ValueError("axis %s is not periodic and has an open face: every node of both of its faces must be wall" % "xyz"[k])
    return np.ascontiguousarray(m != 0, dtype=np.uint8), periodic


def _wall_scale(size_um, periodic, scale0):
    """the sizing factor nearest above scale0 at which every periodic axis is a whole number of grid cells long"""
    axes = [k for k in range(3) if periodic[k]]
    if not axes:
        return scale0
    scale = float(np.ceil(size_um[axes[0]] * scale0 - 1e-9)) / size_um[axes[0]]
    for k in axes[1:]:
        g = size_um[k] * scale
        if abs(g - round(g)) > 1e-9 * g:
            raise ValueError("the periodic axes %s and %s cannot both be a whole number of grid cells long at one sizing factor"
                             % ("xyz"[axes[0]], "xyz"[k]))
    return scale


def wall_plan(size_um, wall_mask, mask_dx_um, periodic, hematocrit=None, plt_ratio=0.07, cells=None, scale=None):
    """what pack_cells decides for a packing inside walls: (plan, mask as uint8, periodic, lumen volume in um^3).  The mask is
    checked against the box, the hematocrit counts cells for the lumen (fluid nodes x mask_dx_um^3), and without a given
    scale the sizing factor is the smallest one above 1.2 / (largest axis) that makes the periodic axes whole grid cells."""
    size_um = [float(s) for s in size_um]
    if len(size_um) != 3 or not all(np.isfinite(s) and s > 0 for s in size_um):
        raise ValueError("size_um must be three positive lengths")
    mask, periodic = _check_walls(wall_mask, mask_dx_um, periodic, size_um)
    volume = float((mask == 0).sum()) * float(mask_dx_um) ** 3
    if volume <= 0:
        raise ValueError("the wall mask has no fluid node")
    if scale is None or scale <= 0.0:
        scale = _wall_scale(size_um, periodic, packing_plan(size_um, hematocrit, plt_ratio, cells, None, volume).scale)
    return packing_plan(size_um, hematocrit, plt_ratio, cells, scale, volume), mask, periodic, volume


def wall_start(plan, mask, mask_dx_um, periodic, margin_um, rng):
    """the initial centres of a packing inside walls, by the rule of pack_cells' docstring: (pos [N][3] in grid cells, the mask's
    spacing and the margin in grid cells)"""
    grid = np.array(plan.grid, dtype=np.float64)
    sizes = plan.sizes_scaled
    n = sum(plan.counts)
    spacing, margin = mask_dx_um * plan.scale, margin_um * plan.scale
    for k in range(3):
        if periodic[k] and abs(mask.shape[k] * spacing - grid[k]) > 1e-9 * grid[k]:
            raise ValueError("the mask and the box disagree: at sizing factor %g the periodic axis %s is %g grid cells long"
                             % (plan.scale, "xyz"[k], mask.shape[k] * spacing))
    douter0 = (float(np.prod(grid)) / (3.141592653589793 / 6.) / n * plan.nominal_fraction) ** (1. / 3.)
    reach = (0.55 * douter0 * float(sizes.max()) + margin) / spacing + 0.5
    wall_s = wall_distance_field(mask, periodic, int(np.ceil(reach)) + 1) * spacing - margin
    pos = np.zeros((n, 3))
    dims = np.array(mask.shape)
    at = 0
    for s, count in enumerate(plan.counts):
        bound = 0.5 * float(sizes[s].min()) * douter0
        if int((wall_s > bound).sum()) < count:
            bound = 0.0
            if not (wall_s > bound).any():
                raise ValueError("no mask node is further than the wall margin from the wall")
        for _ in range(count):
            while True:
                x = rng.random(3) * grid
                node = np.floor(x / spacing + 0.5).astype(np.int64)
                ok = True
                for k in range(3):
                    if periodic[k]:
                        node[k] %= dims[k]
                    elif node[k] > dims[k] - 1:
                        ok = False
                if ok and wall_s[tuple(node)] > bound:
                    break
            pos[at] = x
            at += 1
    return pos, spacing, margin


def pack_cells(size_um, hematocrit=None, plt_ratio=0.07, cells=None, scale=None, rotate=True, max_iter=MAX_ITER_DEFAULT, seed=0,
               steps_per_wait=64, progress=None, wall_mask=None, mask_dx_um=None, periodic=(True, True, True), wall_margin_um=None):
    """Bargiel's force-biased packing of the cell types' enclosing ellipsoids in a periodic box, on the GPU.

    The plan is packing_plan's.  Every ellipsoid starts at a uniform random point of the box, drawn here from
    numpy.random.Generator(PCG64(seed)) in particle order (the reference seeds drand48 with the clock), with the identity
    orientation; the outer diameter shrinks while overlapping pairs push and turn each other (rotate=False: push only), until
    no pair overlaps or max_iter iterations are done.  The device queues steps_per_wait iterations per host wait;
    progress(status) is called after each wait.  Returns a PackResult; see packing_plan for the reference quirks that stay.

    wall_mask (uint8 [nx][ny][nz], 1 = wall, node i at i * mask_dx_um) packs inside walls: a cell near a wall is also pushed
    by its own mirror image across the wall's tangent plane (hc_packing_set_walls).  periodic says which axes wrap; a
    periodic axis must be nodes x mask_dx_um = size_um long, any other needs wall on both faces and the mask inside the box.
    The hematocrit then counts cells for the lumen, fluid nodes x mask_dx_um^3.  With scale=None the sizing factor is raised
    from 1.2 / (largest axis) until the first periodic axis is a whole number of grid cells, so that the packed box is the
    mask's period.  wall_margin_um, default one mask_dx_um, is taken off every wall distance.
    Initial centres with walls: the same PCG64(seed) stream, particle by particle in particle order; a candidate is three
    doubles times the grid, and it is rejected and the next three drawn unless the mask node nearest to it (half up, wrapped
    on periodic axes) has a wall distance, spacing x s_node - margin, above the species' smallest semi-axis at the initial
    outer diameter.  A species with fewer such nodes than cells takes every node with a wall distance above 0 instead."""
    import ctypes as C
    from . import capi, host
    walls = wall_mask is not None
    volume = None
    if walls:
        plan, mask, periodic, volume = wall_plan(size_um, wall_mask, mask_dx_um, periodic, hematocrit, plt_ratio, cells, scale)
        mask_dx_um = float(mask_dx_um)
        margin_um = mask_dx_um if wall_margin_um is None else float(wall_margin_um)
        if not (np.isfinite(margin_um) and margin_um >= 0):
            raise ValueError("wall_margin_um must be finite and not negative")
    else:
        plan = packing_plan(size_um, hematocrit, plt_ratio, cells, scale)
    n = sum(plan.counts)
    if n == 0:
        raise ValueError("no cells to pack")
    if max_iter < 0 or steps_per_wait < 1:
        raise ValueError("max_iter must be >= 0 and steps_per_wait >= 1")
    grid = np.array(plan.grid, dtype=np.int32)
    sizes = np.ascontiguousarray(plan.sizes_scaled)
    counts = np.array(plan.counts, dtype=np.int32)
    rng = np.random.Generator(np.random.PCG64(seed))
    if walls:
        pos, spacing, margin = wall_start(plan, mask, mask_dx_um, periodic, margin_um, rng)
    else:
        pos = np.ascontiguousarray(rng.random((n, 3)) * grid.astype(np.float64))
    host.ensure_init()
    lib = capi.lib()
    ip = C.POINTER(C.c_int)
    handle = C.c_void_p()
    capi.check(lib.hc_packing_create(C.byref(handle), grid.ctypes.data_as(ip), len(counts), capi.dptr(sizes), counts.ctypes.data_as(ip),
                                     capi.dptr(pos), None, plan.nominal_fraction, int(bool(rotate)), 0, 0.0))
    try:
        if walls:
            dims32 = np.array(mask.shape, dtype=np.int32)
            per32 = np.array([int(p) for p in periodic], dtype=np.int32)
            capi.check(lib.hc_packing_set_walls(handle, mask.ctypes.data, dims32.ctypes.data_as(ip), spacing, per32.ctypes.data_as(ip), margin))
        status = np.zeros(12)
        capi.check(lib.hc_packing_run(handle, 0, capi.dptr(status)))
        while not status[1] and int(status[0]) < max_iter:
            capi.check(lib.hc_packing_run(handle, int(min(steps_per_wait, max_iter - int(status[0]))), capi.dptr(status)))
            if progress is not None:
                progress(status)
        quat = np.zeros((n, 4))
        capi.check(lib.hc_packing_state(handle, capi.dptr(pos), capi.dptr(quat), None, None))
    finally:
        lib.hc_packing_destroy(handle)
    res = PackResult(plan, pos * (1. / plan.scale), quat, status, seed)
    res.lumen_volume_um3 = volume   # None without walls
    return res


def pipe_mask(length_um, radius_um, dx_um=0.5, axis=0):
    """uint8 wall mask of a straight pipe along axis: round(length / dx) nodes along it, 2 ceil(radius / dx) + 3 across, fluid
    where a node lies closer than radius / dx nodes to the centre line, so that both cross faces are wall"""
    if axis not in (0, 1, 2):
        raise ValueError("axis must be 0, 1 or 2")
    if not (dx_um > 0 and radius_um > dx_um and length_um >= 2 * dx_um):
        raise ValueError("a pipe needs dx_um > 0, a radius above dx_um and a length of at least two nodes")
    n_len = int(round(length_um / dx_um))
    if abs(n_len * dx_um - length_um) > 1e-9 * length_um:
        raise ValueError("the pipe's length must be a whole number of dx_um, as it is periodic")
    n_cross = 2 * int(np.ceil(radius_um / dx_um)) + 3
    c = (n_cross - 1) / 2.0
    a = np.arange(n_cross) - c
    wall2d = (np.hypot(a[:, None], a[None, :]) >= radius_um / dx_um).astype(np.uint8)
    mask = np.repeat(wall2d[None, :, :], n_len, axis=0)
    return np.ascontiguousarray(np.moveaxis(mask, 0, axis))


def pack_pipe(length_um, radius_um, hematocrit, dx_um=0.5, axis=0, plt_ratio=0.07, cells=None, rotate=True, max_iter=MAX_ITER_DEFAULT,
              seed=0, steps_per_wait=64, progress=None, wall_margin_um=None):
    """pack_cells inside pipe_mask(length_um, radius_um, dx_um, axis): periodic along axis, walls all round.  The box is the
    mask's, (nodes - 1) dx_um across; the result carries the mask as .wall_mask and its spacing as .mask_dx_um."""
    mask = pipe_mask(length_um, radius_um, dx_um, axis)
    size = [(n - 1) * dx_um for n in mask.shape]
    size[axis] = mask.shape[axis] * dx_um
    periodic = tuple(k == axis for k in range(3))
    res = pack_cells(size, hematocrit, plt_ratio, cells, None, rotate=rotate, max_iter=max_iter, seed=seed, steps_per_wait=steps_per_wait,
                     progress=progress, wall_mask=mask, mask_dx_um=dx_um, periodic=periodic, wall_margin_um=wall_margin_um)
    res.wall_mask, res.mask_dx_um, res.periodic = mask, float(dx_um), periodic
    return res


def _main(argv=None):
    """python -m hemocell_amd.packing sX sY sZ [...]: the options of tools/packCells, and --seed"""
    import argparse
    import sys
    usage = ("USAGE: python -m hemocell_amd.packing sX sY sZ [OPTIONAL ARGUMENTS ...]\n"
             "\n"
             "OPTIONAL ARGUMENTS:\n"
             "  --hematocrit <0-1.0>                 -h Hematocrit of the suspension (human blood only)\n"
             "  --plt_ratio <ratio>                     Platelets per red blood cell, default=0.07\n"
             "  --rbc <n>                               Number of red blood cells\n"
             "  --plt <n>                               Number of platelets\n"
             "  --rbc_m <n>                             Number of mouse red blood cells\n"
             "  --plt_m <n>                             Number of mouse wild-type platelets\n"
             "  --plt_mko <n>                           Number of mouse knockout platelets\n"
             "  --wbc <n>                               Number of white blood cells\n"
             "  --vrbc <n>                              Number of stage V gametocytes\n"
             "  --cell <name> <n> <e1> <e2> <diameter>  Custom cell type given by its ellipsoid\n"
             "  --noRotate                              Keep the ellipsoids' orientations fixed\n"
             "  --scale <ratio>                      -s Scale of the neighbourhood grid (expert use)\n"
             "  --maxiter <n>                           Maximum number of iterations\n"
             "  --seed <n>                              Seed of the initial positions, default=0\n"
             "  --outdir <dir>                          Directory the .pos files go to, default=.\n"
             "  --pipe <radius>                         Pack a pipe of this radius [um] along x, sX long and periodic\n"
             "                                          (sY and sZ are replaced by the pipe's cross-section)\n"
             "  --mask <file.npy>                       Pack inside this wall mask, uint8 [nx][ny][nz], 1 = wall\n"
             "  --mask-dx <um>                          Node spacing of the mask (and of --pipe, default=0.5)\n"
             "  --periodic <axes>                       Periodic axes of the mask, e.g. x or xyz, default=xyz\n"
             "  --wall-margin <um>                      Taken off every wall distance, default=one node spacing\n"
             "  --help                                  Print this\n"
             "OUTPUT:\n"
             "  <Cell>.pos for every cell type. The first line holds the number of cells,\n"
             "  every other line one cell as \"Location<X Y Z> Rotation<X Y Z>\".\n"
             "NOTE:\n"
             "  sX, sY, sZ and the output are in [um], not in lattice units\n"
             "  --hematocrit excludes --rbc and --plt\n"
             "  --plt_ratio needs --hematocrit\n")
    ap = argparse.ArgumentParser(prog="python -m hemocell_amd.packing", add_help=False, allow_abbrev=False)
    ap.add_argument("size", nargs="*")
    ap.add_argument("--hematocrit", "-h", type=float)
    ap.add_argument("--plt_ratio", type=float, default=0.07)
    named = (("rbc", "RBC"), ("plt", "PLT"), ("wbc", "WBC"), ("vrbc", "vRBC"), ("rbc_m", "RBC_m"), ("plt_m", "PLT_m"), ("plt_mko", "PLT_mko"))
    order = []

    class Named(argparse.Action):
        def __call__(self, parser, ns, values, option_string=None):
            order.append((dict(named)[self.dest], int(values)))

    class Custom(argparse.Action):
        def __call__(self, parser, ns, values, option_string=None):
            order.append((values[0], int(values[1]), tuple(float(v) for v in values[2:5])))

    for opt, _ in named:
        ap.add_argument("--" + opt, action=Named)
    ap.add_argument("--cell", nargs=5, action=Custom)
    ap.add_argument("--noRotate", action="store_true")
    ap.add_argument("--scale", "-s", type=float)
    ap.add_argument("--maxiter", type=int, default=MAX_ITER_DEFAULT)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--help", action="store_true")
    ap.add_argument("--outdir", default=".")
    ap.add_argument("--pipe", type=float)
    ap.add_argument("--mask")
    ap.add_argument("--mask-dx", dest="mask_dx", type=float, default=0.5)
    ap.add_argument("--periodic", default="xyz")
    ap.add_argument("--wall-margin", dest="wall_margin", type=float)
    ap.error = lambda msg: (sys.stderr.write(msg + "\n\n" + usage), sys.exit(1))
    a = ap.parse_args(argv)
    if a.help:
        sys.stderr.write(usage)
        return 1
    if len(a.size) != 3:
        print("Insufficient arguments.\n")
        sys.stderr.write(usage)
        return 1
    size = [int(float(s)) for s in a.size]   # atoi, packCells.cpp:193-195
    mask, periodic = None, (True, True, True)
    try:
        if a.pipe is not None and a.mask is not None:
            raise ValueError("--pipe excludes --mask")
        if a.pipe is not None:
            mask, periodic = pipe_mask(size[0], a.pipe, a.mask_dx, 0), (True, False, False)
            size = [size[0], (mask.shape[1] - 1) * a.mask_dx, (mask.shape[2] - 1) * a.mask_dx]
        elif a.mask is not None:
            mask, periodic = np.load(a.mask), tuple(c in a.periodic.lower() for c in "xyz")
        if mask is not None:
            plan = wall_plan(size, mask, a.mask_dx, periodic, a.hematocrit, a.plt_ratio, order, a.scale)[0]
        else:
            plan = packing_plan(size, a.hematocrit, a.plt_ratio, order, a.scale)
    except (ValueError, OSError) as e:
        sys.stderr.write("%s, exiting...\n" % e)
        sys.stderr.write(usage)
        return 1
    print("Parameters:")
    print("  Domain Size [um]: ( %g , %g , %g )" % tuple(size) if mask is not None else "  Domain Size [um]: ( %d , %d , %d )" % tuple(size))
    print("  Maximum Iterations : %d" % a.maxiter)
    print("  Scale              : %.6f" % plan.scale)
    print("  Rotation           : %d" % (not a.noRotate))
    print("  Seed               : %d" % a.seed)
    if a.hematocrit is not None:
        print("  Hematocrit    : %.6f" % a.hematocrit)
        print("  PLT/RBC Ratio : %.6f" % a.plt_ratio)
    print("The following cell types are defined:")
    for name, n, dims in zip(plan.names, plan.counts, plan.sizes_um):
        print("  %s\n    No   : %d\n    Sizes: (%.6f , %.6f , %.6f )" % (name, n, dims[0], dims[1], dims[2]))
        print("    Volume: %.6f [um3]." % (4.0 / 3.0 * 3.141592653589793 * dims[0] * dims[1] * dims[2] / 8.0))
    print("\nSizing parameter: %.6f" % plan.scale)
    print("Resolution of collision check: %d x %d x %d" % plan.grid)
    print("Packed box [um]: %.6f x %.6f x %.6f" % plan.box_um)
    print("\nNominal requested volume fraction: %.6f" % plan.nominal_fraction)
    if plan.warning:
        print("*** WARNING ***\n" + plan.warning)
    if mask is not None:
        print("Walls: mask %d x %d x %d nodes at %g um, periodic in %s" % (mask.shape + (a.mask_dx, "".join(c for c, p in zip("xyz", periodic) if p) or "-")))
    print(PROGRESS_HEADER)
    res = pack_cells(size, a.hematocrit, a.plt_ratio, order, a.scale, rotate=not a.noRotate, max_iter=a.maxiter, seed=a.seed,
                     progress=lambda st: print(progress_line(st), flush=True), wall_mask=mask, mask_dx_um=a.mask_dx if mask is not None else None,
                     periodic=periodic, wall_margin_um=a.wall_margin)
    if not res.finished:
        print("WARNING: Force-free packing was NOT achieved! Potential overlaps might still exist.")
    print(" PACKING DONE " if res.finished else " PACKING TERMINATED(!) ")
    res.write_pos(a.outdir)
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(_main())
