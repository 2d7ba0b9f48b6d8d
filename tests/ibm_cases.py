"""Crafted geometries for the per-cell IBM kernels (tests/test_gpu_ibm_edges.py, tests/test_ibm_ref_cpu.py).

A "cell" here is nv vertices wherever the case puts them: the membrane is never evaluated, forces are random values.
build(name, f_limit) returns a dict:
  dims, periodic, mask ([nx][ny][nz] uint8 or None), seat (a centre at which a whole cell of any type fits, for hosts that
  check the placement), counts {type name: cells} (types in the order of TYPES), pos / force [n][3] (types in order, cells in
  order, vertices in order), alive [n] bool, kill_pos (None, or the positions at which the particles with alive == False
  are first put so that advanceParticles removes them: on a boundary node), limit (FORCE_LIMIT on), body (uniform body
  force), controls (the wrong= restatements of tests/ibm_ref.py the case must tell from the right one), expect
  {cell index: {key of ibm_ref.predict: value, or 'tiled': bool, or 'vol_all_gt': bound on the volume with the removed
  particles counted}}, open (None, or the Zou-He planes of the lattice: dict(patches=[(kind, box, values)], code [nx][ny][nz],
  val [slots][4]) in the conventions of tests/open_boundary_ref.py).

TILE_CAP, NODE_CAP, NVPT and the x padding are the constants of hemocell_amd/csrc/ibm_common.h and common.h
(tests/test_ibm_ref_cpu.py checks the copies): a case sits where it claims to only as long as they hold.
"""
import zlib

import numpy as np

K = 22.44                # constant of the conditioned bound |gpu - ref| <= K 2^-53 abs: four times the measured rounding figure 5.61
                         # of the plain double restatement (tests/test_ibm_ref_cpu.py::test_rounding_figure_behind_k)
TILE_CAP = 5832
NODE_CAP = 1536
NVPT = 3
HALO = 2
TYPES = ("rbc", "plt", "big")
NV = dict(rbc=642, plt=66, big=2562)            # RBC_FROM_SPHERE at 600 / ELLIPSOID at 66 / RBC_FROM_SPHERE at 1300 triangles
BIG_MIN_TRIANGLES = 1300
BLOCK = dict(rbc=256, plt=128, big=256)         # threads of a per-cell workgroup: nv > 128 ? 256 : 128

BOX = dict(dims=(48, 48, 48), periodic=(1, 1, 1))
SEAM = dict(dims=(24, 16, 20), periodic=(1, 1, 1))
BRICK = dict(dims=(24, 8, 528), periodic=(1, 1, 1))     # padded x 8..23 (x 6..21) lies in bricks that touch no face
PIPE = dict(dims=(40, 22, 22), periodic=(1, 0, 0))


def pipe_mask(nx, ny, nz):
    """cylinder along x, radius (ny - 2) / 2 about ((ny - 1) / 2, (nz - 1) / 2): solid beyond it"""
    y = np.arange(ny)[:, None] - (ny - 1) / 2.0
    z = np.arange(nz)[None, :] - (nz - 1) / 2.0
    R = (ny - 2) / 2.0
    return np.ascontiguousarray(np.broadcast_to(((y * y + z * z) > R * R)[None], (nx, ny, nz)).astype(np.uint8))


def _fill(rng, bases, nv, lo=0.2, hi=0.8):
    """nv vertices; vertex i lies inside the unit cube above bases[i % len], away from its faces: all 8 weights non-zero"""
    assert len(bases) <= nv, "every base needs a vertex"
    b = np.asarray(bases, dtype=np.float64)[np.arange(nv) % len(bases)]
    return b + rng.uniform(lo, hi, size=(nv, 3))


def _box_bases(rng, o, e, m=100):
    """distinct bases whose stencils span exactly the box of origin o and extents e: its 8 corners and up to m inside"""
    o, e = np.array(o), np.array(e)
    corners = np.array([o + (e - 2) * np.array(c) for c in np.ndindex(2, 2, 2)])
    inner = o + rng.integers(0, e - 1, size=(m, 3))
    return np.unique(np.vstack([corners, inner]), axis=0)


def _cell(rng, kind, o, e, m=100):
    """one cell of the type whose stencils span exactly the box (o, e)"""
    return (kind, _fill(rng, _box_bases(rng, o, e, min(m, NV[kind] - 8)), NV[kind]))


def _forces(rng, n, f_limit):
    d = rng.standard_normal((n, 3))
    d /= np.sqrt((d * d).sum(axis=1))[:, None]
    return d * (f_limit * rng.uniform(0.05, 0.9, size=n))[:, None]


def _case(name, f_limit, lattice, cells, mask=None, seat=None, controls=("shift_z",), expect=None, alive=None, kill_pos=None,
          force=None, open_planes=None):
    """cells: [(type name, positions [nv][3])] in any order; stored type by type"""
    rng = np.random.default_rng(zlib.crc32(("f" + name).encode()))
    counts = {t: sum(1 for k, _ in cells if k == t) for t in TYPES}
    order = sorted(range(len(cells)), key=lambda i: (TYPES.index(cells[i][0]), i))
    assert order == list(range(len(cells))), "list the cells type by type"
    for k, p in cells:
        assert p.shape == (NV[k], 3), (name, k, p.shape)
    pos = np.ascontiguousarray(np.vstack([p for _, p in cells]))
    n = len(pos)
    dims = lattice["dims"]
    return dict(name=name, dims=dims, periodic=lattice["periodic"], mask=mask, seat=seat or tuple(d / 2.0 for d in dims),
                counts=counts, kinds=[k for k, _ in cells], pos=pos, force=_forces(rng, n, f_limit) if force is None else force,
                alive=np.ones(n, bool) if alive is None else alive, kill_pos=kill_pos, limit=True, body=(3e-6, -2e-6, 1e-6),
                controls=tuple(controls), expect=expect or {}, open=open_planes)


def cell_slices(case):
    out, o = [], 0
    for k in case["kinds"]:
        out.append(slice(o, o + NV[k])); o += NV[k]
    return out


# ----------------------------------------------------------------------------------------------------------------------
def _tile(name, e, kind, tiled):
    def b(rng, fl):
        o = (-30, -29, -28)      # negative coordinates: the box wraps to (18, 19, 20) without crossing a face
        return _case(name, fl, BOX, [_cell(rng, kind, o, e)], controls=("shift_z", "truncate"),
                     expect={0: dict(e=e, vol=int(np.prod(e)), tiled=tiled, wraps=(False, False, False))})
    return b


def _node_cap(name, blocks, singles, nodes, tiled):
    def b(rng, fl):
        o = np.array((-40, 7, 11))
        grid = np.array([(i, j, k) for k in range(3) for j in range(8) for i in range(8)])[:blocks]     # disjoint 2 x 2 x 2 blocks
        p = _fill(rng, o + 2 * grid, NV["rbc"])
        free = o + 2 * np.array((7, 7, 2)) if blocks < 192 else o + np.array((0, 0, 6))                 # an unused block
        spots = [d for d in np.ndindex(2, 2, 2)][:singles]
        for s, d in enumerate(spots):        # exactly on a node: phi2(+-1) = 0, one node admitted
            p[len(grid) + s] = free + np.array(d)
        return _case(name, fl, BOX, [("rbc", p)], controls=("shift_z", "truncate"), expect={0: dict(nodes=nodes, tiled=tiled)})
    return b


def _thin(name, dims, e, o, kind, tiled, wraps=None, exceeds=False):
    def b(rng, fl):
        ex = {0: dict(e=e, vol=int(np.prod(e)), tiled=tiled, exceeds=exceeds)}
        if wraps is not None:
            ex[0]["wraps"] = wraps
        return _case(name, fl, dict(dims=dims, periodic=(1, 1, 1)), [_cell(rng, kind, o, e, 50)], expect=ex)
    return b


def _brick(name, o, e, kind, bricks, wall=None, controls=("shift_z",)):
    def b(rng, fl):
        mask = None
        if wall is not None:
            mask = np.zeros(BRICK["dims"], np.uint8); mask[wall] = 1
        return _case(name, fl, BRICK, [_cell(rng, kind, o, e, 40)], mask=mask, seat=(12.0, 4.0, 260.0),
                     controls=controls, expect={0: dict(e=e, bricks=bricks, tiled=True, wraps=(False, False, False))})
    return b


def _seam(name, o, wraps, kind, controls=("shift_z",)):
    def b(rng, fl):
        e = (6, 7, 5)
        return _case(name, fl, SEAM, [_cell(rng, kind, o, e, 30)], controls=controls,
                     expect={0: dict(e=e, wraps=wraps, tiled=True)})
    return b


def _faces(rng, fl):
    """no walls, no periodic axis: one small cell within half a node of each face, one at a corner, one in the middle"""
    dims = (20, 16, 12)
    cells = []
    for axis in range(3):
        for side in (0, 1):
            c = np.array([9.0, 7.0, 5.0]); c[axis] = 0.0 if side == 0 else dims[axis] - 1.0
            p = c + rng.uniform(-2.4, 2.4, size=(NV["plt"], 3))
            p[:, axis] = c[axis] + rng.uniform(-0.45, 0.45, size=NV["plt"])
            cells.append(("plt", p))
    corner = np.array([dims[0] - 1.0, 0.0, dims[2] - 1.0]) + rng.uniform(-0.45, 0.45, size=(NV["plt"], 3))
    cells.append(("plt", corner))
    mid = _cell(rng, "rbc", (6, 4, 3), (8, 8, 6), 60)
    ex = {i + 1: dict(leaves=True, tiled=True) for i in range(7)}
    ex[0] = dict(leaves=False, tiled=True)
    return _case("faces_open", fl, dict(dims=dims, periodic=(0, 0, 0)), [mid] + cells, controls=("no_renormalise",), expect=ex)


def _faces_zou_he(rng, fl):
    """a channel (bounce-back on the y and z faces) with a Zou-He velocity plane at x = 0 and a pressure plane at x = nx - 1: cells
    within half a node of either plane, in mid-channel and in the corners next to the walls, and one cell inside"""
    dims = (24, 17, 19)
    nx, ny, nz = dims
    mask = np.zeros(dims, np.uint8)
    mask[:, 0, :] = mask[:, -1, :] = 1
    mask[:, :, 0] = mask[:, :, -1] = 1
    y = (np.arange(ny) - (ny - 1) / 2.0) / ((ny - 2) / 2.0)
    z = (np.arange(nz) - (nz - 1) / 2.0) / ((nz - 2) / 2.0)
    g = (np.clip(1 - y[:, None] ** 2, 0, None) * np.clip(1 - z[None, :] ** 2, 0, None)).reshape(-1)
    vel = np.stack([0.02 * g, 0.002 * g, -0.001 * g], axis=1)
    rho = 1.0 + rng.uniform(-0.01, 0.01, ny * nz)
    code = -np.ones(dims, np.int64)
    code[0] = (np.arange(ny * nz) << 2 | 0).reshape(ny, nz)                    # VEL_0N, slots 0 .. ny nz - 1
    code[nx - 1] = ((ny * nz + np.arange(ny * nz)) << 2 | 3).reshape(ny, nz)    # PRES_0P, the next ny nz slots
    val = np.zeros((2 * ny * nz, 4)); val[:ny * nz, :3] = vel; val[:ny * nz, 3] = 1.0; val[ny * nz:, 3] = rho
    patches = [(0, (0, 0, 0, ny - 1, 0, nz - 1), vel), (3, (nx - 1, nx - 1, 0, ny - 1, 0, nz - 1), rho)]
    cells = []
    for x in (0.0, nx - 1.0):
        p = np.array([x, 8.0, 9.0]) + rng.uniform(-2.4, 2.4, size=(NV["plt"], 3))
        p[:, 0] = x + rng.uniform(-0.45, 0.45, size=NV["plt"])
        cells.append(("plt", p))
    for c in ((0.0, 1.0, 1.0), (nx - 1.0, ny - 2.0, nz - 2.0), (0.0, ny - 2.0, 1.0)):   # next to the walls: y, z in (0.55, 1.45) off the face
        cells.append(("plt", np.array(c) + rng.uniform(-0.45, 0.45, size=(NV["plt"], 3))))
    mid = _cell(rng, "rbc", (8, 5, 6), (8, 7, 6), 60)
    ex = {i + 1: dict(leaves=True, tiled=True) for i in range(5)}
    ex[0] = dict(leaves=False, tiled=True)
    return _case("faces_zou_he", fl, dict(dims=dims, periodic=(0, 0, 0)), [mid] + cells, mask=mask, seat=(12.0, 8.0, 9.0),
                 controls=("no_renormalise", "admit_walls"), expect=ex, open_planes=dict(patches=patches, code=code, val=val))


def _exact(rng, fl):
    """on nodes, on half-integers (the tie of floor(p + 0.5)), and the doubles next to both, at positive and negative
    coordinates (|p| >= 1: the differences p - node are exact)"""
    special = []
    for s in (5.0, 5.5, -3.0, -3.5):
        special += [s, np.nextafter(s, np.inf), np.nextafter(s, -np.inf)]
    p = np.array([6.0, 4.0, 7.0]) + rng.uniform(0.2, 0.8, size=(NV["plt"], 3))
    i = 0
    for axis in range(3):
        for s in special:
            p[i, axis] = s; i += 1
    for s in special:                      # special on all three axes at once
        p[i] = (s, s, s); i += 1
    assert i <= NV["plt"]
    return _case("exact_positions", fl, SEAM, [("plt", p)], controls=("shift_z", "truncate"), expect={0: dict(tiled=True)})


def _walls(rng, fl):
    """cell 0: one vertex with 7 of its 8 nodes masked; cell 1: one vertex with exactly one node masked"""
    mask = np.zeros(SEAM["dims"], np.uint8)
    b0, b1 = np.array((8, 5, 6)), np.array((15, 9, 12))
    for d in np.ndindex(2, 2, 2):
        if d != (1, 0, 1):
            mask[tuple(b0 + d)] = 1
    mask[tuple(b1 + (0, 1, 1))] = 1
    cells = []
    for b in (b0, b1):
        others = np.array([b + (3, 0, 0), b + (0, 3, 0), b + (0, 0, 3), b + (3, 3, 0), b + (-3, 0, 2), b + (2, -3, 0)])
        cells.append(("plt", _fill(rng, np.vstack([b[None], others]), NV["plt"])))
    return _case("walls_7_and_1_of_8", fl, SEAM, cells, mask=mask, seat=(12.0, 13.0, 3.0), controls=("admit_walls", "no_renormalise"),
                 expect={0: dict(tiled=True), 1: dict(tiled=True)})


def _near_wall(rng, mask, dims, x0, x1, want):
    """positions in the pipe between x0 and x1 whose stencil holds both a fluid and a boundary node"""
    out = []
    R, cy, cz = (dims[1] - 2) / 2.0, (dims[1] - 1) / 2.0, (dims[2] - 1) / 2.0
    while len(out) < want:
        a, r = rng.uniform(0.3, 1.2), R - rng.uniform(0.3, 1.6)
        p = np.array([rng.uniform(x0, x1), cy + r * np.cos(a), cz + r * np.sin(a)])
        b = np.floor(p).astype(int)
        m = mask[b[0] % dims[0], b[1]:b[1] + 2, b[2]:b[2] + 2]
        if m.any() and not m.all():
            out.append(p)
    return np.array(out)


def _pipe_hug(rng, fl):
    mask = pipe_mask(*PIPE["dims"])
    p = _near_wall(rng, mask, PIPE["dims"], 37.0, 43.0, NV["rbc"])       # across the periodic x face as well
    return _case("pipe_wall_hug", fl, PIPE, [("rbc", p)], mask=mask, seat=(20.0, 10.5, 10.5), controls=("admit_walls", "no_renormalise"),
                 expect={0: dict(tiled=True, wraps=(True, False, False))})


def _lanes(n):
    def b(rng, fl):
        slots = [(6 + 12 * i, 6 + 12 * j, 6 + 12 * k) for i in range(4) for j in range(4) for k in range(4)]
        rng.shuffle(slots)
        cells = []
        for c in range(2 * n):
            kind = "rbc" if c < n else "plt"
            o = np.array(slots[c]) + rng.integers(-3, 3, size=3)
            cells.append(_cell(rng, kind, o, (5, 6, 7), 20))
        return _case("lanes_%d" % n, fl, BOX, cells, expect={c: dict(tiled=True) for c in range(2 * n)})
    return b


def _big(rng, fl):
    p = _fill(rng, _box_bases(rng, (20, 10, -4), (8, 9, 7), 40), NV["big"])
    return _case("big_mesh", fl, BOX, [("big", p)], expect={0: dict(tiled=False, wraps=(False, False, True))})


def _dead(rng, fl):
    """cell 0 loses 40 particles, among them the first and last of the cell and both sides of a 256-thread stride; their stored
    positions are then spread over the pipe, where they would take the box past TILE_CAP; cell 1 is complete; cell 2, a
    platelet, has lost every particle (no live vertex in its workgroup: block_bbox has nothing to reduce)"""
    mask = pipe_mask(*PIPE["dims"])
    live0 = _fill(rng, _box_bases(rng, (8, 8, 8), (6, 6, 6), 30), NV["rbc"])
    gone = np.unique(np.r_[0, 255, 256, 511, 512, 641, rng.choice(NV["rbc"], 34, replace=False)])
    alive = np.ones(2 * NV["rbc"], bool); alive[gone] = False
    p0 = live0.copy()
    far = np.array([[4.0, 4.5, 10.0], [36.0, 17.0, 10.0], [20.0, 10.0, 4.0], [20.0, 10.0, 17.0]])
    p0[gone] = far[np.arange(len(gone)) % 4] + rng.uniform(0.2, 0.8, size=(len(gone), 3))
    p1 = _fill(rng, _box_bases(rng, (15, 9, 7), (6, 6, 6), 30), NV["rbc"])
    p2 = _fill(rng, _box_bases(rng, (24, 8, 9), (5, 5, 5), 20), NV["plt"])                  # a platelet that lost every particle
    gone = np.r_[gone, 2 * NV["rbc"] + np.arange(NV["plt"])]
    alive = np.r_[alive, np.zeros(NV["plt"], bool)]
    pos = np.vstack([p0, p1, p2])
    kill = pos.copy()
    kill[gone] = np.array([5.0, 0.0, 0.0]) + rng.uniform(-0.3, 0.3, size=(len(gone), 3))     # nearest node: the solid corner
    f = _forces(rng, len(pos), fl)
    f[gone[:3]] *= 5.0 * fl / np.sqrt((f[gone[:3]] ** 2).sum(axis=1))[:, None]     # removed and above the limit: not capped either
    c = _case("dead_vertices", fl, PIPE, [("rbc", p0), ("rbc", p1), ("plt", p2)], mask=mask, seat=(20.0, 10.5, 10.5), controls=("dead_take_part",),
              alive=alive, kill_pos=kill, force=f, expect={0: dict(e=(6, 6, 6), tiled=True, vol_all_gt=TILE_CAP), 1: dict(tiled=True)})
    return c


def _force_cap(rng, fl):
    cells = [_cell(rng, "rbc", (5, 6, 7), (6, 6, 6), 30),
             _cell(rng, "plt", (14, 3, 12), (5, 5, 5), 20)]
    n = NV["rbc"] + NV["plt"]
    f = _forces(rng, n, fl)
    for i, s in ((0, 1.5), (255, 10.0), (256, 1e3), (641, 2.0), (642, 3.0), (n - 1, 1.0 + 1e-9)):
        f[i] *= s * fl / np.sqrt((f[i] * f[i]).sum())
    f[300] = (fl, 0.0, 0.0)                              # exactly at the limit: stays
    f[301] = (0.0, -fl * (1.0 - 1e-9), 0.0)              # just below: stays
    return _case("force_cap", fl, SEAM, cells, controls=("no_cap",), force=f, expect={0: dict(tiled=True), 1: dict(tiled=True)})


BUILDERS = {
    "tile_18_18_18": _tile("tile_18_18_18", (18, 18, 18), "rbc", True),
    "tile_19_18_17": _tile("tile_19_18_17", (19, 18, 17), "plt", True),
    "tile_18_18_19": _tile("tile_18_18_19", (18, 18, 19), "rbc", False),
    "nodes_1535": _node_cap("nodes_1535", 191, 7, 1535, True),
    "nodes_1536": _node_cap("nodes_1536", 192, 0, 1536, True),
    "nodes_1537": _node_cap("nodes_1537", 192, 1, 1537, False),
    "thin_2_2_1458": _thin("thin_2_2_1458", (4, 4, 1460), (2, 2, 1458), (1, 1, 1), "plt", True, (False, False, False)),
    "thin_2_1458_2": _thin("thin_2_1458_2", (4, 1460, 4), (2, 1458, 2), (1, 1, 1), "rbc", True, (False, False, False)),
    "thin_1458_2_2": _thin("thin_1458_2_2", (1460, 4, 4), (1458, 2, 2), (1, 1, 1), "rbc", True, (False, False, False)),
    "thin_3_2_972": _thin("thin_3_2_972", (4, 4, 1460), (3, 2, 972), (0, 1, 200), "plt", True, (False, False, False)),
    "thin_2_3_972_seam": _thin("thin_2_3_972_seam", (4, 4, 1460), (2, 3, 972), (1, 0, 1000), "rbc", True, (False, False, True)),
    "thin_whole_axis": _thin("thin_whole_axis", (4, 4, 1458), (2, 2, 1458), (1, 1, 700), "rbc", True, (False, False, True)),
    "thin_axis_plus_one": _thin("thin_axis_plus_one", (4, 4, 1457), (2, 2, 1458), (1, 1, 700), "plt", False, None, True),
    "bricks_64": _brick("bricks_64", (8, 2, 0), (2, 2, 512), "rbc", 64),
    "bricks_65": _brick("bricks_65", (8, 2, 0), (2, 2, 513), "plt", 65),
    "bricks_lane_63_wall": _brick("bricks_lane_63_wall", (8, 2, 0), (2, 2, 512), "rbc", 64, wall=(8, 2, 511), controls=("admit_walls", "no_renormalise")),
    "brick_wall_next_door": _brick("brick_wall_next_door", (8, 2, 2), (2, 2, 6), "plt", 1, wall=(8, 2, 8)),
    "brick_ends_on_8": _brick("brick_ends_on_8", (8, 2, 3), (2, 2, 6), "plt", 2, wall=(8, 2, 8), controls=("admit_walls", "no_renormalise")),
    "seam_x": _seam("seam_x", (21, 5, 7), (True, False, False), "rbc"),
    "seam_y": _seam("seam_y", (9, 12, 7), (False, True, False), "plt"),
    "seam_z": _seam("seam_z", (9, 5, 17), (False, False, True), "rbc"),
    "seam_yz": _seam("seam_yz", (9, 12, 17), (False, True, True), "rbc"),
    "seam_xyz": _seam("seam_xyz", (21, 12, 17), (True, True, True), "plt"),
    "seam_negative": _seam("seam_negative", (-3, -4, -2), (True, True, True), "rbc", controls=("shift_z", "truncate")),
    "seam_far": _seam("seam_far", (2 * 24 + 21, -3 * 16 + 12, 20 + 17), (True, True, True), "rbc", controls=("shift_z", "truncate")),
    "faces_open": _faces,
    "faces_zou_he": _faces_zou_he,
    "exact_positions": _exact,
    "walls_7_and_1_of_8": _walls,
    "pipe_wall_hug": _pipe_hug,
    "big_mesh": _big,
    "dead_vertices": _dead,
    "force_cap": _force_cap,
}
for _n in (1, 7, 8, 9, 16, 17, 23):
    BUILDERS["lanes_%d" % _n] = _lanes(_n)
NAMES = list(BUILDERS)
_cache = {}


def build(name, f_limit):
    key = (name, float(f_limit))
    if key not in _cache:
        _cache[key] = BUILDERS[name](np.random.default_rng(zlib.crc32(name.encode())), float(f_limit))
    return _cache[key]
