"""Geometries for the lattice's geometry bookkeeping and a numpy restatement of its rule -- test infrastructure only.

hcl_set_mask (hemocell_amd/csrc/lattice.hip) turns a bounce-back mask into node classes and an active-span map, and every
lattice kernel rides on the two:

* a solid node none of whose 18 D3Q19 neighbours is fluid is INERT (class 2): full-way bounce-back returns every population to
  where it came from, so the collide neither loads nor stores it.  Neighbours wrap on periodic y / z axes and do not exist
  beyond a non-periodic y / z face; in x they are looked up in the slab's HALO halo planes, which Lattice.defineBounceBack
  fills with the wrapped planes of a periodic lattice and with wall otherwise; a neighbour beyond the outer halo plane is
  unknown, and the node then stays active;
* an inert node that shares a 128-byte line -- 16 consecutive nodes of the slab's padded numbering -- with a node that is not
  inert goes back to class 1 (PROMOTION), so that a line of a population array is written completely or not at all;
* per x-plane every row of nz nodes keeps one span [z0, z1) that leaves out its leading and trailing inert nodes, thread t of
  a plane serves the t-th node of the concatenated spans, and every 256-thread block finds its rows by a search in that map.

classes() restates the first two as a specification (shifted arrays, no node loop) and span_report() describes the third.  The
geometries below are the smallest found that still hold the properties tests/test_lattice_geometry_cpu.py proves for them; the
GPU tests of tests/test_gpu_lattice_geometry.py rest on those properties.
"""
import numpy as np

HALO = 2
LINE = 16      # doubles of one 128-byte line
BLOCK = 256    # threads of one collide block

T19 = [1 / 3] + [1 / 18] * 3 + [1 / 36] * 6 + [1 / 18] * 3 + [1 / 36] * 6


def O_T():
    """the D3Q19 weights in the Palabos order"""
    return list(T19)


def random_populations(rng, n, amp=0.02):
    """fBar = f - t_i around rest equilibrium (0) with a smooth-ish random perturbation"""
    return amp * rng.standard_normal((n, 19)) * np.array(O_T())[None, :]


# the D3Q19 velocities in the Palabos order
D3Q19 = [(0, 0, 0), (-1, 0, 0), (0, -1, 0), (0, 0, -1), (-1, -1, 0), (-1, 1, 0), (-1, 0, -1), (-1, 0, 1), (0, -1, -1), (0, -1, 1),
         (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, -1, 0), (1, 0, 1), (1, 0, -1), (0, 1, 1), (0, 1, -1)]

# the 18 neighbours: the 6 faces and the 12 edges of the cube around a node
NEIGHBOURS = [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if 1 <= a * a + b * b + c * c <= 2]
FACES = [d for d in NEIGHBOURS if d[0] * d[0] + d[1] * d[1] + d[2] * d[2] == 1]


def with_halo(mask, periodic_x, x0=0, nx=None):
    """the planes x0 - HALO .. x0 + nx + HALO - 1 of the global mask as Lattice.defineBounceBack hands them to the library:
    wrapped when x is periodic, wall (1) outside a non-periodic lattice"""
    mask = np.asarray(mask, dtype=np.uint8)
    nxg = mask.shape[0]
    nx = nxg if nx is None else nx
    xs = np.arange(x0 - HALO, x0 + nx + HALO)
    if periodic_x:
        return mask[xs % nxg].copy()
    out = np.ones((len(xs),) + mask.shape[1:], np.uint8)
    ok = (xs >= 0) & (xs < nxg)
    out[ok] = mask[xs[ok]]
    return out


def plane_stride(ny, nz, padded):
    """nodes from x-plane to x-plane in the slab's numbering: a whole number of lines, plus 8 rows (in whole lines) when padded"""
    xs = -(-ny * nz // LINE) * LINE
    if padded:
        xs += -(-8 * nz // LINE) * LINE
    return xs


def _fluid_at(fluid, d, periodic, yz_wrap):
    """out[x, y, z] = the node (x, y, z) + d is known to be fluid, or lies beyond the outer halo plane (unknown: counts)"""
    dx, dy, dz = d
    nxh = fluid.shape[0]
    src = fluid
    for axis, c in ((1, dy), (2, dz)):
        if c == 0:
            continue
        src = np.roll(src, -c, axis=axis)
        if not (periodic[axis] and yz_wrap):   # nothing lies beyond this face: not a fluid node
            edge = [slice(None)] * 3
            edge[axis] = -1 if c == 1 else 0
            src[tuple(edge)] = False
    if dx:
        out = np.ones_like(src)
        if dx == 1:
            out[:nxh - 1] = src[1:]
        else:
            out[1:] = src[:nxh - 1]
        src = out
    return src


def classes(mask, periodic, padded, x0=0, nx=None, faces_only=False, yz_wrap=True, x_halo_wall=False):
    """(classes, before promotion): uint8 [nx][ny][nz] of the bulk planes of the slab [x0, x0 + nx) of the global mask
    (default: the whole lattice).  Values: 0 fluid, 1 bounce-back, 2 inert, 3..6 the moving-wall classes of the mask.
    faces_only / yz_wrap=False / x_halo_wall are three WRONG rules for the mutation controls: only the 6 face neighbours
    count; y and z never wrap; the halo planes are taken as wall whatever they hold."""
    mask = np.asarray(mask, dtype=np.uint8)
    slab = with_halo(mask, periodic[0], x0, nx)
    if x_halo_wall:
        slab[:HALO] = 1
        slab[-HALO:] = 1
    nxh, ny, nz = slab.shape
    base = np.where((slab >= 3) & (slab <= 6), slab, (slab != 0).astype(np.uint8)).astype(np.uint8)
    fluid = slab == 0
    near = np.zeros(slab.shape, bool)
    for d in (FACES if faces_only else NEIGHBOURS):
        near |= _fluid_at(fluid, d, periodic, yz_wrap)
    before = np.where(~fluid & ~near, 2, base).astype(np.uint8)
    # promotion, in the padded numbering: the padding behind every plane is inert
    xs = plane_stride(ny, nz, padded)
    lines = np.full((nxh, xs), 2, np.uint8)
    lines[:, :ny * nz] = before.reshape(nxh, -1)
    lines = lines.reshape(-1, LINE)
    live = (lines != 2).any(axis=1, keepdims=True)
    lines = np.where(live & (lines == 2), 1, lines).astype(np.uint8)
    after = lines.reshape(nxh, xs)[:, :ny * nz].reshape(nxh, ny, nz)
    return after[HALO:nxh - HALO].copy(), before[HALO:nxh - HALO].copy()


def span_report(cls):
    """What the active-span map of the bulk planes looks like, from their classes [nx][ny][nz]:
    active      [nx]      nodes the collide visits per plane (the sum of the spans' lengths, inert nodes inside them included)
    z0          [nx][ny]  first node of each row's span (nz for an empty row)
    length      [nx][ny]  nodes of each row's span
    empty_rows            rows without a span
    rows_z0               rows with a span that starts at z0 > 0
    inert_inside          inert nodes strictly inside a span
    seams                 (x, y) of the rows that a 256-thread block boundary falls strictly inside
    max_active            the largest plane count, at least 1: what sizes the launch"""
    cls = np.asarray(cls)
    nx, ny, nz = cls.shape
    live = cls != 2
    any_live = live.any(axis=2)
    first = np.where(any_live, live.argmax(axis=2), nz)
    last = np.where(any_live, nz - live[:, :, ::-1].argmax(axis=2), nz)   # one past the last node that is not inert
    length = last - first
    inside = 0
    seams = []
    for x in range(nx):
        cum = np.r_[0, np.cumsum(length[x])]
        for y in range(ny):
            inside += int((~live[x, y, first[x, y]:last[x, y]]).sum())
            lo, hi = int(cum[y]), int(cum[y + 1])
            if hi > lo and (hi - 1) // BLOCK * BLOCK > lo:   # a multiple of 256 in (lo, hi)
                seams.append((x, y))
    active = length.sum(axis=1)
    return dict(active=active, z0=first, length=length, empty_rows=int((length == 0).sum()),
                rows_z0=int(((length > 0) & (first > 0)).sum()), inert_inside=inside, seams=seams,
                max_active=max(int(active.max()), 1))


# ---- the geometries

def _grid(dims):
    return np.mgrid[0:dims[0], 0:dims[1], 0:dims[2]]


def _stenosis():
    dims = (20, 22, 22)
    x, y, z = _grid(dims)
    R = 9.5 - 4.0 * np.exp(-((x - 9.5) / 3.0) ** 2)
    return ((y - 10.5) ** 2 + (z - 10.5) ** 2 > R ** 2).astype(np.uint8)


def _thick_walls():
    m = np.zeros((10, 12, 37), np.uint8)
    m[:, :3, :] = 1
    m[:, 8:, :] = 1
    m[3:6, 5:8, 10:30] = 1
    return m


def _solid_planes():
    m = np.zeros((12, 9, 18), np.uint8)
    m[:, 0, :] = m[:, -1, :] = 1
    m[:, :, 0] = m[:, :, -1] = 1
    m[4:7] = 1
    return m


def _seam_slabs():
    x, y, z = _grid((12, 10, 32))
    return ((x < 3) | (y < 3) | (z < 18)).astype(np.uint8)


def _sphere_seam():
    dims = (14, 13, 19)
    g = _grid(dims)
    d2 = 0.0
    for axis, c in enumerate((0.3, 12.4, 0.2)):
        d = np.abs(g[axis] - c)
        d = np.minimum(d, dims[axis] - d)   # minimum image
        d2 = d2 + d * d
    return (d2 <= 4.5 ** 2).astype(np.uint8)


def _tiny():
    m = np.zeros((9, 5, 3), np.uint8)
    m[3:6] = 1
    return m


def _le_block():
    # fluid layers at z = 0, 1, nz - 2, nz - 1; the block's inert core z = 11 .. 42 holds the aligned line z = 16 .. 31 of
    # every row (a row starts at a multiple of 48, so at a multiple of 16)
    m = np.zeros((8, 6, 48), np.uint8)
    m[2:6, 1:5, 10:44] = 1
    return m


class Geometry:
    def __init__(self, name, periodic, mask):
        self.name, self.periodic, self.mask = name, tuple(int(p) for p in periodic), mask
        self.dims = mask.shape

    def classes(self, padded, **kw):
        return classes(self.mask, self.periodic, padded, **kw)

    def kept(self, padded):
        return int((self.classes(padded)[0] == 2).sum())


GEOMETRIES = {g.name: g for g in (
    Geometry("stenosis", (1, 0, 0), _stenosis()),
    Geometry("thick_walls", (1, 0, 1), _thick_walls()),
    Geometry("solid_planes", (0, 0, 0), _solid_planes()),
    Geometry("seam_slabs", (1, 1, 1), _seam_slabs()),
    Geometry("sphere_seam", (1, 1, 1), _sphere_seam()),
    Geometry("tiny", (1, 1, 1), _tiny()),
    Geometry("all_solid", (1, 1, 1), np.ones((6, 6, 6), np.uint8)),
    Geometry("le_block", (1, 1, 1), _le_block()),
)}
# the non-periodic variant of the stenosis for the open boundaries: its planes x = 0 and nx - 1 see wall in the halo
STENOSIS_OPEN = Geometry("stenosis_open", (0, 0, 0), _stenosis())


# inclusive boxes (x0, x1, y0, y1, z0, z1).  FORCE_BOXES: three overlapping body-force boxes per geometry -- the first wholly
# inside solid, the second across a wall, the third up to the last plane of every axis.  SOURCE_BOX: a scalar source box and
# VISC_BOXES two class boxes that each hold fluid, bounce-back and inert nodes
FORCE_BOXES = {"stenosis": [(2, 6, 0, 1, 0, 6), (4, 12, 1, 8, 5, 15), (10, 19, 6, 21, 8, 21)],
               "seam_slabs": [(0, 2, 1, 5, 3, 20), (1, 7, 2, 6, 15, 25), (5, 11, 4, 9, 20, 31)]}
BOX_FORCES = [(-3e-5, 1e-5, 2e-6), (2e-5, -4e-6, 1e-5), (5e-6, 3e-5, -2e-5)]
SOURCE_BOX = {"stenosis": (3, 8, 0, 12, 0, 12), "seam_slabs": (0, 6, 0, 5, 10, 25), "tiny": (1, 4, 0, 4, 0, 2)}
VISC_BOXES = [(0, 9, 0, 11, 0, 21), (6, 15, 8, 21, 4, 17)]


def box_slices(box):
    x0, x1, y0, y1, z0, z1 = box
    return (slice(x0, x1 + 1), slice(y0, y1 + 1), slice(z0, z1 + 1))


def boxes_overlap(a, b):
    return all(a[2 * d] <= b[2 * d + 1] and b[2 * d] <= a[2 * d + 1] for d in range(3))


# ---- the set-up every comparison against the oracle starts from

OMEGA = 1.0 / 0.9
BODY = (1e-5, -2e-6, 3e-6)   # three non-zero components
SEED = 7


def initial_state(n, seed=SEED):
    """the random state of test_collide_stream_bit_exact_random_state: 0.02 N(0, 1) t_q"""
    return random_populations(np.random.default_rng(seed), n)


def start_state(g, seed=SEED):
    """initial_state on the geometry's lattice, [n][19], with the populations that would have come in through a non-periodic
    face set to 0: nothing lies outside such a face, so the device's upload has no slot for them and the oracle's stream puts
    0 there from the first step on.  Where the face nodes are wall (every geometry here but solid_planes and the open
    stenosis) this changes no fluid node"""
    f = initial_state(int(np.prod(g.dims)), seed).reshape(tuple(g.dims) + (19,))
    for q, c in enumerate(D3Q19):
        for axis in range(3):
            if c[axis] and not g.periodic[axis]:
                face = [slice(None)] * 3
                face[axis] = 0 if c[axis] == 1 else -1
                f[tuple(face) + (q,)] = 0.0
    return f.reshape(-1, 19)


def oracle_lattice(orc, g, mask=None, omega=OMEGA, seed=SEED):
    """the oracle's lattice of a geometry (or of another mask on its dims) with the initial state and the body force.  The
    oracle bounces on every solid node and knows nothing of classes or spans."""
    from oracle import oracle as O
    Lo = O.OracleLattice(orc, *g.dims, g.periodic, omega)
    Lo.set_mask(g.mask if mask is None else mask)
    Lo.f[:] = start_state(g, seed)
    Lo.set_force_uniform(BODY)
    return Lo


def wall_adjacent_solid_node(mask, periodic):
    """a bounce-back node with a fluid neighbour (the middle one in node order): clearing it must change the flow"""
    before = classes(mask, periodic, False)[1]
    idx = np.argwhere((np.asarray(mask) != 0) & (before != 2))
    assert len(idx)
    return tuple(int(v) for v in idx[len(idx) // 2])
