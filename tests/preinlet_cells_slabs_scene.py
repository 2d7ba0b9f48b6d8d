"""The inputs of tests/test_gpu_preinlet_cells_slabs.py as plain numbers, shared with tests/test_preinlet_cells_slabs_cpu.py, which
checks from tests/preinlet_cells_ref.py and numpy alone that they are what the GPU tests claim.

A cell is (type, id, centre, angles).  HALF holds the half extents of the placed meshes on the three axes (hcp_add_cell centres a
mesh on its bounding box), as the library places them; the GPU tests assert them against the placed cells, and the CPU tests
stand an eight-vertex box of those extents in for every cell."""
import numpy as np

import preinlet_cells_ref as PC

PRE = (40, 34, 34)                       # the pre-inlet, periodic along x
CROSS = (34, 34)
STRIDE = 1000
E_SHARE = 4.0                            # the default particle envelope share (hcp_envelope)
SIGN = {"Xneg": -1, "Xpos": 1}
RBC_ANG, PLT_ANG, FLAT = (90.0, 0.0, 0.0), (10.0, 20.0, 30.0), (0.0, 0.0, 0.0)
HALF = {(0, RBC_ANG): (7.821, 7.821, 2.2943089), (1, PLT_ANG): (2.2441067, 1.5099102, 2.4656337), (1, FLAT): (2.501, 1.0879565, 2.501)}


def domain(world):
    """(global planes, planes per slab): 96 as 2 slabs, 120 as 3 -- 40 planes is the narrowest slab that carries an RBC"""
    nxg = 96 if world == 2 else 120
    return nxg, nxg // world


def slab_of(rank, world):
    nxg, nx = domain(world)
    return rank * nx, (rank + 1) * nx


def inlet_rank(direction, world):
    return 0 if SIGN[direction] < 0 else world - 1


def far_rank(direction, world):
    return world - 1 if SIGN[direction] < 0 else 0


def image(window, shift):
    return window[0] + shift[0], window[1] + shift[0]


def margin_ok(direction, world, window, shift):
    """hcp_preinlet_create_slab's rule: the window's image lies in the inlet rank's slab, at least E_SHARE from its inner face"""
    x0, x1 = slab_of(inlet_rank(direction, world), world)
    a, b = image(window, shift)
    return (a >= x0 and b <= x1 - E_SHARE) if SIGN[direction] < 0 else (a >= x0 + E_SHARE and b <= x1)


def box_records(cells, lap_of=None):
    """eight records per cell: the corners of its bounding box, unwrapped by lap_of[id] laps of the pre-inlet"""
    out = []
    for t, cid, centre, ang in cells:
        h = np.array(HALF[(t, tuple(ang))])
        rec = np.zeros(8, dtype=REC)
        k = 0
        for sx in (-1, 1):
            for sy in (-1, 1):
                for sz in (-1, 1):
                    rec["position"][k] = np.array(centre, float) + h * (sx, sy, sz)
                    rec["vertexId"][k] = k
                    k += 1
        rec["position"][:, 0] += (lap_of or {}).get(cid, 0) * PRE[0]
        rec["cellId"], rec["celltype"] = cid, t
        out.append(rec)
    return np.concatenate(out)


REC = np.dtype({"names": ["v", "position", "force", "force_repulsion", "cellId", "vertexId", "restime", "celltype"],
                "formats": [("<f8", 3), ("<f8", 3), ("<f8", 3), ("<f8", 3), "<i8", "<u2", "<u4", "u1"],
                "offsets": [0, 24, 48, 72, 96, 104, 108, 112], "itemsize": 120})   # host.Cells.SV_DTYPE


def owners(cell, world):
    """the ranks on which a vertex of the cell's bounding box has its nearest node"""
    t, cid, centre, ang = cell
    lo, hi = centre[0] - HALF[(t, tuple(ang))][0], centre[0] + HALF[(t, tuple(ang))][0]
    return [r for r in range(world) if np.floor(lo + 0.5) < slab_of(r, world)[1] and np.floor(hi + 0.5) >= slab_of(r, world)[0]]


def holders(cell, world):
    """the ranks hcp_add_cell keeps a cell on: those that own a vertex (nearest node in the slab) or see it within E_SHARE"""
    t, cid, centre, ang = cell
    lo, hi = centre[0] - HALF[(t, tuple(ang))][0], centre[0] + HALF[(t, tuple(ang))][0]
    out = []
    for r in range(world):
        x0, x1 = slab_of(r, world)
        own = np.floor(lo + 0.5) < x1 and np.floor(hi + 0.5) >= x0
        if own or (hi >= x0 - E_SHARE and lo < x1 + E_SHARE):
            out.append(r)
    return out


# ---- 1: one static check
STATIC_WINDOW = (10.0, 36.0)
STATIC_LAPS = {5011: 2}


def static_shift(direction, world):
    """Xneg: the image is [2, 28]; Xpos: it starts 6 planes inside the last slab"""
    x0, _ = slab_of(inlet_rank(direction, world), world)
    return (-8.0, 6.0, 0.0) if SIGN[direction] < 0 else (x0 - 4.0, 6.0, 0.0)


def static_pre_cells():
    """the five cases of test_static_selection_and_copy -- an RBC in the window, a PLT in the window two laps on (STATIC_LAPS),
    a PLT across window_hi, a PLT before the window, a PLT in the window that the shift in y puts outside the domain -- and a
    PLT in the window whose new id a resident of the far rank holds"""
    return [(0, 5007, (23.0, 13.0, 16.5), RBC_ANG), (1, 5011, (14.0, 12.0, 20.0), PLT_ANG), (1, 5012, (36.0, 12.0, 12.0), PLT_ANG),
            (1, 5013, (5.0, 14.0, 14.0), PLT_ANG), (1, 5014, (20.0, 28.0, 16.0), PLT_ANG), (1, 5015, (30.0, 20.0, 12.0), PLT_ANG)]


def static_residents(direction, world):
    """an RBC and a PLT in the middle of the inlet rank's slab, and on the far rank alone the PLT whose id collides"""
    a0, a1 = slab_of(inlet_rank(direction, world), world)
    b0, b1 = slab_of(far_rank(direction, world), world)
    collide = PC.new_id(5015, 0, SIGN[direction], STRIDE)
    return [(0, 1, (0.5 * (a0 + a1), 16.5, 16.5), RBC_ANG), (1, 2, (0.5 * (a0 + a1), 12.0, 26.0), FLAT),
            (1, collide, (0.5 * (b0 + b1), 16.5, 16.5), FLAT)]


def static_more_cells(n=70):
    """n PLTs in the window, more than the 64 + n / 4 slots the domain's PLT region starts with: the region grows"""
    rng = np.random.default_rng(9)
    return [(1, 5300 + k, tuple(np.array((20.0, 14.0, 14.0)) + rng.uniform(-3.0, 3.0, size=3) * (1.0, 0.5, 1.0)), PLT_ANG) for k in range(n)]


# ---- 2: the coupled run (Xneg): a PLT arrives with its leading vertex E_SHARE + 1 planes at most before the inner face
U0 = (0.06, 0.0, 0.0)
COUPLED_WINDOW = (28.0, 34.0)            # a PLT is 5.002 planes long


def coupled_shift(world):
    _, x1 = slab_of(0, world)
    return (x1 - E_SHARE - COUPLED_WINDOW[1], 0.0, 0.0)


def coupled_pre_cells():
    """the trailing vertex starts 0.3 planes upstream of window_lo"""
    return [(1, 5040, (COUPLED_WINDOW[0] - 0.3 + HALF[(1, FLAT)][0], 16.5, 16.5), FLAT)]


def coupled_residents(world):
    """an RBC in the middle of the slab next to the inlet rank's"""
    x0, x1 = slab_of(1, world)
    return [(0, 1, (0.5 * (x0 + x1), 16.5, 16.5), RBC_ANG)]


# ---- 3: the sink two nodes inside the last slab of two
SINK_PLANE = 50.0


def sink_residents():
    """a PLT across the face x = 48 whose leading vertex starts two planes upstream of the sink plane, and one mid-slab on rank 0"""
    h = HALF[(1, FLAT)][0]
    return [(1, 5, (SINK_PLANE - 2.0 - h, 16.5, 16.5), FLAT), (1, 6, (14.0, 16.5, 16.5), FLAT)]


def sink_pre_cells():
    """a PLT upstream of the window that does not reach it during the run"""
    return [(1, 5090, (5.0, 16.5, 16.5), FLAT)]


# ---- 4: the stale plan: one check takes one PLT and brings one
STALE_WINDOW, STALE_SHIFT = (10.0, 36.0), (-8.0, 0.0, 0.0)


def stale_residents():
    """PLT 5 lies wholly on rank 1's side of the face x = 48 and past the sink plane -- rank 0 holds a pure copy of it, in its
    first PLT slot -- and PLT 6 across the face, short of the plane for the whole run, fills that slot when 5 goes: extents
    taken before the check would call 6 a pure copy, which nobody forwards"""
    h = HALF[(1, FLAT)]
    return [(1, 5, (48.2 + h[0], 10.0, 16.5), FLAT), (1, 6, (49.0 - h[0], 23.0, 16.5), FLAT)]


def stale_pre_cells():
    return [(1, 5040, (20.0, 16.5, 16.5), FLAT)]
