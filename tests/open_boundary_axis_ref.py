"""Restatement of the Zou-He open boundaries with the normal along any axis, in numpy -- test infrastructure only.  Built on
tests/open_boundary_ref.py (normal x), which is imported, not copied.

The completion on axis a is the x completion with the roles of x and a exchanged: with p_a[i] the D3Q19 index of direction c_i
with components 0 and a exchanged (an involution), g[i] = f[p_a[i]], the x completion runs on g with the velocity columns 0 and
a exchanged as well (the normal velocity is u[a]; the tangential pair is (u_x, u_z) for y and (u_y, u_x) for z), and the result
goes back through p_a.  Every sum keeps the operand order of open_boundary_ref.complete, so the kernel's zou_he<AXIS> agrees
bit for bit.

A declaration is two arrays over the nodes: ob_code (-1 or slot << 2 | kind, kind as in open_boundary_ref: bit 0 = P, bit 1 =
pressure) and ob_axis (0, 1, 2 where ob_code >= 0).  The completion touches only a fluid node's own populations, and the
bounce-back swap only those of wall nodes, so completing first and handing the state to open_boundary_ref.step / observe
without a declaration runs every stage in the order of the kernels.
"""
import numpy as np

import open_boundary_ref as OB


def perm(axis):
    """p_a: the index of direction c_i with components 0 and `axis` exchanged"""
    c = OB.C.copy()
    c[:, [0, axis]] = c[:, [axis, 0]]
    return np.array([int(np.flatnonzero((OB.C == ci).all(axis=1))[0]) for ci in c])


PERM = [perm(a) for a in range(3)]


def swap_columns(v, axis):
    """columns 0 and `axis` of [m][>= 3] exchanged (a copy)"""
    w = np.array(v, dtype=np.float64, copy=True)
    w[:, [0, axis]] = w[:, [axis, 0]]
    return w


def complete_axis(f, kind, val, axis):
    """f: [m][19] stored-form populations of m nodes of one kind and one axis; val: [m][4] (u_x, u_y, u_z, rho) in lattice axes.
    Returns the completed populations."""
    p = PERM[axis]
    g = OB.complete(np.ascontiguousarray(f[:, p]), kind, swap_columns(val, axis))
    return g[:, p]


def completed(S, mask, ob_code, ob_axis, ob_val):
    """a copy of the post-stream state S [nx][ny][nz][19] with the fluid open-boundary nodes completed"""
    P = S.reshape(-1, 19).copy()
    if ob_code is not None:
        code = np.asarray(ob_code).reshape(-1)
        ax = np.asarray(ob_axis).reshape(-1)
        fluid = mask.reshape(-1) == 0
        for axis in range(3):
            for kind in range(4):
                sel = fluid & (code >= 0) & (ax == axis) & ((code & 3) == kind)
                if sel.any():
                    P[sel] = complete_axis(P[sel], kind, ob_val[code[sel] >> 2], axis)
    return P.reshape(S.shape)


def step(S, mask, periodic, omega, body, ob_code=None, ob_axis=None, ob_val=None, **kw):
    """one collide-stream; open_boundary_ref.step with ob_axis next to ob_code (kw: F, boxes, box_forces, wall_u)"""
    return OB.step(completed(S, mask, ob_code, ob_axis, ob_val), mask, periodic, omega, body, **kw)


def observe(S, mask, periodic, body, F=None, ob_code=None, ob_axis=None, ob_val=None, **kw):
    """(rho, u, Pi_neq) of the completed populations; open_boundary_ref.observe with ob_axis next to ob_code"""
    return OB.observe(completed(S, mask, ob_code, ob_axis, ob_val), mask, periodic, body, F, **kw)


def gathered(S, periodic):
    """what a lattice holds after S [nx][ny][nz][19] was uploaded: the populations that would have come from outside a face
    that is not periodic are 0"""
    S = S.copy()
    for ax in range(3):
        if periodic[ax]:
            continue
        first = [slice(None)] * 3; first[ax] = 0
        last = [slice(None)] * 3; last[ax] = -1
        for q in range(19):
            if OB.C[q][ax] == 1:
                S[tuple(first) + (q,)] = 0.0
            elif OB.C[q][ax] == -1:
                S[tuple(last) + (q,)] = 0.0
    return S


# ---- scenes shared by the CPU and the GPU tests: walled channels that are open along one axis, and an L-shaped duct

OMEGA, BODY = 1.0 / 0.9, (2e-6, 3e-7, -1e-7)
NONPER = (False, False, False)
CHANNEL_DIMS = {0: (24, 17, 19), 1: (17, 24, 19), 2: (19, 17, 24)}   # the open axis is the long one
BENT_DIMS = (20, 18, 11)   # extents along (inlet axis, outlet axis, third axis) of the L-shaped duct


def channel_mask(dims, axis):
    """fluid inside, bounce-back on the four faces whose normal is not `axis`"""
    m = np.zeros(dims, np.uint8)
    for ax in range(3):
        if ax != axis:
            idx = [slice(None)] * 3
            idx[ax] = 0; m[tuple(idx)] = 1
            idx[ax] = -1; m[tuple(idx)] = 1
    return m


def _tent(n):
    """a parabola over n nodes whose first and last are walls"""
    s = (np.arange(n) - (n - 1) / 2.0) / ((n - 2) / 2.0)
    return np.clip(1 - s ** 2, 0, None)


def _box_slices(box):
    return (slice(box[0], box[1] + 1), slice(box[2], box[3] + 1), slice(box[4], box[5] + 1))


def _box_size(box):
    return (box[1] - box[0] + 1) * (box[3] - box[2] + 1) * (box[5] - box[4] + 1)


def velocity_values(box, axis, sign, u_max=0.02):
    """per-node profile on a box (box order: x outermost, z innermost): the normal component u[axis] = sign * parabola over the
    box's extents along the two other axes, the tangential ones 0.1 and -0.05 parabola (all non-zero off the walls)"""
    ext = [box[1] - box[0] + 1, box[3] - box[2] + 1, box[5] - box[4] + 1]
    others = [ax for ax in range(3) if ax != axis]
    p = np.ones(ext)
    for ax in others:
        shape = [1, 1, 1]; shape[ax] = ext[ax]
        p = p * _tent(ext[ax]).reshape(shape)
    p = (u_max * p).reshape(-1)
    u = np.empty((p.size, 3))
    u[:, axis] = sign * p
    u[:, others[0]] = 0.1 * p
    u[:, others[1]] = -0.05 * p
    return u


def density_values(box, seed):
    return 1.0 + np.random.default_rng(seed).uniform(-0.01, 0.01, _box_size(box))


def _planes(dims, axis, lo, hi):
    box = [0, dims[0] - 1, 0, dims[1] - 1, 0, dims[2] - 1]
    box[2 * axis], box[2 * axis + 1] = lo, hi
    return tuple(box)


def channel_patches(layout, axis, dims):
    """[(kind, axis, box, values)] -- kind as in open_boundary_ref (VEL_0N ... PRES_0P name the N / P side of any axis)"""
    n = dims[axis]
    if layout == "original":    # velocity N on the first plane, pressure P over the last three planes
        bv, bp = _planes(dims, axis, 0, 0), _planes(dims, axis, n - 3, n - 1)
        return [(OB.VEL_0N, axis, bv, velocity_values(bv, axis, 1.0)), (OB.PRES_0P, axis, bp, density_values(bp, 21))]
    if layout == "mirrored":    # velocity P on the last plane with an inward (negative) normal velocity, pressure N over the first three
        bv, bp = _planes(dims, axis, n - 1, n - 1), _planes(dims, axis, 0, 2)
        return [(OB.VEL_0P, axis, bv, velocity_values(bv, axis, -1.0)), (OB.PRES_0N, axis, bp, density_values(bp, 22))]
    if layout == "four":        # all four kinds at once, each face split along the first of the other axes
        other = [ax for ax in range(3) if ax != axis][0]
        h = dims[other] // 2
        out = []
        for plane, kinds, seeds in ((0, (OB.VEL_0N, OB.PRES_0N), 23), (n - 1, (OB.VEL_0P, OB.PRES_0P), 24)):
            a, b = list(_planes(dims, axis, plane, plane)), list(_planes(dims, axis, plane, plane))
            a[2 * other + 1] = h - 1; b[2 * other] = h
            a, b = tuple(a), tuple(b)
            out += [(kinds[0], axis, a, velocity_values(a, axis, 1.0)), (kinds[1], axis, b, density_values(b, seeds))]
        return out
    raise ValueError(layout)


def bent_duct(a_in, a_out):
    """an L-shaped walled duct: one arm runs along a_in from the open face a_in = 0, the other along a_out to the open face
    a_out = last; the nodes of the edges of both faces are walls.  Returns (dims, mask, patches): a velocity N inlet on a_in and
    a pressure P outlet on a_out."""
    t = 3 - a_in - a_out
    n_in, n_out, n_t = BENT_DIMS
    dims = [0, 0, 0]
    dims[a_in], dims[a_out], dims[t] = n_in, n_out, n_t
    h, w = 8, 11   # the first arm spans a_out in 1 .. h - 1, the second a_in in w .. n_in - 2
    g = np.meshgrid(*[np.arange(d) for d in dims], indexing="ij")
    ci, co, ct = g[a_in], g[a_out], g[t]
    arm1 = (ci <= n_in - 2) & (co >= 1) & (co <= h - 1)
    arm2 = (ci >= w) & (ci <= n_in - 2) & (co >= 1)
    fluid = (arm1 | arm2) & (ct >= 1) & (ct <= n_t - 2)
    mask = np.where(fluid, 0, 1).astype(np.uint8)
    b_in = [0, dims[0] - 1, 0, dims[1] - 1, 0, dims[2] - 1]
    b_in[2 * a_in], b_in[2 * a_in + 1] = 0, 0
    b_in[2 * a_out], b_in[2 * a_out + 1] = 0, h
    b_out = [0, dims[0] - 1, 0, dims[1] - 1, 0, dims[2] - 1]
    b_out[2 * a_out], b_out[2 * a_out + 1] = n_out - 1, n_out - 1
    b_out[2 * a_in], b_out[2 * a_in + 1] = w - 1, n_in - 1
    b_in, b_out = tuple(b_in), tuple(b_out)
    patches = [(OB.VEL_0N, a_in, b_in, velocity_values(b_in, a_in, 1.0)), (OB.PRES_0P, a_out, b_out, density_values(b_out, 25))]
    return tuple(dims), mask, patches


def corner_box():
    """a walled 11 x 12 x 13 box with a velocity N inlet on its face y = 0 and a pressure P outlet on its face z = last; the
    nodes of the edge where the two faces meet are walls.  In every plane x the outlet nodes of the rows y = 1, 2, ... follow
    the inlet row y = 0 within the first 64 nodes, so one wavefront of a plane launch holds open nodes of two axes.
    Returns (dims, mask, patches)."""
    dims = (11, 12, 13)
    nx, ny, nz = dims
    mask = np.ones(dims, np.uint8)
    mask[1:nx - 1, 0:ny - 1, 1:nz] = 0
    mask[:, 0, nz - 1] = 1
    b_in, b_out = (0, nx - 1, 0, 0, 0, nz - 1), (0, nx - 1, 1, ny - 1, nz - 1, nz - 1)
    patches = [(OB.VEL_0N, 1, b_in, velocity_values(b_in, 1, 1.0)), (OB.PRES_0P, 2, b_out, density_values(b_out, 26))]
    return dims, mask, patches


def axes_per_wave(mask, ob_code, ob_axis, x, rows):
    """the sets of axes of the fluid open nodes that each 64-lane wave of plane x holds among the first `rows` rows.  Asserts
    that every node of those rows is fluid or touches a fluid node: the collide's thread map then walks them whole, thread
    t = y * nz + z, which is also the node order of the plane-indexed observers."""
    nz = mask.shape[2]
    assert exchanging(mask)[x, :rows].all()
    fluid_open = ((mask[x, :rows] == 0) & (ob_code[x, :rows] >= 0)).reshape(-1)
    ax = np.asarray(ob_axis)[x, :rows].reshape(-1)
    return [set(int(a) for a in ax[w:w + 64][fluid_open[w:w + 64]]) for w in range(0, rows * nz, 64)]


def interpolate_phi2(pos, u, mask):
    """interpolationCoefficientsPhi2 on a lattice that is not periodic: the 2 x 2 x 2 nodes around each vertex of pos [n][3],
    tent weights, bounce-back nodes and nodes outside left out, the rest normalised; v = sum_k (u_k w_k) in ascending
    (i, j, k) order, the interpolation kernels' order"""
    dims = np.array(mask.shape)
    out = np.zeros_like(pos)
    for n, p in enumerate(pos):
        c = np.floor(p + 0.5).astype(int)
        d0 = np.where(p < c, -1, 0)
        nodes, w = [], []
        for i in range(2):
            for j in range(2):
                for k in range(2):
                    g = c + d0 + (i, j, k)
                    if (g < 0).any() or (g >= dims).any():
                        continue
                    t = np.clip(1.0 - np.abs(p - g), 0.0, None)
                    wt = t[0] * t[1] * t[2]
                    if wt != 0.0 and mask[tuple(g)] == 0:
                        nodes.append(tuple(g)); w.append(wt)
        assert w, "every stencil node of the vertex is masked"
        total = 0.0
        for wt in w:
            total = total + wt
        coeff = 1.0 / total
        a = np.zeros(3)
        for g, wt in zip(nodes, w):
            a = a + u[g] * (wt * coeff)
        out[n] = a
    return out


def exchanging(mask):
    """the nodes that are fluid or have a fluid neighbour among the 18 directions (no wrap).  Every other bounce-back node
    never exchanges a population with the fluid; the collide kernel may skip it, so what it stores there is not compared."""
    fluid = mask == 0
    near = fluid.copy()
    padded = np.pad(fluid, 1, constant_values=False)
    nx, ny, nz = mask.shape
    for c in OB.C[1:]:
        near |= padded[1 + c[0]:1 + c[0] + nx, 1 + c[1]:1 + c[1] + ny, 1 + c[2]:1 + c[2] + nz]
    return near


def declaration(dims, patches):
    """(ob_code, ob_axis, ob_val) of patches declared in order: slots are handed out in box order, velocity slots start at
    rho = 1 and pressure slots at u = 0"""
    code = -np.ones(dims, np.int64)
    axes = -np.ones(dims, np.int64)
    vals = []
    total = 0
    for kind, axis, box, values in patches:
        n = _box_size(box)
        s = _box_slices(box)
        assert (code[s] < 0).all() and len(values) == n
        code[s] = ((total + np.arange(n)) << 2 | kind).reshape(code[s].shape)
        axes[s] = axis
        v = np.zeros((n, 4)); v[:, 3] = 1.0
        if kind in (OB.VEL_0N, OB.VEL_0P):
            v[:, :3] = values
        else:
            v[:, 3] = values
        vals.append(v)
        total += n
    return code, axes, np.concatenate(vals)


def initial_state(dims, seed=4):
    """random populations in +-0.005 as a lattice without periodic faces holds them after an upload"""
    return gathered(np.random.default_rng(seed).uniform(-0.005, 0.005, size=tuple(dims) + (19,)), NONPER)
