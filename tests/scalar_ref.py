"""Restatement of the CEPAC scalar field's D3Q19 advection-diffusion step in numpy -- test infrastructure only.

The reference leaves the field half finished (param::tau_CEPAC is 0 and is handed to AdvectionDiffusionBGKdynamics where an
omega belongs) and its fluid library is not part of the reference tree, so hemocell_amd/csrc/scalar.hip defines the step and
this file restates it operation for operation: every operation is an IEEE double operation in the kernel's order, so the GPU
(built with -ffp-contract=off) agrees bit for bit.

State: the post-stream populations g[nx][ny][nz][19] in the stored form g_i - t_i (Palabos D3Q19 order), as
Scalar.populations() returns them reshaped; concentration C = 1 + sum_i g_i.  One step on every node:

1. bounce-back nodes (mask != 0, the moving-wall classes included) swap opposite populations: zero scalar flux, no momentum
   term;
2. fluid source nodes (src == k > 0, value C_s = values[k - 1]) set g_i = t_i (Cbar + (3 C) (c_i . u)) with C = C_s and
   Cbar = C_s - 1;
3. every other fluid node: Cbar = ((g_0 + g_1) + g_2) + ... + g_18, C = 1 + Cbar, geq_i = t_i (Cbar + (3 C) (c_i . u)),
   g_i = g_i (1 - omega), then g_i = g_i + omega geq_i;
4. stream: S'(x, i) = P(x - c_i, i), 0 where x - c_i lies outside a non-periodic axis.

u is the advecting velocity (velocity() below): j / rho of the flow's post-stream populations plus half of the body force
(uniform, or that of the last box holding the node) and of the IBM force the flow's collide of the same iteration consumed.
c_i . u is ((c_x u_x + c_y u_y) + c_z u_z) with the zero terms dropped, 0.0 for i = 0.

The kernel skips solid nodes without a fluid neighbour and this file does not; no such node ever exchanges a population with a
fluid node, so the two agree on fluid nodes (and on the visible populations there), which is where the tests compare.
"""
import numpy as np

from tests.open_boundary_ref import C, OPP, T, _cdot, observe

MAX_SOURCES = 8   # HC_MAX_SCALAR_SOURCES


def velocity(f_flow, mask, body, F=None, boxes=None, box_forces=None):
    """the advecting velocity [nx][ny][nz][3] from the flow's post-stream populations f_flow [nx][ny][nz][19]: the u of
    open_boundary_ref.observe (j / rho + (body + F) / 2 in the kernels' order) on fluid nodes, 0 elsewhere"""
    _, u, _ = observe(f_flow, mask, None, body, F=F, boxes=boxes, box_forces=box_forces)
    u = u.copy()
    u[mask != 0] = 0.0
    return u


class Sources:
    """the class byte per node and the table of values: 0 = none, k = values[k - 1]"""

    def __init__(self, shape):
        self.cls = np.zeros(shape, np.uint8)
        self.values = []

    def add(self, box, value):
        """inclusive (x0, x1, y0, y1, z0, z1), clipped to the lattice; a value beyond MAX_SOURCES distinct ones is refused"""
        value = float(value)
        x0, x1, y0, y1, z0, z1 = (int(v) for v in box)
        sel = (slice(max(x0, 0), x1 + 1), slice(max(y0, 0), y1 + 1), slice(max(z0, 0), z1 + 1))
        if self.cls[sel].size == 0:
            return   # wholly outside the lattice: nothing is registered
        cls = self.cls.copy()
        cls[sel] = 0
        used = [k for k in range(len(self.values)) if (cls == k + 1).any()]   # a value painted over gives its slot back
        values = [self.values[k] for k in used]
        if value not in values:
            if len(values) >= MAX_SOURCES:
                raise ValueError("more than %d distinct source values" % MAX_SOURCES)
            values.append(value)
        renumber = np.zeros(len(self.values) + 1, np.uint8)
        for new, k in enumerate(used):
            renumber[k + 1] = new + 1
        cls = renumber[cls]
        cls[sel] = values.index(value) + 1
        self.cls, self.values = cls, values

    def clear(self):
        self.cls[...] = 0
        self.values = []

    def value_field(self):
        """C_s per node (0 where the node has no class)"""
        return np.r_[0.0, np.array(self.values, dtype=np.float64)][self.cls]


def stream(P, periodic):
    """S'(x, i) = P(x - c_i, i); a plane that wrapped around a non-periodic axis came from outside: 0"""
    out = np.zeros_like(P)
    for q in range(19):
        src = P[:, :, :, q]
        for ax, c in enumerate(C[q]):
            if c == 0:
                continue
            src = np.roll(src, int(c), axis=ax)
            if not periodic[ax]:
                idx = [slice(None)] * 3
                idx[ax] = 0 if c == 1 else -1
                src[tuple(idx)] = 0.0
        out[:, :, :, q] = src
    return out


def relax(g, u, omega, src=None, Cs=None):
    """steps 2 and 3 on fluid nodes g [m][19] (in place) with u [m][3]; src [m] bool: the node is a source, of value Cs [m]"""
    Cbar = np.zeros(g.shape[0])
    for q in range(19):
        Cbar = Cbar + g[:, q]
    Cc = 1.0 + Cbar
    if src is None:
        src = np.zeros(g.shape[0], bool)
    if src.any():
        Cc = np.where(src, Cs, Cc)
        Cbar = np.where(src, Cc - 1.0, Cbar)
    C3 = 3.0 * Cc
    one_m_omega = 1.0 - omega
    for q in range(19):
        c_u = _cdot(C[q], u[:, 0], u[:, 1], u[:, 2])
        geq = T[q] * (Cbar + C3 * c_u)
        r = g[:, q] * one_m_omega
        r = r + omega * geq
        g[:, q] = np.where(src, geq, r)
    return g


def step(g, mask, periodic, omega, u, sources=None):
    """one step of the scalar.  g [nx][ny][nz][19] post-stream; mask [nx][ny][nz] (0 = fluid); u [nx][ny][nz][3] the advecting
    velocity; sources: a Sources or None.  Returns the next post-stream state."""
    nx, ny, nz, _ = g.shape
    P = g.reshape(-1, 19).copy()
    wall = mask.reshape(-1) != 0
    P[wall] = P[wall][:, OPP]
    fluid = ~wall
    src = Cs = None
    if sources is not None and sources.values:
        src = sources.cls.reshape(-1)[fluid] != 0
        Cs = sources.value_field().reshape(-1)[fluid]
    P[fluid] = relax(P[fluid], u.reshape(-1, 3)[fluid], omega, src, Cs)
    return stream(P.reshape(nx, ny, nz, 19), periodic)


def concentration(g, mask=None, sources=None):
    """what the observers report: 1 + the sum of the populations in ascending q, and C_s on a fluid source node"""
    Cbar = np.zeros(g.shape[:3])
    for q in range(19):
        Cbar = Cbar + g[..., q]
    out = 1.0 + Cbar
    if sources is not None and sources.values:
        sel = (sources.cls != 0) & (mask == 0 if mask is not None else True)
        out = np.where(sel, sources.value_field(), out)
    return out


def equilibrium(shape, Cv, mask=None):
    """initializeAtEquilibrium at u = 0 on every node: fluid nodes see t_i (C - 1), nodes that are not fluid see 0"""
    g = np.zeros(tuple(shape) + (19,))
    g[...] = T * (float(Cv) - 1.0)
    if mask is not None:
        g[mask != 0] = 0.0
    return g
