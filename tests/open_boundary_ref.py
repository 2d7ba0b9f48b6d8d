"""Restatement of the Zou-He open boundaries with normal x and of one D3Q19 Guo-BGK collide-stream step, in numpy -- test
infrastructure only.

State: the post-stream populations f[nx][ny][nz][19] in the stored form f_i - t_i (Palabos D3Q19 order), as
Lattice.populations() returns them reshaped.  One step, in the order the collide kernel runs it on every node:

1. bounce-back nodes (mask != 0) swap opposite populations; moving-wall classes (mask 3..6) then add Ladd's momentum term;
2. open-boundary nodes complete their unknown populations (complete() below);
3. fluid nodes relax with the Guo-forced BGK (the oracle's collide_guo_bgk) under the body force -- uniform, or that of the
   last box holding the node -- plus the node's own force (the spread IBM force);
4. stream: S'(x, i) = P(x - c_i, i), 0 where x - c_i lies outside a non-periodic axis.

Every operation is an IEEE double operation in the kernel's order, so the GPU (built with -ffp-contract=off) agrees bit for
bit.  Completion, 0N (the five populations with c_x = +1 unknown), in real populations:

    rho = (S_0 + 2 S_-) / (1 - u_x)                       (velocity nodes; pressure nodes: u_x = 1 - (S_0 + 2 S_-) / rho)
    f(1,0,0)   = f(-1,0,0)   + rho u_x / 3
    f(1,+-1,0) = f(-1,-+1,0) + rho (u_x +- u_y) / 6 -+ N_y
    f(1,0,+-1) = f(-1,0,-+1) + rho (u_x +- u_z) / 6 -+ N_z
    N_y = (sum over c = (0,1,.) - sum over c = (0,-1,.)) / 2 - rho u_y / 3, N_z likewise

and 0P mirrored, with rho = (S_0 + 2 S_+) / (1 + u_x).  The opposite populations of a pair share t_i, and the t_i of the
nine c_x = 0 and twice the five outgoing ones sum to 1, so everything is formed in the stored form directly.
"""
import numpy as np

C = np.array([[0, 0, 0], [-1, 0, 0], [0, -1, 0], [0, 0, -1], [-1, -1, 0], [-1, 1, 0], [-1, 0, -1], [-1, 0, 1], [0, -1, -1],
              [0, -1, 1], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [1, -1, 0], [1, 0, 1], [1, 0, -1], [0, 1, 1], [0, 1, -1]])
T = np.array([1. / 3.] + [1. / 18.] * 3 + [1. / 36.] * 6 + [1. / 18.] * 3 + [1. / 36.] * 6)
OPP = [0] + list(range(10, 19)) + list(range(1, 10))

VEL_0N, VEL_0P, PRES_0N, PRES_0P = 0, 1, 2, 3


def complete(f, kind, val):
    """f: [m][19] stored-form populations of m nodes of one kind (completed in place); val: [m][4] (u_x, u_y, u_z, rho)"""
    neg = kind in (VEL_0N, PRES_0N)
    s0 = f[:, 0] + f[:, 2] + f[:, 3] + f[:, 8] + f[:, 9] + f[:, 11] + f[:, 12] + f[:, 17] + f[:, 18]
    sm = f[:, 1] + f[:, 4] + f[:, 5] + f[:, 6] + f[:, 7]
    sp = f[:, 10] + f[:, 13] + f[:, 14] + f[:, 15] + f[:, 16]
    known = s0 + 2.0 * (sm if neg else sp) + 1.0
    if kind in (VEL_0N, VEL_0P):
        ux, uy, uz = val[:, 0], val[:, 1], val[:, 2]
        rho = known / (1.0 - ux) if neg else known / (1.0 + ux)
    else:
        rho = val[:, 3]
        ux = 1.0 - known / rho if neg else known / rho - 1.0
        uy = np.zeros_like(rho); uz = np.zeros_like(rho)
    ny = 0.5 * ((f[:, 11] + f[:, 17] + f[:, 18]) - (f[:, 2] + f[:, 8] + f[:, 9])) - rho * uy / 3.0
    nz = 0.5 * ((f[:, 12] + f[:, 9] + f[:, 17]) - (f[:, 3] + f[:, 8] + f[:, 18])) - rho * uz / 3.0
    if neg:
        f[:, 10] = f[:, 1] + rho * ux / 3.0
        f[:, 13] = f[:, 4] + rho * (ux + uy) / 6.0 - ny
        f[:, 14] = f[:, 5] + rho * (ux - uy) / 6.0 + ny
        f[:, 15] = f[:, 6] + rho * (ux + uz) / 6.0 - nz
        f[:, 16] = f[:, 7] + rho * (ux - uz) / 6.0 + nz
    else:
        f[:, 1] = f[:, 10] - rho * ux / 3.0
        f[:, 4] = f[:, 13] - rho * (ux + uy) / 6.0 + ny
        f[:, 5] = f[:, 14] - rho * (ux - uy) / 6.0 - ny
        f[:, 6] = f[:, 15] - rho * (ux + uz) / 6.0 + nz
        f[:, 7] = f[:, 16] - rho * (ux - uz) / 6.0 - nz
    return f


def real_moments(f):
    """(rho, u) of stored-form populations [m][19] in extended sums (for the invariant checks)"""
    g = f.astype(np.longdouble) + T.astype(np.longdouble)
    rho = g.sum(axis=1)
    j = g @ C.astype(np.longdouble)
    return rho, j / rho[:, None]


def _cdot(c, a0, a1, a2):
    s = None
    for ci, ai in zip(c, (a0, a1, a2)):
        if ci == 0:
            continue
        t = ai if ci == 1 else -ai
        s = t if s is None else s + t
    return 0.0 if s is None else s


def collide_guo(f, F, omega):
    """GuoExternalForceBGKdynamics::collide on [m][19] (in place), F: [m][3]; collide_guo's operation order"""
    r = np.zeros(f.shape[0]); x = np.zeros(f.shape[0]); y = np.zeros(f.shape[0]); z = np.zeros(f.shape[0])
    for q in range(19):
        r = r + f[:, q]
        if C[q][0] == 1: x = x + f[:, q]
        elif C[q][0] == -1: x = x + (-f[:, q])
        if C[q][1] == 1: y = y + f[:, q]
        elif C[q][1] == -1: y = y + (-f[:, q])
        if C[q][2] == 1: z = z + f[:, q]
        elif C[q][2] == -1: z = z + (-f[:, q])
    rhoBar = r
    invRho = 1.0 / (1.0 + rhoBar)
    rho = 1.0 + rhoBar
    Fx, Fy, Fz = F[:, 0], F[:, 1], F[:, 2]
    u0 = x * invRho + Fx / 2.0; u1 = y * invRho + Fy / 2.0; u2 = z * invRho + Fz / 2.0
    j0 = rho * u0; j1 = rho * u1; j2 = rho * u2
    jSqr = j0 * j0 + j1 * j1 + j2 * j2
    one_m_omega = 1.0 - omega
    guo = 1.0 - omega / 2.0
    for q in range(19):
        c_j = _cdot(C[q], j0, j1, j2)
        feq = T[q] * (rhoBar + 3.0 * c_j + invRho * (4.5 * c_j * c_j - 1.5 * jSqr))
        f[:, q] = f[:, q] * one_m_omega
        f[:, q] = f[:, q] + omega * feq
    for q in range(19):
        cx, cy, cz = (float(v) for v in C[q])
        c_u = _cdot(C[q], u0, u1, u2)
        c_u = c_u * 9.0
        ft = ((cx - u0) * 3.0 + c_u * cx) * Fx
        ft = ft + ((cy - u1) * 3.0 + c_u * cy) * Fy
        ft = ft + ((cz - u2) * 3.0 + c_u * cz) * Fz
        ft = ft * T[q]
        ft = ft * guo
        f[:, q] = f[:, q] + ft
    return f


def body_field(shape, body, boxes=None, box_forces=None):
    """the body force of every node [nx][ny][nz][3]: `body`, or the force of the last box (inclusive x0, x1, y0, y1, z0, z1)
    that holds the node -- region_force"""
    b = np.empty(tuple(shape) + (3,))
    b[...] = np.asarray(body, dtype=np.float64)
    if boxes is not None:
        for box, f in zip(boxes, box_forces):
            x0, x1, y0, y1, z0, z1 = (int(v) for v in box)
            b[max(x0, 0):x1 + 1, max(y0, 0):y1 + 1, max(z0, 0):z1 + 1] = np.asarray(f, dtype=np.float64)
    return b


def _complete_open(P, fluid, ob_code, ob_val):
    """complete() on the fluid nodes of P [n][19] that carry a code (in place)"""
    if ob_code is None:
        return
    code = np.asarray(ob_code).reshape(-1)
    for kind in range(4):
        sel = fluid & (code >= 0) & ((code & 3) == kind)
        if sel.any():
            P[sel] = complete(P[sel], kind, ob_val[code[sel] >> 2])


def step(S, mask, periodic, omega, body, ob_code=None, ob_val=None, F=None, boxes=None, box_forces=None, wall_u=None):
    """one collide-stream.  S: [nx][ny][nz][19] post-stream; mask [nx][ny][nz] (0 fluid, 3..6 moving-wall classes, any other
    value bounce-back); body (3,); ob_code [nx][ny][nz]: -1 or slot << 2 | kind; ob_val [slots][4]; F [nx][ny][nz][3]: a
    per-node force added to the body force (the kernel's bx + F0, in that order); boxes / box_forces: body-force boxes, the
    last one holding a node wins; wall_u {class: (3,)}: velocities of the moving-wall classes, applied after the swap as
    f[opp(i)] -= 6 t_i (c_i . u_w) for i = 1..18 in ascending order (the oracle's collide_moving_wall).
    Returns the next post-stream state."""
    nx, ny, nz, _ = S.shape
    P = S.reshape(-1, 19).copy()
    m = mask.reshape(-1)
    wall = m != 0
    P[wall] = P[wall][:, OPP]
    if wall_u is not None:
        for cls, w in wall_u.items():
            sel = m == cls
            if not sel.any():
                continue
            w0, w1, w2 = (float(v) for v in w)
            for q in range(1, 19):
                cx, cy, cz = (float(v) for v in C[q])
                c_u = cx * w0 + cy * w1 + cz * w2
                P[sel, OPP[q]] = P[sel, OPP[q]] - 6.0 * T[q] * c_u
    fluid = ~wall
    _complete_open(P, fluid, ob_code, ob_val)
    Ft = body_field((nx, ny, nz), body, boxes, box_forces).reshape(-1, 3)
    if F is not None:
        Ft = Ft + np.asarray(F, dtype=np.float64).reshape(-1, 3)
    P[fluid] = collide_guo(P[fluid], Ft[fluid], omega)
    P = P.reshape(nx, ny, nz, 19)
    out = np.zeros_like(P)
    for q in range(19):
        src = P[:, :, :, q]
        for ax, c in enumerate(C[q]):
            if c == 0:
                continue
            src = np.roll(src, int(c), axis=ax)
            if not periodic[ax]:   # the plane that wrapped around came from outside
                idx = [slice(None)] * 3
                idx[ax] = 0 if c == 1 else -1
                src[tuple(idx)] = 0.0
        out[:, :, :, q] = src
    return out


def observe(S, mask, periodic, body, F=None, ob_code=None, ob_val=None, boxes=None, box_forces=None):
    """what the observers report on the post-stream state S: per node rho [nx][ny][nz], u = j / rho + (body + F) / 2
    [..][3] and the off-equilibrium momentum flux Pi_neq [..][6] (xx, xy, xz, yy, yz, zz), taken AFTER the completion on
    fluid open-boundary nodes -- the populations the next collide relaxes.  So a velocity node shows u_bc + F / 2 and a
    pressure node its prescribed density.  Plain moments everywhere else, bounce-back nodes included.  IEEE double in the
    order of the kernels' moments(): ascending q, zero components skipped.  `periodic` is unused (S is the gathered state)
    and kept so that the call reads like step()."""
    nx, ny, nz, _ = S.shape
    f = S.reshape(-1, 19).copy()
    _complete_open(f, mask.reshape(-1) == 0, ob_code, ob_val)
    n = f.shape[0]
    r = np.zeros(n); j = [np.zeros(n) for _ in range(3)]
    pi = {k: np.zeros(n) for k in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))}
    for q in range(19):
        r = r + f[:, q]
        for d in range(3):
            if C[q][d] == 1: j[d] = j[d] + f[:, q]
            elif C[q][d] == -1: j[d] = j[d] + (-f[:, q])
        for (a, b) in pi:
            cc = C[q][a] * C[q][b]
            if cc == 1: pi[(a, b)] = pi[(a, b)] + f[:, q]
            elif cc == -1: pi[(a, b)] = pi[(a, b)] + (-f[:, q])
    invRho = 1.0 / (1.0 + r)
    Ft = body_field((nx, ny, nz), body, boxes, box_forces).reshape(-1, 3)
    if F is not None:
        Ft = Ft + np.asarray(F, dtype=np.float64).reshape(-1, 3)
    u = np.stack([j[d] * invRho + Ft[:, d] / 2.0 for d in range(3)], axis=1)
    cs2 = 1.0 / 3.0
    out = np.empty((n, 6))
    for k, (a, b) in enumerate(pi):
        v = pi[(a, b)] - invRho * j[a] * j[b]
        if a == b:
            v = v - cs2 * r
        out[:, k] = v
    return (1.0 + r).reshape(nx, ny, nz), u.reshape(nx, ny, nz, 3), out.reshape(nx, ny, nz, 6)


def pipe_radius(fluid_area):
    """PreInlet::calculateDrivingForce: the radius of a circle with the gathered number of fluid nodes of the plane"""
    return np.sqrt(fluid_area / np.pi)


def driving_force(Re, nu, radius, direction="Xpos"):
    """PreInlet::calculateDrivingForce (helper/preInlet.cpp): u_max = Re nu / (2 R), F = 8 nu (u_max / 2) / R / R, in the
    reference's operation order; the force points along -x for Xpos and +x for Xneg (setDrivingForce)"""
    u_max = Re * nu / (radius * 2)
    F = 8 * nu * (u_max * 0.5) / radius / radius
    return u_max, (-F if direction == "Xpos" else F)
