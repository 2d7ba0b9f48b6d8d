"""Restatement of the output-path observables in extended precision -- test infrastructure only.

What the HDF5 fields, the CellInfo CSV and the FluidInfo / ParticleInfo statistics are made of, written out plainly:

- rho_u(f, F): rho = 1 + sum_i f_i, u = j / rho + F / 2 (f: post-stream populations f_i - t_i [n][19], Palabos D3Q19
  order; F: body force plus spread force [n][3]), as Cell::computeVelocity of the Guo-forced BGK dynamics;
- pi_neq(f): Pi_ab = sum_i c_ia c_ib f_i - j_a j_b / rho - cs2 rhoBar delta_ab, components xx, xy, xz, yy, yz, zz
  (Palabos' momentTemplates::compute_rhoBar_j_PiNeq, the formula the kernel states);
- cell_info(pos, tri, alive, vel): per cell the reference's (helper/cellInfo.cpp) volume (signed six-term triple product
  over the triangles, /6), area (sum of triangle areas), bbox (x0 x1 y0 y1 z0 z1), centroid, velocity and stretch (largest
  vertex-vertex distance).  Removed particles (alive == False) are skipped and centroid / velocity divide by the number
  left (CellPosition); stretch skips pairs that contain one (CellStretch); bbox is taken over the particles left.
  Volume and area are the triangle sums at the stored positions whatever is alive (the reference leaves them undefined
  for an incomplete cell).

Every value is computed in np.longdouble (64-bit significand) or, where that type is plain double, in mpmath at 113 bits,
and rounded to double at the end.  Every function also returns, per output, the sum of the magnitudes of the terms it is
made of ('<name>_abs'), so a comparison can scale its tolerance with how well conditioned the sum is:
|gpu - ref| <= k * 2^-53 * abs.

wrong=<name> gives a deliberately wrong restatement (the mutation controls of the tests): a comparison against it has to
fail by far, or the tolerance would not be able to see a wrong kernel.
"""
import numpy as np

# D3Q19 in Palabos order: the data of oracle/hemo_oracle.c's orc_c (tests/test_observables_cpu.py checks the copy)
C = np.array([[0, 0, 0], [-1, 0, 0], [0, -1, 0], [0, 0, -1], [-1, -1, 0], [-1, 1, 0], [-1, 0, -1], [-1, 0, 1], [0, -1, -1],
              [0, -1, 1], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [1, -1, 0], [1, 0, 1], [1, 0, -1], [0, 1, 1], [0, 1, -1]])
W = [(1, 3)] + [(1, 18)] * 3 + [(1, 36)] * 6 + [(1, 18)] * 3 + [(1, 36)] * 6   # t_i as fractions
PI_PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))                    # xx xy xz yy yz zz

if np.finfo(np.longdouble).eps < 1e-18:
    HP = np.longdouble

    def hp(x):
        return np.asarray(x, dtype=np.float64).astype(np.longdouble)

    def _sqrt(x):
        return np.sqrt(x)

    def _const(num, den):
        return np.longdouble(num) / np.longdouble(den)

    def to_double(x):
        return np.asarray(x, dtype=np.longdouble).astype(np.float64)
else:   # long double is plain double on this platform: 113-bit mpmath numbers in object arrays
    import mpmath
    mpmath.mp.prec = 113
    HP = object
    _mpf = np.vectorize(mpmath.mpf, otypes=[object])
    _msqrt = np.vectorize(mpmath.sqrt, otypes=[object])
    _mfloat = np.vectorize(float, otypes=[np.float64])

    def hp(x):
        return _mpf(np.asarray(x, dtype=np.float64))

    def _sqrt(x):
        return _msqrt(x)

    def _const(num, den):
        return mpmath.mpf(num) / mpmath.mpf(den)

    def to_double(x):
        return _mfloat(np.asarray(x, dtype=object))

CS2 = _const(1, 3)


def t_weights():
    return np.array([_const(a, b) for a, b in W], dtype=HP)


def _moments(f):
    f = hp(f)
    S = np.abs(f).sum(axis=1)
    rhoBar = f.sum(axis=1)
    j = f @ C.astype(HP)                       # [n][3]: sum_i c_ia f_i
    J = np.abs(f) @ np.abs(C).astype(HP)       # sum_i |c_ia f_i|
    return f, rhoBar, S, j, J


def rho_u(f, F, wrong=None):
    """-> dict(rho, u [n][3], rho_abs, u_abs).  wrong='no_half_force': u = j / rho + F"""
    f, rhoBar, S, j, J = _moments(f)
    F = hp(F)
    rho = 1 + rhoBar
    half = 1 if wrong == "no_half_force" else _const(1, 2)
    u = j / rho[:, None] + F * half
    # j / rho: the error of j (sum of |c_ia f_i|) and that of 1 / rho (sum of 1 and |f_i|, relative to rho)
    u_abs = J * ((1 + S) / (rho * rho))[:, None] + np.abs(F) * half
    return dict(rho=to_double(rho), u=to_double(u), rho_abs=to_double(1 + S), u_abs=to_double(u_abs))


def pi_neq(f, wrong=None):
    """-> dict(pi [n][6], pi_abs).  wrong='swap_xy_xz' (components 1 and 2 exchanged) or 'no_cs2' (no cs2 rhoBar term)"""
    f, rhoBar, S, j, J = _moments(f)
    rho = 1 + rhoBar
    pi, pi_abs = [], []
    for a, b in PI_PAIRS:
        cc = (C[:, a] * C[:, b]).astype(HP)
        v = f @ cc - j[:, a] * j[:, b] / rho
        va = np.abs(f) @ np.abs(cc) + J[:, a] * J[:, b] * (1 + S) / (rho * rho)
        if a == b:
            if wrong != "no_cs2":
                v = v - CS2 * rhoBar
            va = va + CS2 * S
        pi.append(v); pi_abs.append(va)
    pi, pi_abs = np.stack(pi, axis=1), np.stack(pi_abs, axis=1)
    if wrong == "swap_xy_xz":
        pi = pi[:, [0, 2, 1, 3, 4, 5]]
    return dict(pi=to_double(pi), pi_abs=to_double(pi_abs))


def equilibrium(rho, u):
    """second-order equilibrium in the stored representation, feq_i - t_i = t_i (rho (1 + 3 c.u + 4.5 (c.u)^2 - 1.5 u.u) - 1)
    [n][19] in extended precision, for rho [n] and u [n][3] given in it"""
    t = t_weights()
    cu = u @ C.T.astype(HP)                    # [n][19]
    uu = (u * u).sum(axis=1)
    return t[None, :] * (rho[:, None] * (1 + 3 * cu + _const(9, 2) * cu * cu - _const(3, 2) * uu[:, None]) - 1)


def cell_info(pos, tri, alive=None, vel=None, stretch=False, wrong=None):
    """pos [nc][nv][3] (or [nv][3]), tri [nt][3] vertex indices, alive [nc][nv] bool (default: all), vel like pos.
    -> dict(volume, area, bbox [nc][6], position [nc][3], n (particles left), complete, and with vel / stretch: velocity,
    stretch), each value with '<name>_abs'.  wrong='centroid_over_nv' (centroid and velocity divided by nv),
    'bbox_all' (bbox over every stored position), 'volume_sign' (one term of the triple product with the wrong sign)"""
    pos = np.asarray(pos, dtype=np.float64)
    one = pos.ndim == 2
    if one:
        pos = pos[None]
    nc, nv, _ = pos.shape
    alive = np.ones((nc, nv), bool) if alive is None else np.asarray(alive, bool).reshape(nc, nv)
    tri = np.asarray(tri, dtype=np.int64)
    p = hp(pos)
    v0, v1, v2 = p[:, tri[:, 0]], p[:, tri[:, 1]], p[:, tri[:, 2]]      # [nc][nt][3]
    terms = [-1 * v2[..., 0] * v1[..., 1] * v0[..., 2], v1[..., 0] * v2[..., 1] * v0[..., 2], v2[..., 0] * v0[..., 1] * v1[..., 2],
             -1 * v0[..., 0] * v2[..., 1] * v1[..., 2], -1 * v1[..., 0] * v0[..., 1] * v2[..., 2], v0[..., 0] * v1[..., 1] * v2[..., 2]]
    if wrong == "volume_sign":
        terms[5] = -1 * terms[5]
    six = _const(1, 6)
    volume = sum(terms).sum(axis=1) * six
    volume_abs = sum(np.abs(t) for t in terms).sum(axis=1) * six
    e1, e2 = v1 - v0, v2 - v0
    n = np.stack([e1[..., 1] * e2[..., 2] - e1[..., 2] * e2[..., 1], e1[..., 2] * e2[..., 0] - e1[..., 0] * e2[..., 2],
                  e1[..., 0] * e2[..., 1] - e1[..., 1] * e2[..., 0]], axis=-1)
    half = _const(1, 2)
    area = (half * _sqrt((n * n).sum(axis=-1))).sum(axis=1)
    # |n| is formed from differences of the stored positions: its error scales with |e1| |e2|, not with |n|
    area_abs = (half * _sqrt((e1 * e1).sum(axis=-1) * (e2 * e2).sum(axis=-1))).sum(axis=1)
    live = alive if wrong != "bbox_all" else np.ones_like(alive)
    bbox = np.empty((nc, 6))
    for d in range(3):
        x = np.where(live, pos[..., d], np.inf)
        bbox[:, 2 * d] = x.min(axis=1)
        bbox[:, 2 * d + 1] = np.where(live, pos[..., d], -np.inf).max(axis=1)
    cnt = alive.sum(axis=1)
    div = np.full(nc, nv) if wrong == "centroid_over_nv" else cnt
    w = hp(alive.astype(np.float64))[..., None]
    out = dict(volume=to_double(volume), volume_abs=to_double(volume_abs), area=to_double(area), area_abs=to_double(area_abs),
               bbox=bbox, n=cnt, complete=cnt == nv,
               position=to_double((p * w).sum(axis=1) / hp(div)[:, None]),
               position_abs=to_double((np.abs(p) * w).sum(axis=1) / hp(div)[:, None]))
    if vel is not None:
        v = hp(np.asarray(vel, dtype=np.float64).reshape(nc, nv, 3))
        out["velocity"] = to_double((v * w).sum(axis=1) / hp(div)[:, None])
        out["velocity_abs"] = to_double((np.abs(v) * w).sum(axis=1) / hp(div)[:, None])
    if stretch:
        st, st_abs = np.zeros(nc), np.zeros(nc)
        for c in range(nc):
            q = p[c][alive[c]]
            best, best_abs = 0, 0
            for i in range(len(q) - 1):   # one row of the pair matrix at a time: meshes of 1500 vertices stay small
                d = q[i + 1:] - q[i]
                d2 = (d * d).sum(axis=1)
                k = int(np.argmax(to_double(d2)))
                if d2[k] > best:
                    best, best_abs = d2[k], (np.abs(q[i + 1 + k]) + np.abs(q[i])).sum()
            st[c] = to_double(_sqrt(np.array([best], dtype=HP)))[0]
            st_abs[c] = to_double(np.array([best_abs], dtype=HP))[0]
        out["stretch"], out["stretch_abs"] = st, st_abs
    if one:
        out = {k: (v[0] if isinstance(v, np.ndarray) else v) for k, v in out.items()}
    return out


def excess(got, ref, ref_abs, k=16.0):
    """largest |got - ref| / (k 2^-53 ref_abs); <= 1 passes.  A zero bound (every term zero) asks for equality."""
    got, ref, ref_abs = (np.asarray(a, dtype=np.float64) for a in (got, ref, ref_abs))
    err = np.abs(got - ref)
    tol = k * 2.0 ** -53 * ref_abs
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(r.max()) if r.size else 0.0
