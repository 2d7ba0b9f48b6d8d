"""Restatement of the immersed-boundary coupling with the three- and four-point delta functions (hcp_type_set_ibm_kernel,
hemocell_amd/csrc/ibm.hip) in extended precision -- test infrastructure only, in the manner of tests/ibm_ref.py, whose
helpers and conventions it uses: values in extended precision rounded to double at the end, every sum returned together with
the sum of the magnitudes of its terms ('<name>_abs').

The reference declares the two functions and implements neither, so the definitions are the standard ones:

  phi3(r) = (1 + sqrt(1 - 3 r^2)) / 3                       |r| <= 0.5
          = (5 - 3 |r| - sqrt(-2 + 6 |r| - 3 r^2)) / 6       0.5 < |r| <= 1.5,  else 0     nodes c - 1, c, c + 1, c = floor(p + 0.5)
  phi4(r) = (3 - 2 |r| + sqrt(1 + 4 |r| - 4 r^2)) / 8        |r| <= 1
          = (5 - 2 |r| - sqrt(-7 + 12 |r| - 4 r^2)) / 8      1 < |r| <= 2,      else 0     nodes f - 1 ... f + 2, f = floor(p)

and the rest is interpolationCoefficientsPhi2: weight = phi(dx) phi(dy) phi(dz), the W^3 nodes in ascending (x, y, z), a node
outside a non-periodic face, a node that is not fluid and a zero weight skipped, the admitted weights divided by their total.
Which branch a distance takes and whether a weight is zero are decided on the doubles the kernel forms (phi_double); the value
is the extended-precision one.

Error scale of a weight.  The outer branches subtract numbers of magnitude one to leave a value that falls to zero like the
square of the distance to the end of the support, so a weight's rounding error is not proportional to the weight.  phi_abs is
the sum of the magnitudes of the terms of phi, the square root counted with the magnitudes under it divided by twice the root
(|d sqrt(B)| = |dB| / (2 sqrt(B))); a weight's scale is the weight plus, per axis, (phi_abs - phi) times the other two factors,
plus ibm_ref's term for a difference p - node that the double does not hold exactly (|p| < 1 only); the division by the total
carries the scales of all admitted weights of the particle, as in ibm_ref.stencil.  A particle within a rounding of the end
of the support on two or three axes at once has a weight that is a product of two or three such remainders, far below the
first-order terms; there the products of two and three per-axis errors count, each error taken as PHI_ROUNDINGS 2^-53 phi_abs,
the bound tests/test_ibm_wide_cpu.py::test_phi_properties holds the kernel's double to.

wrong= : the controls of ibm_ref that make sense here ('no_renormalise', 'admit_walls', 'dead_take_part', 'no_cap'); the
control the issue asks of every case is the other width, which needs no flag: spread(..., W=other).
"""
import numpy as np

from tests import ibm_ref as IR
from tests.observables_ref import HP, hp, to_double, _sqrt

WIDTHS = (3, 4)
PHI_ROUNDINGS = 4.0                          # |phi_double - phi| <= PHI_ROUNDINGS 2^-53 phi_abs
SECOND = hp(PHI_ROUNDINGS) * hp(2.0 ** -53)   # weight of the second-order terms of a product's error scale


def offsets(W):
    return np.array([(i, j, k) for i in range(W) for j in range(W) for k in range(W)])   # idx = (i W + j) W + k


def base(p, W):
    """lowest node of the stencil per axis"""
    p = np.asarray(p, dtype=np.float64)
    return (np.floor(p + 0.5) if W == 3 else np.floor(p)).astype(np.int64) - 1


# ---- the kernel's doubles, operation for operation (hemocell_amd/csrc/ibm_common.h: phi3, phi4)
def phi_double(r, W):
    r = np.abs(np.asarray(r, dtype=np.float64))
    with np.errstate(invalid="ignore"):
        if W == 3:
            inner = (1.0 + np.sqrt(1.0 - 3.0 * r * r)) / 3.0
            outer = (5.0 - 3.0 * r - np.sqrt(-2.0 + 6.0 * r - 3.0 * r * r)) / 6.0
            return np.where(r <= 0.5, inner, np.where(r <= 1.5, outer, 0.0))
        inner = (3.0 - 2.0 * r + np.sqrt(1.0 + 4.0 * r - 4.0 * r * r)) / 8.0
        outer = (5.0 - 2.0 * r - np.sqrt(-7.0 + 12.0 * r - 4.0 * r * r)) / 8.0
        return np.where(r <= 1.0, inner, np.where(r <= 2.0, outer, 0.0))


def phi_hp(R, r_double, W):
    """R: |p - node| in extended precision, r_double: the double the kernel branches on -> (phi, phi_abs)"""
    zero, safe = hp(0.0), hp(1.0)
    r = np.abs(np.asarray(r_double, dtype=np.float64))
    if W == 3:
        sel_in, sel_out = r <= 0.5, (r > 0.5) & (r <= 1.5)
        Bi, Bi_abs = hp(1.0) - hp(3.0) * R * R, hp(1.0) + hp(3.0) * R * R
        Bo, Bo_abs = hp(-2.0) + hp(6.0) * R - hp(3.0) * R * R, hp(2.0) + hp(6.0) * R + hp(3.0) * R * R
        Ai, Ai_abs, Ao, Ao_abs, Di, Do = hp(1.0) + zero * R, hp(1.0) + zero * R, hp(5.0) - hp(3.0) * R, hp(5.0) + hp(3.0) * R, hp(3.0), hp(6.0)
    else:
        sel_in, sel_out = r <= 1.0, (r > 1.0) & (r <= 2.0)
        Bi, Bi_abs = hp(1.0) + hp(4.0) * R - hp(4.0) * R * R, hp(1.0) + hp(4.0) * R + hp(4.0) * R * R
        Bo, Bo_abs = hp(-7.0) + hp(12.0) * R - hp(4.0) * R * R, hp(7.0) + hp(12.0) * R + hp(4.0) * R * R
        Ai, Ai_abs, Ao, Ao_abs, Di, Do = hp(3.0) - hp(2.0) * R, hp(3.0) + hp(2.0) * R, hp(5.0) - hp(2.0) * R, hp(5.0) + hp(2.0) * R, hp(8.0), hp(8.0)
    Bi = np.where(sel_in, Bi, safe); Bo = np.where(sel_out, Bo, safe)       # no root of a negative number outside the branch
    si, so = _sqrt(Bi), _sqrt(Bo)
    inner, inner_abs = (Ai + si) / Di, (Ai_abs + si + Bi_abs / (hp(2.0) * si)) / Di
    outer, outer_abs = (Ao - so) / Do, (Ao_abs + so + Bo_abs / (hp(2.0) * so)) / Do
    return (np.where(sel_in, inner, np.where(sel_out, outer, zero)), np.where(sel_in, inner_abs, np.where(sel_out, outer_abs, zero)))


def stencil(pos, dims, periodic, mask, W, wrong=None, with_abs=False):
    """-> (nodes [n][W^3] int64, -1 where not admitted; weights [n][W^3] extended precision, 0 where not admitted;
    admitted [n][W^3]); with_abs: and the error scale of every weight"""
    p = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    n, off = len(p), offsets(W)
    m = IR._mask3(dims, mask).reshape(-1)
    b = base(p, W)
    P = hp(p)
    # per axis and row: the kernel's double weight, the extended-precision weight and its scale
    rows_d = np.zeros((n, 3, W)); rows = np.zeros((n, 3, W), dtype=HP) + hp(0.0); rows_abs = np.zeros((n, 3, W), dtype=HP) + hp(0.0)
    for i in range(W):
        g = b + i
        d = p - g                                                        # the kernel's doubles
        rows_d[:, :, i] = phi_double(d, W)
        Rx = np.abs(P - hp(g))
        v, va = phi_hp(Rx, d, W)
        lost = np.where(hp(d) == P - hp(g), hp(0.0), Rx)                 # |p - node| where its double is rounded
        rows[:, :, i], rows_abs[:, :, i] = v, va + lost
    N3 = W ** 3
    nodes = np.full((n, N3), -1, np.int64)
    w = np.zeros((n, N3), dtype=HP) + hp(0.0)
    extra = np.zeros((n, N3), dtype=HP) + hp(0.0)
    adm = np.zeros((n, N3), bool)
    for idx, (i, j, k) in enumerate(off):
        flat, ok = IR._resolve(b + off[idx], dims, periodic)
        nonzero = (rows_d[:, 0, i] * rows_d[:, 1, j] * rows_d[:, 2, k]) != 0.0
        a = ok & nonzero
        if wrong != "admit_walls":
            a = a & (m[flat] == 0)
        x, y, z = rows[:, 0, i], rows[:, 1, j], rows[:, 2, k]
        ex, ey, ez = rows_abs[:, 0, i] - np.abs(x), rows_abs[:, 1, j] - np.abs(y), rows_abs[:, 2, k] - np.abs(z)
        nodes[:, idx] = np.where(a, flat, -1)
        w[:, idx] = np.where(a, x * y * z, hp(0.0))
        ax, ay, az = np.abs(x), np.abs(y), np.abs(z)
        extra[:, idx] = np.where(a, ex * ay * az + ax * ey * az + ax * ay * ez + SECOND * (ex * ey * az + ex * ay * ez + ax * ey * ez)
                                 + SECOND * SECOND * ex * ey * ez, hp(0.0))
        adm[:, idx] = a
    if wrong != "no_renormalise":
        tot = w.sum(axis=1)
        total = np.where(tot > 0, tot, hp(1.0))[:, None]
        w = w / total
        extra = extra / total + np.abs(w) * (extra.sum(axis=1)[:, None] / total)
    if with_abs:
        return nodes, w, adm, np.abs(w) + extra
    return nodes, w, adm


def spread(pos, force, rep, alive, dims, periodic, mask, W, f_limit=None, wrong=None):
    """ibm_ref.spread with the W-point stencil"""
    p = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    n, N = len(p), int(np.prod(dims))
    live = IR._live(alive, n, wrong)
    f = hp(np.asarray(force, dtype=np.float64).reshape(n, 3))
    if f_limit is not None and wrong != "no_cap":
        mag = _sqrt((f * f).sum(axis=1))
        over = live & (mag > hp(f_limit))          # a removed particle is not in the list: its force stays
        f = np.where(over[:, None], f * (hp(f_limit) / np.where(over, mag, hp(1.0)))[:, None], f)
    tot = f if rep is None else f + hp(np.asarray(rep, dtype=np.float64).reshape(n, 3))
    nodes, w, adm, w_abs = stencil(p, dims, periodic, mask, W, wrong, with_abs=True)
    sel = adm & live[:, None]
    vi, ki = np.nonzero(sel)
    F = np.zeros((N, 3), dtype=HP) + hp(0.0)
    F_abs = np.zeros((N, 3), dtype=HP) + hp(0.0)
    np.add.at(F, nodes[vi, ki], tot[vi] * w[vi, ki][:, None])
    np.add.at(F_abs, nodes[vi, ki], np.abs(tot[vi]) * w_abs[vi, ki][:, None])
    touched = np.zeros(N, bool)
    touched[nodes[vi, ki]] = True
    has = sel.any(axis=1)
    return dict(F=to_double(F), F_abs=to_double(F_abs), touched=touched, force=to_double(f), force_abs=to_double(np.abs(f)),
                total=to_double(tot[has].sum(axis=0)), total_abs=to_double(F_abs.sum(axis=0)))


def interpolate(pos, alive, u_node, dims, periodic, mask, W, u_abs=None, wrong=None):
    """ibm_ref.interpolate with the W-point stencil"""
    p = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    n = len(p)
    live = IR._live(alive, n, wrong)
    nodes, w, adm, w_abs = stencil(p, dims, periodic, mask, W, wrong, with_abs=True)
    sel = adm & live[:, None]
    at = np.where(sel, nodes, 0)
    ww, wa = np.where(sel, w, hp(0.0)), np.where(sel, w_abs, hp(0.0))
    U = hp(np.asarray(u_node, dtype=np.float64)[at])
    A = np.abs(U) if u_abs is None else hp(np.asarray(u_abs, dtype=np.float64)[at])
    v_abs = (A * np.abs(ww)[:, :, None]).sum(axis=1) + (np.abs(U) * (wa - np.abs(ww))[:, :, None]).sum(axis=1)
    return dict(v=to_double((U * ww[:, :, None]).sum(axis=1)), v_abs=to_double(v_abs))


def needed_nodes(pos, alive, dims, periodic, mask, W):
    """the nodes an interpolation reads (sorted, distinct)"""
    p = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    nodes, _, adm = stencil(p, dims, periodic, mask, W)
    return np.unique(nodes[adm & IR._live(alive, len(p), None)[:, None]])


def predict(pos, alive, dims, periodic, mask, W):
    """The box of one cell's stencil nodes over the particles left: lo = lowest base, hi = highest base + W - 1.
    -> dict(e, vol, exceeds (an extent is larger than a periodic axis), wraps, leaves, nodes (distinct admitted nodes))"""
    p = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    live = IR._live(alive, len(p), None)
    if not live.any():
        return dict(e=(0, 0, 0), vol=0, exceeds=False, wraps=(False,) * 3, leaves=False, nodes=0)
    b = base(p[live], W)
    lo, hi = b.min(axis=0), b.max(axis=0) + W - 1
    e = hi - lo + 1
    exceeds = any(periodic[d] and e[d] > dims[d] for d in range(3))
    ow = [int(lo[d] % dims[d]) if periodic[d] else int(lo[d]) for d in range(3)]
    wraps = tuple(bool(periodic[d] and ow[d] + e[d] > dims[d]) for d in range(3))
    leaves = any((not periodic[d]) and (lo[d] < 0 or hi[d] >= dims[d]) for d in range(3))
    nodes, _, adm = stencil(p[live], dims, periodic, mask, W)
    return dict(e=tuple(int(x) for x in e), vol=int(np.prod(e)), exceeds=exceeds, wraps=wraps, leaves=leaves,
                nodes=int(len(np.unique(nodes[adm]))))


# ----------------------------------------------------------------------------------------------------------------------
# plain double, in the kernels' order of operations
def stencil_double(pos, dims, periodic, mask, W):
    p = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    n, off = len(p), offsets(W)
    m = IR._mask3(dims, mask).reshape(-1)
    b = base(p, W)
    rows = np.stack([phi_double(p - (b + i), W) for i in range(W)], axis=2)     # [n][3][W]
    nodes = np.full((n, W ** 3), -1, np.int64)
    w = np.zeros((n, W ** 3))
    total = np.zeros(n)
    for idx, (i, j, k) in enumerate(off):
        flat, ok = IR._resolve(b + off[idx], dims, periodic)
        weight = rows[:, 0, i] * rows[:, 1, j] * rows[:, 2, k]
        a = ok & (weight != 0.0) & (m[flat] == 0)
        total = total + np.where(a, weight, 0.0)           # total += weight, in visiting order
        nodes[:, idx] = np.where(a, flat, -1)
        w[:, idx] = np.where(a, weight, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        coeff = 1.0 / total
    return nodes, np.where(nodes >= 0, w * coeff[:, None], 0.0)


def spread_double(pos, force, rep, alive, dims, periodic, mask, W, f_limit=None, reverse=False):
    """particle by particle in storage order (reverse: the other way round) -> dict(F [nodes][3] from zero, force)"""
    p = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    n, N = len(p), int(np.prod(dims))
    live = IR._live(alive, n, None)
    f = np.array(force, dtype=np.float64).reshape(n, 3)
    if f_limit is not None:
        mag = np.sqrt((f[:, 0] * f[:, 0] + f[:, 1] * f[:, 1]) + f[:, 2] * f[:, 2])
        over = live & (mag > f_limit)
        f[over] = f[over] * (f_limit / mag[over])[:, None]
    tot = f if rep is None else np.asarray(rep, dtype=np.float64).reshape(n, 3) + f
    nodes, w = stencil_double(p, dims, periodic, mask, W)
    sel = (nodes >= 0) & live[:, None]
    vi, ki = np.nonzero(sel)                                # row-major: particle, then stencil node
    if reverse:
        vi, ki = vi[::-1], ki[::-1]
    F = np.zeros((N, 3))
    np.add.at(F, nodes[vi, ki], tot[vi] * w[vi, ki][:, None])   # unbuffered: one addition after the other
    return dict(F=F, force=f)


def interpolate_double(pos, alive, u_node, dims, periodic, mask, W, reverse=False):
    p = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    live = IR._live(alive, len(p), None)
    nodes, w = stencil_double(p, dims, periodic, mask, W)
    u = np.asarray(u_node, dtype=np.float64)
    v = np.zeros((len(p), 3))
    N3 = W ** 3
    for k in (range(N3 - 1, -1, -1) if reverse else range(N3)):
        sel = (nodes[:, k] >= 0) & live
        v = v + np.where(sel[:, None], u[np.where(sel, nodes[:, k], 0)] * w[:, k][:, None], 0.0)
    return v
