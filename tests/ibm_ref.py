"""Restatement of the immersed-boundary coupling in extended precision -- test infrastructure only.

Written from the reference's core/immersedBoundaryMethod.h (interpolationCoefficientsPhi2) and
core/hemoCellParticleField.cpp (spreadParticleForce, interpolateFluidVelocity), with the helpers and the conventions of
tests/observables_ref.py: values in extended precision rounded to double at the end, every sum returned together with the
sum of the magnitudes of its terms ('<name>_abs'), wrong=<name> for the mutation controls.

- stencil(pos, dims, periodic, mask): per particle the 2 x 2 x 2 nodes that can carry a non-zero tent weight, visited in
  ascending (dx, dy, dz) as the reference's 27-node loop visits them.  The base node is floor(p + 0.5), one lower where
  p < base; phi2(x) = max(0, 1 - |x|); a node is admitted when it is inside the domain (wrapped on a periodic axis: one global
  block, the reference reaches the same nodes through envelope copies), its weight is non-zero and its mask is 0; the
  weights are divided by the admitted total.  Whether a weight is zero is decided on the double the reference forms
  (the differences p - node are exact for |p| >= 1, which every crafted position respects near an integer); its value is
  the extended-precision product.
- spread(...): F[node] = sum over particles of (force_repulsion + force) * weight, force capped to f_limit first
  (FORCE_LIMIT); particles removed from the list (alive == False) take no part and keep their force.
- interpolate(...): v = sum_j u(node_j) * weight_j; u_node is given per node (observables_ref.rho_u of the downloaded
  populations and force field), u_abs its error scale.
- predict(...): what the bounding box of a cell's stencil nodes is: extents, volume, bricks, wraps, distinct nodes.
- spread_double / interpolate_double: the same two sums in plain double, particle by particle in a given order, operation
  for operation as the reference writes them (what a run of the reference would hold bit for bit).

Node indices are z + nz * (y + ny * x); mask is [nx][ny][nz], non-zero = boundary.

wrong= : 'no_renormalise' (weights not divided by the admitted total), 'admit_walls' (the mask is ignored), 'truncate'
(int(p + 0.5) instead of floor: negative coordinates differ), 'admit_zero_weight' (zero-weight nodes are admitted: the
sums do not change, the node count does), 'dead_take_part' (removed particles spread and are interpolated), 'shift_z'
(every node index one too high along z: a wrong tile decode), 'no_cap' (spread without FORCE_LIMIT).
"""
import numpy as np

from tests.observables_ref import HP, hp, to_double, _sqrt

OFFSETS = np.array([(i, j, k) for i in range(2) for j in range(2) for k in range(2)])   # idx = 4 i + 2 j + k


def _base(p, wrong=None):
    c = np.trunc(p + 0.5) if wrong == "truncate" else np.floor(p + 0.5)
    return c.astype(np.int64) - (p < c)


def _phi2_double(x):
    x = 1.0 - np.abs(x)
    return np.where(x > 0.0, x, 0.0)


def _mask3(dims, mask):
    return np.zeros(dims, np.uint8) if mask is None else np.asarray(mask).reshape(dims)


def _resolve(g, dims, periodic):
    """global node coordinates [n][3] -> (flat index, inside): wrapped on periodic axes, outside elsewhere"""
    ok = np.ones(len(g), bool)
    w = g.copy()
    for d in range(3):
        if periodic[d]:
            w[:, d] = np.mod(g[:, d], dims[d])
        else:
            ok &= (g[:, d] >= 0) & (g[:, d] < dims[d])
    w[~ok] = 0
    return (w[:, 0] * dims[1] + w[:, 1]) * dims[2] + w[:, 2], ok


def stencil(pos, dims, periodic, mask, wrong=None, with_abs=False):
    """-> (nodes [n][8] int64, -1 where not admitted; weights [n][8] extended precision, 0 where not admitted; admitted [n][8]);
    with_abs: and the error scale of every weight.  That is the weight itself, except where the reference's double p - node
    is not exact (|p| < 1 only): there phi = 1 - |p - node| carries the rounding of a number of magnitude up to 1 however
    small phi is, and so do the weight, the total and every normalised weight of that particle."""
    p = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    n = len(p)
    m = _mask3(dims, mask).reshape(-1)
    b = _base(p, wrong)
    P = hp(p)
    one = hp(1.0)
    nodes = np.full((n, 8), -1, np.int64)
    w = np.zeros((n, 8), dtype=HP) + hp(0.0)
    extra = np.zeros((n, 8), dtype=HP) + hp(0.0)             # error scale beyond the weight itself
    adm = np.zeros((n, 8), bool)
    for idx, off in enumerate(OFFSETS):
        g = b + off
        flat, ok = _resolve(g + (np.array([0, 0, 1]) if wrong == "shift_z" else 0), dims, periodic)
        d = p - g                                                        # the reference's doubles
        nonzero = (_phi2_double(d[:, 0]) * _phi2_double(d[:, 1]) * _phi2_double(d[:, 2])) != 0.0
        if wrong == "admit_zero_weight":
            nonzero = np.ones(n, bool)
        x = one - np.abs(P - hp(g))
        x = np.where(x > 0, x, hp(0.0))
        a = ok & nonzero
        if wrong != "admit_walls":
            a = a & (m[flat] == 0)
        nodes[:, idx] = np.where(a, flat, -1)
        w[:, idx] = np.where(a, x[:, 0] * x[:, 1] * x[:, 2], hp(0.0))
        adm[:, idx] = a
        lost = np.where(hp(d) == P - hp(g), hp(0.0), np.abs(P - hp(g)))      # per axis: |p - node| where its double is rounded
        extra[:, idx] = np.where(a, lost[:, 0] * x[:, 1] * x[:, 2] + x[:, 0] * lost[:, 1] * x[:, 2] + x[:, 0] * x[:, 1] * lost[:, 2], hp(0.0))
    if wrong != "no_renormalise":
        total = np.where(w.sum(axis=1) > 0, w.sum(axis=1), one)[:, None]
        w = w / total
        extra = extra / total + w * (extra.sum(axis=1)[:, None] / total)
    if with_abs:
        return nodes, w, adm, w + extra
    return nodes, w, adm


def _live(alive, n, wrong):
    if alive is None or wrong == "dead_take_part":
        return np.ones(n, bool)
    return np.asarray(alive, bool).reshape(n)


def spread(pos, force, rep, alive, dims, periodic, mask, f_limit=None, wrong=None):
    """-> dict(F [nodes][3], F_abs, touched [nodes] bool, force [n][3] (after the cap), force_abs, total [3], total_abs [3]);
    rep None: no repulsion force; f_limit None: no cap"""
    p = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    n, N = len(p), int(np.prod(dims))
    live = _live(alive, n, wrong)
    f = hp(np.asarray(force, dtype=np.float64).reshape(n, 3))
    if f_limit is not None and wrong != "no_cap":
        mag = _sqrt((f * f).sum(axis=1))
        over = live & (mag > hp(f_limit))          # a removed particle is not in the list: its force stays
        f = np.where(over[:, None], f * (hp(f_limit) / np.where(over, mag, hp(1.0)))[:, None], f)
    tot = f if rep is None else f + hp(np.asarray(rep, dtype=np.float64).reshape(n, 3))
    nodes, w, adm, w_abs = stencil(p, dims, periodic, mask, wrong, with_abs=True)
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


def interpolate(pos, alive, u_node, dims, periodic, mask, u_abs=None, wrong=None):
    """u_node [nodes][3] (only admitted nodes are read), u_abs its error scale (default |u_node|)
    -> dict(v [n][3], v_abs); removed particles: 0"""
    p = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    n = len(p)
    live = _live(alive, n, wrong)
    nodes, w, adm, w_abs = stencil(p, dims, periodic, mask, wrong, with_abs=True)
    sel = adm & live[:, None]
    at = np.where(sel, nodes, 0)
    ww, wa = np.where(sel, w, hp(0.0)), np.where(sel, w_abs, hp(0.0))
    U = hp(np.asarray(u_node, dtype=np.float64)[at])                     # [n][8][3]
    A = np.abs(U) if u_abs is None else hp(np.asarray(u_abs, dtype=np.float64)[at])
    # a rounded weight moves v by |u| dw, a rounded u by w du
    v_abs = (A * ww[:, :, None]).sum(axis=1) + (np.abs(U) * (wa - ww)[:, :, None]).sum(axis=1)
    return dict(v=to_double((U * ww[:, :, None]).sum(axis=1)), v_abs=to_double(v_abs))


def needed_nodes(pos, alive, dims, periodic, mask):
    """the nodes an interpolation reads (sorted, distinct)"""
    p = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    nodes, _, adm = stencil(p, dims, periodic, mask)
    return np.unique(nodes[adm & _live(alive, len(p), None)[:, None]])


def predict(pos, alive, dims, periodic, mask, pad_x=2, wrong=None):
    """The box of one cell's stencil nodes, over the particles left: lo = lowest base, hi = highest base + 1.
    -> dict(e (extents hi - lo + 1), vol, exceeds (an extent is larger than a periodic axis), wraps (per axis: the box, its
    origin wrapped into the domain, crosses the periodic face), leaves (it reaches beyond a non-periodic face), bricks
    (8 x 8 x 8 bricks the box spans, x counted from pad_x planes below the domain; None when it wraps or leaves), nodes
    (distinct admitted nodes))"""
    p = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    live = _live(alive, len(p), wrong)
    b = _base(p[live])
    lo, hi = b.min(axis=0), b.max(axis=0) + 1
    e = hi - lo + 1
    exceeds = any(periodic[d] and e[d] > dims[d] for d in range(3))
    ow = [int(lo[d] % dims[d]) if periodic[d] else int(lo[d]) for d in range(3)]
    wraps = tuple(bool(periodic[d] and ow[d] + e[d] > dims[d]) for d in range(3))
    leaves = any((not periodic[d]) and (lo[d] < 0 or hi[d] >= dims[d]) for d in range(3))
    bricks = None
    if not (any(wraps) or leaves):
        bricks = 1
        for d in range(3):
            first = ow[d] + (pad_x if d == 0 else 0)
            bricks *= ((first + int(e[d]) - 1) >> 3) - (first >> 3) + 1
    nodes, _, adm = stencil(p[live], dims, periodic, mask, wrong)
    return dict(e=tuple(int(x) for x in e), vol=int(np.prod(e)), exceeds=exceeds, wraps=wraps, leaves=leaves, bricks=bricks,
                nodes=int(len(np.unique(nodes[adm]))))


# ----------------------------------------------------------------------------------------------------------------------
# plain double, in the reference's order of operations
def stencil_double(pos, dims, periodic, mask):
    p = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    n = len(p)
    m = _mask3(dims, mask).reshape(-1)
    b = _base(p)
    nodes = np.full((n, 8), -1, np.int64)
    w = np.zeros((n, 8))
    total = np.zeros(n)
    for idx, off in enumerate(OFFSETS):
        g = b + off
        flat, ok = _resolve(g, dims, periodic)
        d = p - g
        weight = _phi2_double(d[:, 0]) * _phi2_double(d[:, 1]) * _phi2_double(d[:, 2])
        a = ok & (weight != 0.0) & (m[flat] == 0)
        total = total + np.where(a, weight, 0.0)           # total_weight += weight, in visiting order
        nodes[:, idx] = np.where(a, flat, -1)
        w[:, idx] = np.where(a, weight, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        coeff = 1.0 / total
    return nodes, np.where(nodes >= 0, w * coeff[:, None], 0.0)


def spread_double(pos, force, rep, alive, dims, periodic, mask, f_limit=None, reverse=False):
    """particle by particle in storage order (reverse: the other way round) -> dict(F [nodes][3] from zero, force)"""
    p = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    n, N = len(p), int(np.prod(dims))
    live = _live(alive, n, None)
    f = np.array(force, dtype=np.float64).reshape(n, 3)
    if f_limit is not None:
        mag = np.sqrt((f[:, 0] * f[:, 0] + f[:, 1] * f[:, 1]) + f[:, 2] * f[:, 2])
        over = live & (mag > f_limit)
        f[over] = f[over] * (f_limit / mag[over])[:, None]
    tot = f if rep is None else np.asarray(rep, dtype=np.float64).reshape(n, 3) + f
    nodes, w = stencil_double(p, dims, periodic, mask)
    sel = (nodes >= 0) & live[:, None]
    vi, ki = np.nonzero(sel)                                # row-major: particle, then stencil node
    if reverse:
        vi, ki = vi[::-1], ki[::-1]
    F = np.zeros((N, 3))
    np.add.at(F, nodes[vi, ki], tot[vi] * w[vi, ki][:, None])   # unbuffered: one addition after the other
    return dict(F=F, force=f)


def interpolate_double(pos, alive, u_node, dims, periodic, mask, reverse=False):
    p = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    live = _live(alive, len(p), None)
    nodes, w = stencil_double(p, dims, periodic, mask)
    u = np.asarray(u_node, dtype=np.float64)
    v = np.zeros((len(p), 3))
    for k in (range(7, -1, -1) if reverse else range(8)):
        sel = (nodes[:, k] >= 0) & live
        v = v + np.where(sel[:, None], u[np.where(sel, nodes[:, k], 0)] * w[:, k][:, None], 0.0)
    return v
