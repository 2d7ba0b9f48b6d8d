"""tests/observables_ref.py on cases whose answers are known in closed form (no GPU)"""
import math
import os
import re

import numpy as np
import pytest

from tests import observables_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_extended_precision_and_velocity_set():
    """the restatement works in more than double precision, and its D3Q19 set is the oracle's orc_c, entry for entry"""
    assert np.finfo(np.longdouble).eps < 1e-18 or R.HP is object
    src = open(os.path.join(ROOT, "oracle", "hemo_oracle.c")).read()
    body = src[src.index("orc_c[ORC_Q][3] = {"):]
    body = body[:body.index("};")]
    rows = [[int(v) for v in m.split(",")] for m in re.findall(r"\{\s*(-?\d+\s*,\s*-?\d+\s*,\s*-?\d+)\s*\}", body)]
    assert np.array_equal(np.array(rows), R.C)
    t = R.t_weights()
    assert abs(float(t.sum()) - 1.0) < 1e-18 and float((t[:, None] * R.C * R.C).sum(0)[0]) == pytest.approx(1 / 3, abs=1e-18)


def _cube(a, shift=(0.0, 0.0, 0.0)):
    v = np.array([[x, y, z] for x in (0, a) for y in (0, a) for z in (0, a)], dtype=np.float64) + np.array(shift)
    # vertex index = 4 x + 2 y + z (0/1 per axis); two triangles per face, counter-clockwise seen from outside
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    tri = []
    for q in quads:
        tri += [(q[0], q[1], q[2]), (q[0], q[2], q[3])]
    return v, np.array(tri)


def _tetra(s):
    v = s * np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]])
    tri = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]])
    return v, tri


@pytest.mark.parametrize("a,shift", [(1.0, (0, 0, 0)), (1.5, (0.25, -2.0, 3.0)), (0.75, (900.0, 17.0, 16.5))])
def test_cube(a, shift):
    v, tri = _cube(a, shift)
    r = R.cell_info(v, tri, stretch=True)
    assert R.excess(r["volume"], a ** 3, r["volume_abs"], 4) <= 1
    assert R.excess(r["area"], 6 * a * a, r["area_abs"], 4) <= 1
    assert R.excess(r["stretch"], a * math.sqrt(3), r["stretch_abs"], 4) <= 1
    assert r["bbox"].tolist() == [shift[0], shift[0] + a, shift[1], shift[1] + a, shift[2], shift[2] + a]
    assert np.array_equal(r["position"], np.array(shift) + a / 2) and r["n"] == 8 and r["complete"]
    if shift[0] == 900.0:   # far from the origin the triple products cancel: the bound has to scale with them, not with V
        assert r["volume_abs"] > 1e5 * a ** 3
    assert abs(R.cell_info(v, tri, wrong="volume_sign")["volume"] - a ** 3) > 0.1 * a ** 3


def test_regular_tetrahedron_and_reversed_orientation():
    v, tri = _tetra(1.25)
    edge = 1.25 * 2 * math.sqrt(2)
    r = R.cell_info(v, tri)
    assert R.excess(r["volume"], edge ** 3 / (6 * math.sqrt(2)), r["volume_abs"], 4) <= 1
    assert R.excess(r["area"], math.sqrt(3) * edge * edge, r["area_abs"], 4) <= 1
    # the reference formula is signed: a mesh wound the other way round has the negative volume, the same area
    rr = R.cell_info(v, tri[:, ::-1])
    assert rr["volume"] == -r["volume"] and rr["area"] == r["area"]
    c, ct = _cube(2.0, (1.0, 1.0, 1.0))
    assert R.cell_info(c, ct[:, [0, 2, 1]])["volume"] == -8.0


def test_removed_particles():
    """CellPosition / CellStretch of helper/cellInfo.cpp: removed particles are skipped, the centroid is divided by the number
    left; the bbox too is over what is left; volume and area stay the triangle sums at the stored positions"""
    v, tri = _cube(2.0, (10.0, 0.0, 0.0))
    vel = np.arange(24, dtype=np.float64).reshape(8, 3)
    alive = np.ones(8, bool); alive[[3, 5, 6, 7]] = False    # one end of every body diagonal gone
    r = R.cell_info(v[None], tri, alive[None], vel[None], stretch=True)
    assert r["n"][0] == 4 and not r["complete"][0]
    assert np.array_equal(r["position"][0], v[alive].mean(0)) and np.array_equal(r["velocity"][0], vel[alive].mean(0))
    assert r["bbox"][0].tolist() == [10.0, 12.0, 0.0, 2.0, 0.0, 2.0]
    assert R.cell_info(v, tri, alive3 := np.arange(8) < 4)["bbox"].tolist() == [10.0, 10.0, 0.0, 2.0, 0.0, 2.0]
    assert r["stretch"][0] == pytest.approx(math.sqrt(8.0), rel=1e-15)     # the longest pair left is a face diagonal
    assert r["volume"][0] == pytest.approx(8.0, rel=1e-14) and r["area"][0] == pytest.approx(24.0, rel=1e-15)
    w = R.cell_info(v[None], tri, alive[None], vel[None], wrong="centroid_over_nv")
    assert abs(w["position"][0] - r["position"][0]).max() > 1.0
    # a cell that lost particles at one corner: the wrong bbox still holds them
    alive2 = np.ones(8, bool); alive2[7] = False
    assert R.cell_info(v, tri, alive2, wrong="bbox_all")["bbox"][1] == 12.0 and R.cell_info(v, tri, alive2)["bbox"][1] == 12.0
    assert R.cell_info(v, tri, alive3, wrong="bbox_all")["bbox"][1] == 12.0


def _states(n, seed):
    rng = np.random.default_rng(seed)
    rho = R.hp(1.0 + 0.05 * rng.standard_normal(n))
    u = R.hp(0.05 * rng.standard_normal((n, 3)))
    return rng, rho, u


def test_pi_neq_of_the_equilibrium_vanishes():
    """the second-order equilibrium carries Pi = rho cs2 I + rho u u exactly on D3Q19, so its off-equilibrium part is zero; what is
    left comes from rounding the populations to double (|df| <= 2^-53 |f|) and must lie inside the bound"""
    rng, rho, u = _states(500, 1)
    feq = R.equilibrium(rho, u)
    exact = R.pi_neq(R.to_double(feq))    # the populations as doubles
    assert R.excess(exact["pi"], 0.0, exact["pi_abs"], 4) <= 1
    # and the moments of the same state
    r = R.rho_u(R.to_double(feq), np.zeros((500, 3)))
    assert R.excess(r["rho"], R.to_double(rho), r["rho_abs"], 4) <= 1
    assert R.excess(r["u"], R.to_double(u), r["u_abs"], 4) <= 1


def test_pi_neq_returns_the_added_stress():
    """f = feq + eps t_i (c_i c_i - cs2 I):Q / (2 cs2^2): no mass, no momentum, second moment eps Q (D3Q19's fourth moment is
    cs2^2 (delta delta + delta delta + delta delta)) -- pi_neq gives eps Q back, component by component in Palabos order"""
    rng, rho, u = _states(400, 2)
    n = len(rho)
    Q = rng.standard_normal((n, 3, 3)); Q = Q + Q.transpose(0, 2, 1)
    Qh = R.hp(Q)
    eps = R.hp(np.full(n, 1e-3))
    t = R.t_weights()
    cc = np.einsum("qa,qb->qab", R.C, R.C).astype(R.HP)
    cs2 = R.CS2
    trQ = Qh[:, 0, 0] + Qh[:, 1, 1] + Qh[:, 2, 2]
    g = t[None, :] * (np.einsum("qab,nab->nq", cc, Qh) - cs2 * trQ[:, None]) / (2 * cs2 * cs2)
    f = R.to_double(R.equilibrium(rho, u) + eps[:, None] * g)
    r = R.pi_neq(f)
    want = np.stack([float(1e-3) * Q[:, a, b] for a, b in R.PI_PAIRS], axis=1)
    assert R.excess(r["pi"], want, r["pi_abs"], 8) <= 1
    assert np.abs(want).min(axis=0).max() > 0
    for wrong in ("swap_xy_xz", "no_cs2"):
        w = R.pi_neq(f, wrong=wrong)
        assert R.excess(w["pi"], want, r["pi_abs"], 16) > 1e6, wrong


def test_rho_u_of_a_constructed_state():
    """populations built for (rho, u - F/2) return rho and u = j / rho + F / 2"""
    rng, rho, u = _states(300, 3)
    F = 1e-4 * rng.standard_normal((300, 3))
    f = R.to_double(R.equilibrium(rho, u - R.hp(F) / 2))
    r = R.rho_u(f, F)
    assert R.excess(r["rho"], R.to_double(rho), r["rho_abs"], 4) <= 1
    assert R.excess(r["u"], R.to_double(u), r["u_abs"], 8) <= 1
    w = R.rho_u(f, F, wrong="no_half_force")
    assert R.excess(w["u"], R.to_double(u), r["u_abs"], 16) > 1e6
