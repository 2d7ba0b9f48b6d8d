"""Restatement of the reference's Lees-Edwards pass (helper/leesEdwardsBC.h) in numpy -- test infrastructure only.

The pass acts on the post-stream state f[n][19] (node n = z + nz*(y + ny*x), values f_i - t_i, Palabos D3Q19 order), as
LeesEdwardsBCGetPopulations (level 1) and LeesEdwardsBCSetPopulations (level 2) do on one block covering the domain:

- every value is read from the state before the pass and written after it;
- a node of the top layer z = nz-1 (bottom z = 0) is copied, relaxed by collideExternal(rhoBar = plain sum, j = (v, 0, 0),
  thetaBar = 0) -- the BGK ma2 collision with the given moments and no forcing term -- and five of its populations are then
  overwritten with g*s1[src] + (1-g)*s2[src], g = fmod(D, 1), from two nodes s1, s2 of the same layer;
- top: s1 = mod+(ceil(D + x), nx), s2 = mod+(floor(D + x), nx); (target <- source) 3<-3, 6<-16, 8<-8, 16<-6, 18<-18;
- bottom: s1 = mod+(floor(-D + x), nx), s2 = mod+(ceil(-D + x), nx); 7<-15, 9<-9, 12<-12, 15<-7, 17<-17.

Taken literally, swaps and extrapolation for D < 0 included.  Every operation is an IEEE double operation in the order the
reference writes it, so the GPU pass (built with -ffp-contract=off) must agree bit for bit.
"""
import math

import numpy as np

C = np.array([[0, 0, 0], [-1, 0, 0], [0, -1, 0], [0, 0, -1], [-1, -1, 0], [-1, 1, 0], [-1, 0, -1], [-1, 0, 1], [0, -1, -1],
              [0, -1, 1], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [1, -1, 0], [1, 0, 1], [1, 0, -1], [0, 1, 1], [0, 1, -1]])
T = np.array([1. / 3.] + [1. / 18.] * 3 + [1. / 36.] * 6 + [1. / 18.] * 3 + [1. / 36.] * 6)

TOP_MAP = ((3, 3), (6, 16), (8, 8), (16, 6), (18, 18))
BOTTOM_MAP = ((7, 15), (9, 9), (12, 12), (15, 7), (17, 17))
# the sensitivity control: the same pass without the 6 <-> 16 / 7 <-> 15 swaps
TOP_MAP_NOSWAP = ((3, 3), (6, 6), (8, 8), (16, 16), (18, 18))
BOTTOM_MAP_NOSWAP = ((7, 7), (9, 9), (12, 12), (15, 15), (17, 17))


def velocities(nz, shear_rate_lbm):
    """LeesEdwardsBC's constructor: (v_top, v_bottom)"""
    v_half = (nz - 1) * shear_rate_lbm * 0.5
    return -v_half, v_half


def displacement(d, it, nx):
    """updateLECurDisplacement(iter)"""
    return math.fmod(d * it, float(nx))


def collide_external(f, v, omega):
    """f: [m][19] copies, relaxed in place; the operation order of the oracle's feq_bar / collide_guo_bgk"""
    rhoBar = np.zeros(f.shape[0])
    for q in range(19):
        rhoBar = rhoBar + f[:, q]
    invRho = 1.0 / (1.0 + rhoBar)
    j = (v, 0.0, 0.0)
    jSqr = j[0] * j[0] + j[1] * j[1] + j[2] * j[2]
    for q in range(19):
        c_j = float(C[q][0]) * j[0] + float(C[q][1]) * j[1] + float(C[q][2]) * j[2]
        feq = T[q] * (rhoBar + 3.0 * c_j + invRho * (4.5 * c_j * c_j - 1.5 * jSqr))
        f[:, q] = f[:, q] * (1.0 - omega)
        f[:, q] = f[:, q] + omega * feq
    return f


def _mod(a, b):
    return (a % b + b) % b


def layer(f4, z, D, v, omega, top, swaps=True):
    """the new populations [nx][ny][19] of layer z, from the pre-pass state f4 [nx][ny][nz][19]"""
    nx, ny = f4.shape[0], f4.shape[1]
    cur = f4[:, :, z, :].reshape(nx * ny, 19).copy()
    collide_external(cur, v, omega)
    out = cur.reshape(nx, ny, 19)
    g = math.fmod(D, 1.0)
    if top:
        s1 = [_mod(int(math.ceil(D + x)), nx) for x in range(nx)]
        s2 = [_mod(int(math.floor(D + x)), nx) for x in range(nx)]
        mp = TOP_MAP if swaps else TOP_MAP_NOSWAP
    else:
        s1 = [_mod(int(math.floor(-D + x)), nx) for x in range(nx)]
        s2 = [_mod(int(math.ceil(-D + x)), nx) for x in range(nx)]
        mp = BOTTOM_MAP if swaps else BOTTOM_MAP_NOSWAP
    src = f4[:, :, z, :]
    a, b = src[s1], src[s2]   # [nx][ny][19]
    for tq, sq in mp:
        out[:, :, tq] = g * a[:, :, sq] + (1 - g) * b[:, :, sq]
    return out


def le_pass(f, dims, omega, D, v_top, v_bottom, swaps=True):
    """one pass on a post-stream state f [n][19]; returns the new state (f is not changed)"""
    nx, ny, nz = dims
    f4 = np.asarray(f).reshape(nx, ny, nz, 19)
    top = layer(f4, nz - 1, D, v_top, omega, True, swaps)
    bottom = layer(f4, 0, D, v_bottom, omega, False, swaps)
    g4 = f4.copy()
    g4[:, :, nz - 1, :] = top
    g4[:, :, 0, :] = bottom
    return g4.reshape(-1, 19)


def le_pass_inplace(f, dims, omega, D, v_top, v_bottom, swaps=True):
    """the same on a writable view (the oracle's OracleLattice.f)"""
    f[...] = le_pass(f, dims, omega, D, v_top, v_bottom, swaps)
