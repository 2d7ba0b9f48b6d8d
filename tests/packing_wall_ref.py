"""CPU restatement of the packing's wall term, for the wall tests.

tests/packing_wall_ref.cpp holds the arithmetic: it includes tests/packing_ref.cpp unchanged (pair function, step, control
scalars) and restates what hc_packing_set_walls adds -- the three distance passes on integers, the trilinear sample of the
node field (along z, then y, then x) and its analytic gradient, the mirror image with its quaternion (0, z) q (0, n), the
wall slot added after a particle's partners, the wrap on periodic axes only and the wall-node error.  Compiled as
packing_ref.py compiles its file, g++ -O2 -ffp-contract=off; everything is fp64 in the kernels' operation order.  It
shares nothing with hemocell_amd/csrc/packing.hip."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np

import packing_ref as R

_HERE = os.path.dirname(os.path.abspath(__file__))
_DP, _IP = R._DP, R._IP
_d, _i = R._d, R._i
_UP = C.POINTER(C.c_ubyte)
STATUS = R.STATUS


def _u(a):
    return a.ctypes.data_as(_UP)


@functools.lru_cache(maxsize=None)
def lib():
    out = os.path.join(tempfile.mkdtemp(prefix="packing_wall_ref_"), "libpacking_wall_ref.so")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-o", out, os.path.join(_HERE, "packing_wall_ref.cpp")],
                   check=True, capture_output=True, text=True)
    L = C.CDLL(out)
    L.pkwref_field.argtypes = [_UP, _IP, _IP, C.c_int, _DP]
    L.pkwref_field.restype = None
    L.pkwref_truncation.argtypes = [C.c_double, _DP, C.c_int, C.c_double, C.c_double]
    L.pkwref_truncation.restype = C.c_int
    L.pkwref_sample.argtypes = [_DP, _IP, _IP, C.c_double, C.c_double, _DP, _DP]
    L.pkwref_sample.restype = C.c_int
    L.pkwref_image_quat.argtypes = [_DP, _DP, _DP]
    L.pkwref_image_quat.restype = None
    L.pkwref_wall.argtypes = [_DP, _DP, C.c_double, _DP, C.c_double, C.c_int, _DP, _IP]
    L.pkwref_wall.restype = None
    L.pkwref_create.argtypes = [_IP, C.c_int, _DP, _IP, _DP, _DP, C.c_double, C.c_int, C.c_int, C.c_double, _UP, _IP, C.c_double, _IP, C.c_double]
    L.pkwref_create.restype = C.c_void_p
    L.pkwref_run.argtypes = [C.c_void_p, C.c_int]
    L.pkwref_run.restype = None
    L.pkwref_status.argtypes = [C.c_void_p, _DP]
    L.pkwref_status.restype = None
    L.pkwref_state.argtypes = [C.c_void_p, _DP, _DP, _DP, _DP]
    L.pkwref_state.restype = None
    L.pkwref_snode.argtypes = [C.c_void_p, _DP]
    L.pkwref_snode.restype = None
    L.pkwref_destroy.argtypes = [C.c_void_p]
    L.pkwref_destroy.restype = None
    L.pkwref_check.argtypes = [C.c_void_p, _DP, _DP, C.c_double, _IP]
    L.pkwref_check.restype = C.c_double
    return L


def _i3(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def truncation(Douter, sizes, spacing, margin):
    """R in nodes: ceil((0.55 Douter (largest axis of any species) + margin) / spacing + 1/2) + 1"""
    s = np.ascontiguousarray(sizes, dtype=np.float64).reshape(-1, 3)
    return lib().pkwref_truncation(float(Douter), _d(s), len(s), float(spacing), float(margin))


def field(mask, periodic, R_nodes):
    """s_node = sqrt(min(d^2, R^2)) - 1/2 by the three separable passes"""
    m = np.ascontiguousarray(mask, dtype=np.uint8)
    out = np.zeros(m.shape)
    lib().pkwref_field(_u(m), _i(_i3(m.shape)), _i(_i3([int(bool(p)) for p in periodic])), int(R_nodes), _d(out))
    return out


def brute_force_field(mask, periodic, R_nodes):
    """the same field from the definition: the minimum over all wall nodes of the squared minimum-image distance, in numpy"""
    m = np.asarray(mask, dtype=bool)
    wall = np.argwhere(m)
    idx = np.indices(m.shape).reshape(3, -1).T
    best = np.full(len(idx), R_nodes * R_nodes, dtype=np.int64)
    for lo in range(0, len(wall), 256):
        d = idx[:, None, :] - wall[None, lo:lo + 256, :]
        for k in range(3):
            if periodic[k]:
                n = m.shape[k]
                d[:, :, k] = (d[:, :, k] + n // 2) % n - n // 2
        best = np.minimum(best, (d * d).sum(axis=2).min(axis=1))
    return (np.sqrt(best.astype(np.float64)) - 0.5).reshape(m.shape)


def sample(snode, periodic, spacing, margin, x):
    """(s, n, ok) at x (grid cells)"""
    f = np.ascontiguousarray(snode, dtype=np.float64)
    out = np.zeros(4)
    ok = lib().pkwref_sample(_d(f), _i(_i3(f.shape)), _i(_i3([int(bool(p)) for p in periodic])), float(spacing), float(margin),
                             _d(np.ascontiguousarray(x, dtype=np.float64)), _d(out))
    return out[0], out[1:].copy(), bool(ok)


def image_quat(q, n):
    out = np.zeros(4)
    lib().pkwref_image_quat(_d(np.ascontiguousarray(q, dtype=np.float64)), _d(np.ascontiguousarray(n, dtype=np.float64)), _d(out))
    return out


def wall(size, q, s, n, Douter2, rotate):
    """a particle against its mirror image across the plane at distance s along -n, as the wall slot and hc_packing_walls
    evaluate it: force, torque, candidate (Douter2 unless it overlaps), kind, evals, capped; lambda and fscl for the tests"""
    out, flags = np.zeros(9), np.zeros(3, dtype=np.int32)
    a = [np.ascontiguousarray(v, dtype=np.float64) for v in (size, q, n)]
    lib().pkwref_wall(_d(a[0]), _d(a[1]), float(s), _d(a[2]), float(Douter2), int(rotate), _d(out), _i(flags))
    return {"f": out[0:3].copy(), "t": out[3:6].copy(), "candidate": out[6], "lambda": out[7], "fscl": out[8],
            "kind": int(flags[0]), "evals": int(flags[1]), "capped": int(flags[2])}


class WallPacking:
    """the restated packing with walls: create runs Packing::init and the first force evaluation with the wall slot"""

    def __init__(self, grid, sizes, counts, pos, quat, nominal, rotate, mask, spacing, periodic, margin, ntau=102400, epsilon=0.1):
        self.grid = _i3(grid)
        self.sizes = np.ascontiguousarray(sizes, dtype=np.float64).reshape(-1, 3)
        self.counts = _i3(counts)
        self.n = int(self.counts.sum())
        pos = np.ascontiguousarray(pos, dtype=np.float64).reshape(self.n, 3)
        q = None if quat is None else np.ascontiguousarray(quat, dtype=np.float64).reshape(self.n, 4)
        self.mask = np.ascontiguousarray(mask, dtype=np.uint8)
        self._h = lib().pkwref_create(_i(self.grid), len(self.counts), _d(self.sizes), _i(self.counts), _d(pos), None if q is None else _d(q),
                                      float(nominal), int(bool(rotate)), int(ntau), float(epsilon), _u(self.mask), _i(_i3(self.mask.shape)),
                                      float(spacing), _i(_i3([int(bool(p)) for p in periodic])), float(margin))

    def run(self, steps):
        lib().pkwref_run(self._h, int(steps))
        return self.status()

    def status(self):
        st = np.zeros(14)
        lib().pkwref_status(self._h, _d(st))
        d = dict(zip(STATUS, st[:11]))
        for k in ("steps", "finished", "Nsf", "error", "maxeval"):
            d[k] = int(d[k])
        d["pairs"], d["wall_slots"], d["truncation"] = int(st[11]), int(st[12]), int(st[13])
        return d

    def state(self):
        pos, quat, f, t = np.zeros((self.n, 3)), np.zeros((self.n, 4)), np.zeros((self.n, 3)), np.zeros((self.n, 3))
        lib().pkwref_state(self._h, _d(pos), _d(quat), _d(f), _d(t))
        return pos, quat, f, t

    def snode(self):
        out = np.zeros(self.mask.shape)
        lib().pkwref_snode(self._h, _d(out))
        return out

    def check(self, pos, quat, Douter):
        """brute force at Douter: (smallest f_AB over pairs and wall slots, overlapping pairs, overlapping wall slots,
        evaluations that gave nothing, particles without a normal)"""
        c = np.zeros(4, dtype=np.int32)
        best = lib().pkwref_check(self._h, _d(np.ascontiguousarray(pos, dtype=np.float64)), _d(np.ascontiguousarray(quat, dtype=np.float64)),
                                  float(Douter), _i(c))
        return best, int(c[0]), int(c[1]), int(c[2]), int(c[3])

    def __del__(self):
        if getattr(self, "_h", None):
            lib().pkwref_destroy(self._h)
            self._h = None
