"""CPU restatement of the ellipsoid force-bias packing step, for the packing tests.

The arithmetic lives in tests/packing_ref.cpp (the step of DESIGN §6 "packing": pair contact function, bounded root
search, ascending-index sums, motion, control scalars); this module compiles it with g++ -O2 -ffp-contract=off, as
tests/cabi is compiled, and wraps it in numpy.  It shares nothing with hemocell_amd/csrc/packing.hip."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_DP = C.POINTER(C.c_double)
_IP = C.POINTER(C.c_int)

STATUS = ("steps", "finished", "Douter", "Dinner", "Pactual", "DensityNominal", "Force_step", "Relax", "Nsf", "error", "maxeval")


def _d(a):
    return a.ctypes.data_as(_DP)


def _i(a):
    return a.ctypes.data_as(_IP)


@functools.lru_cache(maxsize=None)
def lib():
    out = os.path.join(tempfile.mkdtemp(prefix="packing_ref_"), "libpacking_ref.so")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-o", out, os.path.join(_HERE, "packing_ref.cpp")],
                   check=True, capture_output=True, text=True)
    L = C.CDLL(out)
    L.pkref_pair.argtypes = [_DP, _DP, _DP, _DP, _DP, C.c_double, C.c_int, _DP, _IP]
    L.pkref_pair.restype = None
    L.pkref_create.argtypes = [_IP, C.c_int, _DP, _IP, _DP, _DP, C.c_double, C.c_int, C.c_int, C.c_double]
    L.pkref_create.restype = C.c_void_p
    L.pkref_run.argtypes = [C.c_void_p, C.c_int]
    L.pkref_run.restype = None
    L.pkref_status.argtypes = [C.c_void_p, _DP]
    L.pkref_status.restype = None
    L.pkref_state.argtypes = [C.c_void_p, _DP, _DP, _DP, _DP]
    L.pkref_state.restype = None
    L.pkref_destroy.argtypes = [C.c_void_p]
    L.pkref_destroy.restype = None
    L.pkref_min_contact.argtypes = [_IP, C.c_int, _DP, _IP, _DP, _DP, C.c_double, _IP, _IP]
    L.pkref_min_contact.restype = C.c_double
    return L


def pair(sizeA, qA, sizeB, qB, rij, Douter2, rotate):
    """one pair as Packing::calc_forces(e, ei, ej) sees it; qA, qB = (s, p) before Quaternion(s, p) normalises.
    Returns a dict: lambda, fscl (= 4 f_AB(lambda), 0 when the pair gives nothing), n, fA, tA, fB, tB (increments),
    kind (0 nothing, 1 no overlap, 2 overlap), evals, capped."""
    a = [np.ascontiguousarray(x, dtype=np.float64) for x in (sizeA, qA, sizeB, qB, rij)]
    out = np.zeros(17)
    flags = np.zeros(3, dtype=np.int32)
    lib().pkref_pair(_d(a[0]), _d(a[1]), _d(a[2]), _d(a[3]), _d(a[4]), float(Douter2), int(rotate), _d(out), _i(flags))
    return {"lambda": out[0], "fscl": out[1], "n": out[2:5].copy(), "fA": out[5:8].copy(), "tA": out[8:11].copy(),
            "fB": out[11:14].copy(), "tB": out[14:17].copy(), "kind": int(flags[0]), "evals": int(flags[1]), "capped": int(flags[2])}


class Packing:
    """the restated Packing: create runs Packing::init and the first calc_forces, run(n) up to n iterations"""

    def __init__(self, grid, sizes, counts, pos, quat=None, nominal=0.5, rotate=True, ntau=102400, epsilon=0.1):
        self.grid = np.ascontiguousarray(grid, dtype=np.int32)
        self.sizes = np.ascontiguousarray(sizes, dtype=np.float64).reshape(-1, 3)
        self.counts = np.ascontiguousarray(counts, dtype=np.int32)
        self.n = int(self.counts.sum())
        pos = np.ascontiguousarray(pos, dtype=np.float64).reshape(self.n, 3)
        q = None if quat is None else np.ascontiguousarray(quat, dtype=np.float64).reshape(self.n, 4)
        self._h = lib().pkref_create(_i(self.grid), len(self.counts), _d(self.sizes), _i(self.counts), _d(pos),
                                     None if q is None else _d(q), float(nominal), int(bool(rotate)), int(ntau), float(epsilon))

    def run(self, steps):
        lib().pkref_run(self._h, int(steps))
        return self.status()

    def status(self):
        st = np.zeros(12)
        lib().pkref_status(self._h, _d(st))
        d = dict(zip(STATUS, st[:11]))
        for k in ("steps", "finished", "Nsf", "error", "maxeval"):
            d[k] = int(d[k])
        d["pairs"] = int(st[11])
        return d

    def state(self):
        pos, quat, f, t = np.zeros((self.n, 3)), np.zeros((self.n, 4)), np.zeros((self.n, 3)), np.zeros((self.n, 3))
        lib().pkref_state(self._h, _d(pos), _d(quat), _d(f), _d(t))
        return pos, quat, f, t

    def __del__(self):
        if getattr(self, "_h", None):
            lib().pkref_destroy(self._h)
            self._h = None


def min_contact(grid, sizes, counts, pos, quat, Douter):
    """brute force over all pairs, minimum image: (smallest f_AB, pairs with f_AB < 1, pairs whose root search gave nothing)"""
    grid = np.ascontiguousarray(grid, dtype=np.int32)
    sizes = np.ascontiguousarray(sizes, dtype=np.float64)
    counts = np.ascontiguousarray(counts, dtype=np.int32)
    pos = np.ascontiguousarray(pos, dtype=np.float64)
    quat = np.ascontiguousarray(quat, dtype=np.float64)
    ov, sk = C.c_int(0), C.c_int(0)
    m = lib().pkref_min_contact(_i(grid), len(counts), _d(sizes), _i(counts), _d(pos), _d(quat), float(Douter), C.byref(ov), C.byref(sk))
    return m, ov.value, sk.value


def initial_positions(grid, n, seed):
    """deviation 4 of the design: uniform times the box from numpy's PCG64, in particle order"""
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.random((n, 3)) * np.asarray(grid, dtype=np.float64)
