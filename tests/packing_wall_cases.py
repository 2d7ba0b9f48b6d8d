"""Starts and inputs for the wall tests of the packing (tests/test_packing_wall_cpu.py, tests/test_gpu_packing_walls.py), all
from numpy.random.Generator(PCG64(seed)).  Sizes are the scaled ones of the other packing tests (1.2 / 8.4 per um).

  field_mask()   24 x 20 x 16 nodes, periodic in x: slabs on the y and z faces and a sphere of radius 4 nodes centred at
                 x = 22, so that it straddles the periodic face
  plates()       grid 12 x 12 x 8, not periodic in z: 22 RBC + 8 PLT between two plates (mask 24 x 24 x 17 at spacing 0.5,
                 margin 0.1), nominal fraction 0.9, so that the first diameter is 4.04 and most particles overlap a plate or
                 each other; the first four keep the identity orientation, whose principal axis lies along the normal
  pipe_start()   what pack_pipe hands to the device for PIPE at HEMATOCRIT; tests/test_packing_wall_cpu.py records in its
                 docstring how HEMATOCRIT, ITERATION_CAP and END_STEPS were found
  probe_inputs() 60 wall configurations: RBC, PLT and sphere, random and identity quaternions, s from deep overlap through the
                 exact touch s = sqrt(n^T A n) to beyond the slot's cut-off, and below the 1e-6 floor
"""
import numpy as np

from hemocell_amd import packing

SCALE = 1.2 / 8.4
RBC = np.array([8.4, 4.4, 8.4]) * SCALE
PLT = np.array([2.4, 1.05, 2.4]) * SCALE
WBC = np.array([8.4, 8.4, 8.4]) * SCALE


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def field_mask():
    mask = np.zeros((24, 20, 16), dtype=np.uint8)
    mask[:, 0, :] = mask[:, -1, :] = 1
    mask[:, :, 0] = mask[:, :, -1] = 1
    i, j, k = np.indices(mask.shape)
    dx = np.minimum((i - 22) % 24, (22 - i) % 24)
    mask[dx * dx + (j - 9) ** 2 + (k - 7) ** 2 <= 16] = 1
    assert mask[0, 9, 7] == 1 and mask[20, 9, 7] == 1 and mask[2, 9, 7] == 1 and mask[3, 9, 7] == 0
    return mask


class Plates:
    grid = (12, 12, 8)
    counts = (22, 8)
    sizes = np.ascontiguousarray([RBC, PLT])
    nominal = 0.9
    spacing, margin = 0.5, 0.1
    periodic = (True, True, False)

    def __init__(self):
        rng = _rng(21)
        n = sum(self.counts)
        self.n = n
        self.pos = rng.random((n, 3)) * np.array([12.0, 12.0, 6.4]) + np.array([0.0, 0.0, 0.8])
        q = rng.normal(size=(n, 4))
        q /= np.linalg.norm(q, axis=1)[:, None]
        q[:4] = (1.0, 0.0, 0.0, 0.0)
        self.quat = np.ascontiguousarray(q)
        self.mask = np.zeros((24, 24, 17), dtype=np.uint8)
        self.mask[:, :, 0] = self.mask[:, :, -1] = 1


def plates():
    return Plates()


def probe_inputs():
    """size [60][3], quat [60][4] (not normalised: the probe does that), s, unit normal, Douter2, and a tag per row"""
    rng = _rng(22)
    size, quat, s, normal, d2, tags = [], [], [], [], [], []
    for name, sz in (("RBC", RBC), ("PLT", PLT), ("WBC", WBC)):
        for orient in ("identity", "random", "random", "random"):
            q = np.array([1.0, 0, 0, 0]) if orient == "identity" else rng.normal(size=4)
            n = rng.normal(size=3)
            n /= np.linalg.norm(n)
            if orient == "identity":
                n = np.array([0.0, 0.0, -1.0])
            D = float(rng.uniform(0.9, 1.3))
            # the touch: s = (D / 2) sqrt(n^T X n) with X = Q^T diag(size^2) Q of the normalised quaternion
            qq = q / np.linalg.norm(q)
            p, w = qq[1:], qq[0]
            K = np.array([[0, -p[2], p[1]], [p[2], 0, -p[0]], [-p[1], p[0], 0]])
            Q = 2.0 * (np.outer(p, p) - w * K + (w * w - 0.5) * np.eye(3))
            touch = 0.5 * D * np.sqrt(n @ (Q.T @ np.diag(sz ** 2) @ Q) @ n)
            for kind, val in (("deep", 0.2 * touch), ("near_in", touch * (1 - 4e-4)), ("touch", touch), ("near_out", touch * (1 + 4e-4)),
                              ("far", 0.56 * D * sz.max())):
                size.append(sz); quat.append(q); s.append(val); normal.append(n); d2.append(D * D)
                tags.append("%s/%s/%s" % (name, orient, kind))
    assert len(tags) == 60
    # below the floor and at it: the pair is evaluated at 1e-6
    s[0], s[5], s[10] = 0.0, -0.3, 1e-6
    tags[0], tags[5], tags[10] = tags[0] + "@0", tags[5] + "@neg", tags[10] + "@floor"
    return (np.ascontiguousarray(size), np.ascontiguousarray(quat), np.array(s), np.ascontiguousarray(normal), np.array(d2), tags)


PIPE = dict(length_um=24.0, radius_um=20.0, dx_um=0.5, wall_margin_um=1.0, seed=1)
HEMATOCRIT = 0.25
ITERATION_CAP = 5000
END_STEPS = 4392


def pipe_start(hematocrit=HEMATOCRIT):
    """(plan, mask, periodic, pos, spacing, margin)"""
    mask = packing.pipe_mask(PIPE["length_um"], PIPE["radius_um"], PIPE["dx_um"], 0)
    size = [mask.shape[0] * PIPE["dx_um"], (mask.shape[1] - 1) * PIPE["dx_um"], (mask.shape[2] - 1) * PIPE["dx_um"]]
    plan, mask, periodic, _ = packing.wall_plan(size, mask, PIPE["dx_um"], (True, False, False), hematocrit)
    rng = np.random.Generator(np.random.PCG64(PIPE["seed"]))
    pos, spacing, margin = packing.wall_start(plan, mask, PIPE["dx_um"], periodic, PIPE["wall_margin_um"], rng)
    return plan, mask, periodic, pos, spacing, margin
