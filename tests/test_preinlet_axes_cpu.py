"""The pre-inlet's fluid coupling in six directions without a GPU: the C ABI and its binding name the new entry points and the
library exports them, the driving force as a vector, and the in-plane index conventions of hcl_plane_velocity_axis."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["hcl_plane_velocity_axis", "hcl_preinlet_create", "hcl_preinlet_apply", "hcl_preinlet_iterate",
               "hcl_preinlet_destroy"]
DIRECTIONS = {"Xneg": (0, 1.0), "Xpos": (0, -1.0), "Yneg": (1, 1.0), "Ypos": (1, -1.0), "Zneg": (2, 1.0), "Zpos": (2, -1.0)}


def test_header_binding_and_library_name_the_new_abi():
    src = open(os.path.join(ROOT, "include", "hemocell_amd.h")).read()
    for n in NEW_SYMBOLS:
        assert re.search(r"^int\s+" + n + r"\s*\(", src, flags=re.M), n
    assert re.search(r"^typedef\s+struct\s+hc_preinlet\s+hc_preinlet\s*;", src, flags=re.M)
    from hemocell_amd import capi, host
    lib = ctypes.CDLL(capi.LIB_PATH)
    for n in NEW_SYMBOLS:
        assert n in capi.SIGNATURES, n
        assert hasattr(lib, n), "libhemocell_amd.so does not export " + n
    assert callable(host.Lattice.planeVelocityAxis) and callable(host.Lattice.planeVelocity)
    for n in ("applyPreInlet", "iterate", "sent", "destroy"):
        assert callable(getattr(host.PreInlet, n)), n


def _driving_force_ref(Re, nu, area, direction):
    """PreInlet::calculateDrivingForce and setDrivingForce restated: R = sqrt(A / pi), u_max = Re nu / (R 2),
    F = 8 nu (u_max 0.5) / R / R on the direction's axis, + for *neg and - for *pos"""
    radius = math.sqrt(area / math.pi)
    u_max = Re * nu / (radius * 2)
    force = 8 * nu * (u_max * 0.5) / radius / radius
    axis, sign = DIRECTIONS[direction]
    F = [0.0, 0.0, 0.0]
    F[axis] = sign * force
    return radius, u_max, tuple(F)


@pytest.mark.parametrize("area", [1257, 317, 52])
def test_driving_force_vector_in_six_directions(area):
    from hemocell_amd import host
    Re, nuP, dx, dt = 0.5, 1.1e-6, 5e-7, 1e-7   # the fixture case of tests/test_preinlet_cpu.py
    nu = nuP * dt / (dx * dx)
    for d in DIRECTIONS:
        R, u_max, F = host.preinlet_driving_force_vector(Re, nu, area, d)
        assert (R, u_max, tuple(F)) == _driving_force_ref(Re, nu, area, d), d
        axis, sign = DIRECTIONS[d]
        assert len(F) == 3 and F[axis] * sign > 0 and all(F[a] == 0.0 for a in range(3) if a != axis)
    for d in ("Xpos", "Xneg"):   # bit for bit the scalar function on its two directions
        R, u_max, Fx = host.preinlet_driving_force(Re, nu, area, d)
        assert host.preinlet_driving_force_vector(Re, nu, area, d) == (R, u_max, (Fx, 0.0, 0.0))
    with pytest.raises(host.HcError, match="Xpos and Xneg"):
        host.preinlet_driving_force(Re, nu, area, "Zpos")
    with pytest.raises(host.HcError, match="unknown direction"):
        host.preinlet_driving_force_vector(Re, nu, area, "Wpos")


def test_in_plane_index_conventions():
    """y * nz + z, x * nz + z, x * ny + y: the node's offset with the axis removed, the remaining axes in lattice order"""
    from hemocell_amd import host
    dims = (11, 12, 13)
    x, y, z = [c.reshape(-1) for c in np.meshgrid(*[np.arange(d) for d in dims], indexing="ij")]
    coords = (x, y, z)
    for axis in range(3):
        others = [a for a in range(3) if a != axis]
        got = host.plane_index(dims, axis, coords[others[0]], coords[others[1]])
        want = np.ravel_multi_index((coords[others[0]], coords[others[1]]), (dims[others[0]], dims[others[1]]))
        assert np.array_equal(got, want), axis
        assert got.min() == 0 and got.max() == dims[others[0]] * dims[others[1]] - 1
    assert np.array_equal(host.plane_index(dims, 0, y, z), y * 13 + z)
    assert np.array_equal(host.plane_index(dims, 1, x, z), x * 13 + z)
    assert np.array_equal(host.plane_index(dims, 2, x, y), x * 12 + y)
    with pytest.raises(host.HcError, match="axis"):
        host.plane_index(dims, 3, 0, 0)
