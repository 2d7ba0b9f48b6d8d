"""The any-axis restatement of the Zou-He open boundaries (tests/open_boundary_axis_ref.py) against the pinned x restatement."""
import numpy as np
import pytest

import open_boundary_axis_ref as AX
import open_boundary_ref as OB

STEPS = 50
# the largest population difference measured between a y- or z-face channel and its transposed x-face twin over 50 steps
# (test_axis_channel_equals_the_transposed_x_channel prints the figure of every case), and the bound: ten times that
MEASURED_SYMMETRY_DIFFERENCE = 1.717e-16
SYMMETRY_BOUND = 10 * MEASURED_SYMMETRY_DIFFERENCE


def _guard(S, mask, code, axes, val):
    """finite, and |rho - 1| < 0.1 on fluid nodes (completed moments), as the x tests ask of every compared run"""
    assert np.isfinite(S).all()
    rho, _, _ = AX.observe(S, mask, AX.NONPER, AX.BODY, None, code, axes, val)
    dev = float(np.abs(rho[mask == 0] - 1.0).max())
    assert dev < 0.1, dev


@pytest.mark.parametrize("axis", [1, 2])
def test_permutations(axis):
    p = AX.PERM[axis]
    assert sorted(p) == list(range(19)) and np.array_equal(p[p], np.arange(19))   # an involution
    swapped = OB.C.copy()
    swapped[:, [0, axis]] = swapped[:, [axis, 0]]
    assert np.array_equal(OB.C[p], swapped)            # C -> C with the two columns exchanged
    assert np.array_equal(OB.T[p], OB.T)               # keeps the weights
    opp = np.array(OB.OPP)
    assert np.array_equal(p[opp], opp[p])              # commutes with the opposite
    assert not np.array_equal(p, np.arange(19))
    assert np.array_equal(AX.PERM[0], np.arange(19))


def test_axis_0_is_the_x_restatement_bit_for_bit():
    """the `four` layout of tests/test_gpu_open_boundary.py (all four kinds on a walled 24 x 17 x 19 channel), 50 steps"""
    dims = AX.CHANNEL_DIMS[0]
    mask = AX.channel_mask(dims, 0)
    code, axes, val = AX.declaration(dims, AX.channel_patches("four", 0, dims))
    assert set(int(k) for k in code[code >= 0] & 3) == {0, 1, 2, 3} and (axes[code >= 0] == 0).all()
    S = AX.initial_state(dims)
    R = S.copy()
    for _ in range(STEPS):
        S = AX.step(S, mask, AX.NONPER, AX.OMEGA, AX.BODY, code, axes, val)
        R = OB.step(R, mask, AX.NONPER, AX.OMEGA, AX.BODY, code, val)
        assert np.array_equal(S, R)
    _guard(S, mask, code, axes, val)
    ra, ua, pa = AX.observe(S, mask, AX.NONPER, AX.BODY, None, code, axes, val)
    rb, ub, pb = OB.observe(S, mask, AX.NONPER, AX.BODY, None, code, val)
    assert np.array_equal(ra, rb) and np.array_equal(ua, ub) and np.array_equal(pa, pb)
    assert not np.array_equal(S, OB.step(S, mask, AX.NONPER, AX.OMEGA, AX.BODY))   # the declaration matters


@pytest.mark.parametrize("layout", ["original", "mirrored", "four"])
@pytest.mark.parametrize("axis", [1, 2])
def test_axis_channel_equals_the_transposed_x_channel(axis, layout):
    """A channel open along y (z) against the x-face channel of the same restatement with x and y (z) exchanged in the mask,
    the declaration, the values, the body force and the initial populations, 50 steps.  The two agree only to rounding: the
    completion is the same arithmetic on permuted populations, but the collide's moment sums run in index order, which the
    permutation changes.  Measured, the largest population difference on a fluid node at any of
    the 50 steps: axis 1 1.717e-16 (original), 1.618e-16 (mirrored), 8.413e-17 (four); axis 2 8.717e-17, 1.331e-16, 1.665e-16
    (populations are of order 5e-3 to 5e-2, so this is a few ulp).  The bound is ten times the largest figure, 1.717e-15:
    headroom for rounding across libm and numpy builds; it stays far below the 1e-9 to which coupled runs agree."""
    dims = AX.CHANNEL_DIMS[axis]
    p = AX.PERM[axis]
    mask = AX.channel_mask(dims, axis)
    code, axes, val = AX.declaration(dims, AX.channel_patches(layout, axis, dims))
    assert (axes[code >= 0] == axis).all()
    body = np.array(AX.BODY)
    # the twin: every array with node axes 0 and `axis` exchanged, vectors with components 0 and `axis` exchanged
    mask_x, code_x = np.ascontiguousarray(mask.swapaxes(0, axis)), np.ascontiguousarray(code.swapaxes(0, axis))
    axes_x = np.where(code_x >= 0, 0, -1)
    val_x = AX.swap_columns(val, axis)
    body_x = AX.swap_columns(body[None, :], axis)[0]
    S = AX.initial_state(dims)
    X = np.ascontiguousarray(S.swapaxes(0, axis)[..., p])
    worst = 0.0
    for _ in range(STEPS):
        S = AX.step(S, mask, AX.NONPER, AX.OMEGA, body, code, axes, val)
        X = AX.step(X, mask_x, AX.NONPER, AX.OMEGA, body_x, code_x, axes_x, val_x)
        _guard(S, mask, code, axes, val)
        _guard(X, mask_x, code_x, axes_x, val_x)
        back = X.swapaxes(0, axis)[..., p]
        worst = max(worst, float(np.abs(S - back)[mask == 0].max()))
    print("axis %d, %s: largest population difference to the transposed x channel over %d steps: %.3e" % (axis, layout, STEPS, worst))
    assert worst <= SYMMETRY_BOUND, worst
    assert not np.array_equal(S, OB.step(S, mask, AX.NONPER, AX.OMEGA, body))
