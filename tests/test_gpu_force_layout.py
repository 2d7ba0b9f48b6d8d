"""The IBM force field is stored node by node, F[x+2][y][z][3]: the per-cell spread kernel (LDS node list,
one flush of all three components), its per-vertex fallback and the gather-form spread write that record; the collide, the
interpolation and the downloads read it.  The atomic spread must give the reproducible spread's field to the rounding of its
sums, and hcl_download_ibm_force keeps returning [x][y][z][3] over the bulk nodes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NX, NY, NZ = 48, 34, 34
# across the periodic seam, next to the pipe wall (mask tile and stencils that lose nodes to the wall), in the lumen
CELLS = [((46.5, 14.2, 15.1), (90, 0, 0)), ((18.0, 14.5, 9.6), (90, 20, 0)), ((30.0, 17.0, 17.0), (70, 30, 10))]


def _spread(gpu, reproducible, scale=1.0, forces=None, padded=False):
    """one spread of seeded vertex forces into a fresh pipe lattice; scale > 1 blows the first cell up beyond the tile of the
    per-cell kernel (per-vertex fallback with direct atomics)"""
    lib = gpu.capi.lib()
    gpu.check(lib.hc_set_reproducible_spread(1 if reproducible else 0))
    gpu.check(lib.hc_debug_force_plane_padding(1 if padded else 0))
    try:
        P = gpu.base_parameters()
        mask, _ = gpu.pipe_mask(NX, NY, NZ)
        L = gpu.Lattice(NX, NY, NZ, (1, 0, 0), 1.0 / P.tau)
        L.defineBounceBack(mask); L.latticeEquilibrium(); L.setExternalVector((0.0, 0.0, 0.0))
        h = gpu.HemoCell(L, P); cf = h.cellfields
        cf.addCellType(gpu.CellType.rbc(P), 1)
        for c, a in CELLS:
            assert cf.addCell(0, c, a)
        pos = cf.positions
        nv = 642
        c0 = pos[:nv].mean(0)
        pos[:nv] = c0 + scale * (pos[:nv] - c0)
        cf.positions = pos
        cf.forces = forces if forces is not None else 1e-4 * np.random.default_rng(5).standard_normal(pos.shape)
        cf.spreadParticleForce(False)
        F = L.ibm_force()
        L.destroy()
        return F, mask
    finally:
        gpu.check(lib.hc_set_reproducible_spread(0))
        gpu.check(lib.hc_debug_force_plane_padding(0))


@pytest.mark.parametrize("scale,padded", [(1.0, False), (1.0, True), (1.5, False)])
def test_atomic_spread_equals_reproducible_spread(gpu, scale, padded):
    """the per-cell kernel (and, scale 1.5, its per-vertex fallback) against the gather form, which sums in a fixed order"""
    Fa, mask = _spread(gpu, False, scale, padded=padded)
    Fr, _ = _spread(gpu, True, scale, padded=padded)
    assert np.abs(Fr).max() > 0
    assert np.abs(Fa - Fr).max() <= 1e-14 * np.abs(Fr).max(), np.abs(Fa - Fr).max()
    touched = np.abs(Fr).sum(1) != 0
    assert np.array_equal(np.abs(Fa).sum(1) != 0, touched)          # the same nodes, nothing written elsewhere
    assert not touched[mask.reshape(-1) != 0].any()                  # stencils admit fluid nodes only
    x = np.nonzero(touched.reshape(NX, NY * NZ).any(1))[0]
    assert 0 in x and NX - 1 in x                                    # the seam cell spreads onto both ends of the pipe


@pytest.mark.parametrize("reproducible", [False, True])
def test_downloaded_force_keeps_its_layout(gpu, reproducible):
    """every vertex carries the force g = (1, -2, 4) * 1e-6: node by node the three downloaded components are g times one sum of
    weights, so the ratios are exact (the gather form sums in one order for all components; the atomic kernels in the order the
    hardware takes them, hence the tolerance there)"""
    n = len(CELLS) * 642
    g = np.array([1.0, -2.0, 4.0]) * 1e-6
    F, _ = _spread(gpu, reproducible, forces=np.tile(g, (n, 1)))
    touched = F[:, 0] != 0
    assert touched.sum() > 1000
    tol = 0.0 if reproducible else 1e-14 * np.abs(F).max()
    assert np.abs(F[:, 1] + 2.0 * F[:, 0]).max() <= tol and np.abs(F[:, 2] - 4.0 * F[:, 0]).max() <= tol
    assert (F[touched, 0] > 0).all()
    # the weights of every vertex sum to one: the field carries the whole force of the cells
    assert abs(F[:, 0].sum() - n * g[0]) <= 1e-12 * n * g[0]
