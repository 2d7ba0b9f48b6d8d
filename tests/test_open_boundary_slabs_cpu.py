"""slab.open_boundary_rows -- the clipping and row selection behind SlabRunner.add_open_boundary / set_open_velocity /
set_open_density -- against plain numpy loops: boxes that cover one slab, straddle two or three, or miss one; the per-rank
node lists put together in rank order are the global box order; per-node values reach the right rank and row."""
import numpy as np
import pytest

from hemocell_amd.slab import open_boundary_rows

NXG, NY, NZ = 48, 5, 7


def _box_nodes(box):
    return [(x, y, z) for x in range(box[0], box[1] + 1) for y in range(box[2], box[3] + 1) for z in range(box[4], box[5] + 1)]


BOXES = {
    "one slab": (13, 20, 0, NY - 1, 0, NZ - 1),
    "whole first plane": (0, 0, 0, NY - 1, 0, NZ - 1),
    "last plane": (NXG - 1, NXG - 1, 1, 3, 2, 5),
    "two slabs": (10, 14, 1, 3, 0, NZ - 1),
    "three slabs": (11, 35, 2, 2, 1, 4),
    "everything": (0, NXG - 1, 0, NY - 1, 0, NZ - 1),
    "one node on a face plane": (24, 24, 3, 3, 3, 3),
}


@pytest.mark.parametrize("world", [1, 2, 3, 4])
@pytest.mark.parametrize("name", sorted(BOXES))
def test_box_is_clipped_and_translated(world, name):
    box = BOXES[name]
    g = _box_nodes(box)
    nx = NXG // world
    u = np.random.default_rng(3).uniform(-1, 1, (len(g), 3))
    rho = 1.0 + np.arange(len(g)) * 1e-3
    seen_nodes, seen_rows, missed = [], [], 0
    for rank in range(world):
        x0 = rank * nx
        local, nodes, rows, vals = open_boundary_rows(box, x0, nx, 3, u)
        want = [(k, (x - x0, y, z)) for k, (x, y, z) in enumerate(g) if x0 <= x < x0 + nx]
        assert [tuple(int(c) for c in n) for n in nodes] == [n for _, n in want]
        assert rows.tolist() == [k for k, _ in want]
        assert np.array_equal(vals, u[[k for k, _ in want]].reshape(-1, 3))
        if not want:
            missed += 1
            assert local is None and len(nodes) == 0 and vals.shape == (0, 3)
        else:
            # the clipped box, walked in box order, is the node list: slots within a rank stay in box order
            assert local[0] == max(box[0], x0) - x0 and local[1] == min(box[1], x0 + nx - 1) - x0 and local[2:] == box[2:]
            assert _box_nodes(local) == [n for _, n in want]
            assert 0 <= local[0] <= local[1] < nx
        r1 = open_boundary_rows(box, x0, nx, 1, rho)[3]
        assert np.array_equal(r1.reshape(-1), rho[rows])
        one = open_boundary_rows(box, x0, nx, 3, (0.1, 0.2, 0.3))[3]      # one value for all
        assert one.shape == (len(rows), 3) and (one == np.array([0.1, 0.2, 0.3])).all()
        seen_nodes += [(n[0] + x0, n[1], n[2]) for _, n in want]
        seen_rows += rows.tolist()
    assert seen_nodes == g and seen_rows == list(range(len(g)))           # rank order = global box order
    if name == "one slab" and world == 4:
        assert missed == 3
    if name == "three slabs" and world == 4:
        assert missed == 1
    if name == "two slabs" and world == 4:
        assert missed == 2


def test_node_list_keeps_list_order_and_routes_values():
    rng = np.random.default_rng(5)
    g = np.stack([rng.integers(0, NXG, 40), rng.integers(0, NY, 40), rng.integers(0, NZ, 40)], axis=1)
    rho = rng.uniform(0.99, 1.01, 40)
    got = np.full(40, np.nan)
    for rank in range(3):
        x0, nx = rank * 16, 16
        local, nodes, rows, vals = open_boundary_rows(g, x0, nx, 1, rho)
        assert local is None
        assert (np.diff(rows) > 0).all()
        assert np.array_equal(nodes + [x0, 0, 0], g[rows])
        assert ((nodes[:, 0] >= 0) & (nodes[:, 0] < nx)).all()
        assert np.isnan(got[rows]).all()
        got[rows] = vals.reshape(-1)
    assert np.array_equal(got, rho)


def test_two_node_list_is_not_taken_for_a_box():
    """an [n][3] list of two nodes has six numbers, as a box has; the shape decides"""
    g = [[3, 1, 2], [30, 4, 6]]
    _, nodes, rows, _ = open_boundary_rows(g, 24, 24)
    assert rows.tolist() == [1] and nodes.tolist() == [[6, 4, 6]]
