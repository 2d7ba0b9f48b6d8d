"""The geometries of tests/lattice_geometry_cases.py hold the properties the GPU tests of tests/test_gpu_lattice_geometry.py
rest on (no GPU): a geometry that loses its property fails here instead of passing vacuously there.  Also: three wrong
classification rules differ from the right one on the geometries meant to tell them apart, and one missing bounce changes the
oracle's fluid populations within the 9 steps the GPU tests run."""
import numpy as np
import pytest

import lattice_geometry_cases as G

PADDED = [False, True]


def _report(name, padded):
    g = G.GEOMETRIES[name]
    cls, before = g.classes(padded)
    return g, cls, before, G.span_report(cls)


def _differs(g, padded, **wrong):
    return int((g.classes(padded, **wrong)[0] != g.classes(padded)[0]).sum())


@pytest.mark.parametrize("padded", PADDED)
@pytest.mark.parametrize("name", list(G.GEOMETRIES) + ["stenosis_open"])
def test_classes_and_spans_are_consistent(name, padded):
    """for every geometry: fluid stays 0, only solid nodes without a fluid neighbour turn inert, promotion only takes nodes
    back, every node that is not inert lies in its row's span, and the spans hold nothing else but the inert nodes counted"""
    g = G.STENOSIS_OPEN if name == "stenosis_open" else G.GEOMETRIES[name]
    cls, before = g.classes(padded)
    r = G.span_report(cls)
    assert np.array_equal(cls == 0, g.mask == 0) and np.array_equal(before == 0, g.mask == 0)
    assert np.all(before[cls == 2] == 2) and np.all(np.isin(cls[before == 2], (1, 2)))
    assert np.array_equal(cls[before != 2], before[before != 2])
    assert int(r["length"].sum()) - r["inert_inside"] == int((cls != 2).sum())
    assert np.array_equal(r["active"], r["length"].sum(axis=1))
    z = np.arange(g.dims[2])[None, None, :]
    in_span = (z >= r["z0"][:, :, None]) & (z < (r["z0"] + r["length"])[:, :, None])
    assert np.all(in_span[cls != 2])


@pytest.mark.parametrize("padded", PADDED)
def test_stenosis(padded):
    g, cls, before, r = _report("stenosis", padded)
    assert g.dims == (20, 22, 22) and g.periodic == (1, 0, 0)
    assert (cls == 2).sum() == 1296 and (before == 2).sum() == 3592
    assert r["empty_rows"] == 30 and r["rows_z0"] == 20
    counts = sorted(set(r["active"].tolist()))
    assert len(counts) == 4 and counts[0] == 304 and counts[-1] == 448          # one max_active over planes of different counts
    assert len(r["seams"]) == 18
    assert len({cls[x].tobytes() for x in range(g.dims[0])}) > 4                # the geometry changes from plane to plane
    assert _differs(g, padded, faces_only=True) == 288


@pytest.mark.parametrize("padded", PADDED)
def test_stenosis_open(padded):
    """the non-periodic variant: the same classes, and the inlet plane x = 0 has inert corners and rows that start at z0 > 0"""
    g = G.STENOSIS_OPEN
    cls, _ = g.classes(padded)
    r = G.span_report(cls)
    assert g.periodic == (0, 0, 0) and (cls == 2).sum() == 1296
    assert cls[0, 0, 0] == 2 and cls[0, -1, -1] == 2
    assert ((r["length"][0] > 0) & (r["z0"][0] > 0)).any() and ((r["length"][-1] > 0) & (r["z0"][-1] > 0)).any()
    assert (g.mask[0] == 0).any() and (g.mask[-1] == 0).any()


@pytest.mark.parametrize("padded", PADDED)
def test_thick_walls(padded):
    g, cls, before, r = _report("thick_walls", padded)
    assert g.dims == (10, 12, 37) and g.periodic == (1, 0, 1) and g.dims[2] % 2 == 1 and g.dims[2] % G.LINE != 0
    assert (cls == 2).sum() == 1736
    assert r["empty_rows"] == 30 and r["rows_z0"] == 10
    assert r["inert_inside"] == 16
    assert len(r["seams"]) == 10
    # the nodes behind the faces y = 2 and y = 8 are inert: what the moving-wall test leaves unvisited
    assert np.all(cls[:, 0, :16] == 2) and np.all(cls[:, 11, 16:32] == 2) and np.all(cls[:, 2, :] == 1) and np.all(cls[:, 8, :] == 1)


@pytest.mark.parametrize("padded", PADDED)
def test_solid_planes(padded):
    g, cls, before, r = _report("solid_planes", padded)
    assert g.dims == (12, 9, 18) and g.periodic == (0, 0, 0)
    assert (cls == 2).sum() == 162
    assert (r["active"] == 0).sum() == 1 and r["active"][5] == 0                 # cum[ny] == 0 on one plane
    assert np.all(g.mask[4:7] == 1) and (g.mask[:4] == 0).any() and (g.mask[7:] == 0).any()   # two unconnected chambers


@pytest.mark.parametrize("padded", PADDED)
def test_seam_slabs(padded):
    g, cls, before, r = _report("seam_slabs", padded)
    assert g.dims == (12, 10, 32) and g.periodic == (1, 1, 1)
    assert (cls == 2).sum() == 736
    assert (r["active"] == 0).sum() == 1
    assert _differs(g, padded, yz_wrap=False) == 1696
    assert _differs(g, padded, x_halo_wall=True) == 256
    assert _differs(g, padded, faces_only=True) == 576
    assert len(set(r["active"].tolist())) == 3                                    # planes of 0, 256 and 288 active nodes
    # empty rows between live ones: some plane has an empty row with live rows on both sides
    live = r["length"] > 0
    assert any(live[x, y] and not live[x, y + 1] and live[x, y + 2:].any() for x in range(g.dims[0]) for y in range(g.dims[1] - 2))


@pytest.mark.parametrize("padded", PADDED)
def test_sphere_seam(padded):
    g, cls, before, r = _report("sphere_seam", padded)
    assert g.dims == (14, 13, 19) and g.periodic == (1, 1, 1)
    assert (before == 2).sum() == 131 and (cls == 2).sum() == 0
    # the sphere lies across all three periodic seams
    assert g.mask[0, 0, 0] and g.mask[-1, 0, 0] and g.mask[0, -1, 0] and g.mask[0, 0, -1] and g.mask[-1, -1, -1]


@pytest.mark.parametrize("padded", PADDED)
def test_tiny(padded):
    g, cls, before, r = _report("tiny", padded)
    assert g.dims == (9, 5, 3) and g.dims[1] * g.dims[2] == 15 and G.plane_stride(5, 3, False) == 16   # a plane below one line
    assert (cls == 2).sum() == 15 and (r["active"] == 0).sum() == 1


@pytest.mark.parametrize("padded", PADDED)
def test_all_solid(padded):
    g, cls, before, r = _report("all_solid", padded)
    assert np.all(cls == 2) and not r["active"].any() and r["max_active"] == 1


@pytest.mark.parametrize("padded", PADDED)
def test_le_block(padded):
    """the Lees-Edwards geometry: the four layers the pass touches are fluid, and inert nodes stay strictly inside spans"""
    g, cls, before, r = _report("le_block", padded)
    assert g.periodic == (1, 1, 1)
    assert not g.mask[:, :, [0, 1, -2, -1]].any()
    assert (cls == 2).sum() == r["inert_inside"] == 64
    assert len(r["seams"]) > 0


@pytest.mark.parametrize("name", list(G.FORCE_BOXES))
def test_force_boxes(name):
    """three overlapping boxes: wholly inside solid, across a wall, up to the last plane of every axis"""
    g = G.GEOMETRIES[name]
    a, b, c = G.FORCE_BOXES[name]
    assert g.mask[G.box_slices(a)].all()
    assert g.mask[G.box_slices(b)].any() and not g.mask[G.box_slices(b)].all()
    assert (c[1], c[3], c[5]) == tuple(d - 1 for d in g.dims) and not g.mask[G.box_slices(c)].all()
    assert G.boxes_overlap(a, b) and G.boxes_overlap(b, c)


@pytest.mark.parametrize("padded", PADDED)
def test_source_and_class_boxes_hold_every_kind_of_node(padded):
    for name, box in G.SOURCE_BOX.items():
        cls = G.GEOMETRIES[name].classes(padded)[0]
        assert set(np.unique(cls[G.box_slices(box)])) == {0, 1, 2}, name
    cls = G.GEOMETRIES["stenosis"].classes(padded)[0]
    for box in G.VISC_BOXES:
        assert set(np.unique(cls[G.box_slices(box)])) == {0, 1, 2}
    assert G.boxes_overlap(*G.VISC_BOXES)


def test_plane_stride():
    assert G.plane_stride(22, 22, False) == 496 and G.plane_stride(22, 22, True) == 496 + 176
    assert G.plane_stride(12, 37, False) == 448 and G.plane_stride(12, 37, True) == 448 + 304
    assert G.plane_stride(6, 48, False) == 288 and G.plane_stride(6, 48, True) == 288 + 384


@pytest.mark.parametrize("padded", PADDED)
@pytest.mark.parametrize("wrong,names", [(dict(faces_only=True), ["stenosis", "seam_slabs"]),
                                         (dict(yz_wrap=False), ["seam_slabs"]),
                                         (dict(x_halo_wall=True), ["seam_slabs"])])
def test_mutant_rules_differ(wrong, names, padded):
    """each wrong rule gives another class map on the geometries meant to tell it from the right one"""
    for name in names:
        assert _differs(G.GEOMETRIES[name], padded, **wrong) > 0, name


@pytest.mark.parametrize("name", ["stenosis", "seam_slabs"])
def test_a_lost_bounce_shows(orc, name):
    """the oracle alone: 9 steps from the random state, and again with one wall-adjacent solid node cleared.  The fluid
    populations differ, so one wrong class on the device cannot hide behind the initial state"""
    g = G.GEOMETRIES[name]
    node = G.wall_adjacent_solid_node(g.mask, g.periodic)
    assert g.mask[node] == 1
    holed = g.mask.copy()
    holed[node] = 0
    fluid = g.mask.reshape(-1) == 0
    out = []
    for mask in (g.mask, holed):
        Lo = G.oracle_lattice(orc, g, mask)
        Lo.collide_stream(9)
        out.append(Lo.f[fluid].copy())
        Lo.destroy()
    assert np.isfinite(out[0]).all() and np.isfinite(out[1]).all()
    assert not np.array_equal(out[0], out[1])
    assert (np.abs(out[0] - out[1]).max(axis=1) > 0).sum() > 1   # and not on one node only
