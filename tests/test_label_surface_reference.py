"""tests/label_surface_reference.py judged without a GPU, by properties that do not follow from how it is written: the counts of the
smallest closed surfaces, the signed volume in exact integers, the manifold rule of the edges, vertices inside their cells, the quads
per axis against the differing face pairs, the triangle split and the order."""
import numpy as np
import pytest

import label_surface_reference as SR

CASES = [
    ((8, 8, 8), None, None, 0.5, 1),
    ((8, 8, 8), (1, 3, 1), (5, 4, 7), 0.4, 2),
    ((9, 7, 17), None, None, 0.5, 3),
    ((9, 7, 17), (1, 1, 3), (7, 5, 11), 0.6, 4),
    ((40, 27, 19), None, None, 0.5, 5),
    ((40, 27, 19), (3, 5, 1), (30, 17, 13), 0.3, 6),
    ((40, 27, 19), (7, 9, 11), (1, 15, 7), 0.5, 7),   # a box one voxel thick
]


@pytest.fixture(scope="module")
def surfaces():
    out = []
    for dims, origin, extent, density, seed in CASES:
        labels = SR.random_labels(dims, density, seed, labels=(3, 9))
        out.append((labels, origin, extent, SR.surface(labels, [3], origin, extent)))
    return out


def test_one_voxel_and_a_full_brick():
    labels = np.zeros((8, 8, 8), dtype=np.uint8)
    labels[4, 2, 6] = 3   # (x, y, z) = (6, 2, 4)
    s = SR.surface(labels, [3])
    assert (s["set_voxels"], s["vertices"], s["quads"], s["quads_axis"]) == (1, 8, 6, (2, 2, 2))
    assert (s["vertex"]["edges"] == 3).all() and s["cell_min"] == (5, 1, 3) and s["cell_max"] == (6, 2, 4)
    # the eight vertices sit a third of the way from the voxel's centre along each axis... in sixths: cell + sum / 6
    assert sorted(set(s["vertex"]["sum"].reshape(-1).tolist())) == [1, 5]
    assert sorted(np.abs(s["vertex"]["normal"]).reshape(-1).tolist()) == [1] * 24
    full = SR.surface(np.full((8, 8, 8), 3, dtype=np.uint8), [3])
    assert full["set_voxels"] == 512 and full["quads"] == 6 * 64 and full["quads_axis"] == (128, 128, 128) and full["vertices"] == 9 ** 3 - 7 ** 3
    assert full["cell_min"] == (-1, -1, -1) and full["cell_max"] == (7, 7, 7)
    empty = SR.surface(np.zeros((8, 8, 8), dtype=np.uint8), [3])
    assert (empty["vertices"], empty["quads"], empty["cell_min"], empty["cell_max"]) == (0, 0, (8, 8, 8), (-1, -1, -1))
    assert empty["indices"].shape == (0, 4) and empty["positions"].shape == (0, 3)


def test_signed_volume_is_the_number_of_voxels(surfaces):
    for labels, origin, extent, s in surfaces:
        centre2 = 2 * s["vertex"]["cell"].astype(np.int64) + 1   # the cell's centre, doubled
        assert SR.sixfold_volume_doubled(centre2, s["indices"]) == 6 * 8 * s["set_voxels"], (labels.shape, origin)


def test_every_edge_is_in_two_or_four_quads(surfaces):
    for labels, origin, extent, s in surfaces:
        uses = SR.edge_uses(s["indices"])
        assert set(uses.values()) <= {2, 4}, (labels.shape, origin)
        # and a directed edge is never walked twice the same way by the quads at a 2-edge: the orientation is consistent
        directed = {}
        for q in s["indices"].tolist():
            for i in range(4):
                e = (q[i], q[(i + 1) % 4])
                directed[e] = directed.get(e, 0) + 1
        assert all(directed.get((b, a), 0) == n for (a, b), n in directed.items())


def test_vertices_lie_inside_their_cells(surfaces):
    for labels, origin, extent, s in surfaces:
        v = s["vertex"]
        assert ((v["edges"] >= 3) & (v["edges"] <= 12)).all()
        assert (v["sum"].astype(int) <= 2 * v["edges"].astype(int)[:, None]).all()   # 0 <= sum / (2 edges) <= 1
        assert (np.abs(v["normal"]) <= 4).all() and ((v["corners"] != 0) & (v["corners"] != 255)).all()
        p = SR.positions_of(v)
        assert (p >= v["cell"]).all() and (p <= v["cell"] + 1).all()


def test_quads_per_axis_are_the_differing_face_pairs(surfaces):
    for labels, origin, extent, s in surfaces:
        S = SR.the_set(labels, [3], origin, extent)
        assert s["quads_axis"] == SR.differing_face_pairs(S) and sum(s["quads_axis"]) == s["quads"]
        assert s["set_voxels"] == int(S.sum())


def test_triangles_are_the_stated_split(surfaces):
    for labels, origin, extent, s in surfaces[:4]:
        t = SR.surface(labels, [3], origin, extent, triangles=True)
        q = s["indices"]
        assert t["indices"].shape == (s["quads"], 6) and t["indices"].dtype == np.uint32
        assert np.array_equal(t["indices"], np.stack([q[:, 0], q[:, 1], q[:, 2], q[:, 0], q[:, 2], q[:, 3]], axis=1))
        assert np.array_equal(SR.quads_of(t["indices"], True), q)
        assert np.array_equal(t["vertex"], s["vertex"])


def test_the_order_is_the_stated_one(surfaces):
    for labels, origin, extent, s in surfaces:
        h = s["vertex"]["cell"].astype(np.int64) + 1
        keys = [((z >> 3, y >> 3, x >> 3), (z & 7, y & 7, x & 7)) for x, y, z in h.tolist()]
        assert keys == sorted(keys) and len(set(keys)) == len(keys)
        # quads: by their owner (always their first index), then by axis: the axis is the one the quad's four cells agree on
        owner_axis = []
        for q in s["indices"].tolist():
            cells = h[q]
            same = [a for a in range(3) if len(set(cells[:, a].tolist())) == 1]
            assert len(same) == 1 and (cells[0] <= cells).all()
            owner_axis.append((q[0], same[0]))
        assert owner_axis == sorted(owner_axis) and len(set(owner_axis)) == len(owner_axis)


def test_several_labels_and_the_positions():
    labels = SR.random_labels((9, 7, 17), 0.6, 11, labels=(3, 9, 200))
    both = SR.surface(labels, [3, 200])
    merged = np.where(np.isin(labels, [3, 200]), 5, 0).astype(np.uint8)
    one = SR.surface(merged, [5])
    assert np.array_equal(both["vertex"], one["vertex"]) and np.array_equal(both["indices"], one["indices"])
    scale, offset = (0.7, 0.7, 2.5), (-10.0, 3.25, 100.0)
    p = SR.surface(labels, [3, 200], scale=scale, offset=offset)["positions"]
    assert p.dtype == np.float32
    v = both["vertex"]
    exact = (v["cell"] + v["sum"] / (2.0 * v["edges"][:, None])) * np.asarray(scale) + np.asarray(offset)
    assert np.abs(p - exact).max() < 1e-4
    s, o = SR.unit_cube((9, 1, 17))
    assert s == (np.float32(0.125), np.float32(0.0), np.float32(0.0625)) and o == (0.0, 0.0, 0.0)
