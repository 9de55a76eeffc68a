"""tests/label_islands_reference.py checked on its own: against scipy.ndimage.label (the partition into components and their sizes),
against closed forms (checkerboards) and against its own constructions; and the properties of the noise constructions that make the
GPU cases (tests/test_gpu_label_islands.py) worth running: enough islands, ties of sizes that max_islands cuts through, enough
enclosed islands."""
import numpy as np
import pytest
from scipy import ndimage

import label_islands_reference as IR
from region_grow_reference import brick_snake, plane_snake

DIMS = (40, 24, 19)
# (q, connectivity): (islands, largest, singletons)
NOISE = {(0.35, 6): (836, 3370, 528), (0.10, 26): (307, 241, 162)}
# (q, connectivity of the background): (enclosed islands, their voxels)
HOLES = {(0.75, 6): (989, 2520), (0.85, 26): (45, 65)}


def labels_of(mask, label=1):
    return np.where(mask, label, 0).astype(np.uint8)


def tie_cut(sizes):
    """the smallest n >= 1 for which the islands at positions n - 1 and n of the order have the same size (None: no tie)"""
    return next((n for n in range(1, len(sizes)) if sizes[n - 1] == sizes[n]), None)


def same_partition(lab, S, connectivity):
    """the reference's components are scipy's: a one-to-one map between the two labellings over S"""
    other, n = ndimage.label(S, structure=np.ones((3, 3, 3)) if connectivity == 26 else None)
    pairs = np.unique(np.stack([lab[S], other[S]]), axis=1)
    assert pairs.shape[1] == n == len(np.unique(pairs[0])) == len(np.unique(pairs[1]))
    return n


@pytest.mark.parametrize("q,connectivity", list(NOISE))
def test_noise_against_scipy_and_the_floors(q, connectivity):
    m = IR.noise_mask(DIMS, q)
    labels = labels_of(m, 3)
    S, lab, firsts, sizes, border = IR.find(labels, [3], connectivity)
    assert np.array_equal(S, m)
    n = same_partition(lab, S, connectivity)
    islands, largest, singletons = NOISE[(q, connectivity)]
    assert (n, int(sizes.max()), int((sizes == 1).sum())) == (islands, largest, singletons)
    other, _ = ndimage.label(S, structure=np.ones((3, 3, 3)) if connectivity == 26 else None)
    assert sorted(sizes) == sorted(np.bincount(other[S])[1:])
    # a first voxel is the smallest linear index of its island
    for f in firsts[:50]:
        assert np.flatnonzero(lab == f)[0] == f
    res, after, position = IR.islands(labels, [3], connectivity, table=n + 5)
    assert res["islands"] == n >= 100 and res["table_entries"] == n and res["spared"] == 0
    got = [e["voxels"] for e in res["table"]]
    assert got == sorted(got, reverse=True) and res["largest"] == got[0] and sum(got) == res["set_voxels"] == int(m.sum())
    for a, b in zip(res["table"], res["table"][1:]):   # the order is total: equal sizes by first voxel
        fa, fb = (a["first"][0] + 40 * (a["first"][1] + 24 * a["first"][2])), (b["first"][0] + 40 * (b["first"][1] + 24 * b["first"][2]))
        assert a["voxels"] > b["voxels"] or (a["voxels"] == b["voxels"] and fa < fb)
    cut = tie_cut(got)
    assert cut is not None and cut < 16   # equal sizes among the 16 largest: a max_islands that lands inside a tie
    assert np.array_equal(after, labels) and res["relabelled"] == 0 and res["kept"] == n   # the default rule keeps everything as it is
    assert (position >= 0).sum() == m.sum() and (position[~m] == -1).all()


def test_useless_density():
    """35 % at 26-connectivity is one body and a speck: the GPU cases use 10 % there"""
    assert IR.islands(labels_of(IR.noise_mask(DIMS, 0.35)), [1], 26)[0]["islands"] == 2


@pytest.mark.parametrize("q,connectivity", list(HOLES))
def test_holes(q, connectivity):
    m = IR.noise_mask(DIMS, q)
    labels = labels_of(m, 2)
    res, after, _ = IR.fill_holes(labels, 2, None, connectivity)
    enclosed, voxels = HOLES[(q, connectivity)]
    assert (res["dropped"], res["dropped_voxels"], res["kept"]) == (enclosed, voxels, 0) and enclosed >= 30
    assert res["relabelled"] == voxels and res["spared"] >= 1
    # scipy: the background components that touch no face of the volume
    other, n = ndimage.label(~m, structure=np.ones((3, 3, 3)) if connectivity == 26 else None)
    outer = np.unique(np.concatenate([other[0].ravel(), other[-1].ravel(), other[:, 0].ravel(), other[:, -1].ravel(), other[:, :, 0].ravel(), other[:, :, -1].ravel()]))
    inner = ~m & ~np.isin(other, outer)
    assert np.array_equal(after == 2, m | inner) and int(inner.sum()) == voxels and n == res["islands"] + res["spared"]
    # up to n voxels only
    small, after_small, _ = IR.fill_holes(labels, 2, 2, connectivity)
    sizes = np.bincount(other[inner])
    sizes = sizes[sizes > 0]
    assert small["dropped"] == int((sizes <= 2).sum()) and small["kept"] == int((sizes > 2).sum()) and small["relabelled"] == int(sizes[sizes <= 2].sum())
    assert np.array_equal(after_small == 2, m | (inner & (np.bincount(other.ravel())[other] <= 2)))


@pytest.mark.parametrize("n,connectivity,islands", [(16, 6, 2048), (64, 6, 131072), (16, 26, 1)])
def test_checkerboards(n, connectivity, islands):
    res, _, position = IR.islands(labels_of(IR.checkerboard(n)), [1], connectivity, table=4)
    assert res["islands"] == islands and res["set_voxels"] == n ** 3 // 2
    if connectivity == 6:   # all of one voxel: the order is the first voxels'
        assert [e["first"] for e in res["table"]] == [(0, 0, 0), (2, 0, 0), (4, 0, 0), (6, 0, 0)] and res["largest"] == 1
        z, y, x = np.nonzero(IR.checkerboard(n))
        assert np.array_equal(position[z, y, x], np.arange(len(z)))


def test_corner_contacts_alone():
    m = IR.diagonal_checkerboard(16)
    assert IR.islands(labels_of(m), [1], 26)[0]["islands"] == 1
    assert IR.islands(labels_of(m), [1], 6)[0]["islands"] == int(m.sum()) == 1024
    assert same_partition(IR.find(labels_of(m), [1], 26)[1], m, 26) == 1


def test_snakes_are_one_island():
    for m in (brick_snake(), plane_snake()):
        for connectivity in (6, 26):
            res, _, _ = IR.islands(labels_of(m), [1], connectivity, table=1)
            z, y, x = np.argwhere(m)[0]
            assert res["islands"] == 1 and res["largest"] == int(m.sum()) and res["table"][0]["first"] == (x, y, z) == (0, 0, z)


def test_the_rule_the_box_and_the_border():
    labels = np.zeros((8, 10, 12), dtype=np.uint8)
    labels[1:4, 1:4, 1:4] = 5      # 27 voxels
    labels[5, 5, 5:9] = 5          # 4
    labels[6, 8, 1:3] = 6          # 2, another label
    labels[0, 0, 11] = 5           # 1, on three faces
    labels[2, 7, 9:11] = 5         # 2: ties with nothing of label 5 but with label 6's when both are in the source
    res, after, _ = IR.keep_largest(labels, 5, 1, table=8)
    assert (res["islands"], res["kept"], res["dropped"], res["kept_voxels"], res["dropped_voxels"], res["relabelled"]) == (4, 1, 3, 27, 7, 7)
    assert (after == 5).sum() == 27 and (after == 6).sum() == 2 and res["bbox_min"] == (5, 0, 0) and res["bbox_max"] == (11, 7, 5)
    assert [e["label"] for e in res["table"]] == [5, 0, 0, 0] and [e["kept"] for e in res["table"]] == [True, False, False, False]
    assert [e["border"] for e in res["table"]] == [False, False, False, True]
    res, after, _ = IR.remove_small(labels, 5, 3, erase_label=9)
    assert (res["kept"], res["dropped"], res["relabelled"]) == (2, 2, 3) and (after == 9).sum() == 3
    res, after, _ = IR.split(labels, 5, 20, 2, drop_label=0, table=8)
    assert (after == 20).sum() == 27 and (after == 21).sum() == 4 and (after == 5).sum() == 0 and [e["label"] for e in res["table"]] == [20, 21, 0, 0]
    # equal sizes are ordered by first voxel: (9, 7, 2) comes before (1, 8, 6)
    res, after, _ = IR.islands(labels, [5, 6], 6, max_islands=3, keep_label=30, label_step=1, table=8)
    assert [e["voxels"] for e in res["table"]] == [27, 4, 2, 2, 1] and res["table"][2]["first"] == (9, 7, 2) and res["table"][3]["first"] == (1, 8, 6)
    assert (after[2, 7, 9:11] == 32).all() and (after[6, 8, 1:3] == 6).all() and res["table"][3]["label"] == 6 and res["table"][4]["label"] == 5
    # measuring writes nothing; a mixed island that is left has label -1
    labels[5, 5, 9] = 6
    res, after, _ = IR.islands(labels, [5, 6], 6, drop_label=0, max_islands=1, measure=True, table=8)
    assert np.array_equal(after, labels) and res["relabelled"] == 0 and res["dropped"] == 4 and res["table"][1]["label"] == -1 and res["table"][1]["voxels"] == 5
    # a box cuts: the block is two islands inside a box that leaves out its middle layer... of a ring
    ring = np.zeros((3, 9, 9), dtype=np.uint8)
    ring[1, 2:7, 2:7] = 1
    ring[1, 3:6, 3:6] = 0
    assert IR.islands(ring, [1])[0]["islands"] == 1
    res, after, _ = IR.islands(ring, [1], origin=(0, 3, 0), extent=(9, 3, 3), drop_label=7, max_islands=1)
    assert res["islands"] == 2 and res["set_voxels"] == 6 and res["relabelled"] == 3 and (after == 7).sum() == 3 and (after == 1).sum() == 13
    # spare_border is against the box's faces
    res, _, _ = IR.islands(ring, [1], origin=(2, 3, 1), extent=(5, 3, 1), spare_border=True)
    assert res["islands"] == 0 and res["spared"] == 2
    res, _, _ = IR.islands(ring, [1], spare_border=True)
    assert res["islands"] == 1 and res["spared"] == 0
