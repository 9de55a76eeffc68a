"""tests/label_morph_reference.py checked on its own: closed forms for a single voxel, the duality of erosion and dilation, the order
close ⊇ S ⊇ open and idempotence, volume faces, and scipy.ndimage with the conventions of include/tbrm_morphology.h."""
import numpy as np
import pytest

import label_morph_reference as MR

SHAPES = [(40, 24, 19), (24, 17, 10), (5, 6, 3), (16, 16, 16)]
RADII = (1, 2, 3, 9)


def single(dims, at):
    m = np.zeros(dims[::-1], dtype=bool)
    m[at[2], at[1], at[0]] = True
    return m


@pytest.mark.parametrize("r,count", [(1, 7), (2, 25), (3, 63), (8, 833), (9, 1159)])
def test_a_single_voxel_dilates_to_an_octahedron_or_a_cube(r, count):
    m = single((40, 40, 40), (20, 20, 20))
    assert (2 * r + 1) * (2 * r * r + 2 * r + 3) // 3 == count
    assert int(MR.dilate(m, r, 6).sum()) == count
    assert int(MR.dilate(m, r, 26).sum()) == (2 * r + 1) ** 3
    z, y, x = np.nonzero(MR.dilate(m, r, 6))
    assert (abs(x - 20) + abs(y - 20) + abs(z - 20)).max() == r


@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("dims", SHAPES, ids=lambda d: "x".join(map(str, d)))
def test_duality_order_and_idempotence(dims, connectivity):
    S = MR.blobs(dims)
    assert 0 < S.sum() < S.size
    for r in (1, 2, 3):
        assert np.array_equal(MR.erode(S, r, connectivity), ~MR.dilate(~S, r, connectivity))
        assert np.array_equal(MR.dilate(S, r, connectivity), ~MR.erode(~S, r, connectivity))
        opened, closed = MR.operate(S, MR.OPEN, r, connectivity), MR.operate(S, MR.CLOSE, r, connectivity)
        assert not (opened & ~S).any() and not (S & ~closed).any()
        assert np.array_equal(MR.operate(opened, MR.OPEN, r, connectivity), opened)
        assert np.array_equal(MR.operate(closed, MR.CLOSE, r, connectivity), closed)


def test_the_blobs_survive_an_opening():
    """the inputs of the GPU tests must leave something for open at radius 2 to keep (white noise does not)"""
    S = MR.blobs((40, 24, 19))
    assert MR.operate(S, MR.OPEN, 2, 6).any() and MR.operate(S, MR.OPEN, 1, 26).any()
    rng = np.random.default_rng(7)
    assert not MR.operate(rng.uniform(size=(19, 24, 40)) < 0.3, MR.OPEN, 2, 6).any()


@pytest.mark.parametrize("connectivity", [6, 26])
def test_volume_faces(connectivity):
    solid = np.ones((10, 17, 24), dtype=bool)
    assert MR.erode(solid, 9, connectivity).all()          # outside counts as set: a solid volume survives
    slab = np.zeros_like(solid)
    slab[:, :, :5] = True                                  # touches five faces, one free face at x = 5
    assert np.array_equal(MR.erode(slab, 2, connectivity), np.broadcast_to(np.arange(24) < 3, slab.shape))
    corner = single((24, 17, 10), (0, 0, 0))               # nothing wraps
    grown = MR.dilate(corner, 2, connectivity)
    assert int(grown.sum()) == (10 if connectivity == 6 else 27) and not grown[:, :, 3:].any() and not grown[3:].any()


def test_morph_fields():
    labels = np.zeros((10, 17, 24), dtype=np.uint8)
    labels[3:7, 5:12, 8:16] = 4
    labels[5, 8, 16] = 9                                   # next to the block, not writable below
    R, got, after = MR.morph(labels, MR.DILATE, 1, [4], 7, 6, writable=[0])
    block = 4 * 7 * 8
    shell = 2 * (4 * 7 + 4 * 8 + 7 * 8)
    assert int(R.sum()) == block + shell and got["source_voxels"] == block and got["result_voxels"] == block + shell
    assert got["added"] == shell - 1 == got["relabelled"] and got["removed"] == 0 and after[5, 8, 16] == 9
    assert got["bbox_min"] == (7, 4, 2) and got["bbox_max"] == (16, 12, 7)
    _, got, after = MR.morph(labels, MR.ERODE, 1, [4], -1, 6)
    assert got["removed"] == block - 2 * 5 * 6 and got["relabelled"] == 0 and np.array_equal(after, labels)
    _, got, after = MR.morph(labels, MR.ERODE, 1, [4], 4, 26, origin=(8, 5, 3), extent=(4, 7, 4), erase_label=2)
    assert got["removed"] == got["relabelled"] == int((after == 2).sum()) and (after[:, :, 12:] != 2).all()
    _, got, _ = MR.morph(labels, MR.OPEN, 5, [1], 1)
    assert got["bbox_min"] == (24, 17, 10) and got["bbox_max"] == (-1, -1, -1) and got["source_voxels"] == 0
    assert [MR.launches(MR.DILATE, r) for r in (1, 8, 9, 17)] == [1, 1, 2, 3] and MR.launches(MR.CLOSE, 9, 3) == 6


@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("dims", SHAPES, ids=lambda d: "x".join(map(str, d)))
def test_against_scipy(dims, connectivity):
    ndi = pytest.importorskip("scipy.ndimage")
    S = MR.blobs(dims, seed=11)
    structure = ndi.generate_binary_structure(3, 1 if connectivity == 6 else 3)
    for r in RADII:
        d = ndi.binary_dilation(S, structure, iterations=r)
        e = ndi.binary_erosion(S, structure, iterations=r, border_value=1)
        assert np.array_equal(MR.dilate(S, r, connectivity), d), r
        assert np.array_equal(MR.erode(S, r, connectivity), e), r
        assert np.array_equal(MR.operate(S, MR.OPEN, r, connectivity), ndi.binary_dilation(e, structure, iterations=r)), r
        assert np.array_equal(MR.operate(S, MR.CLOSE, r, connectivity), ndi.binary_erosion(d, structure, iterations=r, border_value=1)), r
