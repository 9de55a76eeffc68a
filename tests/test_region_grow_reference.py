"""tests/region_grow_reference.py against scipy.ndimage.label where scipy is there, and its constructions against the sizes
include/tbrm_segment.h's tests rely on."""
import numpy as np
import pytest

import region_grow_reference as GR

STRUCT = {6: [[[0, 0, 0], [0, 1, 0], [0, 0, 0]], [[0, 1, 0], [1, 1, 1], [0, 1, 0]], [[0, 0, 0], [0, 1, 0], [0, 0, 0]]], 26: np.ones((3, 3, 3), dtype=int)}


def noise(dims, dtype, seed=7):
    rng = np.random.default_rng(seed)
    if np.dtype(dtype) == np.float32:
        return rng.uniform(0.0, 1.0, size=dims[::-1]).astype(np.float32)
    return rng.integers(0, GR.top_of(dtype) + 1, size=dims[::-1]).astype(dtype)


def threshold(dtype, share):
    return share if np.dtype(dtype) == np.float32 else int(share * GR.top_of(dtype))


def components(cand, connectivity):
    """(label image, sizes by label) by the reference itself: fill from the first unlabelled candidate, again and again"""
    lab = np.zeros(cand.shape, dtype=np.int32)
    sizes = [0]
    left = cand.copy()
    while left.any():
        z, y, x = np.argwhere(left)[0]
        seed = np.zeros_like(cand)
        seed[z, y, x] = True
        region, _ = GR.fill(cand, seed, connectivity)
        lab[region] = len(sizes)
        sizes.append(int(region.sum()))
        left &= ~region
    return lab, sizes


@pytest.mark.parametrize("connectivity", [6, 26])
def test_against_scipy_label(connectivity):
    ndimage = pytest.importorskip("scipy.ndimage")
    vol = noise((24, 17, 10), np.uint16)
    cand, _, _ = GR.candidates(vol, 0, threshold(np.uint16, 0.35))
    want, n = ndimage.label(cand, structure=STRUCT[connectivity])
    lab, sizes = components(cand, connectivity)
    assert len(sizes) - 1 == n
    # the same partition: every component of one is one component of the other
    pairs = set(zip(want[cand].tolist(), lab[cand].tolist()))
    assert len(pairs) == n
    # and grow() from a seed is that seed's component, whatever other seeds lie in it
    z, y, x = np.argwhere(want == np.argmax(np.bincount(want[cand])))[0]
    region, res, _ = GR.grow(vol, [(x, y, z), (x, y, z)], 0, threshold(np.uint16, 0.35), -1, connectivity)
    assert np.array_equal(region, want == want[z, y, x]) and res["voxels"] == int(region.sum()) and res["seeds_taken"] == 2


def test_noise_table():
    """the figures the GPU tests' noise cases stand on: u16, default_rng(7), (40, 24, 19)"""
    vol = noise((40, 24, 19), np.uint16)
    cand35, _, _ = GR.candidates(vol, 0, threshold(np.uint16, 0.35))
    cand20, _, _ = GR.candidates(vol, 0, threshold(np.uint16, 0.20))
    assert int(cand35.sum()) == 6428 and int(cand20.sum()) == 3661
    _, s6 = components(cand35, 6)
    assert len(s6) - 1 == 810 and max(s6) == 4174
    assert max(components(cand35, 26)[1]) == 6424
    assert max(components(cand20, 6)[1]) == 30
    assert max(components(cand20, 26)[1]) == 3599


def test_brick_snake():
    m = GR.brick_snake()
    assert m.shape == (8, 8, 8) and int(m.sum()) == 143 and m[0, 0, 0]
    seed = np.zeros_like(m)
    seed[0, 0, 0] = True
    region, steps = GR.fill(m, seed, 6)
    assert np.array_equal(region, m) and steps == 142   # one path: a plain dilation adds one voxel per step
    assert GR.synchronous_brick_passes(m, seed, 6) == 1


def test_plane_snake():
    m = GR.plane_snake()
    assert m.shape == (24, 24, 24) and int(m.sum()) == 299
    seed = np.zeros_like(m)
    seed[3, 0, 0] = True
    region, steps = GR.fill(m, seed, 6)
    assert np.array_equal(region, m) and steps == 298
    assert GR.synchronous_brick_passes(m, seed, 6) + 1 == 28   # 27 passes that move the region and the one that finds nothing left


def test_contacts():
    for a, b in (((7, 7, 7), (8, 8, 8)), ((7, 7, 3), (8, 8, 3)), ((2, 3, 4), (3, 4, 4))):   # a corner, an edge, a face diagonal in one brick
        m = np.zeros((16, 16, 16), dtype=bool)
        m[a[2], a[1], a[0]] = m[b[2], b[1], b[0]] = True
        vol = GR.mask_volume(m, np.uint8)
        for connectivity, want in ((26, 2), (6, 1)):
            _, res, _ = GR.grow(vol, [a], 100, 255, -1, connectivity)
            assert res["voxels"] == want and res["bbox_min"] == a and res["bbox_max"] == (b if want == 2 else a)


def test_modes():
    vol = noise((16, 16, 16), np.uint8, seed=3)
    labels = np.zeros(vol.shape, dtype=np.uint8)
    labels[:, :, 8] = 3   # a wall
    # no seeds: the threshold mask
    region, res, after = GR.grow(vol, None, 10, 200, 5, 6, labels)
    assert np.array_equal(region, (vol >= 10) & (vol <= 200)) and res["relabelled"] == res["voxels"] and (after[region] == 5).all()
    # the wall blocks when label 3 is not writable
    region, res, _ = GR.grow(vol, [(0, 0, 0)], 0, 255, 1, 6, labels, writable=[0])
    assert res["voxels"] == 16 * 16 * 8 and res["bbox_max"] == (7, 15, 15)
    region, res, _ = GR.grow(vol, [(0, 0, 0)], 0, 255, 1, 6, labels, writable=[0, 3])
    assert res["voxels"] == 16 ** 3
    # a box stops the growth; a seed outside it is ignored
    _, res, _ = GR.grow(vol, [(0, 0, 0), (12, 12, 12)], 0, 255, -1, 26, origin=(0, 0, 0), extent=(5, 6, 7))
    assert res["voxels"] == 5 * 6 * 7 and res["seeds_taken"] == 1
    # relative: the range around the first seed's value, clamped
    v0 = int(vol[2, 1, 0])
    _, res, _ = GR.grow(vol, [(0, 1, 2)], -300, 20, -1, 6, relative=True)
    assert (res["lo_used"], res["hi_used"]) == (0.0, float(min(v0 + 20, 255)))
    f = noise((5, 6, 3), np.float32)
    f[1, 2, 3] = np.nan
    _, res, _ = GR.grow(f, [(3, 2, 1)], -0.1, 0.1, -1, 6, relative=True)
    assert res["voxels"] == 0 and res["bbox_min"] == (5, 6, 3) and res["bbox_max"] == (-1, -1, -1)
    region, res, _ = GR.grow(f, None, 0.0, 1.0, -1, 6)
    assert res["voxels"] == 5 * 6 * 3 - 1 and not region[1, 2, 3]
