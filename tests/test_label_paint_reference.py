"""The reference of the paint brush (tests/label_paint_reference.py) against what it restates, without a GPU: the three-case integer
rule against a brute force in fractions.Fraction that clamps the parameter t and measures the exact distance; a ball against the
margin's reference; the tie case; the size of the largest product the rule forms; the interpreter's counts."""
import numpy as np
import pytest

import label_margin_reference as MR
import label_paint_reference as PR


def random_stroke(rng, dims, n):
    return [tuple(int(rng.integers(-12, 8 * d + 12)) for d in dims) for _ in range(n)]


@pytest.mark.parametrize("seed", range(6))
def test_the_rule_is_the_clamped_distance(seed):
    rng = np.random.default_rng(seed)
    dims = (11, 9, 10)
    n = 1 + seed % 3
    weights = tuple(int(w) for w in rng.integers(1, 40, size=3))
    limit = int(rng.integers(30, 3000)) * min(weights)
    points = random_stroke(rng, dims, n)
    assert PR.admissible(points, weights, limit, dims)
    got = PR.within_stroke(points, weights, limit, dims)
    want = np.zeros_like(got)
    for a, b in PR.segments_of(points):
        want |= PR.within_segment_slowly(a, b, weights, limit, dims)
    assert np.array_equal(got, want)
    assert got.any() or n == 1


def test_a_zero_length_segment_is_a_ball():
    dims, w, limit = (11, 9, 10), (3, 5, 2), 2000
    p = (41, 30, 37)
    assert np.array_equal(PR.within_stroke([p], w, limit, dims), PR.within_stroke([p, p], w, limit, dims))
    assert np.array_equal(PR.within_stroke([p], w, limit, dims), PR.within_segment_slowly(p, p, w, limit, dims))


def test_a_ball_at_a_voxel_centre_is_the_margins_expand():
    dims, centre, radius = (21, 19, 17), (10, 9, 8), 5
    weights, margin_limit = (256, 256, 256), 256 * radius * radius
    seed = np.zeros(dims[::-1], dtype=bool)
    seed[centre[2], centre[1], centre[0]] = True
    want = MR.expand(seed, weights, margin_limit)
    got = PR.within_stroke([tuple(8 * c for c in centre)], weights, 64 * margin_limit, dims)
    assert np.array_equal(got, want)
    assert int(got.sum()) == 515
    # anisotropic weights too
    weights, margin_limit = (256, 256, 3265), 256 * 30
    assert np.array_equal(PR.within_stroke([tuple(8 * c for c in centre)], weights, 64 * margin_limit, dims), MR.expand(seed, weights, margin_limit))


def test_the_tie_case_is_not_empty():
    dims, points, weights, limit = PR.tie_case()
    at = PR.within_stroke(points, weights, limit, dims)
    below = PR.within_stroke(points, weights, limit - 1, dims)
    assert not (below & ~at).any()
    assert int((at & ~below).sum()) == 70


def test_the_largest_product_fits():
    dims, points, weights, limit = PR.extreme_case()
    assert PR.admissible(points, weights, limit, dims)
    track = []
    (a, b), = PR.segments_of(points)
    got = PR.within_segment(a, b, weights, limit, dims, track)
    assert 2 ** 61 <= track[0] < 2 ** 63  # as large as the bounds let it get, and inside int64
    assert np.array_equal(got, PR.within_segment_slowly(a, b, weights, limit, dims))
    # the coordinate bounds alone: ee and de below 2^56
    far = [(-PR.MAX_COORD, -PR.MAX_COORD, -PR.MAX_COORD)]
    track = []
    PR.within_segment(far[0], far[0], (PR.MAX_WEIGHT,) * 3, 1, (2, 2, 2), track)
    assert track[0] < 2 ** 56


def test_the_interpreter_counts():
    dims = (13, 11, 9)
    labels = PR.blob_labels(dims)
    vol = PR.volume(dims, np.uint8)
    points = [(20, 30, 40), (70, 50, 30)]
    M, res, after = PR.paint(labels, vol, points, (1, 1, 1), 400, PR.PAINT, [2], 2, gate=(64, 255), origin=(1, 2, 0), extent=(10, 8, 9), writable=[0, 1])
    box = PR.box_mask(labels.shape, (1, 2, 0), (10, 8, 9))
    assert res["stamp_voxels"] == int((M & box).sum()) and res["segments"] == 1
    assert not (M & (vol < 64)).any()
    changed = after != labels
    assert res["relabelled"] == int(changed.sum()) == res["added"] > 0
    assert not (changed & ~box).any() and not (changed & ~M).any()
    assert set(np.unique(labels[changed])) <= {0, 1}
    M2, res2, after2 = PR.paint(after, vol, points, (1, 1, 1), 400, PR.ERASE, [2], -1, erase_label=0)  # measuring, no gate, no box
    assert res2["relabelled"] == 0 and res2["removed"] == int((M2 & (after == 2)).sum()) > 0 and np.array_equal(after2, after)


def test_the_work_box():
    dims = (40, 27, 19)
    pts = [(-30, 100, 60), (50, 120, 60)]
    wb = PR.work_box(pts, (1, 1, 1), 16 * 16, dims)
    M = PR.within_stroke(pts, (1, 1, 1), 16 * 16, dims)
    z, y, x = np.nonzero(M)
    assert wb[0][0] <= x.min() and x.max() <= wb[1][0] and wb[0][1] <= y.min() and y.max() <= wb[1][1] and wb[0][2] <= z.min() and z.max() <= wb[1][2]
    assert wb == ((0, 11, 6), (8, 17, 9))
    assert PR.work_box(pts, (1, 1, 1), 16 * 16, dims, (20, 0, 0), (20, 27, 19)) is None
    assert PR.work_bricks(pts, (1, 1, 1), 16 * 16, dims) == 2 * 2 * 2
