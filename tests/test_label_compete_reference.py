"""The two statements of competitive growing in tests/label_compete_reference.py against each other and against what is known in
closed form, without a GPU: the heap Dijkstra over packed keys and the synchronous relaxation agree key for key on noise; on flat
data the answer is a weighted L1 Voronoi partition with ties to the smaller label and, under a limit, an L1 ball; the snakes of
tests/region_grow_reference.py are corridors whose costs are the distance along the path."""
import numpy as np
import pytest

import label_compete_reference as CR
import region_grow_reference as GR


def both(vol, labels, seeds, lo, hi, **kw):
    a = CR.compete(vol, labels, seeds, lo, hi, solver="dijkstra", **kw)
    b = CR.compete(vol, labels, seeds, lo, hi, solver="relax", **kw)
    assert np.array_equal(a[3], b[3]), int((a[3] != b[3]).sum())
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    return a


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32])
@pytest.mark.parametrize("dims", CR.SHAPES)
def test_dijkstra_equals_the_relaxation_on_noise(dims, dtype):
    vol, labels, lo, hi, frange = CR.noise_case(dims, dtype)
    claimed = 0
    for step_cost, shift in CR.PARAMS:
        kw = dict(step_cost=step_cost, value_shift=shift, writable=[0], frange=frange)
        res, after, costs, keys = both(vol, labels, CR.SEEDS, lo, hi, **kw)
        assert res["claimed"] > 0 and res["seed_voxels"] == int(np.isin(labels, CR.SEEDS).sum())
        assert np.array_equal(after[labels == CR.WALL], labels[labels == CR.WALL]) and np.array_equal(after[np.isin(labels, CR.SEEDS)], labels[np.isin(labels, CR.SEEDS)])
        limit = CR.binding_limit(costs)
        bound, _, bcosts, _ = both(vol, labels, CR.SEEDS, lo, hi, cost_limit=limit, **kw)
        assert bound["claimed"] <= res["claimed"] and bound["max_cost"] <= limit
        inside = bcosts != CR.UNREACHED
        assert np.array_equal(bcosts[inside], costs[inside]) and (costs[~inside & (costs != CR.UNREACHED)] > limit).all()   # the limit only prunes
        passes, k = CR.synchronous_brick_passes(vol, labels, CR.SEEDS, lo, hi, **kw)
        assert np.array_equal(k, keys) and 1 <= passes <= 12
        claimed += res["claimed"]
    assert claimed > 0
    if dtype == np.float32:
        assert np.isnan(vol).sum() > 1 and np.isnan(vol[labels == CR.SEEDS[0]]).sum() >= 1   # NaN voxels and a NaN seed


def test_flat_data_is_a_weighted_l1_voronoi_partition():
    dims = (13, 11, 9)
    vol = np.full(dims[::-1], 100, dtype=np.uint8)
    labels = np.zeros(dims[::-1], dtype=np.uint8)
    sites = {5: (2, 3, 1), 2: (10, 7, 6), 7: (6, 1, 8)}   # label: (x, y, z)
    for l, (x, y, z) in sites.items():
        labels[z, y, x] = l
    z, y, x = np.indices(labels.shape)
    for step in ((1, 1, 1), (2, 3, 5)):
        dist = {l: step[0] * abs(x - sx) + step[1] * abs(y - sy) + step[2] * abs(z - sz) for l, (sx, sy, sz) in sites.items()}
        order = sorted(sites)
        best = np.minimum.reduce([(dist[l] << 8) | l for l in order])          # ties to the smaller label
        res, after, costs, _ = both(vol, labels, list(sites), 0, 255, step_cost=step, value_shift=0)
        assert np.array_equal(after, (best & 255).astype(np.uint8)) and np.array_equal(costs, (best >> 8).astype(np.uint32))
        assert res["claimed"] == labels.size - 3 and res["seed_voxels"] == 3
        limit = 7
        res, after, costs, _ = both(vol, labels, list(sites), 0, 255, step_cost=step, value_shift=0, cost_limit=limit)
        ball = (best >> 8) <= limit                                               # under a limit: L1 balls
        assert np.array_equal(after, np.where(ball, best & 255, labels).astype(np.uint8)) and res["claimed"] == int(ball.sum()) - 3
        assert np.array_equal(costs != CR.UNREACHED, ball) and res["max_cost"] == int((best >> 8)[ball].max())


def test_zero_step_cost_on_flat_data_leaves_every_seed_alone():
    labels = np.zeros((4, 6, 9), dtype=np.uint8)
    labels[1, 2, 3:6] = (7, 2, 5)          # adjacent seeds of three labels: at cost 0 the smallest would eat the others
    vol = np.full(labels.shape, 9, dtype=np.uint16)
    res, after, costs, _ = both(vol, labels, [2, 5, 7], 0, 65535, step_cost=(0, 0, 0), value_shift=0)
    assert np.array_equal(after[1, 2, 3:6], (7, 2, 5)) and res["seed_voxels"] == 3
    assert res["claimed"] == labels.size - 3 and res["claimed_per_label"] == {2: labels.size - 3} and res["max_cost"] == 0 and (costs == 0).all()


SNAKES = {"brick": GR.brick_snake(), "plane": GR.plane_snake()}
SNAKE_FACTS = {"brick": (143, 1), "plane": (299, 27)}   # (voxels, synchronous brick passes)


@pytest.mark.parametrize("name", sorted(SNAKES))
def test_snakes_are_corridors(name):
    mask = SNAKES[name]
    vol, labels = CR.corridor_case(mask)
    res, after, costs, _ = both(vol, labels, [1], 0, 255, step_cost=(1, 1, 1), writable=[0])
    assert res["claimed"] == int(mask.sum()) - 1 and np.array_equal(after == 1, mask) and res["max_cost"] == int(mask.sum()) - 1   # one path through all
    region, steps = GR.fill(mask, labels == 1, 6)
    assert steps == res["max_cost"] and np.array_equal(region, mask)
    passes, _ = CR.synchronous_brick_passes(vol, labels, [1], 0, 255, step_cost=(1, 1, 1), writable=[0])
    assert (int(mask.sum()), passes) == SNAKE_FACTS[name]
    limit = 40
    res, after, costs, _ = both(vol, labels, [1], 0, 255, step_cost=(1, 1, 1), writable=[0], cost_limit=limit)
    assert res["claimed"] == limit == res["max_cost"]


def test_the_largest_key_is_the_unreached_word():
    """cost 2^24 - 1 from label 255 packs to 0xFFFFFFFF: it claims nothing; from label 254, and at one less from 255, it claims"""
    n = 258                                                # the cost 2^24 - 1 takes many steps of the largest weight: a row long enough
    vol = np.zeros((1, 1, n), dtype=np.uint16)
    vol[0, 0, 1:] = 65535                                  # one step of 65535 + 65535, then 65535 each: 65535 * 256 = 2^24 - 256 at x = 255
    for seed, claimed in ((255, 255), (254, 255)):
        labels = np.zeros((1, 1, n), dtype=np.uint8)
        labels[0, 0, 0] = seed
        res, _, costs, _ = both(vol, labels, [seed], 0, 65535, step_cost=(65535, 0, 0))
        assert res["claimed"] == claimed and res["max_cost"] == 65535 * 256
    vol[0, 0, 255] = 65535 - 255                           # the step into x = 255 costs 255 more: 2^24 - 1 exactly
    for seed, claimed in ((255, 254), (254, 255)):
        labels = np.zeros((1, 1, n), dtype=np.uint8)
        labels[0, 0, 0] = seed
        res, _, costs, _ = both(vol, labels, [seed], 0, 65535, step_cost=(65535, 0, 0))
        assert res["claimed"] == claimed, (seed, res)
