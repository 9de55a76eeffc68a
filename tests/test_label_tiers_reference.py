"""tests/label_tiers_reference.py judged without a GPU: the islands reference composed crop by crop is the islands reference run whole,
and every case of tests/test_gpu_label_tiers.py is above the tier it claims and has vertices, quads or components on both sides of the
boundary it is about — computed from the references' own output. A case that does not straddle its boundary proves nothing about the
code behind it. Run with -s for the counts, the evidence and the references' times."""
import time

import numpy as np
import pytest

import label_islands_reference as IR
import label_surface_reference as SR
import label_tiers_reference as LT

REFERENCE_SECONDS = 5.0   # the budget of a case's CPU part; the references take 0.2 .. 2 s on these sparse volumes


# ---- the bookkeeping ---------------------------------------------------------------------------------------------------------------------
def test_counts_and_positions_restate_the_headers():
    assert LT.surface_blocks((80, 64, 48)) == 11 * 9 * 7 and LT.box_bricks((80, 64, 48)) == 10 * 8 * 6
    assert LT.surface_blocks(LT.TWO_TILES) == 1560 and LT.surface_blocks(LT.TWO_TILES, *LT.TWO_TILES_BOXES["box"]) == 1188
    assert LT.surface_blocks(LT.LONG) == 131074 and LT.box_bricks(LT.LONG) == 131072 and LT.surface_blocks(LT.LONG, *LT.LONG_SMALL_BOX) == 152
    assert LT.surface_blocks(LT.WIDE) == 1026 * 1025 and LT.box_bricks(LT.WIDE) == 1025 * 1024
    assert LT.box_bricks(LT.ISLANDS_TWO_TILES) == 1224 and LT.box_bricks(LT.ISLANDS_TWO_TILES, *LT.ISLANDS_BOXES["box"]) == 1088
    # a box that ends on a brick face has one more block of cells than bricks along that axis: the cells h = e
    assert LT.block_range((16, 16, 16), (8, 0, 3), (8, 5, 5)) == ((1, 0, 0), (2, 1, 2)) and LT.brick_range((16, 16, 16), (8, 0, 3), (8, 5, 5)) == ((1, 0, 0), (1, 1, 1))
    # x fastest, then y, then z, from the range's first block on
    assert int(LT.block_index((8, 0, 0), (16, 16, 16))) == 1 and int(LT.block_index((0, 8, 0), (16, 16, 16))) == 3 and int(LT.block_index((0, 0, 8), (16, 16, 16))) == 9
    assert int(LT.brick_index((15, 9, 8), (16, 16, 16))) == 7 and int(LT.brick_index((15, 9, 8), (16, 16, 16), (8, 8, 8), (8, 8, 8))) == 0
    assert LT.block_index(np.asarray([[79, 48, 48], [80, 48, 48]]), LT.TWO_TILES).tolist() == [1023, 1024]


def test_place_keeps_the_patterns_apart():
    a, b = LT.ball((5, 5, 5), 2.0), LT.snake(7)
    labels = LT.place((40, 20, 10), [a, b], [(1, 1, 1), (8, 3, 2)])
    assert (labels > 0).sum() == (a > 0).sum() + (b > 0).sum() and np.array_equal(labels[2:3, 3:5, 8:15], b)
    with pytest.raises(AssertionError):
        LT.place((40, 20, 10), [a, b], [(1, 1, 1), (7, 3, 2)])   # one voxel between them
    with pytest.raises(AssertionError):
        LT.place((40, 20, 10), [a, b], [(1, 1, 1), (34, 3, 2)])  # leaves the volume
    assert IR.islands(LT.snake(20), [3], 6)[0]["islands"] == 1 and (LT.snake(20) > 0).sum() == 20 + 6


# ---- the islands, crop by crop, are the islands run whole -------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [6, 26])
def test_islands_by_crops_equal_the_reference_run_whole(connectivity):
    dims = (64, 48, 24)
    density = {6: 0.3, 26: 0.08}[connectivity]
    patterns = [LT.cluster((20, 14, 9), density, 5), LT.ball((9, 9, 9), 3.3), LT.snake(22), LT.cluster((17, 12, 6), density, 6, corners=[(16, 11, 5)])]
    anchors = [(0, 3, 2), (30, 4, 12), (25, 30, 5), (47, 36, 18)]   # the first touches the face x = 0, the last the three far faces
    labels = LT.place(dims, patterns, anchors)
    labels[3, 40, 5] = 9   # another label, in no crop: not of the set
    crops = LT.crops_of(dims, patterns, anchors)
    rules = [dict(measure=True, table=400), dict(measure=True, table=7), dict(min_voxels=4, drop_label=7, table=9), dict(min_voxels=3, keep_label=5, drop_label=0, table=400),
             dict(min_voxels=2, keep_label=8, table=3)]
    for rule in rules:
        got, got_after = LT.islands_by_crops(labels, crops, [3], connectivity, **rule)
        want, want_after, _ = IR.islands(labels, [3], connectivity, **rule)
        assert set(got) == set(IR.FIELDS) == set(want)
        for k in IR.FIELDS:
            if k != "table":
                assert got[k] == want[k], (k, got[k], want[k], rule)
        assert len(got["table"]) == len(want["table"])
        for i, (a, b) in enumerate(zip(got["table"], want["table"])):
            assert a == b, (i, a, b, rule)
        assert np.array_equal(got_after, want_after), rule
        assert want["islands"] > 20 and (rule["table"] < 400 or {e["border"] for e in want["table"]} == {False, True})
    with pytest.raises(AssertionError):
        LT.islands_by_crops(labels, crops, [3], connectivity, max_islands=2)              # the verdict would depend on the other islands
    with pytest.raises(AssertionError):
        LT.islands_by_crops(labels, crops, [3], connectivity, spare_border=True)
    with pytest.raises(AssertionError):
        LT.islands_by_crops(labels, crops, [3, 9], connectivity, measure=True)            # a voxel of the set in no crop
    with pytest.raises(AssertionError):
        LT.islands_by_crops(labels, LT.crops_of(dims, patterns, anchors, margin=1), [3], connectivity, measure=True)


# ---- the surface cases --------------------------------------------------------------------------------------------------------------------
def quad_blocks(want, dims, origin, extent):
    """per quad the blocks of its four vertices, int64 [quads, 4]"""
    return LT.vertex_blocks(want["vertex"], dims, origin, extent)[want["indices"].astype(np.int64)]


def a_quad_across(qb, low, high):
    """is there a quad with a vertex in block `low` and one in block `high`?"""
    return bool(((qb == low).any(axis=1) & (qb == high).any(axis=1)).any())


def report(name, **what):
    print("\n%s: %s" % (name, ", ".join("%s %s" % (k.replace("_", " "), v) for k, v in what.items())))


@pytest.mark.parametrize("box", ["whole", "box"])
def test_surface_two_tiles_case(box):
    labels, origin, extent, want, seconds = LT.surface_reference("two_tiles", box)
    dims = LT.TWO_TILES
    blocks = LT.surface_blocks(dims, origin, extent)
    vb, qb = LT.vertex_blocks(want["vertex"], dims, origin, extent), quad_blocks(want, dims, origin, extent)
    report("surface, two tiles, " + box, blocks=blocks, vertices=want["vertices"], quads=want["quads"], vertices_below_1024=int((vb < LT.TILE).sum()),
           vertices_from_1024=int((vb >= LT.TILE).sum()), quad_in_1023_and_1024=a_quad_across(qb, 1023, 1024), reference_seconds="%.2f" % seconds)
    assert LT.TILE < blocks <= 2 * LT.TILE
    assert (vb < LT.TILE).sum() > 500 and (vb >= LT.TILE).sum() > 500
    assert a_quad_across(qb, LT.TILE - 1, LT.TILE)
    if box == "box":
        assert min(origin) >= 8 and want["vertices"] < LT.surface_reference("two_tiles", "whole")[3]["vertices"]
    assert seconds < REFERENCE_SECONDS


def test_surface_long_case():
    labels, origin, extent, want, seconds = LT.surface_reference("long")
    dims = LT.LONG
    blocks = LT.surface_blocks(dims)
    vb, qb = LT.vertex_blocks(want["vertex"], dims), quad_blocks(want, dims, None, None)
    trips = sorted(set((vb // LT.COUNT_TRIP).tolist()))
    first_pattern = LT.long_case()[2][0]
    report("surface, long", blocks=blocks, vertices=want["vertices"], quads=want["quads"], count_trips_with_vertices=trips, cell_min=want["cell_min"], cell_max=want["cell_max"],
           quad_across_65536=bool(((qb < LT.COUNT_TRIP).any(axis=1) & (qb >= LT.COUNT_TRIP).any(axis=1)).any()), quad_in_1023_and_1024=a_quad_across(qb, 1023, 1024),
           reference_seconds="%.2f" % seconds)
    assert 2 * LT.COUNT_TRIP < blocks <= 3 * LT.COUNT_TRIP          # a workgroup of the capped grid takes a second and a third octet
    assert trips == [0, 1, 2]                                        # and has something to add on each of its trips
    assert all((vb == k).any() for k in (0, LT.COUNT_TRIP, 2 * LT.COUNT_TRIP))   # the same eight lanes find vertices on all three
    # the least x is found in the blocks 0 and 65537 only, by lanes that have blocks with vertices (65536; 131073) still to come
    assert set(vb[want["vertex"]["cell"][:, 0] == want["cell_min"][0]].tolist()) == {0, LT.COUNT_TRIP + 1} and (vb == 2 * LT.COUNT_TRIP + 1).any()
    assert ((qb < LT.COUNT_TRIP).any(axis=1) & (qb >= LT.COUNT_TRIP).any(axis=1)).any()
    assert a_quad_across(qb, LT.COUNT_TRIP - 1, LT.COUNT_TRIP) and a_quad_across(qb, 0, LT.COUNT_TRIP + 1) and a_quad_across(qb, LT.TILE - 1, LT.TILE)
    # the bounding box meets from different trips: its low corner is the first pattern's (trip 0), its high corner the last voxel's (trips 1 and 2)
    assert want["cell_min"] == tuple(v - 1 for v in first_pattern[0]) == (1, -1, -1) and want["cell_max"] == (524287, 8, 4)
    assert all(min(o[1:]) >= 1 for o, _ in LT.long_case()[2][1:])   # no other pattern reaches the faces y = 0 and z = 0
    assert int(vb[np.argmax(want["vertex"]["cell"][:, 0])]) >= LT.COUNT_TRIP and int(vb[np.argmin(want["vertex"]["cell"][:, 0])]) < LT.COUNT_TRIP
    assert 24 * 524287 + 12 < 2 ** 24 and SR.MAX_DIM == dims[0]      # the largest numerator of a position there is
    assert seconds < REFERENCE_SECONDS
    small = LT.surface_reference("long", "small")
    assert LT.surface_blocks(dims, *LT.LONG_SMALL_BOX) < LT.COUNT_TRIP and small[3]["vertices"] > 0 and small[4] < REFERENCE_SECONDS


def test_surface_wide_case():
    labels, origin, extent, want, seconds = LT.surface_reference("wide")
    dims = LT.WIDE
    blocks = LT.surface_blocks(dims)
    vb, qb = LT.vertex_blocks(want["vertex"], dims), quad_blocks(want, dims, None, None)
    tiles = sorted(set((vb // LT.TILE).tolist()))
    report("surface, wide", blocks=blocks, tiles=-(-blocks // LT.TILE), vertices=want["vertices"], quads=want["quads"], tiles_with_vertices=tiles,
           quad_across_2_20=a_quad_across(qb, LT.TOP_TRIP - 1, LT.TOP_TRIP), last_block_has_a_vertex=bool((vb == blocks - 1).any()), reference_seconds="%.2f" % seconds)
    assert blocks > LT.TOP_TRIP and -(-blocks // LT.TILE) == 1028    # the top scan takes a second trip, over four tiles
    assert tiles[0] == 0 and any(100 < t < 900 for t in tiles) and sum(t >= LT.TILE for t in tiles) >= 3
    assert a_quad_across(qb, LT.TILE - 1, LT.TILE) and a_quad_across(qb, LT.TOP_TRIP - 1, LT.TOP_TRIP)
    assert (vb == blocks - 1).any() and want["cell_max"] == (8199, 8191, 1)
    assert seconds < REFERENCE_SECONDS


# ---- the islands cases --------------------------------------------------------------------------------------------------------------------
def islands_in_bricks(labels, position, dims, origin, extent, low, high):
    """the islands (positions in the order) that have voxels in brick `low` and in brick `high` of the box"""
    z, y, x = np.nonzero(position >= 0)
    k = LT.brick_index(np.stack([x, y, z], axis=1), dims, origin, extent)
    pos = position[z, y, x]
    return sorted(set(pos[k == low].tolist()) & set(pos[k == high].tolist()))


@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("box", ["whole", "box"])
def test_islands_two_tiles_case(box, connectivity):
    labels = LT.islands_two_tiles_labels()
    dims = LT.ISLANDS_TWO_TILES
    origin, extent = LT.ISLANDS_BOXES[box]
    t0 = time.perf_counter()
    want, _, position = IR.islands(labels, LT.SOURCE, connectivity, origin=origin, extent=extent, measure=True, table=8)
    seconds = time.perf_counter() - t0
    bricks = LT.box_bricks(dims, origin, extent)
    z, y, x = np.nonzero(position >= 0)
    k = LT.brick_index(np.stack([x, y, z], axis=1), dims, origin, extent)
    across = [islands_in_bricks(labels, position, dims, origin, extent, b, b + 1) for b in range(1022, 1026)]
    report("islands, two tiles, %s, %d-connected" % (box, connectivity), bricks=bricks, islands=want["islands"], set_voxels=want["set_voxels"],
           set_bricks_below_1024=len(set(k[k < LT.TILE].tolist())), set_bricks_from_1024=len(set(k[k >= LT.TILE].tolist())), islands_across_1022_to_1026=across,
           reference_seconds="%.2f" % seconds)
    assert LT.TILE < bricks <= 2 * LT.TILE
    assert len(set(k[k < LT.TILE].tolist())) > 900 and len(set(k[k >= LT.TILE].tolist())) > 50
    snake = set(across[0]) & set(across[1]) & set(across[2]) & set(across[3])
    assert len(snake) == 1, across    # one island runs through the bricks 1022 .. 1026: a merge joins slots of the two tiles
    if box == "box":
        assert min(LT.brick_range(dims, origin, extent)[0]) == 0 and max(LT.brick_range(dims, origin, extent)[0]) >= 1
    assert seconds < REFERENCE_SECONDS


@pytest.mark.parametrize("name", ["wide", "long"])
def test_islands_by_crops_cases(name):
    labels, crops, boxes = {"wide": LT.wide_case, "long": LT.long_case}[name]()
    dims = labels.shape[::-1]
    bricks = LT.box_bricks(dims)
    k = LT.brick_index(LT.set_voxels(labels, LT.SOURCE), dims)
    tiles = sorted(set((k // LT.TILE).tolist()))
    seconds = {}
    for connectivity in (6, 26):
        t0 = time.perf_counter()
        want, _ = LT.islands_by_crops(labels, crops, LT.SOURCE, connectivity, measure=True, table=8)
        if name == "wide":
            LT.islands_by_crops(labels, crops, LT.SOURCE, connectivity, min_voxels=4, drop_label=7, table=8)
        seconds[connectivity] = time.perf_counter() - t0
        assert want["islands"] >= (30 if connectivity == 6 else len(crops)) and want["set_voxels"] == len(k)
    report("islands, " + name, bricks=bricks, tiles=-(-bricks // LT.TILE), set_voxels=len(k), tiles_with_set_voxels=tiles, reference_seconds={c: "%.2f" % s for c, s in seconds.items()})
    assert tiles[0] == 0 and len(tiles) >= 4
    # one connected pattern lies across the bricks 1023 | 1024: a merge joins slots of the first two tiles
    ball = boxes[1]
    assert int(LT.brick_index(ball[0], dims)) == LT.TILE - 1 and int(LT.brick_index(tuple(v - 1 for v in ball[1]), dims)) >= LT.TILE and (k == LT.TILE - 1).any() and (k == LT.TILE).any()
    if name == "wide":
        assert bricks > LT.TOP_TRIP and -(-bricks // LT.TILE) == 1025     # the top scan takes a second trip, over one tile
        assert any(100 < t < 900 for t in tiles) and tiles[-1] == LT.TILE and (k == bricks - 1).any()
        # the snake lies across the bricks 2^20 - 1 | 2^20: a merge joins a slot of the top scan's first trip to one of its second
        o, e = boxes[4]
        assert int(LT.brick_index(o, dims)) == LT.TOP_TRIP - 1 and int(LT.brick_index((e[0] - 1, o[1], o[2]), dims)) > LT.TOP_TRIP
        assert (k == LT.TOP_TRIP - 1).any() and (k == LT.TOP_TRIP).any()
    else:
        assert bricks == 128 * LT.TILE and tiles[-1] == 127 and 63 in tiles
        assert want["table"] and max(e["first"][0] for e in want["table"]) > 500000   # first voxels near 2^19 along x in the table
    assert max(seconds.values()) < REFERENCE_SECONDS
