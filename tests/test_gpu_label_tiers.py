"""The label surface and the label islands on the GPU in boxes beyond one tile of their scans (1024 blocks of cells / bricks), beyond one
trip of the surface's capped count grid (65536 blocks) and beyond one trip of the scans' top level (2^20 blocks / bricks) — the sizes of
the project's own volumes, which the shapes of tests/test_gpu_label_surface.py and tests/test_gpu_label_islands.py stay below. The cases
are tests/label_tiers_reference.py's; tests/test_label_tiers_reference.py shows without a GPU that each lies across the boundaries it is
about. Every comparison is exact equality against label_surface_reference and label_islands_reference, as in those two files, whose
`check` and `same` are used as they stand. Run with -s for the scratch the handles took at the top tier."""
import numpy as np
import pytest

import label_islands_reference as IR
import label_surface_reference as SR
import label_tiers_reference as LT
from test_gpu_label_islands import same
from test_gpu_label_surface import check, make_res

pytestmark = pytest.mark.gpu

TRANSFORM = dict(scale=(0.7, 0.7, 2.5), offset=(-10.0, 3.25, 100.0))


# ---- the surface -----------------------------------------------------------------------------------------------------------------------------
def either_way(tunables, res, name, box="whole", triangles=False, scale=None, offset=None):
    """test_gpu_label_surface.either_way on a case of label_tiers_reference: the extraction and the measuring form under surface_skip 1
    and 0 against the reference; the blocks evaluated and skipped are the blocks of the range. Returns the result under 1"""
    labels, origin, extent, want, _ = LT.surface_reference(name, box)
    dims = labels.shape[::-1]
    out = []
    try:
        for skip in (1, 0):
            tunables("surface_skip", skip)
            got = res.label_surface(LT.SOURCE, origin, extent, triangles=triangles, scale=scale, offset=offset)
            check(got, want, dims, origin, extent, triangles, scale, offset, (name, box, triangles, scale, skip))
            assert got["blocks_evaluated"] + got["blocks_skipped"] == LT.surface_blocks(dims, origin, extent)
            m = res.measure_label_surface(LT.SOURCE, origin, extent)
            assert m["written"] == 0 and m["launches"] == 4 and all(m[k] == want[k] for k in SR.FIELDS), (m, skip)
            assert m["blocks_evaluated"] + m["blocks_skipped"] == LT.surface_blocks(dims, origin, extent)
            out.append(got)
    finally:
        tunables("surface_skip", 1)
    assert out[1]["blocks_skipped"] == 0
    return out[0]


def four_ways(tunables, res, name, box="whole"):
    """quads and triangles, in voxel coordinates and under a transform"""
    got = either_way(tunables, res, name, box)
    either_way(tunables, res, name, box, triangles=True)
    either_way(tunables, res, name, box, **TRANSFORM)
    either_way(tunables, res, name, box, triangles=True, **TRANSFORM)
    return got


def test_surface_two_tiles(gpu, tunables):
    """1560 blocks, and 1188 from block (1, 1, 1) on: k_surface_scan_tiles and k_surface_scan_top over two tiles, tile_base[1] in the emit's
    bases and in the look of a quad that has vertices in the blocks 1023 and 1024"""
    labels = LT.two_tiles_labels()
    with make_res(LT.TWO_TILES, labels) as res:
        for box in ("whole", "box"):
            got = four_ways(tunables, res, "two_tiles", box)
            assert got["vertices"] > 5000


def test_surface_the_counts_second_and_third_trip(gpu, tunables):
    """131074 blocks on the 2048 workgroups of k_surface_count: every lane adds the counts and the bounds of up to three blocks and commits
    once. The first pattern alone gives the low corner of the bounding box, the last voxel of the volume the high one; the positions
    there have the largest numerators there are."""
    labels = LT.long_case()[0]
    first = LT.long_case()[2][0]
    with make_res(LT.LONG, labels) as res:
        got = four_ways(tunables, res, "long")
        assert got["cell_min"] == tuple(v - 1 for v in first[0]) and got["cell_max"] == (524287, 8, 4) and got["blocks_skipped"] > 130000
        far = got["vertex"]["cell"][:, 0] == 524287
        assert far.sum() >= 4 and got["positions"][far].tobytes() == SR.positions_of(got["vertex"][far]).tobytes()
        assert 524287.0 <= got["positions"][far, 0].min() and got["positions"][far, 0].max() <= 524288.0
        # a box of fewer blocks than one trip, on the same handle: nothing is allocated
        before = res.surface_counters()
        small = either_way(tunables, res, "long", "small", triangles=True)
        assert 0 < small["vertices"] < got["vertices"]
        after = res.surface_counters()
        assert after["scratch_allocations"] == before["scratch_allocations"] and after["scratch_bytes"] == before["scratch_bytes"]


def test_surface_the_top_scans_second_trip(gpu, tunables):
    """1026 x 1025 blocks in 1028 tiles: k_surface_scan_top takes its loop twice and carries the sum of the first 1024 tiles into the bases
    of the last four, where the last rows of the volume and its last corner lie"""
    labels = LT.wide_case()[0]
    with make_res(LT.WIDE, labels) as res:
        got = four_ways(tunables, res, "wide")
        assert got["cell_max"] == (8199, 8191, 1) and got["blocks_skipped"] > 1000000
        print("\nsurface, %d blocks: %s" % (LT.surface_blocks(LT.WIDE), res.surface_counters()))


# ---- the islands -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def found_once():
    """label_islands_reference.islands finds the islands of the same bytes, set, connectivity and box once for all the rules a test
    runs over them (the 26-connected search is two seconds of the reference each time)"""
    real, memo = IR.find, {}

    def find(labels, source, connectivity=6, origin=None, extent=None):
        key = (labels.shape, hash(labels.tobytes()), tuple(source), connectivity, origin, extent)
        if key not in memo:
            memo[key] = real(labels, source, connectivity, origin, extent)
        return memo[key]

    IR.find = find
    yield
    IR.find = real


def counts_of(after):
    return np.bincount(after.ravel(), minlength=256)


@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("box", ["whole", "box"])
def test_islands_two_tiles(gpu, found_once, box, connectivity):
    """1224 bricks, and 1088 from brick (0, 0, 1) on: the slots of the bricks from 1024 on lie at tile_base[1], and the snake through the
    bricks 1022 .. 1026 is one island of slots of both tiles — measured, and under keep the largest, remove the small and split"""
    labels = LT.islands_two_tiles_labels()
    origin, extent = LT.ISLANDS_BOXES[box]
    rules = [dict(measure=True), dict(max_islands=1, keep_label=-1, drop_label=0), dict(max_islands=0, min_voxels=3, keep_label=-1, drop_label=0),
             dict(max_islands=200, keep_label=20, label_step=1, drop_label=-1)]
    with make_res(LT.ISLANDS_TWO_TILES, labels) as res:
        for rule in rules:
            res.upload_label_volume(labels)
            got, after = same(res, labels, LT.SOURCE, connectivity, table=8, origin=origin, extent=extent, **rule)
            assert got["islands"] > 5000 and got["table_entries"] == 8 and got["largest"] >= 35
            assert np.array_equal(res.label_statistics()["count"], counts_of(after)), rule
            if not rule.get("measure"):
                assert got["relabelled"] > 0
        assert res.islands_counters()["local_components"] >= 4 * got["islands"]


def by_crops(res, labels, crops, connectivity, table, **rule):
    """test_gpu_label_islands.same against the islands composed crop by crop: every field, the table, the label volume afterwards and
    the counts per label of the statistics; (result, labels after)"""
    got = res.label_islands(LT.SOURCE, connectivity, table=table, **rule)
    want, after = LT.islands_by_crops(labels, crops, LT.SOURCE, connectivity, table=table, **rule)
    for k in IR.FIELDS:
        if k != "table":
            assert got[k] == want[k], (k, {f: got[f] for f in IR.FIELDS if f != "table"}, {f: want[f] for f in IR.FIELDS if f != "table"}, connectivity, rule)
    assert len(got["table"]) == len(want["table"])
    for i, (a, b) in enumerate(zip(got["table"], want["table"])):
        assert a == b, (i, a, b, connectivity, rule)
    down = res.download_label_volume()
    assert np.array_equal(down, after), (connectivity, rule, int((down != after).sum()))
    assert np.array_equal(res.label_statistics()["count"], counts_of(after)), (connectivity, rule)
    return got, after


def test_islands_the_top_scans_second_trip(gpu):
    """1025 x 1024 bricks in 1025 tiles: k_islands_scan_top takes its loop twice; the slots of the last tile lie behind all the others, and
    the snake across the bricks 2^20 - 1 | 2^20 is one island of slots of both trips"""
    labels, crops, boxes = LT.wide_case()
    with make_res(LT.WIDE, labels) as res:
        for connectivity in (6, 26):
            got, _ = by_crops(res, labels, crops, connectivity, 8, measure=True)
            assert got["islands"] >= len(crops) and got["relabelled"] == 0
            assert any(e["first"][1] > 8000 for e in got["table"]) and any(e["first"][1] < 100 for e in got["table"])
        top = res.islands_counters()
        print("\nislands, %d bricks: %s" % (LT.box_bricks(LT.WIDE), top))
        # a box of one brick on the same handle takes no scratch; its islands are the reference's of the volume's first corner
        near = np.ascontiguousarray(labels[:, :40, :40])
        small = res.label_islands(LT.SOURCE, 6, measure=True, origin=(8, 8, 0), extent=(8, 8, 2), table=4)
        want, _, _ = IR.islands(near, LT.SOURCE, 6, measure=True, origin=(8, 8, 0), extent=(8, 8, 2), table=4)
        assert small["islands"] > 0 and small["table"] == want["table"]
        assert all(small[k] == want[k] for k in IR.FIELDS[:9]), (small, want)
        now = res.islands_counters()
        assert now["scratch_allocations"] == top["scratch_allocations"] and now["scratch_bytes"] == top["scratch_bytes"] and now["islands_calls"] == top["islands_calls"] + 1
        # a writing call: the small islands, wherever they lie, become label 7
        got, after = by_crops(res, labels, crops, 6, 8, min_voxels=4, keep_label=-1, drop_label=7)
        assert got["dropped"] > 20 and got["kept"] >= 3 and got["relabelled"] == got["dropped_voxels"] == int((after == 7).sum())
        assert got["bbox_min"][1] < 100 and got["bbox_max"][1] > 8184


def test_islands_first_voxels_half_a_million_along_x(gpu):
    """65536 x 2 bricks in 128 tiles, measured: the first voxels of the islands at the far end, x up to 524287, through the 32-bit keys
    and the table's decoding"""
    labels, crops, boxes = LT.long_case()
    with make_res(LT.LONG, labels) as res:
        for connectivity in (6, 26):
            got, _ = by_crops(res, labels, crops, connectivity, 400, measure=True)
            assert len(crops) <= got["islands"] == got["table_entries"]
            assert max(e["first"][0] for e in got["table"]) > 524272 and min(e["first"][0] for e in got["table"]) == 2
