"""Euclidean margins of labels (include/tbrm_margin.h) on the GPU against tests/label_margin_reference.py. The results are integers and
bytes: every comparison is exact equality — of the downloaded label volume, of every field of the result, of every distance."""
import numpy as np
import pytest
import torch

from tbraymarcherplugin_amd import abi, synthetic as S
import label_margin_reference as GR
import label_morph_reference as MR

pytestmark = pytest.mark.gpu

SHAPES = [(40, 24, 19), (24, 17, 10), (5, 6, 3), (16, 16, 16), (24, 24, 24), (40, 40, 40)]   # the morphology tests' shapes
BOXES = [((11, 5, 3), (13, 9, 7)), ((17, 9, 4), (1, 1, 1)), ((8, 8, 8), (8, 8, 8)), ((3, 2, 16), (30, 20, 3)), ((21, 0, 0), (1, 24, 19))]   # the grow tests' boxes
ISO, ANISO = (1, 1, 1), (256, 400, 1600)
ids = lambda d: "x".join(map(str, d))


def blob_labels(dims, seed=7):
    """label 3 on smoothed-noise blobs, label 7 on other blobs beside them, 0 elsewhere"""
    labels = np.zeros(dims[::-1], dtype=np.uint8)
    labels[MR.blobs(dims, seed + 1)] = 7
    labels[MR.blobs(dims, seed)] = 3
    return labels


def make_res(dims, labels=None):
    res = abi.Resources(dims, abi.FMT_G8, False, False, 0)
    res.upload_volume(np.zeros(dims[::-1], dtype=np.uint8))   # the call never reads the data
    if labels is not None:
        res.upload_label_volume(labels)
    return res


def same(res, labels, op, weights, limit, source, new_label, **kw):
    """one call on the handle and in the reference: every field of the result and the label volume afterwards; (result, labels after)"""
    got = res.margin_labels(op, weights, limit, source, new_label, **kw)
    _, want, after = GR.margin(labels, op, weights, limit, source, new_label, **kw)
    where = (labels.shape, GR.OP_NAMES[op], weights, limit, source, new_label, kw)
    for k in GR.FIELDS:
        assert got[k] == want[k], (k, got, want, where)
    assert got["launches"] == GR.launches(op), (got, where)
    down = res.download_label_volume()
    assert np.array_equal(down, after), (where, int((down != after).sum()), np.argwhere(down != after)[:5])
    return got, after


# ---- blobs ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights, scale", [(ISO, 1), (ANISO, 256)], ids=["iso", "aniso"])
@pytest.mark.parametrize("dims", SHAPES, ids=ids)
def test_blobs(gpu, dims, weights, scale):
    labels = blob_labels(dims)
    assert (labels == 3).any()
    moved = 0
    with make_res(dims, labels) as res:
        for op in GR.OPS:
            for r in (1, 2, 3):
                res.upload_label_volume(labels)
                got, _ = same(res, labels, op, weights, scale * r * r, [3], 3, erase_label=9)
                moved += got["added"] + got["removed"]
    assert moved > 0


# ---- reach beyond one brick, and the bit window's edge ----------------------------------------------------------------------------
LONG = 140
POINTS = (0, 7, 8, 69, 139)


def long_case(axis):
    """(dims, weights, the label volume with single voxels of label 1 along the long axis)"""
    dims = [9, 10, 11]
    dims[axis] = LONG
    weights = [4096, 4096, 4096]
    weights[axis] = 1
    labels = np.zeros(dims[::-1], dtype=np.uint8)
    for k, at in enumerate(POINTS):
        xyz = [(3 + 2 * k) % dims[0], (1 + 3 * k) % dims[1], (2 + 5 * k) % dims[2]]
        xyz[axis] = at
        labels[xyz[2], xyz[1], xyz[0]] = 1
    return tuple(dims), tuple(weights), labels


@pytest.mark.parametrize("reach", [8, 9, 17, 63, 64])
@pytest.mark.parametrize("axis", [0, 1, 2], ids=["x", "y", "z"])
def test_long_axis(gpu, axis, reach):
    """64 on the long axis and (at 64: limit 4096) 1 on the others; expand of the points, and the counterpart: shrink of everything
    but the points, which must leave exactly the complement of the expansion"""
    dims, weights, labels = long_case(axis)
    limit = reach * reach
    want_reach = [1 if reach == 64 else 0] * 3
    want_reach[axis] = reach
    with make_res(dims, labels) as res:
        got, after = same(res, labels, GR.EXPAND, weights, limit, [1], 1)
        assert got["reach"] == tuple(want_reach) and got["added"] > 0
        res.upload_label_volume(labels)
        got2, after2 = same(res, labels, GR.SHRINK, weights, limit, [0], 0, erase_label=1)   # the complement's counterpart
        assert np.array_equal(after2, after) and got2["removed"] == got["added"]
        res.upload_label_volume(labels)
        want = GR.distance(labels == 1, weights, limit)
        for inside, source in ((False, [1]), (True, [0])):   # to the points; and from inside everything but the points to its complement
            d = res.label_distance(source, weights, limit, inside=inside)
            assert np.array_equal(d, want), (inside, np.argwhere(d != want)[:5])


def test_large_isotropic_reach(gpu):
    dims = (40, 40, 40)
    labels = np.zeros(dims[::-1], dtype=np.uint8)
    for x, y, z in [(0, 0, 0), (20, 20, 20), (39, 17, 8), (8, 31, 39), (23, 24, 7)]:
        labels[z, y, x] = 2
    with make_res(dims, labels) as res:
        got, after = same(res, labels, GR.EXPAND, ISO, 17 * 17, [2], 2)
        assert got["reach"] == (17, 17, 17) and 0 < got["added"] < 40 ** 3 - 5
        res.upload_label_volume(labels)
        got2, after2 = same(res, labels, GR.SHRINK, ISO, 17 * 17, [0], 0, erase_label=2)
        assert np.array_equal(after2, after)


# ---- single voxels: brick corners and volume corners ----------------------------------------------------------------------------
BALLS = {1: 7, 2: 19, 3: 27, 4: 33, 9: 123}


@pytest.mark.parametrize("at", [(7, 7, 7), (8, 8, 8), (0, 0, 0), (39, 23, 18)], ids=ids)
def test_single_voxels(gpu, at):
    dims = (40, 24, 19)
    labels = np.zeros(dims[::-1], dtype=np.uint8)
    labels[at[2], at[1], at[0]] = 1
    with make_res(dims, labels) as res:
        for limit, ball in BALLS.items():
            res.upload_label_volume(labels)
            got, after = same(res, labels, GR.EXPAND, ISO, limit, [1], 1)
            if at in ((7, 7, 7), (8, 8, 8)):
                assert got["result_voxels"] == ball   # clear of the faces
            got, _ = same(res, after, GR.SHRINK, ISO, limit, [1], 1)
            assert got["result_voxels"] >= 1
        res.upload_label_volume(labels)
        got, after = same(res, labels, GR.OPEN, ISO, 1, [1], 1)   # a single voxel does not survive an opening
        assert got["result_voxels"] == 0 and got["removed"] == 1 and not after.any()
        res.upload_label_volume(labels)
        got, _ = same(res, labels, GR.CLOSE, ISO, 4, [1], 1)      # and a closing leaves it alone
        assert got["added"] == got["removed"] == 0 and got["bbox_min"] == dims and got["bbox_max"] == (-1, -1, -1)


# ---- ragged bricks and volume faces ---------------------------------------------------------------------------------------------
def test_ragged_bricks_and_volume_faces(gpu):
    dims = (20, 17, 13)
    n = 20 * 17 * 13
    labels = np.zeros(dims[::-1], dtype=np.uint8)
    labels[8:, 12:, 16:] = 2   # x 16 .. 19, y 12 .. 16, z 8 .. 12: fills the ragged last bricks and touches three volume faces
    with make_res(dims, labels) as res:
        for r in (1, 2):
            res.upload_label_volume(labels)
            got, after = same(res, labels, GR.SHRINK, ISO, r * r, [2], 2)
            # eaten from the three free sides only: the volume faces do not shrink it, the padding beyond them never counts as unset
            assert np.array_equal(after == 2, np.pad(np.ones((5 - r, 5 - r, 4 - r), dtype=bool), ((8 + r, 0), (12 + r, 0), (16 + r, 0))))
        for weights, limit in ((ISO, 9), (ANISO, 256 * 9)):
            res.upload_label_volume(labels)
            same(res, labels, GR.EXPAND, weights, limit, [2], 2)
            res.upload_label_volume(labels)
            same(res, labels, GR.CLOSE, weights, limit, [2], 2)
        # label 0 is in the source: the zero padding of the ragged bricks would qualify
        res.upload_label_volume(labels)
        got, _ = same(res, labels, GR.EXPAND, ISO, 75, [0], 0)
        assert got["source_voxels"] == n - 5 * 5 * 4 and got["result_voxels"] == n
        solid = np.full(dims[::-1], 6, dtype=np.uint8)
        res.upload_label_volume(solid)
        before = res.margin_counters()
        for op in (GR.SHRINK, GR.OPEN, GR.CLOSE, GR.EXPAND):
            got, _ = same(res, solid, op, ISO, 9, [6], 6)   # a solid volume survives every operator
            assert got["result_voxels"] == n and got["added"] == got["removed"] == 0
        c = res.margin_counters()
        assert c["bricks_computed"] == before["bricks_computed"] and c["bricks_written"] == before["bricks_written"]   # the classes gave every brick
        assert c["margin_calls"] == before["margin_calls"] + 4 and c["launches"] == before["launches"] + 18
        for op in GR.OPS:                                   # the dual: an empty source
            got, _ = same(res, solid, op, ANISO, 256 * 4, [1], 1)
            assert got["source_voxels"] == got["result_voxels"] == 0
        assert res.margin_counters()["bricks_computed"] == before["bricks_computed"]


# ---- the tunable and the counters -----------------------------------------------------------------------------------------------
def test_margin_skip_changes_nothing_but_the_count(gpu, tunables):
    dims = (40, 40, 40)
    labels = blob_labels(dims, seed=3)
    labels[:, :, 24:] = 0          # an empty part ...
    labels[:16, :16, :16] = 3      # ... and full bricks: both kinds of brick the classes give
    one = np.zeros(dims[::-1], dtype=np.uint8)
    one[20, 20, 20] = 1
    full = np.full(dims[::-1], 1, dtype=np.uint8)
    with make_res(dims, labels) as res:
        for weights, limit in ((ISO, 4), (ANISO, 256 * 9), ((1, 1, 1), 81)):
            for op in GR.OPS:
                results, computed = [], []
                for skip in (1, 0):
                    tunables("margin_skip", skip)
                    res.upload_label_volume(labels)
                    before = res.margin_counters()["bricks_computed"]
                    got, after = same(res, labels, op, weights, limit, [3], 3, erase_label=9)
                    results.append((got, after))
                    computed.append(res.margin_counters()["bricks_computed"] - before)
                assert results[0][0] == results[1][0] and np.array_equal(results[0][1], results[1][1])
                assert computed[1] == 125 * (2 if op in (GR.OPEN, GR.CLOSE) else 1) and 0 < computed[0] < computed[1], (computed, GR.OP_NAMES[op])
        tunables("margin_skip", 1)
        res.upload_label_volume(one)
        before = res.margin_counters()
        same(res, one, GR.EXPAND, ISO, 9, [1], 1)
        c = res.margin_counters()
        assert 1 <= c["bricks_computed"] - before["bricks_computed"] <= 27 and c["bricks_written"] - before["bricks_written"] <= 8
        assert c["margin_calls"] == before["margin_calls"] + 1 and c["launches"] == before["launches"] + 3
        res.upload_label_volume(one)
        same(res, one, GR.EXPAND, ISO, 81, [1], 1)   # a reach of 9: two bricks either side
        assert 1 <= res.margin_counters()["bricks_computed"] - c["bricks_computed"] <= 125
        res.upload_label_volume(full)
        c = res.margin_counters()
        for op in GR.OPS:
            same(res, full, op, ISO, 81, [1], 1)
        assert res.margin_counters()["bricks_computed"] == c["bricks_computed"]
        tunables("margin_skip", 0)
        same(res, full, GR.SHRINK, ISO, 81, [1], 1)
        assert res.margin_counters()["bricks_computed"] == c["bricks_computed"] + 125


# ---- boxes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights, limit", [(ISO, 4), (ANISO, 256 * 9)], ids=["iso", "aniso"])
def test_boxes(gpu, weights, limit):
    dims = SHAPES[0]
    labels = blob_labels(dims, seed=13)
    with make_res(dims, labels) as res:
        for origin, extent in BOXES:
            for op in GR.OPS:
                res.upload_label_volume(labels)
                _, after = same(res, labels, op, weights, limit, [3], 3, origin=origin, extent=extent)
                outside = np.ones(labels.shape, dtype=bool)
                outside[origin[2]:origin[2] + extent[2], origin[1]:origin[1] + extent[1], origin[0]:origin[0] + extent[0]] = False
                assert np.array_equal(after[outside], labels[outside])
        # an all-zero extent is the whole volume, whatever the origin
        res.upload_label_volume(labels)
        same(res, labels, GR.CLOSE, weights, limit, [3], 3, origin=(3, 3, 3), extent=(0, 0, 0))
    # the set outside the box acts on the inside: a slab that ends one voxel short of the box
    labels = np.zeros(dims[::-1], dtype=np.uint8)
    labels[:, :, :8] = 4
    with make_res(dims, labels) as res:
        got, after = same(res, labels, GR.EXPAND, ISO, 9, [4], 4, origin=(8, 8, 8), extent=(8, 8, 8))
        assert got["source_voxels"] == 0 and got["added"] == got["result_voxels"] == 3 * 8 * 8 and got["bbox_max"] == (10, 15, 15)
        res.upload_label_volume(labels)
        got, _ = same(res, labels, GR.SHRINK, ISO, 4, [4], 4, origin=(4, 0, 0), extent=(4, 24, 19))
        assert got["removed"] == 2 * 24 * 19 and got["bbox_min"] == (6, 0, 0) and got["bbox_max"] == (7, 23, 18)


# ---- masks ----------------------------------------------------------------------------------------------------------------------
def test_writable_blocks_joins_and_not_leaves(gpu):
    dims = (24, 17, 10)
    labels = np.zeros(dims[::-1], dtype=np.uint8)
    labels[:, :, 12:] = 5            # a finished segment beside the blobs
    blob = MR.blobs(dims, seed=17)
    labels[blob & (labels == 0)] = 3
    with make_res(dims, labels) as res:
        got, after = same(res, labels, GR.EXPAND, ISO, 4, [3], 3, writable=[0])
        assert got["added"] > 0 and np.array_equal(after == 5, labels == 5)        # label 5 is a wall for joins
        assert got["result_voxels"] > got["source_voxels"] + got["added"]          # ... though the result reaches into it
        res.upload_label_volume(labels)
        got, after = same(res, labels, GR.EXPAND, ISO, 4, [3], 3, writable=[0, 5])
        assert (after == 5).sum() < (labels == 5).sum() and got["result_voxels"] == got["source_voxels"] + got["added"]
        res.upload_label_volume(labels)
        got, after = same(res, labels, GR.SHRINK, ANISO, 256, [3], 3, writable=[], erase_label=8)   # leaves are the source's own voxels
        assert got["removed"] == (after == 8).sum() > 0 and got["added"] == 0
        res.upload_label_volume(labels)
        got, _ = same(res, labels, GR.CLOSE, ISO, 4, [3], 3, writable=[])
        assert got["added"] == 0 and got["relabelled"] == 0


def test_multi_label_source_new_labels_and_measuring(gpu):
    dims = (24, 17, 10)
    labels = blob_labels(dims, seed=19)
    with make_res(dims, labels) as res:
        for op in GR.OPS:
            res.upload_label_volume(labels)
            same(res, labels, op, ANISO, 256 * 4, [3, 7], 7, erase_label=1)   # the union of two labels; joins get one of them
        res.upload_label_volume(labels)
        got, after = same(res, labels, GR.EXPAND, ISO, 2, [3], 200)       # a margin as a label of its own, not in the source
        assert got["added"] == (after == 200).sum() == got["relabelled"] > 0
        got, _ = same(res, after, GR.EXPAND, ISO, 2, [3], 200)            # again: the margin holds new_label already
        assert got["added"] > 0 and got["relabelled"] == 0
        got, _ = same(res, after, GR.OPEN, ISO, 4, [255, 0, 64], -1)      # labels at both ends of the mask words; measure only
        assert got["source_voxels"] == (after == 0).sum() and got["relabelled"] == 0
        for op in GR.OPS:                                                 # measuring changes nothing (same() compares the bytes)
            got, still = same(res, after, op, ISO, 3, [3], -1)
            assert np.array_equal(still, after) and got["relabelled"] == 0 and got["added"] + got["removed"] > 0


# ---- state ----------------------------------------------------------------------------------------------------------------------
CAM = S.default_camera(64, 48)
TILE = abi.Tile(0, 0, 64, 48)


def lit_handle(dims, vol, labels):
    res = abi.Resources(dims, abi.FMT_G16)
    res.upload_volume(vol)
    res.set_tf_lut(abi.color_curve_to_lut(S.tf_keys("A")))
    res.set_windowing(abi.WindowingParams(0.5, 0.9, True, False))
    res.upload_label_volume(labels)
    for i in (0, 1):
        res.add_dir_light(S.light(i), True, S.default_world())
    return res


def test_state_after_a_writing_and_a_measuring_call(gpu):
    dims = (48, 40, 44)
    vol = S.make_volume_numpy(dims, np.uint16, 0x5EED0002)
    labels = np.where(vol >= np.percentile(vol, 70), 1, 0).astype(np.uint8)   # label 1: red, half transparent
    rp = abi.RaymarchParams(100.0, 1, True)
    world = S.default_world()
    weights, limit = abi.margin_weights((1.0, 1.0, 2.5), 2.0)
    with lit_handle(dims, vol, labels) as res:
        light = res.download_light_volume()
        plain = res.raymarch_lit(CAM, TILE, rp, world)
        m = res.margin_labels("open", weights, limit, [1], -1)   # a measure-only call changes nothing at all
        assert m["removed"] > 0 and m["relabelled"] == 0
        assert np.array_equal(res.download_label_volume(), labels)
        assert np.array_equal(res.raymarch_lit(CAM, TILE, rp, world), plain)
        counters = res.path_counters()
        got, after = same(res, labels, GR.OPEN, weights, limit, [1], 1)
        assert {k: got[k] for k in GR.FIELDS if k != "relabelled"} == {k: m[k] for k in GR.FIELDS if k != "relabelled"}
        assert res.path_counters() == counters   # the call's waits are its own, its scratch was taken by the measuring call
        frame = res.raymarch_lit(CAM, TILE, rp, world)
        assert not np.array_equal(frame, plain)
        stats = res.label_statistics()
        assert np.array_equal(res.download_light_volume(), light)   # nothing on the data side moved
        # a second writing call inside a box, with labels of its own for what joins and what leaves
        got2, after2 = same(res, after, GR.EXPAND, ISO, 9, [1], 2, origin=(5, 4, 3), extent=(30, 33, 20), erase_label=0)
        frame2 = res.raymarch_lit(CAM, TILE, rp, world)
        stats2 = res.label_statistics()
    with lit_handle(dims, vol, after) as fresh:   # the same volume, the same lights, the downloaded labels uploaded
        assert np.array_equal(fresh.raymarch_lit(CAM, TILE, rp, world), frame)
        assert np.array_equal(fresh.label_statistics(), stats)
        fresh.upload_label_volume(after2)
        assert np.array_equal(fresh.raymarch_lit(CAM, TILE, rp, world), frame2)
        assert np.array_equal(fresh.label_statistics(), stats2)
    assert stats[1]["count"] == (after == 1).sum() == got["result_voxels"]
    assert stats2[2]["count"] == got2["added"] == (after2 == 2).sum() and stats2[1]["count"] == stats[1]["count"]


# ---- the distance map -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(40, 24, 19), (24, 17, 10)], ids=ids)
def test_label_distance(gpu, tunables, dims):
    labels = blob_labels(dims, seed=31)
    mask = labels == 3
    with make_res(dims, labels) as res:
        for weights, limit in ((ISO, 9), (ISO, 5), (ANISO, 256 * 9)):
            for inside in (False, True):
                want = GR.distance(mask, weights, limit, inside)
                assert ((want != GR.FAR) & (want != 0)).any() and (want == GR.FAR).any()
                for skip in (1, 0):
                    tunables("margin_skip", skip)
                    got = res.label_distance([3], weights, limit, inside=inside)   # the whole volume: more than one chunk of slices
                    assert got.dtype == np.uint32 and got.shape == want.shape
                    assert np.array_equal(got, want), (weights, limit, inside, skip, np.argwhere(got != want)[:5])
                tunables("margin_skip", 1)
                for origin, extent in BOXES[:3] if dims == (40, 24, 19) else [((3, 2, 1), (9, 11, 8))]:
                    got = res.label_distance([3], weights, limit, origin=origin, extent=extent, inside=inside)
                    cut = want[origin[2]:origin[2] + extent[2], origin[1]:origin[1] + extent[1], origin[0]:origin[0] + extent[0]]
                    assert np.array_equal(got, cut), (weights, limit, inside, origin, extent)
            # thresholding the map is the operator: the measure-only counts of expand and shrink
            outer, inner = res.label_distance([3], weights, limit), res.label_distance([3], weights, limit, inside=True)
            m = res.margin_labels("expand", weights, limit, [3], -1)
            assert m["result_voxels"] == int((outer != GR.FAR).sum()) and m["added"] == int(((outer != GR.FAR) & (outer != 0)).sum())
            m = res.margin_labels("shrink", weights, limit, [3], -1)
            assert m["result_voxels"] == int((inner == GR.FAR).sum()) and m["removed"] == int(((inner != GR.FAR) & (inner != 0)).sum())
        assert np.array_equal(res.download_label_volume(), labels)   # a map writes no label


# ---- allocation -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grown_first", [False, True], ids=["fresh", "grown"])
def test_repeated_calls_allocate_nothing(gpu, grown_first):
    dims = (40, 24, 19)
    labels = blob_labels(dims, seed=23)
    with make_res(dims, labels) as res:
        if grown_first:
            res.grow_region([(0, 0, 0)], 0, 255, -1, 6)   # takes the boards' scratch
        after = labels
        _, after = same(res, after, GR.CLOSE, ANISO, 256 * 9, [3], 3)   # the whole volume, the largest range: takes the margins' scratch
        res.label_distance([3], ISO, 9)
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        allocs = res.path_counters()["operator_alloc_calls"]
        for k, (op, weights, limit, kw) in enumerate([(GR.CLOSE, ANISO, 256 * 9, {}), (GR.OPEN, ISO, 1, {}), (GR.EXPAND, ISO, 81, {}),
                                                      (GR.SHRINK, ISO, 4, dict(origin=(8, 8, 8), extent=(8, 8, 8))), (GR.CLOSE, ISO, 289, {})]):
            _, after = same(res, after, op, weights, limit, [3], 3 if k != 2 else -1, **kw)
            res.label_distance([3], weights, limit, inside=bool(k & 1), **kw)
            torch.cuda.synchronize()
            assert torch.cuda.mem_get_info()[0] == free0, k
        assert res.path_counters()["operator_alloc_calls"] == allocs
        c = res.margin_counters()
        assert c["margin_calls"] == 12
        g = res.grow_region([(0, 0, 0)], 0, 255, -1, 6)   # region growing finds its scratch usable after the margins worked in it
        assert g["voxels"] == 40 * 24 * 19
        m = res.morph_labels("dilate", 1, [3], -1)        # and so does the morphology
        assert m["result_voxels"] == int(MR.dilate(after == 3, 1, 6).sum())


# ---- handles and refusals -------------------------------------------------------------------------------------------------------
def test_handles(gpu):
    dims = (24, 17, 10)
    vol = np.zeros(dims[::-1], dtype=np.uint8)
    with abi.Resources(dims, abi.FMT_G8) as res:
        with pytest.raises(abi.TbrmError) as e:
            res.margin_labels("close", ISO, 1, [1], 1)        # no volume yet
        assert e.value.code == abi.ERR_NOT_INITIALIZED
        res.upload_volume(vol)
        for label in (1, -1):                                # no label volume: nothing to take the set from, measuring included
            with pytest.raises(abi.TbrmError) as e:
                res.margin_labels("close", ISO, 1, [1], label)
            assert e.value.code == abi.ERR_NOT_INITIALIZED
        with pytest.raises(abi.TbrmError) as e:
            res.label_distance([1], ISO, 1)
        assert e.value.code == abi.ERR_NOT_INITIALIZED
        res.attach_empty_labels()
        assert res.margin_labels("close", ISO, 1, [1], 1)["result_voxels"] == 0
        assert (res.label_distance([1], ISO, 4) == GR.FAR).all() and (res.label_distance([1], ISO, 4, inside=True) == 0).all()
    with abi.Resources(dims, abi.FMT_G8, False, False, 0, rgb=True) as res:   # a colour handle has no label volume
        res.upload_volume(vol)
        with pytest.raises(abi.TbrmError) as e:
            res.margin_labels("expand", ISO, 1, [0], -1)
        assert e.value.code == abi.ERR_NOT_INITIALIZED
        with pytest.raises(abi.TbrmError) as e:
            res.label_distance([0], ISO, 1)
        assert e.value.code == abi.ERR_NOT_INITIALIZED
    with abi.Resources((32, 32, 64), abi.FMT_G16, owned=abi.Slab(0, 32)) as part:
        with pytest.raises(abi.TbrmError) as e:
            part.margin_labels("expand", ISO, 1, [0], -1)
        assert e.value.code == abi.ERR_UNSUPPORTED
        with pytest.raises(abi.TbrmError) as e:
            part.label_distance([0], ISO, 1)
        assert e.value.code == abi.ERR_UNSUPPORTED


def test_refusals(gpu):
    dims = (24, 17, 10)
    labels = blob_labels(dims, seed=29)
    with make_res(dims, labels) as res:
        good = dict(op=abi.MARGIN_CLOSE, weights=ISO, limit=4, source=[3], new_label=3)
        bad = [dict(op=4), dict(op=-1), dict(weights=(0, 1, 1)), dict(weights=(1, 1, 0)), dict(limit=0), dict(limit=2 ** 31), dict(limit=2 ** 32 - 1),
               dict(limit=65 * 65), dict(weights=(4096, 4096, 1), limit=65 * 65), dict(weights=(256, 400, 1600), limit=255),
               dict(new_label=256), dict(new_label=-2), dict(erase_label=256), dict(erase_label=-1),
               dict(origin=(23, 0, 0), extent=(2, 1, 1)), dict(origin=(0, 0, 0), extent=(1, 0, 1)), dict(origin=(-1, 0, 0), extent=(2, 1, 1)),
               dict(origin=(0, 0, 0), extent=(24, 17, 11))]
        for change in bad:
            with pytest.raises(abi.TbrmError) as e:
                res.margin_labels(**{**good, **change})
            assert e.value.code == abi.ERR_INVALID_ARG, change
        d = res.margin_desc(**good)
        d.reserved = 1
        out = abi.MARGIN_RESULT()
        assert res.lib.tbrm_margin_labels(res.handle, d, out) == abi.ERR_INVALID_ARG and b"reserved" in res.lib.tbrm_last_error()
        # the distance map: the same table, and the buffer's size
        d = res.margin_desc(**good)
        buf = np.zeros(24 * 17 * 10, dtype=np.uint32)
        assert res.lib.tbrm_label_distance(res.handle, d, 0, buf.ctypes.data, buf.nbytes - 4) == abi.ERR_INVALID_ARG and b"out_bytes" in res.lib.tbrm_last_error()
        assert res.lib.tbrm_label_distance(res.handle, d, 0, buf.ctypes.data, buf.nbytes + 4) == abi.ERR_INVALID_ARG
        d.limit = 0
        assert res.lib.tbrm_label_distance(res.handle, d, 0, buf.ctypes.data, buf.nbytes) == abi.ERR_INVALID_ARG
        d = res.margin_desc(**{**good, "new_label": 300})
        assert res.lib.tbrm_label_distance(res.handle, d, 0, buf.ctypes.data, buf.nbytes) == abi.ERR_INVALID_ARG   # the ignored fields must be valid
        assert np.array_equal(res.download_label_volume(), labels) and res.margin_counters()["margin_calls"] == 0
        got, _ = same(res, labels, GR.EXPAND, ISO, 64 * 64, [3], 3)   # the largest reach: the whole volume joins
        assert got["result_voxels"] == 24 * 17 * 10 and got["reach"] == (64, 64, 64)
        res.upload_label_volume(labels)
        got, _ = same(res, labels, GR.EXPAND, (2 ** 19, 2 ** 31 - 1, 2 ** 31 - 1), 2 ** 31 - 1, [3], 3)   # the largest limit: sums just below 2^32
        assert got["reach"] == (63, 1, 1)
