"""Smoothing of labels (include/tbrm_smooth.h) on the GPU against tests/label_smooth_reference.py. The results are integers and bytes:
every comparison is exact equality — of the downloaded label volume and of every field of the result. The inputs are judged without
a GPU in tests/test_label_smooth_reference.py."""
import itertools

import numpy as np
import pytest
import torch

from tbraymarcherplugin_amd import abi, synthetic as S
import label_margin_reference as GR
import label_morph_reference as MR
import label_smooth_reference as SR
import region_grow_reference as RR

pytestmark = pytest.mark.gpu

ids = lambda d: "x".join(map(str, d))
BOXES = [((11, 5, 3), (13, 9, 7)), ((17, 9, 4), (1, 1, 1)), ((8, 8, 8), (8, 8, 8)), ((3, 2, 16), (30, 20, 3)), ((21, 0, 0), (1, 24, 19))]   # the grow tests' boxes


def make_res(dims, labels=None, vol=None):
    res = abi.Resources(dims, abi.FMT_G8, False, False, 0)
    res.upload_volume(vol if vol is not None else np.zeros(dims[::-1], dtype=np.uint8))   # smoothing never reads the data
    if labels is not None:
        res.upload_label_volume(labels)
    return res


def same(res, labels, radius, source, new_label, **kw):
    """one call on the handle and in the reference: every field of the result and the label volume afterwards; (result, labels after)"""
    got = res.smooth_labels(radius, source, new_label, **kw)
    _, want, after = SR.smooth(labels, radius, source, new_label, **kw)
    where = (labels.shape, radius, source, new_label, kw)
    for k in SR.FIELDS:
        assert got[k] == want[k], (k, got, want, where)
    assert got["launches"] == kw.get("iterations", 1), (got, where)
    down = res.download_label_volume()
    assert np.array_equal(down, after), (where, int((down != after).sum()), np.argwhere(down != after)[:5])
    return got, after


def fresh(res, labels, radius, source, new_label, **kw):
    res.upload_label_volume(labels)
    return same(res, labels, radius, source, new_label, **kw)


# ---- noise: every single count matters ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("density", SR.NOISE_DENSITIES)
@pytest.mark.parametrize("dims", SR.NOISE_SHAPES, ids=ids)
def test_noise(gpu, dims, density):
    labels = SR.noise(dims, density)
    moved = 0
    with make_res(dims, labels) as res:
        for radius, rank, iterations in itertools.product(SR.NOISE_RADII, SR.NOISE_RANKS, SR.NOISE_ITERATIONS):
            got, _ = fresh(res, labels, radius, [1], 1, rank=rank, iterations=iterations)
            assert got["reach"] == tuple(iterations * r for r in radius)
            moved += got["added"] + got["removed"]
    assert moved > 0


# ---- the window's edges: one, two and three bricks along each axis ----------------------------------------------------------------
@pytest.mark.parametrize("axis", [0, 1, 2], ids=["x", "y", "z"])
def test_window_edges(gpu, axis):
    dims = SR.long_dims(axis)
    dots = SR.points(axis)
    with make_res(dims, dots) as res:
        for r in SR.EDGE_RADII:
            radius = SR.long_radius(axis, r)
            for end, rank in itertools.product(SR.HALF_ENDS, SR.HALF_RANKS):
                got, _ = fresh(res, SR.half_space(axis, end), radius, [1], 1, rank=rank)
                assert got["added"] + got["removed"] > 0, (r, end, rank)
            for rank in SR.POINT_RANKS:
                got, _ = fresh(res, dots, radius, [1], 1, rank=rank)
                assert got["added"] > 0, (r, rank)


@pytest.mark.parametrize("axis", [0, 1, 2], ids=["x", "y", "z"])
def test_largest_reach(gpu, axis):
    """radius 16, four passes: a reach of 64 along an axis of 140 voxels"""
    dims = SR.long_dims(axis, SR.REACH_LONG)
    radius = SR.long_radius(axis, 16, 0)
    dots = SR.points(axis, SR.REACH_LONG, SR.REACH_POINTS)
    want_reach = tuple(64 if c == axis else 0 for c in range(3))
    with make_res(dims, dots) as res:
        got, after = same(res, dots, radius, [1], 1, rank=(0, 1), iterations=4)
        assert got["reach"] == want_reach and got["result_voxels"] == int((after == 1).sum()) > 5 * 65
        got, _ = fresh(res, SR.half_space(axis, 69, SR.REACH_LONG), radius, [1], 1, rank=(1, 3), iterations=4)
        assert got["added"] > 0
        # a box in the middle: the range is the box grown by the whole reach, the points beyond it act on it through four passes
        origin, extent = [0, 0, 0], list(dims)
        origin[axis], extent[axis] = 60, 12
        got, _ = fresh(res, dots, radius, [1], 1, rank=(0, 1), iterations=4, origin=origin, extent=extent)
        assert got["added"] > 0 and got["source_voxels"] == int(dots[tuple(slice(60, 72) if 2 - c == axis else slice(None) for c in range(3))].sum())


def test_radius_16_on_all_three_axes(gpu):
    dims = (40, 40, 40)
    labels = SR.noise(dims, 0.5)
    with make_res(dims, labels) as res:
        for rank in ((1, 2), (127, 256)):
            got, _ = fresh(res, labels, (16, 16, 16), [1], 1, rank=rank)
            assert got["reach"] == (16, 16, 16) and got["added"] > 0 and got["removed"] > 0


# ---- ties, and the clipped box ------------------------------------------------------------------------------------------------------
def test_nothing_is_set_at_a_tie(gpu):
    dims = (17, 9, 24)
    board = SR.checkerboard(dims)
    tie = SR.ties(board == 1, (1, 1, 1))
    assert tie.sum() > 0
    with make_res(dims, board) as res:
        _, after = same(res, board, (1, 1, 1), [1], 1)
        assert not (after == 1)[tie].any()
        _, after = fresh(res, 1 - board, (1, 1, 1), [1], 1)     # the other colour: the same ties, unset again
        assert not (after == 1)[SR.ties(board == 0, (1, 1, 1))].any()


@pytest.mark.parametrize("at", [(7, 7, 7), (8, 8, 8), (0, 0, 0), (39, 23, 18), (39, 0, 8)], ids=ids)
def test_single_voxels_give_the_clipped_box(gpu, at):
    dims = (40, 24, 19)
    labels = np.zeros(dims[::-1], dtype=np.uint8)
    labels[at[2], at[1], at[0]] = 1
    with make_res(dims, labels) as res:
        for radius in ((1, 1, 1), (2, 2, 2), (3, 2, 1), (9, 0, 4), (16, 16, 16)):
            got, _ = fresh(res, labels, radius, [1], 1, rank=(0, 1))
            box = 1
            for c in range(3):
                box *= min(at[c] + radius[c], dims[c] - 1) - max(at[c] - radius[c], 0) + 1
            assert got["result_voxels"] == box == got["added"] + 1, (radius, got)
            lo = tuple(max(at[c] - radius[c], 0) for c in range(3))
            hi = tuple(min(at[c] + radius[c], dims[c] - 1) for c in range(3))
            assert got["bbox_min"] == tuple(min(l, a) for l, a in zip(lo, at)) and got["bbox_max"] == hi


# ---- cross-checks against the morphology on one handle, by bytes ---------------------------------------------------------------------
def test_rank_zero_is_the_dilation_and_27_of_28_the_erosion(gpu):
    dims = (40, 24, 19)
    labels = SR.blob_labels(dims)
    sparse = np.zeros(dims[::-1], dtype=np.uint8)
    sparse[(2, 9, 18, 11), (3, 20, 8, 23), (5, 39, 17, 0)] = 3
    with make_res(dims, labels) as res:
        def after(call, start):
            res.upload_label_volume(start)
            got = call()
            return got, res.download_label_volume()

        for r, start in ((1, labels), (3, labels), (9, sparse)):
            a, smooth_bytes = after(lambda: res.smooth_labels((r, r, r), [3], 3, rank=(0, 1)), start)
            b, morph_bytes = after(lambda: res.morph_labels("dilate", r, [3], 3, connectivity=26), start)
            assert np.array_equal(smooth_bytes, morph_bytes), r
            assert all(a[k] == b[k] for k in MR.FIELDS) and a["added"] > 0 and not (smooth_bytes == 3).all()
        for k in (2, 3, 5):
            a, one = after(lambda: res.smooth_labels((1, 1, 1), [3], 3, rank=(0, 1), iterations=k), sparse)
            b, two = after(lambda: res.smooth_labels((k, k, k), [3], 3, rank=(0, 1)), sparse)
            assert np.array_equal(one, two) and a["reach"] == b["reach"] == (k, k, k) and a["launches"] == k and b["launches"] == 1
            assert all(a[f] == b[f] for f in SR.FIELDS)
        a, smooth_bytes = after(lambda: res.smooth_labels((1, 1, 1), [3], 3, rank=(27, 28), erase_label=9), labels)
        b, morph_bytes = after(lambda: res.morph_labels("erode", 1, [3], 3, connectivity=26, erase_label=9), labels)
        assert np.array_equal(smooth_bytes, morph_bytes) and all(a[k] == b[k] for k in MR.FIELDS) and a["removed"] > 0 and (smooth_bytes == 3).any()


# ---- ragged bricks, volume faces, the full volume and the empty source -----------------------------------------------------------------
def test_ragged_bricks_and_volume_faces(gpu):
    dims = (20, 17, 13)
    n = 20 * 17 * 13
    labels = np.zeros(dims[::-1], dtype=np.uint8)
    labels[8:, 12:, 16:] = 2   # x 16 .. 19, y 12 .. 16, z 8 .. 12: fills the ragged last bricks and touches three volume faces
    with make_res(dims, labels) as res:
        for radius in ((1, 1, 1), (2, 2, 2), (3, 2, 1)):
            got, after = fresh(res, labels, radius, [2], 2)
            # the faces have no vote: the corner block is its own median except for its free corner and edges
            assert got["added"] == 0 and 0 < got["removed"] < 4 * 5 * 5 and (after == 2)[12, 16, 19]
        for rank in ((1, 3), (0, 1), (27, 28)):
            fresh(res, labels, (2, 1, 3), [2], 2, rank=rank, iterations=2)
        # label 0 is in the source: the zero padding of the ragged bricks would qualify
        got, _ = fresh(res, labels, (4, 4, 4), [0], 0, rank=(0, 1))
        assert got["source_voxels"] == n - 5 * 5 * 4 and got["result_voxels"] == n
        solid = np.full(dims[::-1], 6, dtype=np.uint8)
        res.upload_label_volume(solid)
        before = res.smooth_counters()
        for radius, rank, iterations in (((1, 1, 1), (1, 2), 1), ((16, 16, 16), (255, 256), 2), ((3, 0, 9), (0, 1), 3), ((1, 1, 1), (27, 28), 4)):
            got, _ = same(res, solid, radius, [6], 6, rank=rank, iterations=iterations)   # a full volume stays full
            assert got["result_voxels"] == n and got["added"] == got["removed"] == 0
        c = res.smooth_counters()
        assert c["bricks_computed"] == before["bricks_computed"] and c["bricks_written"] == before["bricks_written"]   # the classes gave every brick
        assert c["smooth_calls"] == before["smooth_calls"] + 4 and c["launches"] == before["launches"] + 10
        for radius, rank in (((1, 1, 1), (1, 2)), ((16, 16, 16), (0, 1)), ((2, 1, 0), (1, 256))):   # the dual: an empty source
            got, _ = same(res, solid, radius, [1], 1, rank=rank)
            assert got["source_voxels"] == got["result_voxels"] == 0
        assert res.smooth_counters()["bricks_computed"] == before["bricks_computed"]


# ---- the tunable and the counters -----------------------------------------------------------------------------------------------------
def test_smooth_skip_changes_nothing_but_the_count(gpu, tunables):
    dims = (40, 40, 40)
    labels = SR.blob_labels(dims, seed=3)
    labels[:, :, 24:] = 0          # an empty part ...
    labels[:16, :16, :16] = 3      # ... and full bricks: both kinds of brick the classes give
    with make_res(dims, labels) as res:
        for radius, rank, iterations in (((1, 1, 1), (1, 2), 1), ((2, 1, 0), (1, 3), 2), ((3, 9, 1), (2, 3), 1), ((1, 1, 1), (0, 1), 3)):
            results, computed = [], []
            for skip in (1, 0):
                tunables("smooth_skip", skip)
                before = res.smooth_counters()["bricks_computed"]
                results.append(fresh(res, labels, radius, [3], 3, rank=rank, iterations=iterations, erase_label=9))
                computed.append(res.smooth_counters()["bricks_computed"] - before)
            assert results[0][0] == results[1][0] and np.array_equal(results[0][1], results[1][1])
            assert computed[1] == 125 * iterations and 0 < computed[0] < computed[1], (computed, radius)
        tunables("smooth_skip", 1)
        one = np.zeros(dims[::-1], dtype=np.uint8)
        one[20, 20, 20] = 1
        before = res.smooth_counters()
        fresh(res, one, (3, 3, 3), [1], 1, rank=(0, 1))
        c = res.smooth_counters()
        assert 1 <= c["bricks_computed"] - before["bricks_computed"] <= 27 and c["bricks_written"] - before["bricks_written"] <= 8
        assert c["smooth_calls"] == before["smooth_calls"] + 1 and c["launches"] == before["launches"] + 1
        fresh(res, one, (9, 9, 9), [1], 1, rank=(0, 1))   # two bricks either side
        assert 27 < res.smooth_counters()["bricks_computed"] - c["bricks_computed"] <= 125


# ---- boxes ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius, iterations", [((1, 1, 1), 1), ((3, 2, 1), 2)], ids=["r1", "r321x2"])
def test_boxes(gpu, radius, iterations):
    dims = (40, 24, 19)
    labels = SR.blob_labels(dims, seed=13)
    with make_res(dims, labels) as res:
        for origin, extent in BOXES:
            for rank in ((1, 2), (1, 3)):
                _, after = fresh(res, labels, radius, [3], 3, rank=rank, iterations=iterations, origin=origin, extent=extent)
                outside = np.ones(labels.shape, dtype=bool)
                outside[origin[2]:origin[2] + extent[2], origin[1]:origin[1] + extent[1], origin[0]:origin[0] + extent[0]] = False
                assert np.array_equal(after[outside], labels[outside])
        # an all-zero extent is the whole volume, whatever the origin
        fresh(res, labels, radius, [3], 3, iterations=iterations, origin=(3, 3, 3), extent=(0, 0, 0))
    # the set outside the box acts on the inside: a slab that ends one voxel short of the box
    labels = np.zeros(dims[::-1], dtype=np.uint8)
    labels[:, :, :8] = 4
    with make_res(dims, labels) as res:
        got, _ = same(res, labels, (3, 0, 0), [4], 4, rank=(0, 1), origin=(8, 8, 8), extent=(8, 8, 8))
        assert got["source_voxels"] == 0 and got["added"] == got["result_voxels"] == 3 * 8 * 8 and got["bbox_max"] == (10, 15, 15)


# ---- masks ----------------------------------------------------------------------------------------------------------------------------
def test_sources_of_several_labels_writable_and_measuring(gpu):
    dims = (24, 17, 10)
    labels = SR.blob_labels(dims, seed=19)
    labels[:, :, 20:] = 5            # a finished segment
    with make_res(dims, labels) as res:
        fresh(res, labels, (1, 1, 1), [3, 7], 7, erase_label=1)                   # the union of two labels; joins get one of them
        fresh(res, labels, (2, 1, 1), [255, 0, 64], 64, rank=(1, 3))              # labels at both ends of the mask words
        got, after = fresh(res, labels, (2, 2, 2), [3], 3, rank=(1, 4), writable=[0])
        assert got["added"] > 0 and np.array_equal(after == 5, labels == 5) and np.array_equal(after == 7, labels == 7)   # walls for joins
        assert got["result_voxels"] > got["source_voxels"] + got["added"] - got["removed"]                              # ... though the result reaches into them
        got, after = fresh(res, labels, (2, 2, 2), [3], 3, rank=(1, 4), writable=[0, 7])
        assert (after == 7).sum() < (labels == 7).sum()
        got, after = fresh(res, labels, (1, 1, 1), [3], 3, rank=(2, 3), writable=[], erase_label=8)   # leaves are the source's own voxels
        assert got["removed"] == (after == 8).sum() > 0 and got["added"] == 0
        got, after = fresh(res, labels, (1, 1, 1), [3], 200, rank=(1, 3))         # what joins as a label of its own
        assert got["added"] == (after == 200).sum() > 0
        for radius, rank in (((1, 1, 1), (1, 2)), ((3, 2, 1), (1, 3))):           # measuring changes nothing (same() compares the bytes)
            got, still = same(res, after, radius, [3], -1, rank=rank)
            assert np.array_equal(still, after) and got["relabelled"] == 0 and got["added"] + got["removed"] > 0


# ---- state ------------------------------------------------------------------------------------------------------------------------------
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
    labels = np.where(vol >= np.percentile(vol, 50), 1, 0).astype(np.uint8)   # label 1: red, half transparent
    rp = abi.RaymarchParams(100.0, 1, True)
    world = S.default_world()
    radius = abi.smooth_radii((1.0, 1.0, 2.5), 2.0)
    assert radius == (2, 2, 1)
    with lit_handle(dims, vol, labels) as res:
        light = res.download_light_volume()
        plain = res.raymarch_lit(CAM, TILE, rp, world)
        m = res.smooth_labels(radius, [1], -1)   # a measure-only call changes nothing at all
        assert m["removed"] > 0 and m["added"] > 0 and m["relabelled"] == 0
        assert np.array_equal(res.download_label_volume(), labels)
        assert np.array_equal(res.raymarch_lit(CAM, TILE, rp, world), plain)
        counters = res.path_counters()
        got, after = same(res, labels, radius, [1], 1)
        assert {k: got[k] for k in SR.FIELDS if k != "relabelled"} == {k: m[k] for k in SR.FIELDS if k != "relabelled"}
        assert res.path_counters() == counters   # the call's waits are its own, its scratch was taken by the measuring call
        frame = res.raymarch_lit(CAM, TILE, rp, world)
        assert not np.array_equal(frame, plain)
        stats = res.label_statistics()
        assert np.array_equal(res.download_light_volume(), light)   # nothing on the data side moved
        want_next = MR.morph(after, MR.CLOSE, 2, [1], 1, connectivity=26)
        next_ = res.morph_labels("close", 2, [1], 1, connectivity=26)
        after_next = res.download_label_volume()
    with lit_handle(dims, vol, np.zeros_like(after)) as other:   # a fresh handle that gets the same bytes through update_label_region
        other.update_label_region((0, 0, 0), after)
        assert np.array_equal(other.raymarch_lit(CAM, TILE, rp, world), frame)
        assert np.array_equal(other.label_statistics(), stats)
        assert other.morph_labels("close", 2, [1], 1, connectivity=26) == next_
        assert np.array_equal(other.download_label_volume(), after_next)
    assert all(next_[k] == want_next[1][k] for k in MR.FIELDS) and np.array_equal(after_next, want_next[2])
    assert stats[1]["count"] == (after == 1).sum() == got["result_voxels"]


# ---- allocation -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grown_first", [False, True], ids=["fresh", "grown"])
def test_repeated_calls_allocate_nothing(gpu, grown_first):
    dims = (40, 24, 19)
    labels = SR.blob_labels(dims, seed=23)
    cases = [((1, 1, 1), (1, 2), 1, {}), ((16, 16, 16), (1, 2), 1, {}), ((3, 2, 1), (1, 3), 3, {}), ((2, 2, 2), (0, 1), 1, dict(origin=(8, 8, 8), extent=(8, 8, 8))),
             ((16, 0, 4), (2, 3), 4, {})]
    with make_res(dims, labels) as res:
        if grown_first:
            res.grow_region([(0, 0, 0)], 0, 255, -1, 6)   # takes the boards' scratch
        after = labels
        _, after = same(res, after, (1, 1, 1), [3], 3)   # the first call takes what it needs
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        allocs = res.path_counters()["operator_alloc_calls"]
        for k in range(20):
            radius, rank, iterations, kw = cases[k % len(cases)]
            _, after = same(res, after, radius, [3], 3 if k % 3 else -1, rank=rank, iterations=iterations, **kw)
            torch.cuda.synchronize()
            assert torch.cuda.mem_get_info()[0] == free0, k
        assert res.path_counters()["operator_alloc_calls"] == allocs
        assert res.smooth_counters()["smooth_calls"] == 21
        g = res.grow_region([(0, 0, 0)], 0, 255, -1, 6)   # region growing finds its scratch usable after the smoothing worked in it
        assert g["voxels"] == 40 * 24 * 19
        m = res.morph_labels("dilate", 1, [3], -1)        # and so does the morphology
        assert m["result_voxels"] == int(MR.dilate(after == 3, 1, 6).sum())


# ---- handles and refusals ---------------------------------------------------------------------------------------------------------------
def test_handles(gpu):
    dims = (24, 17, 10)
    vol = np.zeros(dims[::-1], dtype=np.uint8)
    with abi.Resources(dims, abi.FMT_G8) as res:
        with pytest.raises(abi.TbrmError) as e:
            res.smooth_labels(1, [1], 1)        # no volume yet
        assert e.value.code == abi.ERR_NOT_INITIALIZED
        res.upload_volume(vol)
        for label in (1, -1):                  # no label volume: nothing to take the set from, measuring included
            with pytest.raises(abi.TbrmError) as e:
                res.smooth_labels(1, [1], label)
            assert e.value.code == abi.ERR_NOT_INITIALIZED
        res.attach_empty_labels()
        assert res.smooth_labels(1, [1], 1)["result_voxels"] == 0
        assert res.smooth_labels(1, [0], 0)["result_voxels"] == 24 * 17 * 10
    with abi.Resources(dims, abi.FMT_G8, False, False, 0, rgb=True) as res:   # a colour handle has no label volume
        res.upload_volume(vol)
        with pytest.raises(abi.TbrmError) as e:
            res.smooth_labels(1, [0], -1)
        assert e.value.code == abi.ERR_NOT_INITIALIZED
    with abi.Resources((32, 32, 64), abi.FMT_G16, owned=abi.Slab(0, 32)) as part:
        with pytest.raises(abi.TbrmError) as e:
            part.smooth_labels(1, [0], -1)
        assert e.value.code == abi.ERR_UNSUPPORTED


def test_refusals(gpu):
    dims = (24, 17, 10)
    labels = SR.blob_labels(dims, seed=29)
    with make_res(dims, labels) as res:
        good = dict(radius=(1, 1, 1), source=[3], new_label=3)
        bad = [(dict(radius=(17, 1, 1)), b"radius[0]"), (dict(radius=(1, 1, 17)), b"radius[2]"), (dict(radius=(1, -1, 1)), b"radius[1]"), (dict(radius=(0, 0, 0)), b"radius"),
               (dict(iterations=0), b"iterations"), (dict(iterations=65), b"iterations"), (dict(iterations=-1), b"iterations"),
               (dict(radius=(1, 1, 16), iterations=5), b"iterations"), (dict(radius=(2, 1, 1), iterations=33), b"iterations"),
               (dict(rank=(1, 0)), b"rank_den"), (dict(rank=(1, 257)), b"rank_den"), (dict(rank=(0, -2)), b"rank_den"),
               (dict(rank=(2, 2)), b"rank_num"), (dict(rank=(-1, 2)), b"rank_num"), (dict(rank=(256, 256)), b"rank_num"),
               (dict(new_label=256), b"new_label"), (dict(new_label=-2), b"new_label"), (dict(erase_label=256), b"erase_label"), (dict(erase_label=-1), b"erase_label"),
               (dict(origin=(23, 0, 0), extent=(2, 1, 1)), b"box"), (dict(origin=(0, 0, 0), extent=(1, 0, 1)), b"box"), (dict(origin=(-1, 0, 0), extent=(2, 1, 1)), b"box"),
               (dict(origin=(0, 0, 0), extent=(24, 17, 11)), b"box")]
        for change, names in bad:
            with pytest.raises(abi.TbrmError) as e:
                res.smooth_labels(**{**good, **change})
            assert e.value.code == abi.ERR_INVALID_ARG, change
            assert names in str(e.value).encode(), (change, str(e.value))
        d = res.smooth_desc(**good)
        d.reserved = 1
        out = abi.SMOOTH_RESULT()
        assert res.lib.tbrm_smooth_labels(res.handle, d, out) == abi.ERR_INVALID_ARG and b"reserved" in res.lib.tbrm_last_error()
        assert np.array_equal(res.download_label_volume(), labels) and res.smooth_counters()["smooth_calls"] == 0
        # the bounds themselves are admitted
        got, _ = same(res, labels, (16, 16, 16), [3], 3, rank=(255, 256), iterations=4)
        assert got["reach"] == (64, 64, 64)
        fresh(res, labels, (1, 0, 0), [3], 3, rank=(0, 256), iterations=64)
        fresh(res, labels, (0, 2, 1), [3], 3, rank=(0, 1), iterations=32)


# ---- a sequence on one handle: the shared scratch and the lazily merged metadata ------------------------------------------------------------
def test_twelve_random_steps_with_the_other_writers(gpu):
    dims = (40, 24, 19)
    rng = np.random.default_rng(2024)
    vol = rng.integers(0, 256, size=dims[::-1]).astype(np.uint8)
    labels = SR.blob_labels(dims, seed=37)
    kinds = ["smooth", "morph", "smooth", "margin", "grow", "smooth", "region", "smooth", "morph", "margin", "smooth", "grow"]
    with make_res(dims, labels, vol) as res:
        for step, kind in enumerate(kinds):
            o = [int(rng.integers(0, d - 4)) for d in dims]
            e = [int(rng.integers(3, d - a + 1)) for d, a in zip(dims, o)]
            box = dict(origin=tuple(o), extent=tuple(e)) if step % 3 else {}
            source = [3] if step % 2 else [3, 7]
            if kind == "smooth":
                radius = tuple(int(v) for v in rng.integers(0, 4, size=3))
                radius = radius if any(radius) else (1, 1, 1)
                rank = [(1, 2), (1, 3), (2, 3), (0, 1)][int(rng.integers(0, 4))]
                _, labels = same(res, labels, radius, source, 3, rank=rank, iterations=int(rng.integers(1, 4)), erase_label=int(rng.integers(0, 2)) * 7, **box)
            elif kind == "morph":
                op, r, conn = int(rng.integers(0, 4)), int(rng.integers(1, 4)), (6, 26)[int(rng.integers(0, 2))]
                got = res.morph_labels(op, r, source, 3, connectivity=conn, **box)
                _, want, labels = MR.morph(labels, op, r, source, 3, connectivity=conn, **box)
                assert all(got[k] == want[k] for k in MR.FIELDS), (step, got, want)
            elif kind == "margin":
                op, limit = int(rng.integers(0, 4)), int(rng.integers(1, 10))
                got = res.margin_labels(op, (1, 1, 1), limit, source, 3, **box)
                _, want, labels = GR.margin(labels, op, (1, 1, 1), limit, source, 3, **box)
                assert all(got[k] == want[k] for k in GR.FIELDS), (step, got, want)
            elif kind == "grow":
                lo = int(rng.integers(100, 200))
                got = res.grow_region(None, lo, 255, 7, 6, **box)
                _, want, labels = RR.grow(vol, None, lo, 255, 7, 6, labels=labels, **box)
                assert all(got[k] == want[k] for k in ("voxels", "relabelled", "bbox_min", "bbox_max")), (step, got, want)
            else:
                block = rng.integers(0, 9, size=e[::-1]).astype(np.uint8)
                res.update_label_region(o, block)
                labels = labels.copy()
                labels[o[2]:o[2] + e[2], o[1]:o[1] + e[1], o[0]:o[0] + e[0]] = block
            down = res.download_label_volume()
            assert np.array_equal(down, labels), (step, kind, np.argwhere(down != labels)[:5])
        stats = res.label_statistics()
        assert all(int(stats[l]["count"]) == int((labels == l).sum()) for l in range(10))
