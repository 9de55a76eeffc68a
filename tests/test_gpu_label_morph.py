"""Label morphology (include/tbrm_morphology.h) on the GPU against tests/label_morph_reference.py. The results are integers and bytes:
every comparison is exact equality — of the downloaded label volume and of every field of the result."""
import numpy as np
import pytest
import torch

from tbraymarcherplugin_amd import abi, synthetic as S
import label_morph_reference as MR

pytestmark = pytest.mark.gpu

SHAPES = [(40, 24, 19), (24, 17, 10), (5, 6, 3), (16, 16, 16), (24, 24, 24), (40, 40, 40)]   # the grow tests' shapes, 24^3 and 40^3
BOXES = [((11, 5, 3), (13, 9, 7)), ((17, 9, 4), (1, 1, 1)), ((8, 8, 8), (8, 8, 8)), ((3, 2, 16), (30, 20, 3)), ((21, 0, 0), (1, 24, 19))]   # the grow tests' boxes
OP_NAMES = {MR.DILATE: "dilate", MR.ERODE: "erode", MR.OPEN: "open", MR.CLOSE: "close"}
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


def same(res, labels, op, radius, source, new_label, connectivity=6, **kw):
    """one call on the handle and in the reference: every field of the result and the label volume afterwards; (result, labels after)"""
    got = res.morph_labels(op, radius, source, new_label, connectivity, **kw)
    _, want, after = MR.morph(labels, op, radius, source, new_label, connectivity, **kw)
    where = (labels.shape, OP_NAMES[op], radius, source, new_label, connectivity, kw)
    for k in MR.FIELDS:
        assert got[k] == want[k], (k, got, want, where)
    assert got["launches"] == MR.launches(op, radius, abi.get_tunable("morph_steps")), (got, where)
    down = res.download_label_volume()
    assert np.array_equal(down, after), (where, int((down != after).sum()), np.argwhere(down != after)[:5])
    return got, after


# ---- blobs ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("dims", SHAPES, ids=ids)
def test_blobs(gpu, dims, connectivity):
    labels = blob_labels(dims)
    assert (labels == 3).any()
    moved = 0
    with make_res(dims, labels) as res:
        for op in MR.OPS:
            for radius in (1, 2, 3):
                res.upload_label_volume(labels)
                got, _ = same(res, labels, op, radius, [3], 3, connectivity)
                moved += got["added"] + got["removed"]
    assert moved > 0


# ---- more steps than a window holds ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("radius", [8, 9, 17])
def test_morph_steps(gpu, tunables, radius, connectivity):
    """8 steps fill a window, 9 and 17 need a second and a third launch: the ping-pong between the boards and the window's edge.
    The result is the same at one, three and eight steps per launch; launches = ceil(r / steps), twice that for open and close."""
    dims = (40, 40, 40)
    labels = blob_labels(dims, seed=3)
    labels[20, 20, 20] = 3
    with make_res(dims, labels) as res:
        for op in MR.OPS:
            _, want, after = MR.morph(labels, op, radius, [3], 3, connectivity, erase_label=9)
            for steps in (1, 3, 8):
                tunables("morph_steps", steps)
                res.upload_label_volume(labels)
                got = res.morph_labels(op, radius, [3], 3, connectivity, erase_label=9)
                assert {k: got[k] for k in MR.FIELDS} == want, (OP_NAMES[op], steps)
                assert got["launches"] == -(-radius // steps) * (2 if op in (MR.OPEN, MR.CLOSE) else 1)
                assert np.array_equal(res.download_label_volume(), after), (OP_NAMES[op], steps)


# ---- single voxels: brick corners and volume faces ------------------------------------------------------------------------------
@pytest.mark.parametrize("at", [(7, 7, 7), (8, 8, 8), (0, 0, 0), (39, 23, 18)], ids=ids)
def test_single_voxels(gpu, at):
    dims = (40, 24, 19)
    labels = np.zeros(dims[::-1], dtype=np.uint8)
    labels[at[2], at[1], at[0]] = 1
    with make_res(dims, labels) as res:
        for connectivity in (6, 26):
            for radius in (1, 2, 3, 9):
                res.upload_label_volume(labels)
                got, after = same(res, labels, MR.DILATE, radius, [1], 1, connectivity)
                if at in ((7, 7, 7), (8, 8, 8)) and radius == 1:
                    assert got["result_voxels"] == (7 if connectivity == 6 else 27)
                # and back: eroding the dilated voxel by the same radius leaves it where the faces did not clip the dilation
                got, _ = same(res, after, MR.ERODE, radius, [1], 1, connectivity)
                assert got["result_voxels"] >= 1
            res.upload_label_volume(labels)
            got, after = same(res, labels, MR.OPEN, 1, [1], 1, connectivity)   # a single voxel does not survive an opening
            assert got["result_voxels"] == 0 and got["removed"] == 1 and not after.any()
            res.upload_label_volume(labels)
            got, _ = same(res, labels, MR.CLOSE, 2, [1], 1, connectivity)       # and a closing leaves it alone
            assert got["added"] == got["removed"] == 0 and got["bbox_min"] == dims and got["bbox_max"] == (-1, -1, -1)


# ---- ragged bricks and volume faces ---------------------------------------------------------------------------------------------
def test_ragged_bricks_and_volume_faces(gpu):
    dims = (20, 17, 13)
    labels = np.zeros(dims[::-1], dtype=np.uint8)
    labels[8:, 12:, 16:] = 2   # x 16 .. 19, y 12 .. 16, z 8 .. 12: fills the ragged last bricks and touches three volume faces
    with make_res(dims, labels) as res:
        for connectivity in (6, 26):
            for radius in (1, 2):
                res.upload_label_volume(labels)
                got, after = same(res, labels, MR.ERODE, radius, [2], 2, connectivity)
                # eaten from the three free sides only: the volume faces do not erode, the padding beyond them never counts as unset
                assert np.array_equal(after == 2, np.pad(np.ones((5 - radius, 5 - radius, 4 - radius), dtype=bool), ((8 + radius, 0), (12 + radius, 0), (16 + radius, 0))))
            res.upload_label_volume(labels)
            same(res, labels, MR.DILATE, 3, [2], 2, connectivity)
            # label 0 is in the source: the zero padding of the ragged bricks would qualify
            res.upload_label_volume(labels)
            got, _ = same(res, labels, MR.DILATE, 4, [0], 0, connectivity)
            assert got["source_voxels"] == 20 * 17 * 13 - 5 * 5 * 4 and got["result_voxels"] == 20 * 17 * 13
        solid = np.full(dims[::-1], 6, dtype=np.uint8)
        res.upload_label_volume(solid)
        for op in (MR.ERODE, MR.OPEN, MR.CLOSE, MR.DILATE):
            got, _ = same(res, solid, op, 3, [6], 6, 26)   # a solid volume survives every operator
            assert got["result_voxels"] == 20 * 17 * 13 and got["added"] == got["removed"] == 0


# ---- boxes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [6, 26])
def test_boxes(gpu, connectivity):
    dims = SHAPES[0]
    labels = blob_labels(dims, seed=13)
    with make_res(dims, labels) as res:
        for origin, extent in BOXES:
            for op in MR.OPS:
                res.upload_label_volume(labels)
                _, after = same(res, labels, op, 2, [3], 3, connectivity, origin=origin, extent=extent)
                outside = np.ones(labels.shape, dtype=bool)
                outside[origin[2]:origin[2] + extent[2], origin[1]:origin[1] + extent[1], origin[0]:origin[0] + extent[0]] = False
                assert np.array_equal(after[outside], labels[outside])
        # an all-zero extent is the whole volume, whatever the origin
        res.upload_label_volume(labels)
        same(res, labels, MR.CLOSE, 1, [3], 3, connectivity, origin=(3, 3, 3), extent=(0, 0, 0))
    # the set outside the box acts on the inside: a slab that ends one voxel short of the box
    labels = np.zeros(dims[::-1], dtype=np.uint8)
    labels[:, :, :8] = 4
    with make_res(dims, labels) as res:
        got, after = same(res, labels, MR.DILATE, 3, [4], 4, connectivity, origin=(8, 8, 8), extent=(8, 8, 8))
        assert got["source_voxels"] == 0 and got["added"] == got["result_voxels"] == 3 * 8 * 8 and got["bbox_max"] == (10, 15, 15)
        res.upload_label_volume(labels)
        got, _ = same(res, labels, MR.ERODE, 2, [4], 4, connectivity, origin=(4, 0, 0), extent=(4, 24, 19))
        assert got["removed"] == 2 * 24 * 19 and got["bbox_min"] == (6, 0, 0) and got["bbox_max"] == (7, 23, 18)


# ---- masks ----------------------------------------------------------------------------------------------------------------------
def test_writable_blocks_joins_and_not_leaves(gpu):
    dims = (24, 17, 10)
    labels = np.zeros(dims[::-1], dtype=np.uint8)
    labels[:, :, 12:] = 5            # a finished segment beside the blobs
    blob = MR.blobs(dims, seed=17)
    labels[blob & (labels == 0)] = 3
    with make_res(dims, labels) as res:
        got, after = same(res, labels, MR.DILATE, 2, [3], 3, 6, writable=[0])
        assert got["added"] > 0 and np.array_equal(after == 5, labels == 5)        # label 5 is a wall for joins
        assert got["result_voxels"] > got["source_voxels"] + got["added"]          # ... though the result reaches into it
        res.upload_label_volume(labels)
        got, after = same(res, labels, MR.DILATE, 2, [3], 3, 6, writable=[0, 5])
        assert (after == 5).sum() < (labels == 5).sum() and got["result_voxels"] == got["source_voxels"] + got["added"]
        res.upload_label_volume(labels)
        got, after = same(res, labels, MR.ERODE, 1, [3], 3, 26, writable=[], erase_label=8)   # leaves are the source's own voxels
        assert got["removed"] == (after == 8).sum() > 0 and got["added"] == 0
        res.upload_label_volume(labels)
        got, _ = same(res, labels, MR.CLOSE, 2, [3], 3, 26, writable=[])
        assert got["added"] == 0 and got["relabelled"] == 0


def test_multi_label_source_and_new_labels(gpu):
    dims = (24, 17, 10)
    labels = blob_labels(dims, seed=19)
    with make_res(dims, labels) as res:
        for op in MR.OPS:
            res.upload_label_volume(labels)
            same(res, labels, op, 2, [3, 7], 7, 26, erase_label=1)     # the union of two labels; joins get one of them
        res.upload_label_volume(labels)
        got, after = same(res, labels, MR.DILATE, 1, [3], 200, 6)      # a margin as a label of its own, not in the source
        assert got["added"] == (after == 200).sum() == got["relabelled"] > 0
        got, _ = same(res, after, MR.DILATE, 1, [3], 200, 6)           # again: the margin holds new_label already
        assert got["added"] > 0 and got["relabelled"] == 0
        got, _ = same(res, after, MR.OPEN, 2, [255, 0, 64], -1, 6)     # labels at both ends of the mask words
        assert got["source_voxels"] == (after == 0).sum()


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
    with lit_handle(dims, vol, labels) as res:
        light = res.download_light_volume()
        plain = res.raymarch_lit(CAM, TILE, rp, world)
        counters = res.path_counters()
        # a measure-only call changes nothing at all
        m = res.morph_labels("open", 2, [1], -1, 26)
        assert m["removed"] > 0 and m["relabelled"] == 0
        measured = res.path_counters()   # no operator ran, nothing of theirs was launched or waited for; the scratch is the one allocation
        assert {**measured, "operator_alloc_calls": 0} == {**counters, "operator_alloc_calls": 0}
        assert measured["operator_alloc_calls"] == counters["operator_alloc_calls"] + 1
        assert np.array_equal(res.download_label_volume(), labels)
        assert np.array_equal(res.raymarch_lit(CAM, TILE, rp, world), plain)
        counters = res.path_counters()
        got, after = same(res, labels, MR.OPEN, 2, [1], 1, 26)
        assert {k: got[k] for k in MR.FIELDS if k != "relabelled"} == {k: m[k] for k in MR.FIELDS if k != "relabelled"}
        assert res.path_counters() == counters   # nor for the writing call, which finds the scratch taken
        frame = res.raymarch_lit(CAM, TILE, rp, world)
        assert not np.array_equal(frame, plain)
        stats = res.label_statistics()
        assert np.array_equal(res.download_light_volume(), light)   # nothing on the data side moved
        # a second writing call inside a box, with labels of its own for what joins and what leaves
        got2, after2 = same(res, after, MR.DILATE, 3, [1], 2, 6, origin=(5, 4, 3), extent=(30, 33, 20), erase_label=0)
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


# ---- skipping, counters, allocation ---------------------------------------------------------------------------------------------
def test_windows_skipped_by_class(gpu):
    dims = (40, 40, 40)
    labels = np.zeros(dims[::-1], dtype=np.uint8)
    labels[20, 20, 20] = 1
    with make_res(dims, labels) as res:
        assert res.morph_counters() == {"morph_calls": 0, "step_launches": 0, "windows": 0, "bricks_written": 0}
        same(res, labels, MR.DILATE, 1, [1], 1, 26)
        c = res.morph_counters()
        assert c["morph_calls"] == 1 and c["step_launches"] == 1 and 1 <= c["windows"] <= 27 and c["bricks_written"] == 1
        full = np.full(dims[::-1], 1, dtype=np.uint8)
        res.upload_label_volume(full)
        same(res, full, MR.ERODE, 9, [1], 1, 6)
        same(res, full, MR.DILATE, 9, [1], 1, 6)
        c2 = res.morph_counters()
        assert c2["windows"] == c["windows"] and c2["step_launches"] == c["step_launches"] + 4 and c2["bricks_written"] == 1   # no window, nothing written
        same(res, full, MR.DILATE, 2, [0], 0, 6)   # the dual: an empty set
        assert res.morph_counters()["windows"] == c["windows"]


def test_counters_add_up_and_a_handle_that_grew_allocates_nothing(gpu, tunables):
    dims = (40, 24, 19)
    labels = blob_labels(dims, seed=23)
    with make_res(dims, labels) as res:
        allocs0 = res.path_counters()["operator_alloc_calls"]
        res.grow_region([(0, 0, 0)], 0, 255, -1, 6)   # takes the scratch
        assert res.path_counters()["operator_alloc_calls"] == allocs0 + 1
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        syncs = res.path_counters()["operator_host_syncs"]
        launches = written = 0
        after = labels
        for k, (op, radius, steps) in enumerate([(MR.CLOSE, 2, 8), (MR.OPEN, 1, 8), (MR.DILATE, 9, 8), (MR.ERODE, 9, 2), (MR.CLOSE, 5, 1)]):
            tunables("morph_steps", steps)
            before = res.morph_counters()
            got, after = same(res, after, op, radius, [3], 3 if k != 2 else -1, 6 if k % 2 else 26)
            launches += got["launches"]
            c = res.morph_counters()
            assert c["morph_calls"] == k + 1 and c["step_launches"] == launches
            assert c["windows"] - before["windows"] <= got["launches"] * 5 * 3 * 3            # a brick at most once per launch
            assert (c["bricks_written"] > before["bricks_written"]) == (got["relabelled"] > 0)
            assert torch.cuda.mem_get_info()[0] == free0, k
        p = res.path_counters()
        assert p["operator_alloc_calls"] == allocs0 + 1 and p["operator_host_syncs"] == syncs   # the calls' waits are their own
        g = res.grow_region([(0, 0, 0)], 0, 255, -1, 6)   # region growing finds its scratch usable after morphology worked in it
        assert g["voxels"] == 40 * 24 * 19


# ---- handles and refusals -------------------------------------------------------------------------------------------------------
def test_handles(gpu):
    dims = (24, 17, 10)
    vol = np.zeros(dims[::-1], dtype=np.uint8)
    with abi.Resources(dims, abi.FMT_G8) as res:
        with pytest.raises(abi.TbrmError) as e:
            res.morph_labels("close", 1, [1], 1)        # no volume yet
        assert e.value.code == abi.ERR_NOT_INITIALIZED
        res.upload_volume(vol)
        for label in (1, -1):                           # no label volume: nothing to take the set from, measuring included
            with pytest.raises(abi.TbrmError) as e:
                res.morph_labels("close", 1, [1], label)
            assert e.value.code == abi.ERR_NOT_INITIALIZED
        res.attach_empty_labels()
        assert res.morph_labels("close", 1, [1], 1)["result_voxels"] == 0
    with abi.Resources(dims, abi.FMT_G8, False, False, 0, rgb=True) as res:   # a colour handle has no label volume
        res.upload_volume(vol)
        with pytest.raises(abi.TbrmError) as e:
            res.morph_labels("dilate", 1, [0], -1)
        assert e.value.code == abi.ERR_NOT_INITIALIZED
    with abi.Resources((32, 32, 64), abi.FMT_G16, owned=abi.Slab(0, 32)) as part:
        with pytest.raises(abi.TbrmError) as e:
            part.morph_labels("dilate", 1, [0], -1)
        assert e.value.code == abi.ERR_UNSUPPORTED


def test_refusals(gpu):
    dims = (24, 17, 10)
    labels = blob_labels(dims, seed=29)
    with make_res(dims, labels) as res:
        good = dict(op=abi.MORPH_CLOSE, radius=2, source=[3], new_label=3)
        bad = [dict(op=4), dict(op=-1), dict(radius=0), dict(radius=65), dict(radius=-3), dict(connectivity=18), dict(connectivity=0),
               dict(new_label=256), dict(new_label=-2), dict(erase_label=256), dict(erase_label=-1),
               dict(origin=(23, 0, 0), extent=(2, 1, 1)), dict(origin=(0, 0, 0), extent=(1, 0, 1)), dict(origin=(-1, 0, 0), extent=(2, 1, 1)),
               dict(origin=(0, 0, 0), extent=(24, 17, 11))]
        for change in bad:
            with pytest.raises(abi.TbrmError) as e:
                res.morph_labels(**{**good, **change})
            assert e.value.code == abi.ERR_INVALID_ARG, change
        d = res.morph_desc(**good)
        d.reserved = 1
        out = abi.MORPH_RESULT()
        assert res.lib.tbrm_morph_labels(res.handle, d, out) == abi.ERR_INVALID_ARG and b"reserved" in res.lib.tbrm_last_error()
        assert np.array_equal(res.download_label_volume(), labels) and res.morph_counters()["morph_calls"] == 0
        got, _ = same(res, labels, MR.DILATE, 64, [3], 3, 6)   # the largest radius: the whole volume joins
        assert got["result_voxels"] == 24 * 17 * 10
