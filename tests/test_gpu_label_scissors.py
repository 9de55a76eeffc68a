"""View-space scissors (include/tbrm_scissors.h) on the GPU against tests/label_scissors_reference.py. The results are integers and
bytes: every comparison is exact equality — of the downloaded label volume and of every field of the result. The inputs are judged
without a GPU in tests/test_label_scissors_reference.py."""
import numpy as np
import pytest
import torch

from tbraymarcherplugin_amd import abi, synthetic as S
import label_morph_reference as MR
import label_scissors_reference as SR

pytestmark = pytest.mark.gpu

CASES = {name: (dims, p, mask) for name, dims, p, mask in SR.gpu_cases()}
VERDICTS = {name: (dims, p, mask) for name, dims, p, mask in SR.verdict_cases()}


def make_res(dims, labels=None, vol=None):
    res = abi.Resources(dims, abi.FMT_G8, False, False, 0)
    res.upload_volume(vol if vol is not None else np.zeros(dims[::-1], dtype=np.uint8))   # scissors never read the data
    if labels is not None:
        res.upload_label_volume(labels)
    return res


def rows(p):
    return abi.make_scissors_projection(p["u"], p["v"], p["w"], p["w_min"], p["w_max"], p["width"], p["height"])


def same(res, labels, p, mask, op, source, new_label, **kw):
    """one call on the handle and in the reference: every field of the result and the label volume afterwards; (result, labels after)"""
    got = res.scissor_labels(rows(p), mask, op, source, new_label, **kw)
    _, want, after = SR.scissors(labels, p, mask, op, source, new_label, **kw)
    where = (labels.shape, op, source, new_label, kw)
    for k in SR.FIELDS:
        assert got[k] == want[k], (k, got, want, where)
    bricks = SR.box_bricks(labels.shape[::-1], kw.get("origin"), kw.get("extent"))
    assert 0 <= got["bricks_inside"] + got["bricks_outside"] + got["bricks_projected"] <= bricks, (got, where)
    down = res.download_label_volume()
    assert np.array_equal(down, after), (where, int((down != after).sum()), np.argwhere(down != after)[:5])
    return got, after


def fresh(res, labels, p, mask, op, source, new_label, **kw):
    res.upload_label_volume(labels)
    return same(res, labels, p, mask, op, source, new_label, **kw)


def either_way(tunables, res, labels, p, mask, op, source, new_label, **kw):
    """the call under scissors_skip 1 and 0: identical labels and results; under 0 every brick of the range is projected"""
    bricks = SR.box_bricks(labels.shape[::-1], kw.get("origin"), kw.get("extent"))
    out = []
    try:
        for skip in (1, 0):
            tunables("scissors_skip", skip)
            out.append(fresh(res, labels, p, mask, op, source, new_label, **kw))
    finally:
        tunables("scissors_skip", 1)
    assert {k: out[0][0][k] for k in SR.FIELDS} == {k: out[1][0][k] for k in SR.FIELDS} and np.array_equal(out[0][1], out[1][1])
    assert out[1][0]["bricks_projected"] == bricks and out[1][0]["bricks_inside"] == out[1][0]["bricks_outside"] == 0 and out[1][0]["launches"] == 1
    assert out[0][0]["bricks_projected"] <= bricks and out[0][0]["launches"] == 4
    return out[0]


# ---- every case, every operator, both ways ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_cases(gpu, tunables, name):
    dims, p, mask = CASES[name]
    labels = SR.blob_labels(dims, seed=7)
    moved = 0
    with make_res(dims, labels) as res:
        for op in SR.OPS:
            got, _ = either_way(tunables, res, labels, p, mask, op, [3], 3, erase_label=9)
            moved += got["added"] + got["removed"]
        # an empty and a full source set: the verdict from S alone, and what it must not decide
        got, after = either_way(tunables, res, np.zeros_like(labels), p, mask, SR.FILL_INSIDE, [3], 3)
        assert got["added"] == int(SR.in_M(p, mask, dims).sum()) == int((after == 3).sum()) > 0
        got, after = either_way(tunables, res, np.full_like(labels, 3), p, mask, SR.ERASE_INSIDE, [3], 3, erase_label=0)
        assert got["removed"] == int(SR.in_M(p, mask, dims).sum()) == int((after == 0).sum())
        got, _ = either_way(tunables, res, np.zeros_like(labels), p, mask, SR.ERASE_OUTSIDE, [3], 3)
        assert got["bricks_projected"] == 0 and got["added"] == got["removed"] == 0
        got, _ = either_way(tunables, res, np.full_like(labels, 3), p, mask, SR.FILL_OUTSIDE, [3], 3)
        assert got["bricks_projected"] == 0 and got["added"] == got["removed"] == 0
    assert moved > 0


# ---- boxes -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SR.BOX_CASES)
def test_boxes(gpu, tunables, name):
    dims, p, mask = CASES[name]
    labels = SR.blob_labels(dims, seed=13)
    with make_res(dims, labels) as res:
        for origin, extent in SR.BOXES:
            for op in (SR.ERASE_INSIDE, SR.FILL_OUTSIDE) if origin[0] & 1 else (SR.ERASE_OUTSIDE, SR.FILL_INSIDE):
                _, after = either_way(tunables, res, labels, p, mask, op, [3], 3, origin=origin, extent=extent)
                outside = ~SR.box_mask(labels.shape, origin, extent)
                assert np.array_equal(after[outside], labels[outside])
        fresh(res, labels, p, mask, SR.ERASE_INSIDE, [3], 3, origin=(3, 3, 3), extent=(0, 0, 0))   # an all-zero extent is the whole volume


# ---- masks of labels ---------------------------------------------------------------------------------------------------------------------
def test_sources_of_several_labels_writable_and_measuring(gpu, tunables):
    dims, p, mask = CASES["oblique"]
    labels = SR.blob_labels(dims, seed=19)
    labels[:, :, 30:] = 5            # a finished segment
    with make_res(dims, labels) as res:
        fresh(res, labels, p, mask, SR.ERASE_INSIDE, [3, 7], 7, erase_label=1)           # the union of two labels
        fresh(res, labels, p, mask, SR.FILL_INSIDE, [255, 0, 64], 64)                    # labels at both ends of the mask words
        got, after = either_way(tunables, res, labels, p, mask, SR.FILL_INSIDE, [3], 3, writable=[0])
        assert got["added"] > 0 and np.array_equal(after == 5, labels == 5) and np.array_equal(after == 7, labels == 7)   # walls for joins
        assert got["result_voxels"] > got["source_voxels"] + got["added"]                                                 # ... though the result reaches into them
        got, after = fresh(res, labels, p, mask, SR.FILL_OUTSIDE, [3], 3, writable=[0, 7])
        assert (after == 7).sum() < (labels == 7).sum() and np.array_equal(after == 5, labels == 5)
        got, after = fresh(res, labels, p, mask, SR.ERASE_OUTSIDE, [3], 3, writable=[], erase_label=8)   # leaves are the source's own voxels
        assert got["removed"] == (after == 8).sum() > 0 and got["added"] == 0
        got, after = fresh(res, labels, p, mask, SR.FILL_INSIDE, [3], 200)                # what joins as a label of its own
        assert got["added"] == (after == 200).sum() > 0
        for op in SR.OPS:                                                                 # measuring changes nothing (same() compares the bytes)
            got, still = same(res, after, p, mask, op, [3], -1)
            assert np.array_equal(still, after) and got["relabelled"] == 0 and got["added"] + got["removed"] > 0


# ---- the verdicts and the counters -------------------------------------------------------------------------------------------------------
def test_verdicts(gpu, tunables):
    dims, p, half = VERDICTS["half"]
    labels = SR.blob_labels(dims, seed=3)   # mixed boards nearly everywhere: the verdict from S decides little
    bricks = SR.box_bricks(dims)
    with make_res(dims, labels) as res:
        before = res.scissors_counters()
        assert before == {"scissors_calls": 0, "launches": 0, "bricks_projected": 0, "bricks_written": 0}
        projected = launches = 0
        for name in ("set", "clear"):   # the volume wholly in frame and in depth: the corners decide every brick
            for op in SR.OPS:
                got, _ = fresh(res, labels, p, VERDICTS[name][2], op, [3], 3, erase_label=9)
                assert got["bricks_projected"] == 0, (name, op, got)
                assert got["bricks_inside" if name == "set" else "bricks_outside"] > 0 and got["bricks_outside" if name == "set" else "bricks_inside"] == 0
                launches += got["launches"]
        got, _ = fresh(res, np.where(labels == 3, 3, 7).astype(np.uint8), p, VERDICTS["set"][2], SR.FILL_INSIDE, [3, 7], 3)   # a full source under a fill: S alone
        assert got["bricks_inside"] == got["bricks_outside"] == got["bricks_projected"] == 0
        launches += got["launches"]
        states = SR.brick_states(p, half, dims)
        for op in SR.OPS:
            got, _ = either_way(tunables, res, labels, p, half, op, [3], 3, erase_label=9)
            assert 0 < got["bricks_projected"] < bricks, got
            assert got["bricks_inside"] <= states["inside"] and got["bricks_outside"] <= states["outside"] and got["bricks_inside"] + got["bricks_outside"] > 0
            projected += got["bricks_projected"] + bricks
            launches += got["launches"] + 1
        c = res.scissors_counters()
        assert c["scissors_calls"] == 8 + 1 + 8 and c["launches"] == launches and c["bricks_projected"] == projected and c["bricks_written"] > 0
        # a box: the range is the box's bricks
        tunables("scissors_skip", 0)
        try:
            got, _ = fresh(res, labels, p, half, SR.ERASE_INSIDE, [3], 3, origin=(3, 2, 16), extent=(30, 20, 3))
        finally:
            tunables("scissors_skip", 1)
        assert got["bricks_projected"] == 15 == res.scissors_counters()["bricks_projected"] - projected


# ---- state -------------------------------------------------------------------------------------------------------------------------------
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
    """the lasso is drawn on the frame's own camera: the rows are abi.scissors_projection of it"""
    dims = (48, 40, 44)
    vol = S.make_volume_numpy(dims, np.uint16, 0x5EED0002)
    labels = np.where(vol >= np.percentile(vol, 50), 1, 0).astype(np.uint8)   # label 1: red, half transparent
    rp = abi.RaymarchParams(100.0, 1, True)
    world = S.default_world()
    projection = abi.scissors_projection(dims, world, CAM)
    p = SR.of_struct(projection)
    mask = abi.scissors_polygon([(12.0, 6.0), (40.5, 10.0), (30.0, 24.0), (50.0, 40.0), (16.0, 36.0)], 64, 48)
    assert 0 < SR.in_M(p, mask, dims).sum() < labels.size
    with lit_handle(dims, vol, labels) as res:
        light = res.download_light_volume()
        plain = res.raymarch_lit(CAM, TILE, rp, world)
        m = res.scissor_labels(projection, mask, "erase_inside", [1], -1)   # a measure-only call changes nothing at all
        assert m["removed"] > 0 and m["added"] == 0 and m["relabelled"] == 0
        assert np.array_equal(res.download_label_volume(), labels)
        assert np.array_equal(res.raymarch_lit(CAM, TILE, rp, world), plain)
        counters = res.path_counters()
        got, after = same(res, labels, p, mask, SR.ERASE_INSIDE, [1], 1)
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


# ---- allocation --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grown_first", [False, True], ids=["fresh", "grown"])
def test_a_mask_no_larger_allocates_nothing(gpu, grown_first):
    dims = SR.SHAPES[0]
    labels = SR.blob_labels(dims, seed=23)
    names = ["oblique_checkerboard", "single_pixel", "33x1", "along_x", "shear", "one_brick"]   # 77 x 53 first; none of the others is larger
    with make_res(dims, labels) as res:
        if grown_first:
            res.grow_region([(0, 0, 0)], 0, 255, -1, 6)   # takes the boards' scratch
        after = labels
        _, after = same(res, after, *CASES[names[0]][1:], SR.ERASE_INSIDE, [3], 3)   # the first call takes what it needs
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        allocs = res.path_counters()["operator_alloc_calls"]
        for k in range(18):
            dims_k, p, mask = CASES[names[k % len(names)]]
            if dims_k != dims:
                continue
            _, after = same(res, after, p, mask, SR.OPS[k % 4], [3], 3 if k % 3 else -1)
            torch.cuda.synchronize()
            assert torch.cuda.mem_get_info()[0] == free0, k
        assert res.path_counters()["operator_alloc_calls"] == allocs
        _, after = same(res, after, *CASES["wide"][1:], SR.ERASE_INSIDE, [3], 3)   # a larger mask: the staging grows, once
        assert res.path_counters()["operator_alloc_calls"] == allocs + 1
        _, after = same(res, after, *CASES["deep"][1:], SR.FILL_INSIDE, [3], 3)
        assert res.path_counters()["operator_alloc_calls"] == allocs + 1
        g = res.grow_region([(0, 0, 0)], 0, 255, -1, 6)   # region growing finds its scratch usable after the scissors worked in it
        assert g["voxels"] == 40 * 24 * 19
        m = res.morph_labels("dilate", 1, [3], -1)        # and so does the morphology
        assert m["result_voxels"] == int(MR.dilate(after == 3, 1, 6).sum())


# ---- handles and refusals ----------------------------------------------------------------------------------------------------------------
def test_handles(gpu):
    dims = (24, 17, 10)
    vol = np.zeros(dims[::-1], dtype=np.uint8)
    p = rows(SR.proj((4, 0, 0, 0), (0, 4, 0, 0), (0, 0, 0, 4), 1, 4, 24, 17))
    mask = SR.half_plane(24, 17, 10)
    with abi.Resources(dims, abi.FMT_G8) as res:
        with pytest.raises(abi.TbrmError) as e:
            res.scissor_labels(p, mask, 0, [1], 1)        # no volume yet
        assert e.value.code == abi.ERR_NOT_INITIALIZED
        res.upload_volume(vol)
        for label in (1, -1):                  # no label volume: nothing to take the set from, measuring included
            with pytest.raises(abi.TbrmError) as e:
                res.scissor_labels(p, mask, 0, [1], label)
            assert e.value.code == abi.ERR_NOT_INITIALIZED
        res.attach_empty_labels()
        assert res.scissor_labels(p, mask, "fill_inside", [1], 1)["result_voxels"] == 10 * 17 * 10
        assert res.scissor_labels(p, mask, "erase_inside", [0, 1], 0)["result_voxels"] == 14 * 17 * 10
    with abi.Resources(dims, abi.FMT_G8, False, False, 0, rgb=True) as res:   # a colour handle has no label volume
        res.upload_volume(vol)
        with pytest.raises(abi.TbrmError) as e:
            res.scissor_labels(p, mask, 0, [0], -1)
        assert e.value.code == abi.ERR_NOT_INITIALIZED
    with abi.Resources((32, 32, 64), abi.FMT_G16, owned=abi.Slab(0, 32)) as part:
        with pytest.raises(abi.TbrmError) as e:
            part.scissor_labels(p, mask, 0, [0], -1)
        assert e.value.code == abi.ERR_UNSUPPORTED


def test_refusals(gpu):
    dims = (24, 17, 10)
    labels = SR.blob_labels(dims, seed=29)
    good = SR.proj((4, 0, 0, 0), (0, 4, 0, 0), (0, 0, 0, 4), 1, 4, 40, 17)
    mask = SR.half_plane(40, 17, 10)
    lim = 2 ** 46
    with make_res(dims, labels) as res:
        bad = [(dict(width=0), b"width"), (dict(width=16385), b"width"), (dict(height=0), b"height"), (dict(height=16385), b"height"),
               (dict(u=(lim // 23 + 1, 0, 0, 0)), b"row u"), (dict(u=(0, 0, 0, -lim)), b"row u"), (dict(v=(0, 0, lim // 9 + 1, 0)), b"row v"),
               (dict(w=(0, lim // 16, 0, 4)), b"row w"), (dict(w=(-2 ** 63, 0, 0, 4)), b"row w"), (dict(w_min=0), b"w_min"), (dict(w_min=-5), b"w_min"),
               (dict(w_min=5), b"w_max"), (dict(w_max=0), b"w_max")]
        for change, names in bad:
            with pytest.raises(abi.TbrmError) as e:
                res.scissor_labels(rows({**good, **change}), mask, 0, [3], 3)
            assert e.value.code == abi.ERR_INVALID_ARG, change
            assert names in str(e.value).encode(), (change, str(e.value))
        calls = [(dict(op=4), b"op"), (dict(op=-1), b"op"), (dict(new_label=256), b"new_label"), (dict(new_label=-2), b"new_label"), (dict(erase_label=256), b"erase_label"),
                 (dict(erase_label=-1), b"erase_label"), (dict(origin=(23, 0, 0), extent=(2, 1, 1)), b"box"), (dict(origin=(0, 0, 0), extent=(1, 0, 1)), b"box"),
                 (dict(origin=(-1, 0, 0), extent=(2, 1, 1)), b"box"), (dict(origin=(0, 0, 0), extent=(24, 17, 11)), b"box")]
        for change, names in calls:
            with pytest.raises(abi.TbrmError) as e:
                res.scissor_labels(**{**dict(projection=rows(good), mask=mask, op=0, source=[3], new_label=3), **change})
            assert e.value.code == abi.ERR_INVALID_ARG, change
            assert names in str(e.value).encode(), (change, str(e.value))
        for wrong, names in ((mask[:-1], b"n_words"), (SR.half_plane(65, 17, 10), b"n_words"), (np.where(np.arange(2)[None, :] == 1, 0x100, mask).astype(np.uint32), b"mask_words")):
            with pytest.raises(abi.TbrmError) as e:   # (40 pixels: bit 8 of a row's second word is pixel 40)
                res.scissor_labels(rows(good), wrong, 0, [3], 3)
            assert e.value.code == abi.ERR_INVALID_ARG and names in str(e.value).encode(), str(e.value)
        d = res.scissors_desc(rows(good), 0, [3], 3)
        d.reserved = 1
        out = abi.SCISSORS_RESULT()
        assert res.lib.tbrm_scissors_labels(res.handle, d, mask.ctypes.data_as(abi.C.c_void_p), mask.size, out) == abi.ERR_INVALID_ARG and b"reserved" in res.lib.tbrm_last_error()
        assert np.array_equal(res.download_label_volume(), labels) and res.scissors_counters()["scissors_calls"] == 0
        # the bounds themselves are admitted
        edge = SR.proj(((lim - 1) // 23, 0, 0, 0), (0, 0, 0, lim - 1), (0, 0, 0, lim - 1), lim - 1, 2 ** 63 - 1, 16384, 1)
        same(res, labels, edge, SR.all_set(16384, 1), SR.ERASE_INSIDE, [3], 3)   # every voxel at pixel (0, 1): outside the one row
        assert np.array_equal(res.download_label_volume(), labels)
        edge["v"] = [0, 0, 0, lim - 2]
        got, _ = same(res, labels, edge, SR.all_set(16384, 1), SR.ERASE_INSIDE, [3], 3)
        assert got["removed"] == (labels == 3).sum()
