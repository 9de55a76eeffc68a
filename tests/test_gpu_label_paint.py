"""The paint brush (include/tbrm_paint.h) on the GPU against tests/label_paint_reference.py. The results are integers and bytes: every
comparison is exact equality — of the downloaded label volume and of every field of the result. Every case runs under paint_skip 1
and 0. The reference is judged without a GPU in tests/test_label_paint_reference.py."""
import numpy as np
import pytest
import torch

from tbraymarcherplugin_amd import abi
import label_morph_reference as MR
import label_paint_reference as PR

pytestmark = pytest.mark.gpu

FMT = {np.uint8: abi.FMT_G8, np.uint16: abi.FMT_G16, np.float32: abi.FMT_R32_FLOAT}
R3 = ((1, 1, 1), 24 * 24)   # a brush of exactly 3 voxels


def make_res(dims, labels=None, vol=None):
    vol = vol if vol is not None else np.zeros(dims[::-1], dtype=np.uint8)   # without a gate the brush never reads the data
    res = abi.Resources(dims, FMT[vol.dtype.type], False, False, 0)
    res.upload_volume(vol)
    if labels is not None:
        res.upload_label_volume(labels)
    return res


def same(res, labels, vol, points, weights, limit, op, source, new_label, **kw):
    """one call on the handle and in the reference: every field of the result and the label volume afterwards; (result, labels after)"""
    got = res.paint_labels(points, weights, limit, op, source, new_label, **kw)
    _, want, after = PR.paint(labels, vol, points, weights, limit, op, source, new_label, **kw)
    where = (labels.shape, op, source, new_label, kw)
    for k in PR.FIELDS:
        assert got[k] == want[k], (k, got, want, where)
    bricks = PR.work_bricks(points, weights, limit, labels.shape[::-1], kw.get("origin"), kw.get("extent"))
    assert got["bricks_whole"] + got["bricks_untouched"] + got["bricks_evaluated"] == bricks and got["launches"] == (3 if bricks else 0), (got, bricks, where)
    down = res.download_label_volume()
    assert np.array_equal(down, after), (where, int((down != after).sum()), np.argwhere(down != after)[:5])
    return got, after


def either_way(tunables, res, labels, vol, points, weights, limit, op, source, new_label, **kw):
    """the call under paint_skip 1 and 0, each on freshly uploaded labels: identical labels and results; under 0 every brick of the
    range is evaluated"""
    out = []
    try:
        for skip in (1, 0):
            tunables("paint_skip", skip)
            res.upload_label_volume(labels)
            out.append(same(res, labels, vol, points, weights, limit, op, source, new_label, **kw))
    finally:
        tunables("paint_skip", 1)
    assert {k: out[0][0][k] for k in PR.FIELDS} == {k: out[1][0][k] for k in PR.FIELDS} and np.array_equal(out[0][1], out[1][1])
    assert out[1][0]["bricks_whole"] == out[1][0]["bricks_untouched"] == 0
    return out[0]


def most_candidates(points, weights, limit, dims):
    """the most segments whose grown box meets one brick of the volume (from the definition's reach, brick by brick)"""
    n = [PR.reach8(limit, w) for w in weights]
    best = 0
    for bz in range((dims[2] + 7) // 8):
        for by in range((dims[1] + 7) // 8):
            for bx in range((dims[0] + 7) // 8):
                lo = [8 * b for b in (bx, by, bz)]
                hi = [min(8 * b + 7, d - 1) for b, d in zip((bx, by, bz), dims)]
                best = max(best, sum(all(-((-(min(a[c], b[c]) - n[c])) // 8) <= hi[c] and (max(a[c], b[c]) + n[c]) // 8 >= lo[c] for c in range(3))
                                     for a, b in PR.segments_of(points)))
    return best


# ---- shapes and strokes, both operators, both ways ------------------------------------------------------------------------------------------
STROKES = {
    "one_brick_ball": ((8, 8, 8), [(28, 30, 33)], *R3),
    "one_brick_segment": ((8, 8, 8), [(4, 4, 4), (60, 50, 20)], (1, 1, 1), 150),
    "ragged_point_outside": ((40, 27, 19), [(-20, 100, 60), (50, 120, 170), (330, 230, 90)], *R3),           # the first and the last lie outside
    "ragged_across_a_face": ((40, 27, 19), [(290, 100, 70), (360, 104, 70)], (1, 1, 1), 40 * 40),
    "tie": (*PR.tie_case(),),
    "diagonal": ((40, 27, 19), [(10, 10, 10), (300, 200, 140)], (1, 1, 1), 17 * 17),
    "zero_length_segment": ((40, 27, 19), [(100, 100, 100), (100, 100, 100), (100, 100, 100)], *R3),
    "anisotropic": ((40, 27, 19), [(60, 60, 40), (250, 150, 100)], None, None),                                  # the brush of 0.7 x 0.7 x 2.5 mm voxels, 2 mm
    "heavy_weights": ((24, 16, 16), [(90, 60, 60), (110, 70, 66)], (65535, 40000, 65535), 2 ** 30 - 1),
}


def brush_of(name):
    dims, points, weights, limit = STROKES[name]
    if weights is None:
        weights, limit = abi.paint_brush((0.7, 0.7, 2.5), 2.0)
    return dims, points, weights, limit


@pytest.mark.parametrize("name", sorted(STROKES))
def test_strokes(gpu, tunables, name):
    dims, points, weights, limit = brush_of(name)
    assert PR.admissible(points, weights, limit, dims)
    labels = PR.blob_labels(dims, seed=7)
    with make_res(dims, labels) as res:
        got, after = either_way(tunables, res, labels, None, points, weights, limit, PR.PAINT, [3], 3)
        assert got["added"] > 0 and got["stamp_voxels"] == int(PR.within_stroke(points, weights, limit, dims).sum()) >= got["added"]
        got, after = either_way(tunables, res, labels, None, points, weights, limit, PR.ERASE, [3, 2], 3, erase_label=9)
        assert got["removed"] == int((after == 9).sum())
        # an empty and a full source set
        got, after = either_way(tunables, res, np.zeros_like(labels), None, points, weights, limit, PR.PAINT, [3], 3)
        assert got["added"] == got["stamp_voxels"] == int((after == 3).sum()) > 0
        got, after = either_way(tunables, res, np.full_like(labels, 3), None, points, weights, limit, PR.ERASE, [3], 3, erase_label=0)
        assert got["removed"] == got["stamp_voxels"] == int((after == 0).sum())
        got, _ = either_way(tunables, res, np.full_like(labels, 3), None, points, weights, limit, PR.PAINT, [3], 3)
        assert got["added"] == got["removed"] == got["relabelled"] == 0 and got["stamp_voxels"] > 0   # the stamp is counted whatever S decides
    if name == "tie":
        with make_res(dims, np.zeros_like(labels)) as res:
            at = res.paint_labels(points, weights, limit, "paint", [1], 1)["added"]
            res.upload_label_volume(np.zeros_like(labels))
            assert at - res.paint_labels(points, weights, limit - 1, "paint", [1], 1)["added"] == 70


def test_whole_bricks(gpu, tunables):
    dims = (48, 48, 48)
    weights, limit = (1, 1, 1), 160 * 160   # 20 voxels
    points = [(150, 190, 190), (230, 200, 180)]
    labels = PR.blob_labels(dims, seed=11)
    with make_res(dims, labels) as res:
        got, after = either_way(tunables, res, labels, None, points, weights, limit, PR.PAINT, [1], 1)
        assert got["bricks_whole"] > 0 and got["bricks_evaluated"] > 0 and got["bricks_untouched"] == 0, got   # (one segment: its box is the work box)
        M = PR.within_stroke(points, weights, limit, dims)
        full = sum(bool(M[z:z + 8, y:y + 8, x:x + 8].all()) for z in range(0, 48, 8) for y in range(0, 48, 8) for x in range(0, 48, 8))
        assert got["bricks_whole"] <= full   # (a brick inside the stamp but inside no single segment is evaluated)
        vol = PR.volume(dims, np.uint8)
    with make_res(dims, labels, vol) as res:   # with a gate a whole brick reads only the gate
        got, _ = either_way(tunables, res, labels, vol, points, weights, limit, PR.PAINT, [1], 1, gate=(100, 180))
        assert got["bricks_whole"] > 0 and 0 < got["stamp_voxels"] < int(M.sum())
        # one ball that holds a brick's corners
        got, _ = either_way(tunables, res, labels, vol, [(188, 188, 188)], weights, limit, PR.ERASE, [1, 2], 1, erase_label=0)
        assert got["bricks_whole"] > 0


def test_a_long_stroke_has_runs_and_crowded_bricks(gpu, tunables):
    dims = (33, 33, 33)
    weights, limit = (1, 1, 1), 20 * 20   # 2.5 voxels
    points = PR.wiggle(dims, 300)
    assert PR.admissible(points, weights, limit, dims) and len(PR.segments_of(points)) == 299 > 4 * 64
    assert most_candidates(points, weights, limit, dims) > 64
    labels = PR.blob_labels(dims, seed=13)
    with make_res(dims, labels) as res:
        got, _ = either_way(tunables, res, labels, None, points, weights, limit, PR.PAINT, [2], 2)
        assert got["segments"] == 299 and got["added"] > 0
        either_way(tunables, res, labels, None, points, weights, limit, PR.ERASE, [0, 1, 2, 3], 1, erase_label=200, origin=(5, 6, 7), extent=(20, 21, 19))
        # a stroke that spreads through the volume: most bricks meet a few runs only
        spread = PR.wiggle(dims, 200, seed=17, step=40)
        assert PR.admissible(spread, weights, limit, dims)
        got, _ = either_way(tunables, res, labels, None, spread, weights, limit, PR.PAINT, [2], 2)
        assert got["bricks_untouched"] > 0


def test_a_run_that_fills_half_a_wave_reads_no_segment_behind_it(gpu, tunables):
    """forty segments crowded round one voxel: a brick's survivors are the lanes 0 .. 39 of one run, lane 31 among them. Behind them
    the staging still holds the segments 40 .. 63 of an earlier, longer stroke, which pass through the same bricks: were one of them
    read, it would show."""
    dims = (33, 33, 33)
    weights, limit = R3
    earlier, crowded = PR.wiggle(dims, 130, seed=2, step=20), PR.wiggle(dims, 41, seed=102, step=2)
    stamp = PR.within_stroke(crowded, weights, limit, dims)
    lo, hi = PR.work_box(crowded, weights, limit, dims)
    bricks = np.zeros_like(stamp)
    bricks[lo[2] // 8 * 8:hi[2] // 8 * 8 + 8, lo[1] // 8 * 8:hi[1] // 8 * 8 + 8, lo[0] // 8 * 8:hi[0] // 8 * 8 + 8] = True
    behind = np.zeros_like(stamp)
    for a, b in PR.segments_of(earlier)[40:64]:
        behind |= PR.within_segment(a, b, weights, limit, dims)
    assert (behind & ~stamp & bricks).sum() > 100 and most_candidates(crowded, weights, limit, dims) == 40
    labels = np.zeros(dims[::-1], dtype=np.uint8)
    with make_res(dims, labels) as res:
        same(res, labels, None, earlier, weights, limit, PR.PAINT, [1], -1)
        got, after = either_way(tunables, res, labels, None, crowded, weights, limit, PR.PAINT, [1], 1)
        assert got["added"] == int(stamp.sum()) and np.array_equal(after == 1, stamp)


# ---- boxes -------------------------------------------------------------------------------------------------------------------------------
BOXES = [((0, 0, 0), (40, 27, 19)), ((8, 8, 8), (16, 8, 8)), ((3, 5, 7), (29, 11, 5)), ((39, 26, 18), (1, 1, 1)), ((13, 13, 9), (1, 5, 1))]


def test_boxes(gpu, tunables):
    dims, points, weights, limit = brush_of("diagonal")
    labels = PR.blob_labels(dims, seed=17)
    with make_res(dims, labels) as res:
        for k, (origin, extent) in enumerate(BOXES):
            got, after = either_way(tunables, res, labels, None, points, weights, limit, PR.ERASE if k & 1 else PR.PAINT, [3], 3, origin=origin, extent=extent)
            outside = ~PR.box_mask(labels.shape, origin, extent)
            assert np.array_equal(after[outside], labels[outside])
        either_way(tunables, res, labels, None, points, weights, limit, PR.PAINT, [3], 3, origin=(3, 3, 3), extent=(0, 0, 0))   # an all-zero extent is the whole volume
        # a box the stroke misses: nothing is launched, nothing changes
        before = res.paint_counters()
        ball = [(30, 30, 30)]
        got, after = either_way(tunables, res, labels, None, ball, *R3, PR.PAINT, [3], 3, origin=(20, 0, 0), extent=(20, 27, 19))
        assert got["launches"] == 0 and got["stamp_voxels"] == got["added"] == 0 and got["bbox_min"] == dims and got["bbox_max"] == (-1, -1, -1) and np.array_equal(after, labels)
        c = res.paint_counters()
        assert c["paint_calls"] == before["paint_calls"] + 2 and c["launches"] == before["launches"] and c["bricks_evaluated"] == before["bricks_evaluated"]
        # a stroke wholly outside the volume
        got, _ = either_way(tunables, res, labels, None, [(-200, -200, -200), (-100, -150, -90)], *R3, PR.PAINT, [3], 3)
        assert got["launches"] == 0


# ---- masks of labels ---------------------------------------------------------------------------------------------------------------------
def test_sources_of_several_labels_writable_and_measuring(gpu, tunables):
    dims, points, weights, limit = brush_of("diagonal")
    labels = PR.blob_labels(dims, seed=19)
    labels[:, :, 20:] = 5            # a finished segment
    with make_res(dims, labels) as res:
        either_way(tunables, res, labels, None, points, weights, limit, PR.ERASE, [3, 5], 7, erase_label=1)        # the union of two labels
        either_way(tunables, res, labels, None, points, weights, limit, PR.PAINT, [255, 0, 64], 64)                 # labels at both ends of the mask words
        got, after = either_way(tunables, res, labels, None, points, weights, limit, PR.PAINT, [3], 3, writable=[0])
        assert got["added"] > 0 and np.array_equal(after == 5, labels == 5) and np.array_equal(after == 2, labels == 2)   # walls for the brush
        assert got["stamp_voxels"] > got["added"]
        got, after = either_way(tunables, res, labels, None, points, weights, limit, PR.ERASE, [3], 3, writable=[], erase_label=8)   # leaves are the source's own voxels
        assert got["removed"] == (after == 8).sum() > 0 and got["added"] == 0
        got, after = either_way(tunables, res, labels, None, points, weights, limit, PR.PAINT, [3], 200)            # what joins as a label of its own
        assert got["added"] == (after == 200).sum() > 0
        for op in (PR.PAINT, PR.ERASE):                                                                             # measuring changes nothing (same() compares the bytes)
            got, still = same(res, after, None, points, weights, limit, op, [3], -1)
            assert np.array_equal(still, after) and got["relabelled"] == 0 and got["added"] + got["removed"] > 0


# ---- the gate ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,gate", [(np.uint8, (80, 200)), (np.uint8, (0, 255)), (np.uint16, (20000, 65535)), (np.uint16, (300, 300)), (np.float32, (-0.25, 0.5)),
                                        (np.float32, (-3.0e38, 3.0e38))], ids=["u8", "u8_all", "u16", "u16_one_code", "f32", "f32_all_but_nan"])
def test_gate(gpu, tunables, dtype, gate):
    dims, points, weights, limit = brush_of("diagonal")
    vol = PR.volume(dims, dtype, seed=23, nans=400 if dtype == np.float32 else 0)
    if dtype == np.uint16:
        vol[5:12, 5:20, 3:30] = 300
    labels = PR.blob_labels(dims, seed=29)
    stamp = PR.within_stroke(points, weights, limit, dims)
    with make_res(dims, labels, vol) as res:
        got, after = either_way(tunables, res, labels, vol, points, weights, limit, PR.PAINT, [3], 3, gate=gate)
        assert 0 < got["stamp_voxels"] <= int(stamp.sum()) and got["stamp_voxels"] == int((stamp & PR.gate_mask(vol, gate)).sum())
        if dtype == np.float32:
            nan = np.isnan(vol)
            assert (stamp & nan).any() and np.array_equal(after[nan], labels[nan])   # a NaN voxel is never painted
        got, after = either_way(tunables, res, labels, vol, points, weights, limit, PR.ERASE, [3, 1], 3, gate=gate, erase_label=0, origin=(2, 3, 1), extent=(35, 20, 17))
        assert got["removed"] > 0
        ungated, _ = either_way(tunables, res, labels, vol, points, weights, limit, PR.PAINT, [3], 3)   # gate = 0: lo and hi are not read
        assert ungated["stamp_voxels"] == int(stamp.sum())


# ---- counters and allocation -------------------------------------------------------------------------------------------------------------
def test_counters(gpu, tunables):
    dims, points, weights, limit = brush_of("diagonal")
    labels = PR.blob_labels(dims, seed=31)
    with make_res(dims, labels) as res:
        assert res.paint_counters() == {"paint_calls": 0, "launches": 0, "bricks_evaluated": 0, "bricks_written": 0}
        a, _ = same(res, labels, None, points, weights, limit, PR.PAINT, [3], 3)
        res.upload_label_volume(labels)
        b, _ = same(res, labels, None, points, weights, limit, PR.PAINT, [3], -1)
        c = res.paint_counters()
        assert c["paint_calls"] == 2 and c["launches"] == 6 and c["bricks_evaluated"] == a["bricks_evaluated"] + b["bricks_evaluated"] and 0 < c["bricks_written"] <= a["bricks_evaluated"]


@pytest.mark.parametrize("grown_first", [False, True], ids=["fresh", "grown"])
def test_a_stroke_no_longer_allocates_nothing(gpu, grown_first):
    dims = (40, 27, 19)
    labels = PR.blob_labels(dims, seed=37)
    long_stroke = PR.wiggle(dims, 150, seed=5)
    with make_res(dims, labels) as res:
        if grown_first:
            res.grow_region([(0, 0, 0)], 0, 255, -1, 6)   # takes the boards' scratch
        after = labels
        _, after = same(res, after, None, long_stroke, *R3, PR.PAINT, [3], 3)   # the first call takes what it needs
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        allocs = res.path_counters()["operator_alloc_calls"]
        for k in range(8):
            pts = long_stroke if k == 3 else PR.wiggle(dims, 1 + 17 * k, seed=40 + k)
            _, after = same(res, after, None, pts, *R3, PR.ERASE if k & 1 else PR.PAINT, [3], 3 if k % 3 else -1)
            torch.cuda.synchronize()
            assert torch.cuda.mem_get_info()[0] == free0, k
        assert res.path_counters()["operator_alloc_calls"] == allocs
        _, after = same(res, after, None, PR.wiggle(dims, 400, seed=3), *R3, PR.PAINT, [3], 3)   # a longer stroke: the staging grows, once
        assert res.path_counters()["operator_alloc_calls"] == allocs + 1
        _, after = same(res, after, None, PR.wiggle(dims, 380, seed=4), *R3, PR.PAINT, [3], 3)
        assert res.path_counters()["operator_alloc_calls"] == allocs + 1
        g = res.grow_region([(0, 0, 0)], 0, 255, -1, 6)   # region growing finds its scratch usable after the brush worked in it
        assert g["voxels"] == 40 * 27 * 19
        m = res.morph_labels("dilate", 1, [3], -1)        # and so does the morphology
        assert m["result_voxels"] == int(MR.dilate(after == 3, 1, 6).sum())


# ---- state -------------------------------------------------------------------------------------------------------------------------------
def test_state_is_that_of_an_uploaded_box(gpu):
    dims, points, weights, limit = brush_of("diagonal")
    vol = PR.volume(dims, np.uint16, seed=41)
    labels = PR.blob_labels(dims, seed=43)
    with make_res(dims, labels, vol) as res:
        stats0 = res.label_statistics()
        res.paint_labels(points, weights, limit, "paint", [2], -1, gate=(10000, 60000))   # a measuring call changes nothing at all
        assert np.array_equal(res.download_label_volume(), labels) and np.array_equal(res.label_statistics(), stats0)
        got, after = same(res, labels, vol, points, weights, limit, PR.PAINT, [2], 2, gate=(10000, 60000))
        stats = res.label_statistics()
        next_ = res.morph_labels("close", 2, [2], 2, connectivity=26)
        after_next = res.download_label_volume()
    with make_res(dims, np.zeros_like(after), vol) as other:   # a fresh handle that gets the same bytes through update_label_region
        other.update_label_region((0, 0, 0), after)
        assert np.array_equal(other.label_statistics(), stats)
        assert other.morph_labels("close", 2, [2], 2, connectivity=26) == next_
        assert np.array_equal(other.download_label_volume(), after_next)
    assert stats[2]["count"] == (after == 2).sum() == (labels == 2).sum() + got["added"]


# ---- handles and refusals ----------------------------------------------------------------------------------------------------------------
def test_handles(gpu):
    dims = (24, 17, 10)
    vol = np.zeros(dims[::-1], dtype=np.uint8)
    ball = [(80, 64, 40)]
    with abi.Resources(dims, abi.FMT_G8) as res:
        with pytest.raises(abi.TbrmError) as e:
            res.paint_labels(ball, *R3, 0, [1], 1)        # no volume yet
        assert e.value.code == abi.ERR_NOT_INITIALIZED
        res.upload_volume(vol)
        for label in (1, -1):                  # no label volume: nothing to take the set from, measuring included
            with pytest.raises(abi.TbrmError) as e:
                res.paint_labels(ball, *R3, 0, [1], label)
            assert e.value.code == abi.ERR_NOT_INITIALIZED
        res.attach_empty_labels()
        assert res.paint_labels(ball, *R3, "paint", [1], 1)["added"] == 123   # the discrete ball of radius 3
        assert res.paint_labels(ball, *R3, "erase", [1], 1)["removed"] == 123
    with abi.Resources(dims, abi.FMT_G8, False, False, 0, rgb=True) as res:   # a colour handle has no label volume
        res.upload_volume(vol)
        with pytest.raises(abi.TbrmError) as e:
            res.paint_labels(ball, *R3, 0, [0], -1)
        assert e.value.code == abi.ERR_NOT_INITIALIZED
    with abi.Resources((32, 32, 64), abi.FMT_G16, owned=abi.Slab(0, 32)) as part:
        with pytest.raises(abi.TbrmError) as e:
            part.paint_labels(ball, *R3, 0, [0], -1)
        assert e.value.code == abi.ERR_UNSUPPORTED
    for long_dims, refused in (((abi.PAINT_MAX_DIM, 1, 1), False), ((abi.PAINT_MAX_DIM + 1, 1, 1), True)):   # a thread of voxels: the bound on a dimension
        with abi.Resources(long_dims, abi.FMT_G8, False, False, 0) as res:
            res.upload_volume(np.zeros(long_dims[::-1], dtype=np.uint8))
            res.attach_empty_labels()
            far = [(8 * (abi.PAINT_MAX_DIM - 1), 0, 0)]
            if refused:
                with pytest.raises(abi.TbrmError) as e:
                    res.paint_labels(far, *R3, 0, [1], 1)
                assert e.value.code == abi.ERR_UNSUPPORTED and "16384" in str(e.value)
            else:
                assert res.paint_labels(far, *R3, "paint", [1], 1)["added"] == 4 and (res.download_label_volume()[0, 0, -4:] == 1).all()


def test_refusals(gpu):
    dims = (24, 17, 10)
    labels = PR.blob_labels(dims, seed=29)
    good = dict(points=[(10, 20, 30), (100, 50, 40)], weights=(1, 1, 1), limit=576, op=0, source=[3], new_label=3)
    top = abi.PAINT_MAX_COORD
    with make_res(dims, labels) as res:
        bad = [(dict(points=np.zeros((0, 3), dtype=np.int32)), b"n_points"), (dict(points=np.zeros((4097, 3), dtype=np.int32)), b"n_points"),
               (dict(op=2), b"op"), (dict(op=-1), b"op"), (dict(weights=(1, 0, 1)), b"weights[1]"), (dict(weights=(1, 1, 65536)), b"weights[2]"),
               (dict(limit=0), b"limit"), (dict(limit=2 ** 30), b"limit"), (dict(limit=513 * 513), b"reach"), (dict(weights=(300, 300, 1), limit=300 * 512 * 512), b"weights[2]"),
               (dict(points=[(0, 0, 0), (0, top + 1, 0)]), b"point 1"), (dict(points=[(-top - 1, 0, 0)]), b"point 0"),
               (dict(points=[(0, 0, 0), (5, 5, 5), (5 + 32768, 5, 5)]), b"segment 1"), (dict(points=[(0, 0, 0), (200, 0, 0)], weights=(65535, 65535, 65535), limit=65535 * 100), b"segment 0"),
               (dict(new_label=256), b"new_label"), (dict(new_label=-2), b"new_label"), (dict(erase_label=256), b"erase_label"), (dict(erase_label=-1), b"erase_label"),
               (dict(origin=(23, 0, 0), extent=(2, 1, 1)), b"box"), (dict(origin=(0, 0, 0), extent=(1, 0, 1)), b"box"), (dict(origin=(-1, 0, 0), extent=(2, 1, 1)), b"box"),
               (dict(origin=(0, 0, 0), extent=(24, 17, 11)), b"box"),
               (dict(gate=(5, 4)), b"range"), (dict(gate=(-1, 4)), b"range"), (dict(gate=(0, 256)), b"range"), (dict(gate=(1.5, 4)), b"range"), (dict(gate=(float("nan"), 4)), b"range")]
        for change, names in bad:
            with pytest.raises(abi.TbrmError) as e:
                res.paint_labels(**{**good, **change})
            assert e.value.code == abi.ERR_INVALID_ARG, change
            assert names in str(e.value).encode(), (change, str(e.value))
        d = res.paint_desc((1, 1, 1), 576, 0, [3], 3)
        d.gate = 2
        pts = np.asarray(good["points"], dtype=np.int32)
        out = abi.PAINT_RESULT()
        assert res.lib.tbrm_paint_labels(res.handle, d, pts.ctypes.data_as(abi.C.c_void_p), 2, out) == abi.ERR_INVALID_ARG and b"gate" in res.lib.tbrm_last_error()
        assert np.array_equal(res.download_label_volume(), labels) and res.paint_counters()["paint_calls"] == 0
        # the bounds themselves are admitted
        same(res, labels, None, [(top, top, -top), (top - 100, top, -top)], (1, 1, 1), 512 * 512 + 1023, PR.PAINT, [3], 3)   # far outside: nothing to do
        got, _ = same(res, labels, None, [(0, 0, 0), (32767, 0, 0)], *R3, PR.PAINT, [3], -1)   # dd = 2^30 - 65535
        assert got["added"] > 0
    with abi.Resources((16, 8, 8), abi.FMT_R32_FLOAT, False, False, 0) as res:   # float handles: finite as float32
        res.upload_volume(np.zeros((8, 8, 16), dtype=np.float32))
        res.attach_empty_labels()
        for gate in ((0.0, float("inf")), (-1e39, 0.0), (1.0, 0.5)):
            with pytest.raises(abi.TbrmError) as e:
                res.paint_labels(**{**good, "gate": gate})
            assert e.value.code == abi.ERR_INVALID_ARG and b"range" in str(e.value).encode()
        assert res.paint_labels(**{**good, "gate": (-0.5, 0.5)})["added"] > 0
