"""Volume statistics (include/tbrm_volume_stats.h) on the GPU against tests/volume_stats_reference.py. The results are integers:
every comparison is exact equality, except the float64 sum of float data, whose bound is derived where it is used."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tbraymarcherplugin_amd import abi, synthetic as S
import volume_stats_reference as SR

pytestmark = pytest.mark.gpu

SHAPES = [(40, 24, 19),   # bricks 5 x 3 x 3, z ragged
          (24, 17, 10),   # y and z ragged
          (5, 6, 3),      # a single cut brick
          (16, 16, 16)]   # whole bricks only
DTYPES = pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32], ids=["u8", "u16", "f32"])
BINS = (1, 7, 256, 4096)
BOXES = [((11, 5, 3), (13, 9, 7)),    # unaligned, across brick faces
         ((17, 9, 4), (1, 1, 1)),     # a single voxel
         ((8, 8, 8), (8, 8, 8)),      # exactly one whole brick
         ((3, 2, 16), (30, 20, 3)),   # inside the ragged last layer
         ((21, 0, 0), (1, 24, 19))]   # one voxel wide


def top_of(dtype):
    return 255 if np.dtype(dtype) == np.uint8 else 65535


def random_volume(dims, dtype, seed, far_from_zero=False):
    """far_from_zero: no voxel in the bin that holds 0, for 256 bins or more over the full range"""
    rng = np.random.default_rng(seed)
    shape = dims[::-1]
    if np.dtype(dtype) == np.float32:
        v = rng.uniform(-0.25, 1.25, size=shape).astype(np.float32)   # values below 0 and above 1 included
        return np.where(np.abs(v) < 0.01, np.float32(0.5), v) if far_from_zero else v
    return rng.integers(top_of(dtype) // 4 if far_from_zero else 0, top_of(dtype) + 1, size=shape).astype(dtype)


def ranges_of(dtype):
    """(lo, hi): the full range and a sub-range lo > 0, hi < max"""
    if np.dtype(dtype) == np.float32:
        return [(-0.25, 1.25), (0.1, 0.9)]
    top = top_of(dtype)
    return [(0, top), (top // 3, top - top // 3)]


def make_res(dims, dtype, vol=None, light32=False, rgb=False, labels=None):
    res = abi.Resources(dims, abi.DTYPE_FMT[np.dtype(dtype)], light32, False, 0, rgb=rgb)
    if vol is not None:
        res.upload_volume(vol)
    if labels is not None:
        res.upload_label_volume(labels)
    return res


def same_histogram(res, vol, n_bins, lo, hi, origin=None, extent=None, labels_vol=None, labels=None):
    counts, tally = res.volume_histogram(n_bins, lo, hi, origin, extent, labels)
    want_counts, want_tally = SR.histogram(vol, n_bins, lo, hi, origin, extent, labels_vol, labels)
    where = (n_bins, lo, hi, origin, extent, labels)
    assert tally == want_tally, where
    assert np.array_equal(counts, want_counts), where
    assert tally["visited"] == tally["below"] + tally["above"] + tally["nan"] + int(counts.sum())
    return counts, tally


def whole_and_cut(dims, origin=None, extent=None):
    """bricks of the box inside it on all three axes / the others it touches"""
    o = origin if extent is not None else (0, 0, 0)
    e = extent if extent is not None else dims
    whole, touched = 1, 1
    for c in range(3):
        bricks = range(o[c] // 8, (o[c] + e[c] - 1) // 8 + 1)
        whole *= sum(1 for b in bricks if 8 * b >= o[c] and 8 * b + 8 <= o[c] + e[c])
        touched *= len(bricks)
    return whole, touched - whole


# ---- the whole volume ---------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("dims", SHAPES, ids=lambda d: "x".join(map(str, d)))
def test_whole_volume_histogram(gpu, dims, dtype):
    vol = random_volume(dims, dtype, 100 + dims[0], far_from_zero=True)   # no voxel near zero anywhere: only padding is zero
    with make_res(dims, dtype, vol) as res:
        for n_bins in BINS:
            for k, (lo, hi) in enumerate(ranges_of(dtype)):
                counts, tally = same_histogram(res, vol, n_bins, lo, hi)
                assert tally["visited"] == dims[0] * dims[1] * dims[2]
                if k == 0 and n_bins >= 256:   # padding is not data: nothing lands where a zero would
                    zero_bin, _ = (SR.bins_of_floats if dtype == np.float32 else SR.bins_of_codes)(np.zeros(1, dtype=dtype), n_bins, lo, hi)
                    assert zero_bin[0] >= 0 and counts[zero_bin[0]] == 0
        c = res.volume_stats_counters()
        whole, cut = whole_and_cut(dims)
        calls = len(BINS) * 2
        assert c == {"histograms": calls, "label_statistics": 0, "whole_bricks": calls * whole, "cut_bricks": calls * cut}
        if dims == (16, 16, 16):
            assert c["cut_bricks"] == 0 and c["whole_bricks"] == calls * 8
        if dims == (5, 6, 3):
            assert c["whole_bricks"] == 0 and c["cut_bricks"] == calls


# ---- boxes --------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_boxes(gpu, dtype):
    dims = SHAPES[0]
    vol = random_volume(dims, dtype, 7)
    lo, hi = ranges_of(dtype)[1]
    with make_res(dims, dtype, vol) as res:
        for origin, extent in BOXES:
            before = res.volume_stats_counters()
            for n_bins in (7, 256):
                _, tally = same_histogram(res, vol, n_bins, lo, hi, origin, extent)
                assert tally["visited"] == extent[0] * extent[1] * extent[2]
            after = res.volume_stats_counters()
            whole, cut = whole_and_cut(dims, origin, extent)
            assert (after["whole_bricks"] - before["whole_bricks"], after["cut_bricks"] - before["cut_bricks"]) == (2 * whole, 2 * cut), (origin, extent)
        assert whole_and_cut(dims, *BOXES[2]) == (1, 0) and whole_and_cut(dims, *BOXES[0]) == (0, 2 * 2 * 2)
        # an all-zero extent is the whole volume, whatever the origin
        counts, tally = res.volume_histogram(16, lo, hi, (3, 3, 3), (0, 0, 0))
        want, want_tally = SR.histogram(vol, 16, lo, hi)
        assert np.array_equal(counts, want) and tally == want_tally


def test_argument_checks(gpu):
    dims = (24, 17, 10)
    with make_res(dims, np.uint16) as res:
        with pytest.raises(abi.TbrmError) as e:
            res.volume_histogram(16, 0, 65535)   # no volume yet
        assert e.value.code == abi.ERR_NOT_INITIALIZED
        with pytest.raises(abi.TbrmError) as e:
            res.label_statistics()
        assert e.value.code == abi.ERR_NOT_INITIALIZED
        res.upload_volume(np.zeros(dims[::-1], dtype=np.uint16))
        bad = [dict(n_bins=0, lo=0, hi=65535), dict(n_bins=4097, lo=0, hi=65535), dict(n_bins=-3, lo=0, hi=65535),
               dict(n_bins=16, lo=-1, hi=100), dict(n_bins=16, lo=0, hi=65536), dict(n_bins=16, lo=200, hi=100), dict(n_bins=16, lo=0.5, hi=100),
               dict(n_bins=16, lo=0, hi=math.nan),
               dict(n_bins=16, lo=0, hi=65535, origin=(23, 0, 0), extent=(2, 1, 1)), dict(n_bins=16, lo=0, hi=65535, origin=(0, 0, 0), extent=(1, 0, 1)),
               dict(n_bins=16, lo=0, hi=65535, origin=(0, 0, 0), extent=(1, -1, 1)), dict(n_bins=16, lo=0, hi=65535, origin=(-1, 0, 0), extent=(2, 1, 1)),
               dict(n_bins=16, lo=0, hi=65535, origin=(0, 0, 0), extent=(24, 17, 11))]
        for kw in bad:
            with pytest.raises(abi.TbrmError) as e:
                res.volume_histogram(**kw)
            assert e.value.code == abi.ERR_INVALID_ARG, kw
        for origin, extent in (((0, 16, 0), (1, 2, 1)), ((0, 0, 0), (0, 1, 1)), ((0, 0, 10), (1, 1, 1))):
            with pytest.raises(abi.TbrmError) as e:
                res.label_statistics(origin, extent)
            assert e.value.code == abi.ERR_INVALID_ARG
        with pytest.raises(abi.TbrmError) as e:
            res.volume_histogram(16, 0, 65535, labels=[1])   # a mask without a label volume
        assert e.value.code == abi.ERR_NOT_INITIALIZED
        assert res.volume_stats_counters() == {"histograms": 0, "label_statistics": 0, "whole_bricks": 0, "cut_bricks": 0}
        res.volume_histogram(16, 65535, 65535)   # lo == hi is a range of one code
        res.volume_histogram(1, 0, 0, (23, 16, 9), (1, 1, 1))   # the far corner fits exactly
    with make_res(dims, np.float32, np.zeros(dims[::-1], dtype=np.float32)) as res:
        for lo, hi in ((0.5, 0.5), (1.0, 0.0), (0.0, math.inf), (math.nan, 1.0), (0.0, 1e39), (1.0, 1.0 + 1e-12)):   # the last: equal as float32
            with pytest.raises(abi.TbrmError) as e:
                res.volume_histogram(16, lo, hi)
            assert e.value.code == abi.ERR_INVALID_ARG, (lo, hi)


# ---- float edge cases ---------------------------------------------------------------------------------------------------------------
def test_float_edge_cases(gpu):
    dims = (24, 17, 10)
    lo, hi = np.float32(0.125), np.float32(0.7)
    up, down = lambda v: np.nextafter(np.float32(v), np.float32(np.inf)), lambda v: np.nextafter(np.float32(v), np.float32(-np.inf))
    special = np.array([np.nan, -np.nan, np.inf, -np.inf, lo, down(lo), up(lo), hi, down(hi), up(hi), -3.0, -0.0, 0.0, 1.0, 7.5,
                        np.float32(1e-45), np.float32(3e38), np.float32(-3e38)], dtype=np.float32)
    rng = np.random.default_rng(21)
    vol = rng.uniform(-0.5, 1.5, size=dims[::-1]).astype(np.float32)
    flat = vol.reshape(-1)
    flat[rng.choice(flat.size, size=40 * special.size, replace=False)] = np.tile(special, 40)
    with make_res(dims, np.float32, vol) as res:
        for n_bins in BINS + (1000,):
            _, tally = same_histogram(res, vol, n_bins, float(lo), float(hi))
            assert tally["nan"] == 80
        same_histogram(res, vol, 4096, -3e38, 3e38)     # hi - lo overflows float32: scale is 0
        same_histogram(res, vol, 4096, 0.0, 1e-45)      # n / (hi - lo) overflows float32: scale is inf
        same_histogram(res, vol, 7, float(lo), float(hi), (3, 5, 2), (17, 9, 7))
        s = res.label_statistics()
        want = SR.label_statistics(vol)[0]
        assert (int(s[0]["count"]), int(s[0]["nan_count"])) == (want["count"], want["nan_count"]) == (flat.size, 80)
        assert (s[0]["min"], s[0]["max"]) == (-math.inf, math.inf) == (want["min"], want["max"])
        assert math.isnan(want["sum"]) and math.isnan(float(s[0]["sum"]))   # +inf and -inf among the voxels: NaN in any order


# ---- spikes -------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_spike_volume(gpu, dtype):
    """90 % of the voxels at one value (most of a CT is air), the rest random: what the in-wave aggregation is for"""
    dims = SHAPES[0]
    rng = np.random.default_rng(90)
    vol = random_volume(dims, dtype, 91)
    spike = vol.dtype.type(0.3125) if dtype == np.float32 else vol.dtype.type(top_of(dtype) // 3)
    vol[rng.random(vol.shape) < 0.9] = spike
    with make_res(dims, dtype, vol) as res:
        for n_bins in BINS:
            for lo, hi in ranges_of(dtype):
                counts, _ = same_histogram(res, vol, n_bins, lo, hi)
                assert int(counts.max()) >= int(0.85 * vol.size)
        same_histogram(res, vol, 256, *ranges_of(dtype)[0], *BOXES[0])
    const = np.full(dims[::-1], spike)   # every wave holds one value throughout
    with make_res(dims, dtype, const) as res:
        counts, _ = same_histogram(res, const, 256, *ranges_of(dtype)[0])
        assert int(counts.max()) == const.size


# ---- the label mask -----------------------------------------------------------------------------------------------------------------
def random_labels(dims, seed, values=(0, 1, 2, 7, 200, 255)):
    """blocks of 4 x 4 x 4 voxels: some bricks hold one label, most mix several"""
    rng = np.random.default_rng(seed)
    coarse = rng.choice(np.asarray(values, dtype=np.uint8), size=[(d + 3) // 4 for d in dims[::-1]])
    lab = np.repeat(np.repeat(np.repeat(coarse, 4, axis=0), 4, axis=1), 4, axis=2)[:dims[2], :dims[1], :dims[0]]
    lab = np.ascontiguousarray(lab)
    lab[:8, :8, :8] = 7   # one whole brick of one label
    return lab


@DTYPES
def test_label_mask(gpu, dtype):
    dims = SHAPES[0]
    vol, lab = random_volume(dims, dtype, 31), random_labels(dims, 32)
    lo, hi = ranges_of(dtype)[1]
    with make_res(dims, dtype, vol, labels=lab) as res:
        for labels in ([7], [1, 2, 200], [5], [], list(range(256))):   # one, several, an absent one, none at all, all 256
            for origin, extent in ((None, None), BOXES[0]):
                _, tally = same_histogram(res, vol, 256, lo, hi, origin, extent, lab, labels)
                if labels in ([5], []):
                    assert tally["visited"] == 0
        _, tally = same_histogram(res, vol, 7, lo, hi, None, None, lab, list(range(256)))
        assert tally["visited"] == vol.size
        same_histogram(res, vol, 4096, lo, hi)   # and without the mask, labels attached
        res.release_label_volume()
        with pytest.raises(abi.TbrmError) as e:
            res.volume_histogram(16, lo, hi, labels=[1])
        assert e.value.code == abi.ERR_NOT_INITIALIZED


# ---- the device form ----------------------------------------------------------------------------------------------------------------
def test_device_form_adds_to_the_callers_words(gpu):
    dims, dtype = SHAPES[0], np.uint16
    vol = random_volume(dims, dtype, 41)
    n_bins, (lo, hi) = 100, ranges_of(dtype)[1]
    with make_res(dims, dtype, vol) as res:
        res.reserve(1)
        counts, tally = res.volume_histogram(n_bins, lo, hi)
        host = np.concatenate([counts, [tally[k] for k in res.HISTOGRAM_TALLY]]).astype(np.int64)
        buf = torch.zeros(n_bins + 4, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        res.volume_histogram_device(buf.data_ptr(), n_bins, lo, hi)
        res.flush()
        assert np.array_equal(buf.cpu().numpy().astype(np.int64), host)
        c0 = res.path_counters()
        for _ in range(3):   # the words are added to, not overwritten: the caller zeroes them
            res.volume_histogram_device(buf.data_ptr(), n_bins, lo, hi)
        res.flush()
        c1 = res.path_counters()
        assert np.array_equal(buf.cpu().numpy().astype(np.int64), 4 * host)
        assert (c1["operator_alloc_calls"], c1["operator_host_syncs"]) == (c0["operator_alloc_calls"], c0["operator_host_syncs"])
        # two halves of the volume into one buffer: the histogram of the whole
        buf.zero_()
        torch.cuda.synchronize()
        res.volume_histogram_device(buf.data_ptr(), n_bins, lo, hi, (0, 0, 0), (19, 24, 19))
        res.volume_histogram_device(buf.data_ptr(), n_bins, lo, hi, (19, 0, 0), (21, 24, 19))
        res.flush()
        assert np.array_equal(buf.cpu().numpy().astype(np.int64), host)
    with make_res(dims, dtype, vol) as res:   # a handle nobody reserved: its first statistics call takes the scratch, later ones nothing
        buf = torch.zeros(n_bins + 4, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        res.volume_histogram_device(buf.data_ptr(), n_bins, lo, hi)
        c0 = res.path_counters()
        for _ in range(3):
            res.volume_histogram_device(buf.data_ptr(), n_bins, lo, hi)
        res.label_statistics()
        c1 = res.path_counters()
        assert (c1["operator_alloc_calls"], c1["operator_host_syncs"]) == (c0["operator_alloc_calls"], c0["operator_host_syncs"])
        res.flush()
        assert np.array_equal(buf.cpu().numpy().astype(np.int64), 4 * host)


# ---- label statistics ---------------------------------------------------------------------------------------------------------------
def same_statistics(got, want, dtype):
    for label in range(256):
        g, w = got[label], want[label]
        where = (label, g, w)
        assert (int(g["count"]), int(g["nan_count"])) == (w["count"], w["nan_count"]), where
        assert (float(g["min"]), float(g["max"])) == (w["min"], w["max"]), where
        if np.dtype(dtype) == np.float32:
            # any order of float64 additions of n terms is within (n - 1) u sum|v| of the exact sum to first order, u = 2^-53
            # (Higham, Accuracy and Stability of Numerical Algorithms, eq. 4.4); math.fsum is the exact sum, correctly rounded
            n = w["count"] - w["nan_count"]
            assert abs(float(g["sum"]) - w["sum"]) <= n * 2.0 ** -53 * w["abs_sum"], where
        else:
            assert float(g["sum"]) == w["sum"], where


@DTYPES
@pytest.mark.parametrize("with_labels", [False, True], ids=["no_labels", "labels"])
def test_label_statistics(gpu, dtype, with_labels):
    for dims in (SHAPES[0], SHAPES[2]):
        vol = random_volume(dims, dtype, 51)
        if dtype == np.float32:
            vol.reshape(-1)[::97] = np.nan
            vol = vol * np.float32(1000.0)   # (sums that lose bits in float32)
        lab = random_labels(dims, 52) if with_labels else None
        with make_res(dims, dtype, vol, labels=lab) as res:
            whole = res.label_statistics()
            same_statistics(whole, SR.label_statistics(vol, lab), dtype)
            absent = whole[5]
            assert (int(absent["count"]), float(absent["sum"]), float(absent["min"]), float(absent["max"])) == (0, 0.0, math.inf, -math.inf)
            if not with_labels:
                assert int(whole[0]["count"]) == vol.size and all(int(whole[l]["count"]) == 0 for l in range(1, 256))
            boxes = BOXES if dims == SHAPES[0] else [((1, 2, 0), (3, 4, 2))]
            for origin, extent in boxes:
                same_statistics(res.label_statistics(origin, extent), SR.label_statistics(vol, lab, origin, extent), dtype)
            c = res.volume_stats_counters()
            assert c["label_statistics"] == 1 + len(boxes) and c["histograms"] == 0
            w0, c0 = whole_and_cut(dims)
            assert c["whole_bricks"] == w0 + sum(whole_and_cut(dims, *b)[0] for b in boxes)
            assert c["cut_bricks"] == c0 + sum(whole_and_cut(dims, *b)[1] for b in boxes)


# ---- composition --------------------------------------------------------------------------------------------------------------------
def test_statistics_follow_region_updates(gpu):
    dims, dtype = SHAPES[0], np.uint16
    vol, lab = random_volume(dims, dtype, 61), random_labels(dims, 62)
    rng = np.random.default_rng(63)
    (o, e) = BOXES[0]
    block = rng.integers(0, 65536, size=e[::-1]).astype(dtype)
    lab_block = rng.choice(np.array([0, 3, 9], dtype=np.uint8), size=e[::-1])
    vol2, lab2 = vol.copy(), lab.copy()
    vol2[o[2]:o[2] + e[2], o[1]:o[1] + e[1], o[0]:o[0] + e[0]] = block
    lab2[o[2]:o[2] + e[2], o[1]:o[1] + e[1], o[0]:o[0] + e[0]] = lab_block
    with make_res(dims, dtype, vol, labels=lab) as a, make_res(dims, dtype, vol2, labels=lab2) as fresh:
        a.volume_histogram(256, 0, 65535)   # (statistics before the edit: nothing of them is kept)
        a.label_statistics()
        a.update_volume_region(o, block)
        a.update_label_region(o, lab_block)
        for kw in (dict(), dict(origin=(9, 3, 1), extent=(20, 15, 12)), dict(labels=[3, 9, 7])):
            ca, ta = a.volume_histogram(256, 100, 60000, **kw)
            cf, tf = fresh.volume_histogram(256, 100, 60000, **kw)
            assert np.array_equal(ca, cf) and ta == tf
            want, want_t = SR.histogram(vol2, 256, 100, 60000, kw.get("origin"), kw.get("extent"), lab2, kw.get("labels"))
            assert np.array_equal(ca, want) and ta == want_t
        sa, sf = a.label_statistics(), fresh.label_statistics()
        assert sa.tobytes() == sf.tobytes()
        same_statistics(sa, SR.label_statistics(vol2, lab2), dtype)


def test_statistics_leave_the_handle_alone(gpu):
    dims = (40, 24, 19)
    vol = S.make_volume_numpy(dims, np.uint16, 0x5EED0002)
    cam, tile, world = S.default_camera(64, 48), abi.Tile(0, 0, 64, 48), S.default_world()
    rp = abi.RaymarchParams(64.0, 3, True)
    with make_res(dims, np.uint16, vol, labels=random_labels(dims, 71)) as res:
        res.set_tf_lut(abi.color_curve_to_lut(S.TF_A_KEYS))
        res.set_windowing(abi.WindowingParams(0.5, 0.9, True, False))
        res.reserve(2)
        res.clear_light_volume(0.0)
        res.add_dir_light(S.light(0), True, world)
        res.volume_histogram(16, 0, 65535)   # (the first statistics call)
        before = res.raymarch_lit(cam, tile, rp, world)
        lv, digest, region = res.download_light_volume(), res.skipping_digest(), res.volume_region_counters()
        cache = res.light_cache_stats()
        c0 = res.path_counters()
        buf = torch.zeros(256 + 4, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        for _ in range(4):
            res.volume_histogram_device(buf.data_ptr(), 256, 0, 65535)
            res.volume_histogram_device(buf.data_ptr(), 256, 0, 65535, labels=[7])
        c1 = res.path_counters()
        assert (c1["operator_alloc_calls"], c1["operator_host_syncs"]) == (c0["operator_alloc_calls"], c0["operator_host_syncs"])
        res.volume_histogram(4096, 1000, 50000, (3, 3, 3), (30, 20, 10))
        res.label_statistics()
        assert np.array_equal(res.raymarch_lit(cam, tile, rp, world), before)
        assert np.array_equal(res.download_light_volume(), lv)
        assert (res.skipping_digest(), res.volume_region_counters(), res.light_cache_stats()) == (digest, region, cache)
        assert before[..., 3].max() > 0.1


def test_colour_and_float_light_handles_give_the_same_numbers(gpu):
    dims, dtype = SHAPES[1], np.uint16
    vol = random_volume(dims, dtype, 81)
    results = []
    for kw in (dict(), dict(rgb=True), dict(light32=True)):
        with make_res(dims, dtype, vol, **kw) as res:
            counts, tally = res.volume_histogram(256, 10, 60000)
            box_counts, box_tally = res.volume_histogram(7, 10, 60000, (3, 5, 2), (10, 4, 8))
            results.append((counts.tobytes(), tally, box_counts.tobytes(), box_tally, res.label_statistics().tobytes()))
    assert results[0] == results[1] == results[2]
    want, want_t = SR.histogram(vol, 256, 10, 60000)
    assert results[0][0] == want.tobytes() and results[0][1] == want_t


def test_slab_resident_handle_refuses(gpu):
    with abi.Resources((32, 32, 64), abi.FMT_G16, owned=abi.Slab(0, 32)) as res:
        for call in (lambda: res.volume_histogram(16, 0, 65535), lambda: res.volume_histogram_device(256, 16, 0, 65535),
                     lambda: res.label_statistics(), lambda: res.label_statistics((0, 0, 0), (2, 2, 2))):
            with pytest.raises(abi.TbrmError) as e:
                call()
            assert e.value.code == abi.ERR_UNSUPPORTED
        assert res.volume_stats_counters()["histograms"] == 0


# ---- a wave that takes many bricks --------------------------------------------------------------------------------------------------
# The kernels are persistent: a wave strides over the box's bricks, requests the next brick's row before it counts this one, and
# keeps its tallies — and the label statistics the registers of the last one-label brick's label — from brick to brick. On the
# small shapes above the device-sized grid has more waves than bricks, so every wave takes one brick; here the tunable
# stats_groups caps the grid (g workgroups of 4 waves: wave w takes bricks w, w + 4 g, w + 8 g, ...), and one larger volume runs
# the device-sized grid itself.
MIXED = ((np.indices((8, 8, 8)).sum(axis=0) % 3) * 3).astype(np.uint8)   # labels 0, 3 and 6 within one brick


def labels_by_brick(dims, kind):
    """kind(k) for brick k (x fastest, as the kernels count them): the label of a one-label brick, or None for one that mixes labels"""
    nb = [(d + 7) // 8 for d in dims]
    lab = np.zeros([8 * n for n in nb[::-1]], dtype=np.uint8)
    for k in range(nb[0] * nb[1] * nb[2]):
        ix, iy, iz = k % nb[0], (k // nb[0]) % nb[1], k // (nb[0] * nb[1])
        label = kind(k)
        lab[8 * iz:8 * iz + 8, 8 * iy:8 * iy + 8, 8 * ix:8 * ix + 8] = MIXED if label is None else label
    return np.ascontiguousarray(lab[:dims[2], :dims[1], :dims[0]])


# what a wave meets, step by step, with one workgroup on (40, 24, 19) — 45 bricks, the last 15 cut by the ragged z —: label 3 carried
# over two bricks, a mixed brick (the registers stay), 9: the registers of 3 are flushed in mid-loop and start over, 9 carried, back
# to 3, a mixed brick, 9 (for waves 2 and 3 a cut brick already: voxel by voxel), then cut bricks of label 3 and a mixed one
STEPS = (3, 3, None, 9, 9, 3, None, 9, 3, 3, None, 3)


def stepped_labels(dims, stride=4):
    return labels_by_brick(dims, lambda k: STEPS[(k // stride) % len(STEPS)])


def stats_volume(dims, dtype, seed):
    vol = random_volume(dims, dtype, seed)
    if np.dtype(dtype) == np.float32:
        vol.reshape(-1)[::89] = np.nan
        vol = vol * np.float32(1000.0)
    return vol


@DTYPES
@pytest.mark.parametrize("groups", [1, 3])
def test_histogram_over_many_bricks_per_wave(gpu, tunables, dtype, groups):
    dims = SHAPES[0]
    assert 5 * 3 * 3 >= 3 * 4 * groups   # three bricks a wave at the least
    tunables("stats_groups", groups)
    vol, lab = random_volume(dims, dtype, 111), stepped_labels(dims)
    with make_res(dims, dtype, vol, labels=lab) as res:
        for n_bins in (7, 256, 4096):   # 4096: the grid of two workgroups per unit, one LDS copy
            for lo, hi in ranges_of(dtype):
                _, tally = same_histogram(res, vol, n_bins, lo, hi)
                assert tally["visited"] == vol.size
                same_histogram(res, vol, n_bins, lo, hi, None, None, lab, [3, 6])
                same_histogram(res, vol, n_bins, lo, hi, *BOXES[0], lab, [9, 0])
        same_histogram(res, vol, 256, *ranges_of(dtype)[0], (3, 2, 1), (35, 20, 17))   # whole and cut bricks in one wave's run


@DTYPES
@pytest.mark.parametrize("with_labels", [False, True], ids=["no_labels", "labels"])
def test_label_statistics_over_many_bricks_per_wave(gpu, tunables, dtype, with_labels):
    dims = SHAPES[0]
    vol = stats_volume(dims, dtype, 121)
    for groups in (1, 2, 3):   # 1: a wave meets STEPS in order; 2, 3: other interleavings of the same bricks
        tunables("stats_groups", groups)
        lab = stepped_labels(dims) if with_labels else None
        with make_res(dims, dtype, vol, labels=lab) as res:
            got = res.label_statistics()
            same_statistics(got, SR.label_statistics(vol, lab), dtype)
            if with_labels:
                assert all(int(got[l]["count"]) > 0 for l in (0, 3, 6, 9))
            for origin, extent in (BOXES[0], ((3, 2, 1), (35, 20, 17)), ((8, 0, 0), (32, 24, 16))):   # the last: whole bricks only
                same_statistics(res.label_statistics(origin, extent), SR.label_statistics(vol, lab, origin, extent), dtype)


def test_device_sized_grid_on_more_bricks_than_waves(gpu):
    """21 x 20 x 17 = 7140 bricks, ragged along y, against the grid sized to the device: a wave takes a second brick"""
    dims, dtype = (168, 156, 136), np.uint16
    bricks = 21 * 20 * 17
    assert bricks > 16 * torch.cuda.get_device_properties(0).multi_processor_count   # more bricks than the largest grid has waves
    vol = random_volume(dims, dtype, 131)
    # a wave's second brick lies a whole grid further on: 3 again (carried), 9 (flush and start over) or a mixed brick
    lab = labels_by_brick(dims, lambda k: 3 if k < bricks // 2 else (3, 9, None)[k % 3])
    lo, hi = ranges_of(dtype)[1]
    with make_res(dims, dtype, vol, labels=lab) as res:
        same_histogram(res, vol, 256, lo, hi)
        same_histogram(res, vol, 4096, lo, hi)
        same_histogram(res, vol, 256, lo, hi, None, None, lab, [9, 6])
        same_histogram(res, vol, 4096, 0, 65535, None, None, lab, [3])
        same_statistics(res.label_statistics(), SR.label_statistics(vol, lab), dtype)
        res.release_label_volume()
        same_statistics(res.label_statistics(), SR.label_statistics(vol), dtype)
