"""One gate, three callers: k_grow_candidates, k_paint and k_compete_init read a row's stored values and compare them with lo .. hi by
the same two device functions (tbrm_brick_boards.h: row_values, row_gate). Each is asked, in a measuring call, for nothing but the
set the gate lets through, on a volume of 17 x 9 x 8 voxels — ragged bricks along x and y, one layer along z — whose values hold the
range's ends, their neighbours and the format's extremes. The expectation is numpy's (v >= lo) & (v <= hi) on the stored values;
the counts are integers and compared exactly."""
import numpy as np
import pytest

from tbraymarcherplugin_amd import abi
import label_paint_reference as PR

pytestmark = pytest.mark.gpu

DIMS = (17, 9, 8)                          # (x, y, z)
RANGES = {np.uint8: (40, 200), np.uint16: (1000, 60000), np.float32: (-1.5, 2.25)}   # every end is exact in its format
SEED_AT = (5, 3, 2)                        # competitive growing's one seed voxel (x, y, z)
# one ball round the volume's middle that holds every voxel: in eighths of a voxel the farthest centre is (64, 32, 28) away
POINTS, WEIGHTS, LIMIT = [(64, 32, 28)], (1, 1, 1), 64 * 64 + 32 * 32 + 28 * 28


def stored_values(dtype):
    """[z, y, x]: values drawn from the whole format, and at places drawn by the same seed every value the gate could get wrong"""
    lo, hi = RANGES[dtype]
    rng = np.random.default_rng(20)
    n = DIMS[0] * DIMS[1] * DIMS[2]
    if dtype == np.float32:
        f = np.float32
        special = [lo - 1, lo, hi, hi + 1, np.finfo(f).min, np.finfo(f).max, np.finfo(f).tiny, -0.0, np.inf, -np.inf, np.nan,
                   np.nextafter(f(lo), f(-np.inf)), np.nextafter(f(lo), f(np.inf)), np.nextafter(f(hi), f(-np.inf)), np.nextafter(f(hi), f(np.inf))]
        assert f(lo) == lo and f(hi) == hi and f(lo - 1) < f(lo) and f(hi + 1) > f(hi)   # the ends are exact, their neighbours distinct in float32
        v = rng.normal(0.0, 3.0, size=n).astype(f)
    else:
        top = np.iinfo(dtype).max
        special = [lo - 1, lo, hi, hi + 1, 0, top]
        v = rng.integers(0, top + 1, size=n).astype(dtype)
    places = rng.permutation(n)[:4 * len(special)]       # each of them four times, so that they meet ragged rows and whole ones
    v[places] = np.asarray(special * 4, dtype=dtype)
    for s in special:                                    # every one of them is there
        assert (np.isnan(v).any() if s != s else (v == dtype(s)).any()), s
    return v.reshape(DIMS[::-1])


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32], ids=["G8", "G16", "R32F"])
def test_one_gate_three_callers(gpu, dtype):
    lo, hi = RANGES[dtype]
    vol = stored_values(dtype)
    with np.errstate(invalid="ignore"):
        passes = (vol >= dtype(lo)) & (vol <= dtype(hi))  # (a NaN fails both)
    assert 0 < int(passes.sum()) < passes.size
    assert PR.admissible(POINTS, WEIGHTS, LIMIT, DIMS) and PR.within_stroke(POINTS, WEIGHTS, LIMIT, DIMS).all()   # the brush covers the box
    labels = np.zeros(DIMS[::-1], dtype=np.uint8)
    labels[SEED_AT[::-1]] = 1
    is_seed = labels == 1
    with abi.Resources(DIMS, abi.DTYPE_FMT[np.dtype(dtype)], False, False, 0) as res:
        res.upload_volume(vol)
        res.upload_label_volume(labels)
        grown = res.grow_region(None, lo, hi, -1)
        print("grow", grown)
        assert grown["voxels"] == int(passes.sum()) and grown["relabelled"] == 0, grown
        painted = res.paint_labels(POINTS, WEIGHTS, LIMIT, "paint", [], -1, gate=(lo, hi))
        print("paint", painted)
        assert painted["stamp_voxels"] == int(passes.sum()) and painted["relabelled"] == 0, painted
        float_range = abi.compete_float_range(lo, hi) if dtype == np.float32 else None
        competed = res.compete_labels([1], lo, hi, measure_only=True, float_range=float_range)
        print("compete", competed)
        assert competed["seed_voxels"] == 1 and competed["claimable"] == int((passes & ~is_seed).sum()) and competed["relabelled"] == 0, competed
        assert np.array_equal(res.download_label_volume(), labels)   # measuring calls
