"""The numpy restatement of the Euclidean margins (tests/label_margin_reference.py) against scipy's exact Euclidean distance transform,
the lattice-ball sizes, the operators' algebra and the weights' formula — before anything on the GPU is compared with it. No GPU."""
import numpy as np
import pytest
from scipy.ndimage import distance_transform_edt

from tbraymarcherplugin_amd import abi
import label_margin_reference as GR
import label_morph_reference as MR

DIMS = [(40, 24, 19), (24, 17, 10), (5, 6, 3), (40, 40, 40)]
ANISO = (256, 400, 1600)            # spacing 16 : 20 : 40 along x, y, z
ids = lambda d: "x".join(map(str, d))


@pytest.fixture(scope="module")
def blobs():
    return {d: MR.blobs(d) for d in DIMS}


def edt2(mask, sampling=(1.0, 1.0, 1.0)):
    """the squared distance to the nearest unset voxel of `mask`, in integers (sampling as [z, y, x])"""
    return np.rint(distance_transform_edt(mask, sampling=sampling) ** 2).astype(np.int64)


@pytest.mark.parametrize("limit, size", [(1, 7), (2, 19), (3, 27), (4, 33), (9, 123)])
def test_ball_sizes(limit, size):
    mask = np.zeros((19, 24, 40), dtype=bool)
    mask[9, 12, 20] = True
    assert int(GR.expand(mask, (1, 1, 1), limit).sum()) == size == len(GR.offsets((1, 1, 1), limit))
    d = GR.distance(mask, (1, 1, 1), limit)
    assert int((d != GR.FAR).sum()) == size and int(d[9, 12, 20]) == 0 and int(d[d != GR.FAR].max()) <= limit


@pytest.mark.parametrize("dims", DIMS, ids=ids)
def test_isotropic_expand_and_shrink_are_scipys(blobs, dims):
    S = blobs[dims]
    to_set = edt2(~S)
    to_unset = edt2(np.pad(S, 1, constant_values=True))[1:-1, 1:-1, 1:-1]   # outside the volume counts as set
    for r in (1, 2, 3, 5):
        assert np.array_equal(GR.expand(S, (1, 1, 1), r * r), to_set <= r * r), r
        assert np.array_equal(GR.shrink(S, (1, 1, 1), r * r), to_unset > r * r), r
    d = GR.distance(S, (1, 1, 1), 25)
    assert np.array_equal(d != GR.FAR, to_set <= 25) and np.array_equal(d[d != GR.FAR], to_set[to_set <= 25])
    d = GR.distance(S, (1, 1, 1), 9, inside=True)
    assert np.array_equal(d != GR.FAR, to_unset <= 9) and np.array_equal(d[d != GR.FAR], to_unset[to_unset <= 9])


@pytest.mark.parametrize("dims", DIMS, ids=ids)
def test_anisotropic_expand_is_scipys(blobs, dims):
    S = blobs[dims]
    to_set = edt2(~S, sampling=(40, 20, 16))   # [z, y, x]: 1600, 400, 256 squared
    for r in (1, 2, 3, 5):
        assert np.array_equal(GR.expand(S, ANISO, 256 * r * r), to_set <= 256 * r * r), r


GPU_SHAPES = [(40, 24, 19), (24, 17, 10), (5, 6, 3), (16, 16, 16), (24, 24, 24), (40, 40, 40)]   # tests/test_gpu_label_margin.py's


@pytest.mark.parametrize("dims", GPU_SHAPES, ids=ids)
def test_algebra_and_input_choice(dims):
    """open lies inside S, S inside close; and — the GPU tests' shapes and radii on the blobs — every operator's result differs from S
    and from the full and the empty volume, so that a comparison on it compares something (at r = 5 the blobs fill (40, 24, 19) and
    shrink to nothing: the GPU tests stop at 3). (5, 6, 3) is within reach of itself from r = 2 on: there r = 1 is the case that counts."""
    S = MR.blobs(dims)
    for weights, scale in (((1, 1, 1), 1), (ANISO, 256)):
        for r in (1, 2, 3):
            limit = scale * r * r
            results = {op: GR.operate(S, op, weights, limit) for op in GR.OPS}
            assert not (results[GR.OPEN] & ~S).any() and not (S & ~results[GR.CLOSE]).any()
            assert not (results[GR.SHRINK] & ~S).any() and not (S & ~results[GR.EXPAND]).any()
            if dims == (5, 6, 3) and r > 1:
                continue
            for op, R in results.items():
                assert R.any() and not R.all() and not np.array_equal(R, S), (weights, r, GR.OP_NAMES[op])


def test_margin_weights():
    for r in (1.0, 1.5, 2.5, 5.0, 17.3):
        for s in (1.0, 0.7, 3.0):
            assert abi.margin_weights((s, s, s), r * s) == ((256, 256, 256), int(np.floor(256 * np.float64(r * s / s) ** 2))) == GR.margin_weights((s, s, s), r * s)
    w, limit = abi.margin_weights((0.7, 0.7, 2.5), 5.0)
    assert w == (256, 256, int(round((2.5 / 0.7) ** 2 * 256))) == (256, 256, 3265) and limit == int((5.0 / 0.7) ** 2 * 256) == 13061
    assert (w, limit) == GR.margin_weights((0.7, 0.7, 2.5), 5.0)
    assert GR.reaches(w, limit) == (7, 7, 2)
    # the smallest spacing need not be x
    assert abi.margin_weights((2.0, 1.0, 4.0), 3.0) == ((1024, 256, 4096), 2304)
    bad = [((0.0, 1, 1), 1), ((1, -1, 1), 1), ((1, 1, float("nan")), 1), ((1, 1, float("inf")), 1), ((1, 1, 1), 0.0), ((1, 1, 1), -2.0),
           ((1, 1, 1), float("nan")), ((1, 1, 1), float("inf")),
           ((1, 1, 1), 65.0),            # a reach of 65
           ((1, 1, 1), 0.05),            # limit 0
           ((1, 1, 1), 0.7),             # limit 125 < 256: every reach 0
           ((1e-3, 1, 1), 3000.0),       # limit >= 2^31
           ((1, 1e6, 1), 1.0)]           # a weight beyond 32 bits
    for spacing, radius in bad:
        assert GR.margin_weights(spacing, radius) is None, (spacing, radius)
        with pytest.raises(abi.TbrmError) as e:
            abi.margin_weights(spacing, radius)
        assert e.value.code == abi.ERR_INVALID_ARG, (spacing, radius)
    assert abi.margin_weights((1, 1, 1), 64.0) == ((256, 256, 256), 256 * 4096)
