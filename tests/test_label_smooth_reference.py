"""The numpy / scipy restatement of the rank filter (tests/label_smooth_reference.py) against a triple loop, scipy's median filter, its
binary dilation and erosion, the operator's algebra and the radii's formula — before anything on the GPU is compared with it. No GPU."""
import itertools

import numpy as np
import pytest
from scipy.ndimage import binary_dilation, binary_erosion, median_filter

from tbraymarcherplugin_amd import abi
import label_smooth_reference as SR

CUBE = np.ones((3, 3, 3), dtype=bool)
ids = lambda d: "x".join(map(str, d))


def random_mask(dims, density=0.5, seed=5):
    return np.random.default_rng(seed).uniform(0.0, 1.0, size=dims[::-1]) < density


def brute(mask, radius, rank):
    """voxel by voxel: the window clipped to the volume, counted by loops"""
    num, den = rank
    nz, ny, nx = mask.shape
    out = np.zeros_like(mask)
    for z, y, x in itertools.product(range(nz), range(ny), range(nx)):
        c = n = 0
        for k in range(max(z - radius[2], 0), min(z + radius[2], nz - 1) + 1):
            for j in range(max(y - radius[1], 0), min(y + radius[1], ny - 1) + 1):
                for i in range(max(x - radius[0], 0), min(x + radius[0], nx - 1) + 1):
                    n += 1
                    c += int(mask[k, j, i])
        out[z, y, x] = c * den > n * num
    return out


@pytest.mark.parametrize("dims", [(9, 9, 9), (8, 5, 3), (1, 9, 2), (7, 1, 1)], ids=ids)
def test_against_the_triple_loop(dims):
    for density in (0.5, 0.3):
        S = random_mask(dims, density)
        for radius in ((1, 1, 1), (2, 1, 0), (0, 0, 3), (3, 2, 1), (16, 0, 1)):
            for rank in ((1, 2), (1, 3), (2, 3), (0, 1), (27, 28), (255, 256)):
                assert np.array_equal(SR.rank_pass(S, radius, rank), brute(S, radius, rank)), (dims, density, radius, rank)
    S = random_mask(dims)
    twice = brute(brute(S, (1, 1, 1), (1, 2)), (1, 1, 1), (1, 2))
    assert np.array_equal(SR.rank_filter(S, (1, 1, 1), (1, 2), 2), twice)


@pytest.mark.parametrize("radius", [(1, 1, 1), (2, 1, 0), (0, 0, 3), (3, 2, 1), (16, 16, 16), (16, 1, 9), (7, 8, 9)], ids=ids)
def test_the_table_is_the_convolution(radius):
    """label_smooth_reference.by_table against THE definition, scipy's convolution with a box of ones: of a mask and of ones (n)"""
    for dims in ((17, 11, 9), (8, 8, 8), (1, 5, 40)):
        S = random_mask(dims, 0.4, seed=sum(radius))
        assert np.array_equal(SR.by_table(S, radius), SR.by_convolve(S, radius)), (dims, radius)
        ones = np.ones(dims[::-1], dtype=np.int64)
        assert np.array_equal(SR.by_table(ones, radius), SR.by_convolve(ones, radius)), (dims, radius)
    # and which of the two the sums take: the convolution wherever it is affordable
    assert 33 ** 3 * 9 ** 3 <= SR.CONVOLVE_WORK < 33 ** 3 * 40 ** 3


def test_median_is_scipys_in_the_interior():
    S = random_mask((24, 17, 9))
    for radius in ((1, 1, 1), (2, 1, 0), (0, 0, 3), (3, 2, 1)):
        size = (2 * radius[2] + 1, 2 * radius[1] + 1, 2 * radius[0] + 1)   # odd: no ties where the window is whole
        want = median_filter(S.astype(np.uint8), size=size, mode="constant", cval=0).astype(bool)
        got = SR.rank_pass(S, radius, (1, 2))
        inner = (slice(radius[2], 9 - radius[2]), slice(radius[1], 17 - radius[1]), slice(radius[0], 24 - radius[0]))
        assert got[inner].size > 0 and np.array_equal(got[inner], want[inner]), radius
        assert not SR.ties(S, radius)[inner].any()


def test_rank_zero_is_the_box_dilation_and_27_of_28_the_erosion():
    S = random_mask((24, 17, 9), 0.02)
    for r in (1, 2, 3):
        want = binary_dilation(S, structure=CUBE, iterations=r)
        assert np.array_equal(SR.rank_pass(S, (r, r, r), (0, 1)), want), r
        assert np.array_equal(SR.rank_filter(S, (1, 1, 1), (0, 1), r), want), r
        assert np.array_equal(SR.rank_pass(S, (r, r, r), (0, 256)), want), r
    T = random_mask((24, 17, 9), 0.9)
    want = binary_erosion(T, structure=CUBE, border_value=1)
    assert want.any() and np.array_equal(SR.rank_pass(T, (1, 1, 1), (27, 28)), want)
    assert np.array_equal(SR.rank_filter(T, (1, 1, 1), (27, 28), 2), binary_erosion(T, structure=CUBE, iterations=2, border_value=1))
    assert np.array_equal(SR.rank_pass(T, (1, 1, 1), (255, 256)), want)


def test_full_stays_full_empty_stays_empty():
    for dims in ((12, 9, 5), (8, 8, 8), (1, 1, 3)):
        full, empty = np.ones(dims[::-1], dtype=bool), np.zeros(dims[::-1], dtype=bool)
        for radius in ((1, 1, 1), (16, 16, 16), (0, 0, 3)):
            for rank in ((1, 2), (0, 1), (255, 256), (27, 28)):
                assert SR.rank_filter(full, radius, rank, 3).all() and not SR.rank_filter(empty, radius, rank, 3).any()


def test_the_median_commutes_with_the_complement_off_ties():
    S = random_mask((24, 17, 9))
    for radius in ((1, 1, 1), (2, 1, 0), (3, 2, 1)):
        tie = SR.ties(S, radius)
        a, b = SR.rank_pass(S, radius), SR.rank_pass(~S, radius)
        assert np.array_equal(b[~tie], ~a[~tie])
        assert not a[tie].any() and not b[tie].any()          # a tie leaves the voxel unset, whichever side asks
        faces = np.ones(S.shape, dtype=bool)
        faces[1:-1, 1:-1, 1:-1] = False
        assert tie.sum() > 0 and tie[faces].sum() > 0, radius   # clipped windows are even: the faces have ties
    board = SR.checkerboard((9, 9, 9)) == 1
    assert SR.ties(board, (1, 1, 1)).sum() > 0


def test_smooth_radii():
    assert abi.smooth_radii((1, 1, 1), 2.0) == (2, 2, 2) == SR.smooth_radii((1, 1, 1), 2.0)
    assert abi.smooth_radii((0.7, 0.7, 2.5), 2.0) == (3, 3, 1) == SR.smooth_radii((0.7, 0.7, 2.5), 2.0)
    assert abi.smooth_radii((1, 1, 2.5), 3.0) == (3, 3, 1)
    assert abi.smooth_radii((1, 2, 4), 1.0) == (1, 1, 0)        # 0.5 rounds up, 0.25 down
    assert abi.smooth_radii((1, 1, 1), 16.4) == (16, 16, 16)
    for spacing, radius in itertools.product(((1, 1, 1), (0.7, 0.7, 2.5), (2.0, 1.0, 4.0), (0.3, 5.0, 1.0)), (0.2, 0.5, 1.0, 2.0, 3.3, 4.8, 7.0, 16.0)):
        want = SR.smooth_radii(spacing, radius)
        if want is None:
            with pytest.raises(abi.TbrmError) as e:
                abi.smooth_radii(spacing, radius)
            assert e.value.code == abi.ERR_INVALID_ARG
        else:
            assert abi.smooth_radii(spacing, radius) == want
    bad = [((0.0, 1, 1), 1), ((1, -1, 1), 1), ((1, 1, float("nan")), 1), ((1, 1, float("inf")), 1), ((1, 1, 1), 0.0), ((1, 1, 1), -2.0),
           ((1, 1, 1), float("nan")), ((1, 1, 1), float("inf")),
           ((1, 1, 1), 16.5),            # a radius of 17
           ((1, 1, 0.1), 2.0),           # ... along one axis
           ((1, 1, 1), 0.4)]             # every radius 0
    for spacing, radius in bad:
        assert SR.smooth_radii(spacing, radius) is None, (spacing, radius)
        with pytest.raises(abi.TbrmError) as e:
            abi.smooth_radii(spacing, radius)
        assert e.value.code == abi.ERR_INVALID_ARG, (spacing, radius)


# ---- the inputs of tests/test_gpu_label_smooth.py ----------------------------------------------------------------------------------
def moved(S, R):
    return bool(R.any()) and not bool(R.all()) and not np.array_equal(R, S)


def test_gpu_noise_inputs_compare_something():
    """White noise under the full cross of radii, ranks and iterations: where the rank is the noise's own density (1/2 at 0.5, 1/3 at
    0.3) every case gives a result that differs from S, from the full and from the empty volume. A rank away from the density drives
    noise to one of the two — 45 of the 192 cases end full or empty by this reference itself, most of them after three passes — and
    stays in the GPU test all the same: there the counts are compared near 0 and near n. At least three in four cases move."""
    total = moving = 0
    for dims, density in itertools.product(SR.NOISE_SHAPES, SR.NOISE_DENSITIES):
        S = SR.noise(dims, density) == 1
        assert abs(S.mean() - density) < 0.06
        own = (1, 2) if density == 0.5 else (1, 3)
        for radius, rank, iterations in itertools.product(SR.NOISE_RADII, SR.NOISE_RANKS, SR.NOISE_ITERATIONS):
            R = SR.rank_filter(S, radius, rank, iterations)
            total += 1
            moving += moved(S, R)
            if rank == own:
                assert moved(S, R), (dims, density, radius, rank, iterations)
    assert total == 192 and 4 * moving >= 3 * total, (moving, total)


@pytest.mark.parametrize("axis", [0, 1, 2], ids=["x", "y", "z"])
def test_gpu_edge_inputs_compare_something(axis):
    for r in SR.EDGE_RADII:
        radius = SR.long_radius(axis, r)
        for end in SR.HALF_ENDS:
            S = SR.half_space(axis, end) == 1
            for rank in SR.HALF_RANKS:
                assert moved(S, SR.rank_pass(S, radius, rank)), (axis, r, end, rank)
        S = SR.points(axis) == 1
        for rank in SR.POINT_RANKS:
            assert moved(S, SR.rank_pass(S, radius, rank)), (axis, r, rank)
    S = SR.points(axis, 140, SR.REACH_POINTS) == 1
    assert moved(S, SR.rank_filter(S, SR.long_radius(axis, 16, 0), (0, 1), 4))
    H = SR.half_space(axis, 69, 140) == 1
    assert moved(H, SR.rank_filter(H, SR.long_radius(axis, 16, 0), (1, 3), 4))


def test_gpu_other_inputs_compare_something():
    S = SR.noise((40, 40, 40), 0.5) == 1
    for rank in ((1, 2), (127, 256)):
        assert moved(S, SR.rank_pass(S, (16, 16, 16), rank)), rank
    board = SR.checkerboard((17, 9, 24)) == 1
    R = SR.rank_pass(board, (1, 1, 1))
    assert moved(board, R) and not R[SR.ties(board, (1, 1, 1))].any()
    for dims in SR.BLOB_SHAPES:
        S = SR.blob_labels(dims) == 3
        for radius, iterations in ((1, 1), (2, 1), (1, 3), ((3, 2, 1), 2)):
            assert moved(S, SR.rank_filter(S, (radius,) * 3 if np.isscalar(radius) else radius, (1, 2), iterations)), (dims, radius, iterations)
