"""Restatement of include/tbrm_smooth.h's rank filter in numpy / scipy (TEST INFRASTRUCTURE ONLY): c, the set voxels of a window, and
n, the voxels of the window inside the volume, are scipy.ndimage.convolve of the mask and of ones with a box of ones, padded with 0,
in int64; a pass is c * rank_den > n * rank_num. Nothing here is taken from the kernel: no bricks, no bit boards, no sums per axis.

Label volumes and masks are indexed [z, y, x]; origins, extents, radii and reaches are (x, y, z), as in the C-ABI."""
import math

import numpy as np
from scipy.ndimage import convolve

FIELDS = ("source_voxels", "result_voxels", "added", "removed", "relabelled", "bbox_min", "bbox_max", "reach")
MAX_RADIUS = 16
MEDIAN = (1, 2)

_windows = {}   # (shape, radius) -> n: it depends on nothing else


def box_of_ones(radius):
    rx, ry, rz = radius
    return np.ones((2 * rz + 1, 2 * ry + 1, 2 * rx + 1), dtype=np.int64)


def by_convolve(values, radius):
    """the sum of `values` over the window [v - r, v + r] of every voxel, nothing outside the volume: THE definition"""
    return convolve(values.astype(np.int64), box_of_ones(radius), mode="constant", cval=0)


def by_table(values, radius):
    """the same sums from a summed-volume table (inclusion and exclusion over the window's eight corners). scipy's convolve takes
    about 10 ns per voxel and box element: 50 s for c and n of 40^3 voxels under a 33^3 box, which no test may cost. Exact integers
    either way; tests/test_label_smooth_reference.py holds the two equal wherever the convolution is affordable, radius 16 included."""
    rx, ry, rz = radius
    nz, ny, nx = values.shape
    t = np.zeros((nz + 1, ny + 1, nx + 1), dtype=np.int64)
    t[1:, 1:, 1:] = values.astype(np.int64).cumsum(0).cumsum(1).cumsum(2)
    z0, z1 = np.clip(np.arange(nz) - rz, 0, nz), np.clip(np.arange(nz) + rz + 1, 0, nz)
    y0, y1 = np.clip(np.arange(ny) - ry, 0, ny), np.clip(np.arange(ny) + ry + 1, 0, ny)
    x0, x1 = np.clip(np.arange(nx) - rx, 0, nx), np.clip(np.arange(nx) + rx + 1, 0, nx)
    at = lambda z, y, x: t[np.ix_(z, y, x)]
    return (at(z1, y1, x1) - at(z0, y1, x1) - at(z1, y0, x1) - at(z1, y1, x0) + at(z0, y0, x1) + at(z0, y1, x0) + at(z1, y0, x0) - at(z0, y0, x0))


CONVOLVE_WORK = 5e7   # voxels times box elements up to which the sums are scipy's convolution (about half a second)


def window_sums(values, radius):
    work = values.size * (2 * radius[0] + 1) * (2 * radius[1] + 1) * (2 * radius[2] + 1)
    return by_convolve(values, radius) if work <= CONVOLVE_WORK else by_table(values, radius)


def window_sizes(shape, radius):
    """n [z, y, x]: the voxels of the window [v - r, v + r] that lie inside the volume"""
    key = (tuple(shape), tuple(radius))
    if key not in _windows:
        _windows[key] = window_sums(np.ones(shape, dtype=np.int64), radius)
    return _windows[key]


def counts(mask, radius):
    """c [z, y, x]: the set voxels of the window; outside the volume nothing is set"""
    return window_sums(mask, radius)


def rank_pass(mask, radius, rank=MEDIAN):
    num, den = rank
    return counts(mask, radius) * den > window_sizes(mask.shape, radius) * num


def rank_filter(mask, radius, rank=MEDIAN, iterations=1):
    for _ in range(iterations):
        mask = rank_pass(mask, radius, rank)
    return mask


def ties(mask, radius, rank=MEDIAN):
    """the voxels where c * rank_den == n * rank_num"""
    num, den = rank
    return counts(mask, radius) * den == window_sizes(mask.shape, radius) * num


def table(values):
    ok = np.zeros(256, dtype=bool)
    ok[list(values)] = True
    return ok


def smooth(labels, radius, source, new_label, rank=MEDIAN, iterations=1, origin=None, extent=None, writable=None, erase_label=0):
    """(R over the whole volume, the result's fields, the label volume afterwards)"""
    radius = (radius,) * 3 if np.isscalar(radius) else tuple(radius)
    S = table(source)[labels]
    R = rank_filter(S, radius, rank, iterations)
    box = np.zeros_like(S)
    if extent is None or tuple(extent) == (0, 0, 0):
        box[:] = True
    else:
        o = origin if origin is not None else (0, 0, 0)
        box[o[2]:o[2] + extent[2], o[1]:o[1] + extent[1], o[0]:o[0] + extent[0]] = True
    may = table(writable)[labels] if writable is not None else np.ones_like(S)
    added = R & ~S & box & may
    removed = S & ~R & box
    after = labels.copy()
    relabelled = 0
    if new_label >= 0:
        after[added] = new_label
        after[removed] = erase_label
        relabelled = int((after != labels).sum())
    moved = added | removed
    nz, ny, nx = labels.shape
    if moved.any():
        z, y, x = np.nonzero(moved)
        bbox_min, bbox_max = (int(x.min()), int(y.min()), int(z.min())), (int(x.max()), int(y.max()), int(z.max()))
    else:
        bbox_min, bbox_max = (nx, ny, nz), (-1, -1, -1)
    result = {"source_voxels": int((S & box).sum()), "result_voxels": int((R & box).sum()), "added": int(added.sum()), "removed": int(removed.sum()),
              "relabelled": relabelled, "bbox_min": bbox_min, "bbox_max": bbox_max, "reach": tuple(iterations * r for r in radius)}
    return R, result, after


def smooth_radii(spacing, radius):
    """tbrm_host_smooth_radii's formula: (r_x, r_y, r_z), or None where it refuses"""
    vals = list(spacing) + [radius]
    if not all(math.isfinite(v) and v > 0 for v in vals):
        return None
    r = tuple(math.floor(radius / s + 0.5) for s in spacing)
    if max(r) > MAX_RADIUS or max(r) == 0:
        return None
    return r


# ---- the inputs of tests/test_gpu_label_smooth.py: stated here so that tests/test_label_smooth_reference.py can judge them without a GPU
NOISE_SHAPES = [(8, 8, 8), (17, 9, 24), (9, 40, 7), (33, 33, 33)]
NOISE_DENSITIES = (0.5, 0.3)
NOISE_RADII = [(1, 1, 1), (2, 1, 0), (0, 0, 3), (3, 2, 1)]
NOISE_RANKS = [(1, 2), (1, 3), (2, 3)]
NOISE_ITERATIONS = (1, 3)


def noise(dims, density, seed=11):
    """uint8 [z, y, x]: label 1 on white noise of the given density, 0 elsewhere"""
    rng = np.random.default_rng(seed + int(density * 100) + 1000 * dims[0] + dims[1])
    return (rng.uniform(0.0, 1.0, size=dims[::-1]) < density).astype(np.uint8)


LONG = 72
EDGE_RADII = (7, 8, 9, 16)          # along the long axis: one, two and three bricks
HALF_ENDS = (7, 8, 9)               # a half space [0, end] along the long axis
POINTS = (0, 7, 8, 63, 71)
HALF_RANKS = [(1, 3), (2, 5), (0, 1)]   # (at 1 / 2 a half space is its own median; ten set voxels of a window of 17 survive no rank above 10 / 17)
POINT_RANKS = [(0, 1), (1, 256)]        # the dilation; and one vote wins where the clipped window has fewer than 256 voxels
REACH_LONG = 140                        # radius 16 with 4 iterations: a reach of 64
REACH_POINTS = (0, 7, 8, 69, 139)
BLOB_SHAPES = [(40, 24, 19), (24, 17, 10)]


def blob_labels(dims, seed=7):
    """label 3 on smoothed-noise blobs, label 7 on other blobs beside them, 0 elsewhere"""
    from label_morph_reference import blobs
    labels = np.zeros(dims[::-1], dtype=np.uint8)
    labels[blobs(dims, seed + 1)] = 7
    labels[blobs(dims, seed)] = 3
    return labels


def long_dims(axis, long=LONG):
    dims = [9, 9, 9]
    dims[axis] = long
    return tuple(dims)


def long_radius(axis, r, other=1):
    radius = [other] * 3
    radius[axis] = r
    return tuple(radius)


def half_space(axis, end, long=LONG):
    """label 1 on the voxels 0 .. end of the long axis"""
    labels = np.zeros(long_dims(axis, long)[::-1], dtype=np.uint8)
    index = [slice(None)] * 3
    index[2 - axis] = slice(0, end + 1)
    labels[tuple(index)] = 1
    return labels


def points(axis, long=LONG, at=POINTS):
    """single voxels of label 1 along the long axis, spread over the other two"""
    dims = long_dims(axis, long)
    labels = np.zeros(dims[::-1], dtype=np.uint8)
    for k, a in enumerate(at):
        xyz = [(3 + 2 * k) % dims[0], (1 + 3 * k) % dims[1], (2 + 5 * k) % dims[2]]
        xyz[axis] = a
        labels[xyz[2], xyz[1], xyz[0]] = 1
    return labels


def checkerboard(dims):
    z, y, x = np.indices(dims[::-1])
    return ((x + y + z) & 1).astype(np.uint8)
