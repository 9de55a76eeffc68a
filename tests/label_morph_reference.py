"""Restatement of include/tbrm_morphology.h's label morphology in numpy (TEST INFRASTRUCTURE ONLY): unit steps by shifted copies of
the whole mask, padded with 0 for a dilation and with 1 for an erosion, no wrap. Nothing here is taken from the kernels: no bricks,
no bit boards, no windows.

Label volumes and masks are indexed [z, y, x]; origins and extents are (x, y, z), as in the C-ABI."""
import itertools

import numpy as np

DILATE, ERODE, OPEN, CLOSE = 0, 1, 2, 3
OPS = (DILATE, ERODE, OPEN, CLOSE)
OFFSETS_6 = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
OFFSETS_26 = [o for o in itertools.product((-1, 0, 1), repeat=3) if o != (0, 0, 0)]
FIELDS = ("source_voxels", "result_voxels", "added", "removed", "relabelled", "bbox_min", "bbox_max")


def shifted(mask, dx, dy, dz, pad):
    """out[z, y, x] = mask[z - dz, y - dy, x - dx] where that lies inside the volume, else `pad`"""
    out = np.full_like(mask, pad)
    nz, ny, nx = mask.shape

    def span(n, d):
        return (slice(max(d, 0), n + min(d, 0)), slice(max(-d, 0), n + min(-d, 0)))

    (zd, zs), (yd, ys), (xd, xs) = span(nz, dz), span(ny, dy), span(nx, dx)
    out[zd, yd, xd] = mask[zs, ys, xs]
    return out


def dilate(mask, radius, connectivity):
    """`radius` unit steps; outside the volume counts as unset"""
    offsets = OFFSETS_6 if connectivity == 6 else OFFSETS_26
    for _ in range(radius):
        grown = mask.copy()
        for dx, dy, dz in offsets:
            grown |= shifted(mask, dx, dy, dz, False)
        mask = grown
    return mask


def erode(mask, radius, connectivity):
    """`radius` unit steps; outside the volume counts as set"""
    offsets = OFFSETS_6 if connectivity == 6 else OFFSETS_26
    for _ in range(radius):
        kept = mask.copy()
        for dx, dy, dz in offsets:
            kept &= shifted(mask, dx, dy, dz, True)
        mask = kept
    return mask


def operate(mask, op, radius, connectivity):
    if op == DILATE:
        return dilate(mask, radius, connectivity)
    if op == ERODE:
        return erode(mask, radius, connectivity)
    if op == OPEN:
        return dilate(erode(mask, radius, connectivity), radius, connectivity)
    if op == CLOSE:
        return erode(dilate(mask, radius, connectivity), radius, connectivity)
    raise ValueError(op)


def table(values):
    ok = np.zeros(256, dtype=bool)
    ok[list(values)] = True
    return ok


def morph(labels, op, radius, source, new_label, connectivity=6, origin=None, extent=None, writable=None, erase_label=0):
    """(R over the whole volume, the result's fields, the label volume afterwards)"""
    S = table(source)[labels]
    R = operate(S, op, radius, connectivity)
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
              "relabelled": relabelled, "bbox_min": bbox_min, "bbox_max": bbox_max}
    return R, result, after


def launches(op, radius, steps=8):
    """launches of the step kernel: ceil(radius / steps), twice that for open and close"""
    return -(-radius // steps) * (2 if op in (OPEN, CLOSE) else 1)


def blobs(dims, seed=7, size=5, level=0.5):
    """smoothed noise: a box filter of `size` over uniform noise, thresholded — blobs with bridges and pinholes, [z, y, x].
    (White noise at 30 % opens to nothing at radius 2 and would test nothing.)"""
    rng = np.random.default_rng(seed)
    noise = rng.uniform(0.0, 1.0, size=dims[::-1])
    pad = size // 2
    padded = np.pad(noise, pad, mode="reflect")
    acc = np.zeros_like(noise)
    for dz, dy, dx in itertools.product(range(size), repeat=3):
        acc += padded[dz:dz + noise.shape[0], dy:dy + noise.shape[1], dx:dx + noise.shape[2]]
    return acc / size ** 3 > level
