"""Restatement of include/tbrm_margin.h's Euclidean margins in numpy (TEST INFRASTRUCTURE ONLY): the offsets (dx, dy, dz) with
w_x dx^2 + w_y dy^2 + w_z dz^2 <= limit are enumerated and the whole mask is shifted by each, padded with 0, no wrap. Nothing here is
taken from the kernels: no bricks, no bit boards, no separable passes.

Label volumes and masks are indexed [z, y, x]; origins, extents, weights and reaches are (x, y, z), as in the C-ABI."""
import math

import numpy as np

from label_morph_reference import table

EXPAND, SHRINK, OPEN, CLOSE = 0, 1, 2, 3
OPS = (EXPAND, SHRINK, OPEN, CLOSE)
OP_NAMES = {EXPAND: "expand", SHRINK: "shrink", OPEN: "open", CLOSE: "close"}
FAR = 0xFFFFFFFF
MAX_REACH = 64
FIELDS = ("source_voxels", "result_voxels", "added", "removed", "relabelled", "bbox_min", "bbox_max", "reach")


def shifted(mask, dx, dy, dz):
    """out[z, y, x] = mask[z - dz, y - dy, x - dx] where that lies inside the volume, else unset (an offset may exceed the volume)"""
    out = np.zeros_like(mask)
    nz, ny, nx = mask.shape
    if abs(dz) >= nz or abs(dy) >= ny or abs(dx) >= nx:
        return out

    def span(n, d):
        return (slice(max(d, 0), n + min(d, 0)), slice(max(-d, 0), n + min(-d, 0)))

    (zd, zs), (yd, ys), (xd, xs) = span(nz, dz), span(ny, dy), span(nx, dx)
    out[zd, yd, xd] = mask[zs, ys, xs]
    return out


def reaches(weights, limit):
    """per axis the largest n with w n^2 <= limit"""
    return tuple(math.isqrt(limit // w) for w in weights)


def offsets(weights, limit):
    """[(dx, dy, dz, cost)] of every offset within the limit"""
    nx, ny, nz = reaches(weights, limit)
    out = []
    for dz in range(-nz, nz + 1):
        for dy in range(-ny, ny + 1):
            for dx in range(-nx, nx + 1):
                cost = weights[0] * dx * dx + weights[1] * dy * dy + weights[2] * dz * dz
                if cost <= limit:
                    out.append((dx, dy, dz, cost))
    return out


def expand(mask, weights, limit):
    """the voxels of the volume within the limit of a set voxel; outside the volume counts as unset"""
    grown = np.zeros_like(mask)
    if not mask.any():
        return grown
    for dx, dy, dz, _ in offsets(weights, limit):
        grown |= shifted(mask, dx, dy, dz)
    return grown


def shrink(mask, weights, limit):
    """the set voxels further than the limit from every unset voxel of the volume: through the complement taken inside the volume"""
    return ~expand(~mask, weights, limit)


def operate(mask, op, weights, limit):
    if op == EXPAND:
        return expand(mask, weights, limit)
    if op == SHRINK:
        return shrink(mask, weights, limit)
    if op == OPEN:
        return expand(shrink(mask, weights, limit), weights, limit)
    if op == CLOSE:
        return shrink(expand(mask, weights, limit), weights, limit)
    raise ValueError(op)


def distance(mask, weights, limit, inside=False):
    """uint32 [z, y, x]: the weighted squared distance to the nearest set voxel (inside: unset voxel) where it is <= limit, else FAR"""
    src = ~mask if inside else mask
    best = np.full(mask.shape, FAR, dtype=np.uint64)
    if src.any():
        for dx, dy, dz, cost in offsets(weights, limit):
            hit = shifted(src, dx, dy, dz)
            best[hit] = np.minimum(best[hit], cost)
    return best.astype(np.uint32)


def margin(labels, op, weights, limit, source, new_label, origin=None, extent=None, writable=None, erase_label=0):
    """(R over the whole volume, the result's fields, the label volume afterwards)"""
    S = table(source)[labels]
    R = operate(S, op, weights, limit)
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
              "relabelled": relabelled, "bbox_min": bbox_min, "bbox_max": bbox_max, "reach": reaches(weights, limit)}
    return R, result, after


def launches(op):
    """launches of the distance kernels: three per transform, two transforms for open and close"""
    return 3 * (2 if op in (OPEN, CLOSE) else 1)


def margin_weights(spacing, radius):
    """tbrm_host_margin_weights' formula: ((w_x, w_y, w_z), limit), or None where it refuses"""
    vals = list(spacing) + [radius]
    if not all(math.isfinite(v) and v > 0 for v in vals):
        return None
    s = min(spacing)
    w = tuple(int(math.floor((a / s) ** 2 * 256.0 + 0.5)) for a in spacing)
    limit = math.floor((radius / s) ** 2 * 256.0)
    if limit < 1 or limit >= 2 ** 31 or max(w) >= 2 ** 32 - 1:
        return None
    n = reaches(w, limit)
    if max(n) > MAX_REACH or max(n) == 0:
        return None
    return w, limit
