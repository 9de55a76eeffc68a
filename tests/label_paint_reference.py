"""Restatement of include/tbrm_paint.h in numpy int64 / Python integers and fractions (TEST INFRASTRUCTURE ONLY): the distance rule
voxel by voxel, the gate, the operators, the counts, the work box; and the same set by a brute force in fractions.Fraction (the
clamped parameter t and the exact squared distance), which never looks at the rule's three cases. Nothing here is taken from the
kernel: no bricks (but work_bricks, which counts the bricks of the definition's own work box), no runs, no culling.

Label and data volumes are indexed [z, y, x]; origins, extents and voxels are (x, y, z), as in the C-ABI. Points are integers in
eighths of a voxel: the centre of voxel i is at 8 i."""
import math
from fractions import Fraction

import numpy as np

FIELDS = ("stamp_voxels", "added", "removed", "relabelled", "bbox_min", "bbox_max", "segments")
PAINT, ERASE = 0, 1
MAX_POINTS = 4096
MAX_COORD = 1 << 18
MAX_DIM = 16384
MAX_WEIGHT = 65535
MAX_LIMIT = (1 << 30) - 1
MAX_REACH = 64
BRICK = 8


def segments_of(points):
    """[(a, b)] of a stroke: one point is one ball"""
    pts = [tuple(int(c) for c in p) for p in np.asarray(points).reshape(-1, 3)]
    if len(pts) == 1:
        return [(pts[0], pts[0])]
    return list(zip(pts[:-1], pts[1:]))


def reach8(limit, w):
    """the largest n with w n^2 <= limit"""
    return math.isqrt(limit // w)


def admissible(points, weights, limit, dims):
    pts = np.asarray(points).reshape(-1, 3)
    if not (1 <= len(pts) <= MAX_POINTS) or max(dims) > MAX_DIM or np.abs(pts).max() > MAX_COORD:
        return False
    if not all(1 <= w <= MAX_WEIGHT for w in weights) or not (1 <= limit <= MAX_LIMIT):
        return False
    if any((reach8(limit, w) + 7) // 8 > MAX_REACH for w in weights):
        return False
    return all(sum(w * (q - p) ** 2 for w, p, q in zip(weights, a, b)) < 2 ** 30 for a, b in segments_of(pts))


def within_segment(a, b, weights, limit, dims, track=None):
    """bool [z, y, x]: the header's rule in int64, no quotient; track: a list that receives the largest magnitude formed"""
    z, y, x = np.indices(dims[::-1], dtype=np.int64)
    w = [int(v) for v in weights]
    d = [int(b[c]) - int(a[c]) for c in range(3)]
    e = [8 * x - int(a[0]), 8 * y - int(a[1]), 8 * z - int(a[2])]
    dd = sum(w[c] * d[c] * d[c] for c in range(3))
    de = sum(w[c] * d[c] * e[c] for c in range(3))
    ee = sum(w[c] * e[c] * e[c] for c in range(3))
    near = ee <= 2 * (dd + limit)  # every voxel within the segment; behind it the products fit
    ee_n, de_n = np.where(near, ee, 0), np.where(near, de, 0)
    bb = ee_n - 2 * de_n + dd
    lhs, rhs = ee_n * dd - de_n * de_n, limit * dd
    if track is not None:
        track.append(max(int(np.abs(ee).max()), int(np.abs(de).max()), int(np.abs(ee_n * dd).max()), int(np.abs(de_n * de_n).max()), int(rhs), int(np.abs(lhs).max())))
    return near & np.where(de_n <= 0, ee_n <= limit, np.where(de_n >= dd, bb <= limit, lhs <= rhs))


def within_stroke(points, weights, limit, dims):
    m = np.zeros(dims[::-1], dtype=bool)
    for a, b in segments_of(points):
        m |= within_segment(a, b, weights, limit, dims)
    return m


def within_segment_slowly(a, b, weights, limit, dims):
    """the same set from the definition: the point of the segment nearest to v in the metric is a + t d with t = <d, e> / <d, d>
    clamped to [0, 1]; the voxel is within when its exact squared distance to that point is at most limit"""
    out = np.zeros(dims[::-1], dtype=bool)
    w = [int(v) for v in weights]
    d = [int(b[c]) - int(a[c]) for c in range(3)]
    dd = sum(w[c] * d[c] * d[c] for c in range(3))
    for z in range(dims[2]):
        for y in range(dims[1]):
            for x in range(dims[0]):
                e = [8 * x - int(a[0]), 8 * y - int(a[1]), 8 * z - int(a[2])]
                t = Fraction(0) if dd == 0 else min(max(Fraction(sum(w[c] * d[c] * e[c] for c in range(3)), dd), Fraction(0)), Fraction(1))
                out[z, y, x] = sum(w[c] * (e[c] - t * d[c]) ** 2 for c in range(3)) <= limit
    return out


def gate_mask(vol, gate):
    """bool [z, y, x]: lo <= v <= hi in stored units; a NaN passes nothing; float volumes compare in float32"""
    if gate is None:
        return np.ones(vol.shape, dtype=bool) if vol is not None else None
    lo, hi = gate
    if vol.dtype == np.float32:
        with np.errstate(invalid="ignore"):
            return (vol >= np.float32(lo)) & (vol <= np.float32(hi))
    return (vol.astype(np.int64) >= int(lo)) & (vol.astype(np.int64) <= int(hi))


def table(values):
    ok = np.zeros(256, dtype=bool)
    ok[list(values)] = True
    return ok


def box_mask(shape, origin, extent):
    box = np.zeros(shape, dtype=bool)
    if extent is None or tuple(extent) == (0, 0, 0):
        box[:] = True
    else:
        o = origin if origin is not None else (0, 0, 0)
        box[o[2]:o[2] + extent[2], o[1]:o[1] + extent[1], o[0]:o[0] + extent[0]] = True
    return box


def paint(labels, vol, points, weights, limit, op, source, new_label, gate=None, origin=None, extent=None, writable=None, erase_label=0):
    """(M over the whole volume, the result's fields, the label volume afterwards)"""
    dims = labels.shape[::-1]
    S = table(source)[labels]
    M = within_stroke(points, weights, limit, dims)
    if gate is not None:
        M &= gate_mask(vol, gate)
    R = (S | M) if op == PAINT else (S & ~M)
    box = box_mask(S.shape, origin, extent)
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
    result = {"stamp_voxels": int((M & box).sum()), "added": int(added.sum()), "removed": int(removed.sum()), "relabelled": relabelled,
              "bbox_min": bbox_min, "bbox_max": bbox_max, "segments": len(segments_of(points))}
    return M, result, after


def work_box(points, weights, limit, dims, origin=None, extent=None):
    """((x0, y0, z0), (x1, y1, z1)) inclusive: the box cut to the stroke's bounding box grown by the reach; None when they miss"""
    pts = np.asarray(points, dtype=np.int64).reshape(-1, 3)
    if extent is None or tuple(extent) == (0, 0, 0):
        origin, extent = (0, 0, 0), dims
    lo, hi = [], []
    for c in range(3):
        n = reach8(limit, weights[c])
        lo.append(max(origin[c], -((-(int(pts[:, c].min()) - n)) // 8)))  # ceil
        hi.append(min(origin[c] + extent[c] - 1, (int(pts[:, c].max()) + n) // 8))  # floor
        if lo[c] > hi[c]:
            return None
    return tuple(lo), tuple(hi)


def work_bricks(points, weights, limit, dims, origin=None, extent=None):
    wb = work_box(points, weights, limit, dims, origin, extent)
    if wb is None:
        return 0
    n = 1
    for c in range(3):
        n *= wb[1][c] // BRICK - wb[0][c] // BRICK + 1
    return n


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
def blob_labels(dims, seed=7):
    """a few labels in blocks, 0 among them"""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, 4, size=tuple((n + 3) // 4 for n in dims[::-1]), dtype=np.uint8)
    return np.ascontiguousarray(np.kron(coarse, np.ones((4, 4, 4), dtype=np.uint8))[:dims[2], :dims[1], :dims[0]])


def volume(dims, dtype, seed=3, nans=0):
    rng = np.random.default_rng(seed)
    if dtype == np.float32:
        v = rng.uniform(-1.0, 1.0, size=dims[::-1]).astype(np.float32)
        if nans:
            flat = v.reshape(-1)
            flat[rng.choice(flat.size, size=nans, replace=False)] = np.nan
        return v
    return rng.integers(0, np.iinfo(dtype).max + 1, size=dims[::-1]).astype(dtype)


def tie_case():
    """an axis segment whose radius is exactly 3 voxels: (dims, points, weights, limit); voxels at distance exactly 3 are in at
    limit and out at limit - 1"""
    return (24, 16, 16), [(8 * 6, 8 * 8, 8 * 8), (8 * 16, 8 * 8, 8 * 8)], (1, 1, 1), 24 * 24


def extreme_case():
    """the longest admissible diagonal segment under the largest limit (the reach bound then asks for the largest weights), placed so
    that every voxel of the volume passes the early rejection with ee close to its bound 2 (dd + limit) < 2^32 — the products are then
    as large as they get: (dims, points, weights, limit)"""
    w = MAX_WEIGHT
    d = math.isqrt((2 ** 30 - 1) // (3 * w))  # 73: the longest diagonal step with dd < 2^30
    a = (-120, -120, -120)                    # voxel (3, 3, 3) has ee = 3 w 144^2 = 4.08e9, the bound is 4.24e9
    return (4, 4, 4), [a, (a[0] + d, a[1] + d, a[2] + d)], (w, w, w), MAX_LIMIT


def wiggle(dims, n, seed=11, step=12):
    """a stroke of n points that wanders through the volume in steps of at most `step` eighths per axis, leaving it now and then"""
    rng = np.random.default_rng(seed)
    p = np.array([4 * (v - 1) for v in dims], dtype=np.int64)
    out = []
    for _ in range(n):
        out.append(tuple(int(c) for c in p))
        p = p + rng.integers(-step, step + 1, size=3)
        p = np.clip(p, -16, np.array([8 * v + 8 for v in dims]))
    return out
