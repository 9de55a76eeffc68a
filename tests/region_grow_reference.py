"""Restatement of include/tbrm_segment.h's seeded region growing in numpy (TEST INFRASTRUCTURE ONLY): a frontier dilation by shifted
slices, no wrap. Nothing here is taken from the kernels: no bricks, no bit boards.

Volumes and label volumes are indexed [z, y, x]; seeds, origins and extents are (x, y, z), as in the C-ABI."""
import itertools

import numpy as np

OFFSETS_6 = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
OFFSETS_26 = [o for o in itertools.product((-1, 0, 1), repeat=3) if o != (0, 0, 0)]


def top_of(dtype):
    return 255 if np.dtype(dtype) == np.uint8 else 65535


def used_range(vol, lo, hi, seeds=None, relative=False):
    """(lo_used, hi_used, empty): the range the call applies, in stored units"""
    is_float = vol.dtype == np.float32
    if not relative:
        return (float(np.float32(lo)), float(np.float32(hi)), False) if is_float else (float(lo), float(hi), False)
    x, y, z = seeds[0]
    v0 = float(vol[z, y, x])
    if v0 != v0:
        return v0, v0, True
    a, b = v0 + lo, v0 + hi
    if is_float:
        with np.errstate(over="ignore"):
            return float(np.float32(a)), float(np.float32(b)), False
    top = top_of(vol.dtype)
    return float(min(max(a, 0), top)), float(min(max(b, 0), top)), a > top or b < 0


def candidates(vol, lo, hi, labels=None, origin=None, extent=None, writable=None, seeds=None, relative=False):
    """(candidate mask [z, y, x], lo_used, hi_used)"""
    lo_used, hi_used, empty = used_range(vol, lo, hi, seeds, relative)
    if vol.dtype == np.float32:
        with np.errstate(invalid="ignore"):
            cand = (vol >= np.float32(lo_used)) & (vol <= np.float32(hi_used))   # a NaN fails both
    else:
        cand = (vol.astype(np.int64) >= int(lo_used)) & (vol.astype(np.int64) <= int(hi_used))
    if empty:
        cand = np.zeros_like(cand)
    if extent is not None and tuple(extent) != (0, 0, 0):
        box = np.zeros_like(cand)
        o = origin if origin is not None else (0, 0, 0)
        box[o[2]:o[2] + extent[2], o[1]:o[1] + extent[1], o[0]:o[0] + extent[0]] = True
        cand &= box
    if writable is not None:
        ok = np.zeros(256, dtype=bool)
        ok[list(writable)] = True
        cand &= ok[labels] if labels is not None else ok[0]
    return cand, lo_used, hi_used


def shifted(mask, dx, dy, dz):
    """out[z, y, x] = mask[z - dz, y - dy, x - dx] where that lies inside, else False (no wrap)"""
    out = np.zeros_like(mask)
    nz, ny, nx = mask.shape

    def span(n, d):
        return (slice(max(d, 0), n + min(d, 0)), slice(max(-d, 0), n + min(-d, 0)))

    (zd, zs), (yd, ys), (xd, xs) = span(nz, dz), span(ny, dy), span(nx, dx)
    out[zd, yd, xd] = mask[zs, ys, xs]
    return out


def fill(cand, seed_mask, connectivity):
    """the candidates connected to a seed through candidates; (mask, steps of the plain dilation)"""
    offsets = OFFSETS_6 if connectivity == 6 else OFFSETS_26
    region = seed_mask & cand
    frontier = region
    steps = 0
    while frontier.any():
        reach = np.zeros_like(cand)
        for dx, dy, dz in offsets:
            reach |= shifted(frontier, dx, dy, dz)
        frontier = reach & cand & ~region
        region = region | frontier
        steps += int(frontier.any())
    return region, steps


def grow(vol, seeds, lo, hi, label, connectivity=6, labels=None, origin=None, extent=None, writable=None, relative=False):
    """Same arguments as Resources.grow_region, plus the label volume (None: every voxel has label 0).
    -> (region mask [z, y, x], result dict without "passes", the label volume afterwards (None when there is none))"""
    assert connectivity in (6, 26)
    seeds = np.asarray(seeds if seeds is not None else [], dtype=np.int64).reshape(-1, 3)
    cand, lo_used, hi_used = candidates(vol, lo, hi, labels, origin, extent, writable, seeds, relative)
    if len(seeds) == 0:
        region, taken = cand, 0
    else:
        seed_mask = np.zeros_like(cand)
        seed_mask[seeds[:, 2], seeds[:, 1], seeds[:, 0]] = True
        taken = int(cand[seeds[:, 2], seeds[:, 1], seeds[:, 0]].sum())   # (a seed given twice counts twice)
        region, _ = fill(cand, seed_mask, connectivity)
    nz, ny, nx = vol.shape
    res = {"voxels": int(region.sum()), "relabelled": 0, "bbox_min": (nx, ny, nz), "bbox_max": (-1, -1, -1), "seeds_taken": taken,
           "lo_used": lo_used, "hi_used": hi_used}
    if res["voxels"]:
        z, y, x = np.nonzero(region)
        res["bbox_min"] = (int(x.min()), int(y.min()), int(z.min()))
        res["bbox_max"] = (int(x.max()), int(y.max()), int(z.max()))
    after = None if labels is None else labels.copy()
    if label >= 0 and labels is not None:
        res["relabelled"] = int((labels[region] != label).sum())
        after[region] = label
    return region, res, after


# ---- the constructions of the tests ---------------------------------------------------------------------------------------------
def brick_snake():
    """8^3: serpentine rows y in {0, 2, 4, 6} in the planes z in {0, 2, 4, 6}, single-voxel connectors at alternating ends and between
    the planes. One path from the origin through all of its voxels."""
    m = np.zeros((8, 8, 8), dtype=bool)
    x_end, y_dir = 7, 1   # where the path leaves the current row; which way it walks through the rows of the current plane
    y = 0
    for z in (0, 2, 4, 6):
        rows = (0, 2, 4, 6) if y_dir > 0 else (6, 4, 2, 0)
        for k, y in enumerate(rows):
            m[z, y, :] = True
            if k < 3:
                m[z, y + y_dir, x_end] = True   # the connector to the next row, at the end the path arrives at
                x_end = 7 - x_end
        if z < 6:
            m[z + 1, y, x_end] = True           # the connector to the next plane
            x_end = 7 - x_end
            y_dir = -y_dir
    return m


def plane_snake(n=24, z=3):
    """n^3: in the plane z the rows y = 0, 2, .., n - 2 are full, connectors at alternating ends"""
    m = np.zeros((n, n, n), dtype=bool)
    for k, y in enumerate(range(0, n, 2)):
        m[z, y, :] = True
        if y + 2 < n:
            m[z, y + 1, n - 1 if k % 2 == 0 else 0] = True
    return m


def mask_volume(mask, dtype, inside=None, outside=None):
    """a volume that holds `inside` where the mask is set and `outside` elsewhere (defaults: 3/4 and 1/8 of the range)"""
    if np.dtype(dtype) == np.float32:
        a, b = (0.75 if inside is None else inside), (0.125 if outside is None else outside)
    else:
        top = top_of(dtype)
        a, b = (3 * top // 4 if inside is None else inside), (top // 8 if outside is None else outside)
    return np.where(mask, np.asarray(a, dtype=dtype), np.asarray(b, dtype=dtype)).astype(dtype)


def synchronous_brick_passes(cand, seed_mask, connectivity):
    """passes a synchronous brick model needs: per pass every brick converges on its own from its visited bits and the halo of its
    neighbours as they were BEFORE the pass. Counts the passes that change something."""
    nz, ny, nx = cand.shape
    region = seed_mask & cand
    passes = 0
    while True:
        new = region.copy()
        for bz, by, bx in itertools.product(range(0, nz, 8), range(0, ny, 8), range(0, nx, 8)):
            z0, y0, x0 = max(bz - 1, 0), max(by - 1, 0), max(bx - 1, 0)
            sub = (slice(z0, min(bz + 9, nz)), slice(y0, min(by + 9, ny)), slice(x0, min(bx + 9, nx)))
            own = np.zeros_like(cand[sub])
            own[bz - z0:bz - z0 + 8, by - y0:by - y0 + 8, bx - x0:bx - x0 + 8] = True
            filled, _ = fill(cand[sub] & own | region[sub] & ~own, region[sub], connectivity)
            new[sub] |= filled & own
        if (new == region).all():
            return passes
        region = new
        passes += 1
