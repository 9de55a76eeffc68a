"""Placement and bookkeeping for the tests that cross the size tiers of the label surface and the label islands (TEST INFRASTRUCTURE
ONLY): which block of cells or brick of a box a cell or voxel falls in, restated from the order include/tbrm_surface.h and
include/tbrm_islands.h state (x fastest inside the box's range); small patterns placed far apart in an otherwise empty volume; the
islands reference applied pattern by pattern where the volume is too large for it; and the label volumes of the cases, each built
once. There is no algorithm here: the surfaces are label_surface_reference's, the islands label_islands_reference's.

The tiers: the scans work in tiles of 1024 blocks / bricks, their top level takes 1024 tiles a trip (2^20 blocks
/ bricks), and the surface's count kernel launches at most 2048 workgroups of 32 blocks: 65536 blocks a trip.

Label volumes are indexed [z, y, x]; dims, origins, extents, cells, voxels and anchors are (x, y, z), as in the C-ABI."""
import functools
import time

import numpy as np

import label_islands_reference as IR
import label_surface_reference as SR

TILE = 1024                # blocks / bricks to a tile of the scans
COUNT_TRIP = 2048 * 32     # blocks k_surface_count takes per trip of its grid-stride loop
TOP_TRIP = TILE * TILE     # blocks / bricks the top level of a scan takes per trip


# ---- the counts and the order of the two tools ---------------------------------------------------------------------------------------------
def block_range(dims, origin=None, extent=None):
    """(b0, nb) per axis: the blocks of the cells o <= h <= e of the box [o, e)"""
    o, e = SR.resolve_box(dims, origin, extent)
    return tuple(o[c] >> 3 for c in range(3)), tuple((e[c] >> 3) - (o[c] >> 3) + 1 for c in range(3))


def brick_range(dims, origin=None, extent=None):
    """(b0, nb) per axis: the bricks the voxels of the box [o, e) lie in"""
    o, e = SR.resolve_box(dims, origin, extent)
    return tuple(o[c] // 8 for c in range(3)), tuple((e[c] - 1) // 8 - o[c] // 8 + 1 for c in range(3))


def surface_blocks(dims, origin=None, extent=None):
    return int(np.prod(block_range(dims, origin, extent)[1], dtype=np.int64))


def box_bricks(dims, origin=None, extent=None):
    return int(np.prod(brick_range(dims, origin, extent)[1], dtype=np.int64))


def position_in(b0, nb, at):
    b = (np.asarray(at, dtype=np.int64) >> 3) - np.asarray(b0, dtype=np.int64)
    assert ((b >= 0) & (b < np.asarray(nb, dtype=np.int64))).all()
    return (b[..., 2] * nb[1] + b[..., 1]) * nb[0] + b[..., 0]


def block_index(cell_high_corner, dims, origin=None, extent=None):
    """the position k, x fastest, of the block of the cell(s) with the high corner h ([..., 3]) in the box's block range"""
    return position_in(*block_range(dims, origin, extent), cell_high_corner)


def brick_index(voxel, dims, origin=None, extent=None):
    """the position k, x fastest, of the brick of the voxel(s) ([..., 3]) in the box's brick range"""
    return position_in(*brick_range(dims, origin, extent), voxel)


def vertex_blocks(vertex, dims, origin=None, extent=None):
    """per vertex record the block of its cell (the record holds the cell's low corner, h - 1)"""
    return block_index(vertex["cell"].astype(np.int64) + 1, dims, origin, extent)


def set_voxels(labels, source):
    """int64 [n, 3]: the (x, y, z) of the voxels whose label is in `source`"""
    z, y, x = np.nonzero(IR.table_of(source)[labels])
    return np.stack([x, y, z], axis=1).astype(np.int64)


# ---- patterns: uint8 [sz, sy, sx] ------------------------------------------------------------------------------------------------------------
def cluster(shape, density, seed, label=3, corners=()):
    """random voxels in a box of `shape`; `corners`: voxels of the box that are set whatever the draw"""
    out = np.where(np.random.default_rng(seed).random(shape[::-1]) < density, label, 0).astype(np.uint8)
    for x, y, z in corners:
        out[z, y, x] = label
    return out


def ball(shape, radius, label=3):
    """the ball about the middle of a box of `shape`, cut flat where the box is thinner than the ball"""
    centre = tuple((n - 1) // 2 for n in shape)
    return SR.ball_labels(shape, centre, radius, label)


def snake(length, label=3):
    """a 6-connected path along x that steps between two rows every third voxel: [1, 2, length]"""
    out = np.zeros((1, 2, length), dtype=np.uint8)
    for x in range(length):
        y = (x // 3) & 1
        out[0, y, x] = label
        if x and y != ((x - 1) // 3) & 1:
            out[0, 1 - y, x] = label
    return out


def boxes_of(patterns, anchors):
    return [(tuple(a), tuple(a[c] + p.shape[2 - c] for c in range(3))) for p, a in zip(patterns, anchors)]


def place(dims, patterns, anchors):
    """an all-zero uint8 label volume with the patterns copied in at the anchors; no two patterns come within 2 voxels of each other"""
    boxes = boxes_of(patterns, anchors)
    for i, (o, e) in enumerate(boxes):
        assert all(0 <= o[c] and e[c] <= dims[c] for c in range(3)), (i, o, e, dims)
        for j, (p, q) in enumerate(boxes[:i]):
            assert any(o[c] - 2 >= q[c] or p[c] - 2 >= e[c] for c in range(3)), ("patterns within 2 voxels of each other", j, i)
    labels = np.zeros(dims[::-1], dtype=np.uint8)
    for p, (o, e) in zip(patterns, boxes):
        labels[o[2]:e[2], o[1]:e[1], o[0]:e[0]] = p
    return labels


def crops_of(dims, patterns, anchors, margin=2):
    """per pattern the array slices [z, y, x] of its box and `margin` voxels around it, cut to the volume"""
    return [tuple(slice(max(o[c] - margin, 0), min(e[c] + margin, dims[c])) for c in (2, 1, 0)) for o, e in boxes_of(patterns, anchors)]


# ---- the islands reference, crop by crop ---------------------------------------------------------------------------------------------------
def islands_by_crops(labels, crops, source, connectivity=6, max_islands=0, min_voxels=0, keep_label=-1, label_step=0, drop_label=-1,
                     spare_border=False, measure=False, table=0):
    """IR.islands of the whole volume, composed from IR.islands of each crop: (the result dict, the label volume afterwards). Only rules
    whose verdict on an island does not depend on the other islands; every voxel of the set lies in exactly one crop, 2 voxels or more
    from every face of it that is not a face of the volume — so an island is whole in its crop and touches a face there exactly when it
    touches that face of the volume."""
    assert max_islands == 0 and label_step == 0 and not spare_border
    nz, ny, nx = labels.shape
    dims = (nx, ny, nz)
    voxels = set_voxels(labels, source)
    held = np.zeros(len(voxels), dtype=np.int64)
    for crop in crops:
        lo = np.asarray([crop[2].start, crop[1].start, crop[0].start], dtype=np.int64)
        hi = np.asarray([crop[2].stop, crop[1].stop, crop[0].stop], dtype=np.int64)
        inside = ((voxels >= lo) & (voxels < hi)).all(axis=1)
        held += inside
        for c in range(3):
            assert lo[c] == 0 or (voxels[inside, c] - lo[c] >= 2).all(), ("a set voxel within 2 of an inner crop face", crop)
            assert hi[c] == dims[c] or (hi[c] - 1 - voxels[inside, c] >= 2).all(), ("a set voxel within 2 of an inner crop face", crop)
    assert (held == 1).all(), "every voxel of the set lies in exactly one crop"

    after = labels if measure else labels.copy()
    res = dict.fromkeys(("set_voxels", "islands", "spared", "kept", "dropped", "kept_voxels", "dropped_voxels", "largest", "relabelled"), 0)
    bbox_min, bbox_max, entries = list(dims), [-1, -1, -1], []
    for crop in crops:
        at = (crop[2].start, crop[1].start, crop[0].start)
        r, a, _ = IR.islands(labels[crop], source, connectivity, min_voxels=min_voxels, keep_label=keep_label, drop_label=drop_label, measure=measure, table=1 << 30)
        for k in res:
            res[k] = max(res[k], r[k]) if k == "largest" else res[k] + r[k]
        if r["relabelled"]:
            bbox_min = [min(bbox_min[c], r["bbox_min"][c] + at[c]) for c in range(3)]
            bbox_max = [max(bbox_max[c], r["bbox_max"][c] + at[c]) for c in range(3)]
        if not measure:
            after[crop] = a
        for e in r["table"]:
            entries.append(dict(e, first=tuple(e["first"][c] + at[c] for c in range(3))))
    entries.sort(key=lambda e: (-e["voxels"], e["first"][0] + nx * (e["first"][1] + ny * e["first"][2])))   # size descending, first voxel ascending
    assert len(entries) == res["islands"]
    res.update(bbox_min=tuple(bbox_min), bbox_max=tuple(bbox_max), table=entries[:table], table_entries=min(table, len(entries)))
    return res, after


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
SOURCE = [3]
TWO_TILES = (99, 90, 75)            # 13 x 12 x 10 = 1560 blocks
TWO_TILES_BOXES = {"whole": (None, None), "box": ((9, 10, 8), (88, 79, 66))}   # the box: 12 x 11 x 9 = 1188 blocks from block (1, 1, 1) on
LONG = (524288, 9, 5)               # 65537 x 2 x 1 = 131074 blocks; 65536 x 2 x 1 bricks
LONG_SMALL_BOX = ((8000, 0, 0), (600, 9, 5))   # 76 x 2 blocks, around the second pattern
WIDE = (8200, 8192, 2)              # 1026 x 1025 x 1 = 1051650 blocks; 1025 x 1024 x 1 = 1049600 bricks
ISLANDS_TWO_TILES = (136, 64, 72)   # 17 x 8 x 9 = 1224 bricks
ISLANDS_BOXES = {"whole": (None, None), "box": ((3, 2, 9), (130, 60, 63))}     # the box: 17 x 8 x 8 = 1088 bricks from brick (0, 0, 1) on


@functools.lru_cache(maxsize=None)
def two_tiles_labels():
    """sparse random voxels of labels 3 and 9, a ball across the blocks 1023 | 1024 of the whole volume ((9, 6, 6) | (10, 6, 6)) and one
    across the blocks 1023 | 1024 of the box ((4, 9, 8) | (5, 9, 8) of the volume)"""
    labels = SR.random_labels(TWO_TILES, 0.004, 21, labels=(3, 9))
    for centre in ((79, 51, 51), (39, 75, 67)):
        labels[SR.ball_labels(TWO_TILES, centre, 3.3) > 0] = 3
    return labels


@functools.lru_cache(maxsize=None)
def long_case():
    """(labels, crops, patterns' boxes): near x = 0, the only one at the faces y = 0 and z = 0, across the rows y = 7 | 8 (blocks 0 and 65537), across x = 8192 (blocks 1023 | 1024,
    bricks 1023 | 1024), in the middle, and at the far end up to the last voxel (blocks 65535 | 65536 and 131072, 131073)"""
    patterns = [cluster((20, 9, 5), 0.15, 31, corners=[(0, 0, 0)]), ball((9, 7, 3), 3.3), snake(24), cluster((16, 8, 4), 0.15, 32, corners=[(15, 7, 3)])]
    anchors = [(2, 0, 0), (8187, 1, 1), (262132, 6, 2), (524272, 1, 1)]
    return place(LONG, patterns, anchors), crops_of(LONG, patterns, anchors), boxes_of(patterns, anchors)


@functools.lru_cache(maxsize=None)
def wide_case():
    """(labels, crops, patterns' boxes): in tile 0; a disc across x = 8192 of the first rows (blocks and bricks 1023 | 1024); in a middle
    tile; a disc across the blocks 2^20 - 1 | 2^20 ((3, 1022) | (4, 1022)); a snake across the bricks 2^20 - 1 | 2^20 ((0, 1023) |
    (1, 1023)); a cluster in the last rows; one at the last corner, the last voxel set"""
    patterns = [cluster((20, 20, 2), 0.2, 41), ball((12, 12, 2), 5.3), cluster((18, 14, 2), 0.2, 42), ball((12, 12, 2), 5.3), snake(20),
                cluster((20, 14, 2), 0.2, 43), cluster((16, 12, 2), 0.2, 44, corners=[(15, 11, 1)])]
    anchors = [(3, 2, 0), (8186, 1, 0), (4000, 4100, 0), (26, 8168, 0), (2, 8185, 0), (5000, 8178, 0), (8184, 8180, 0)]
    return place(WIDE, patterns, anchors), crops_of(WIDE, patterns, anchors), boxes_of(patterns, anchors)


@functools.lru_cache(maxsize=None)
def islands_two_tiles_labels():
    """label 3 at density 0.08 among label 7, and two snakes of label 3 along x through the bricks (2 .. 6, 4, 7) and (2 .. 6, 4, 8):
    the bricks 1022 .. 1026 of the whole volume and of the box"""
    dims = ISLANDS_TWO_TILES
    labels = np.where(IR.noise_mask(dims, 0.5, 52), 7, 0).astype(np.uint8)
    labels[IR.noise_mask(dims, 0.08, 51)] = 3
    s = snake(35)
    for z in (59, 67):
        labels[z:z + 1, 35:37, 18:53][s > 0] = 3
    return labels


_SURFACES = {}


def surface_reference(name, box="whole"):
    """(labels, origin, extent, SR.surface of it, the seconds that took), computed once per case and box"""
    if (name, box) not in _SURFACES:
        labels, (origin, extent) = {"two_tiles": lambda: (two_tiles_labels(), TWO_TILES_BOXES[box]),
                                    "long": lambda: (long_case()[0], {"whole": (None, None), "small": LONG_SMALL_BOX}[box]),
                                    "wide": lambda: (wide_case()[0], (None, None))}[name]()
        t0 = time.perf_counter()
        want = SR.surface(labels, SOURCE, origin, extent)
        _SURFACES[(name, box)] = (labels, origin, extent, want, time.perf_counter() - t0)
    return _SURFACES[(name, box)]
