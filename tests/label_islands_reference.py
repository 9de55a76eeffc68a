"""Restatement of include/tbrm_islands.h's islands of a label in numpy (TEST INFRASTRUCTURE ONLY): every voxel of the set starts with its
own linear index and takes the smallest index among its neighbours, by shifted slices and no wrap, until nothing changes; what a voxel
ends with is its island's first voxel. Nothing here is taken from the kernels: no bricks, no bit boards, no union-find, no scipy.

Label volumes and masks are indexed [z, y, x]; origins, extents and first voxels are (x, y, z), as in the C-ABI."""
import numpy as np

from region_grow_reference import OFFSETS_6, OFFSETS_26

ANY_SIZE = 0xFFFFFFFFFFFFFFFF
FIELDS = ("set_voxels", "islands", "spared", "kept", "dropped", "kept_voxels", "dropped_voxels", "largest", "relabelled", "bbox_min", "bbox_max",
          "table_entries", "table")


def shifted(a, dx, dy, dz, pad):
    """out[z, y, x] = a[z - dz, y - dy, x - dx] where that lies inside the volume, else `pad`"""
    out = np.full_like(a, pad)
    nz, ny, nx = a.shape

    def span(n, d):
        return (slice(max(d, 0), n + min(d, 0)), slice(max(-d, 0), n + min(-d, 0)))

    (zd, zs), (yd, ys), (xd, xs) = span(nz, dz), span(ny, dy), span(nx, dx)
    out[zd, yd, xd] = a[zs, ys, xs]
    return out


def table_of(values):
    ok = np.zeros(256, dtype=bool)
    ok[list(values)] = True
    return ok


def box_mask(shape, origin=None, extent=None):
    """(mask, (x0, y0, z0), (x1, y1, z1)) of the box [origin, origin + extent); an all-zero extent or none: the whole volume"""
    nz, ny, nx = shape
    if extent is None or tuple(extent) == (0, 0, 0):
        o, e = (0, 0, 0), (nx, ny, nz)
    else:
        o = tuple(origin) if origin is not None else (0, 0, 0)
        e = tuple(o[c] + extent[c] for c in range(3))
    box = np.zeros(shape, dtype=bool)
    box[o[2]:e[2], o[1]:e[1], o[0]:e[0]] = True
    return box, o, e


def first_voxels(S, connectivity):
    """per voxel of S the linear index x + X * (y + Y * z) of the first voxel of its island; S.size outside S"""
    offsets = OFFSETS_6 if connectivity == 6 else OFFSETS_26
    big = S.size
    lab = np.where(S, np.arange(big, dtype=np.int64).reshape(S.shape), big)
    while True:
        new = lab
        for dx, dy, dz in offsets:
            new = np.where(S, np.minimum(new, shifted(new, dx, dy, dz, big)), big)
        if np.array_equal(new, lab):
            return lab
        lab = new


def find(labels, source, connectivity=6, origin=None, extent=None):
    """the islands of the set, unordered: (S, per-voxel first-voxel index, firsts, sizes, border bits)"""
    assert connectivity in (6, 26)
    box, o, e = box_mask(labels.shape, origin, extent)
    S = table_of(source)[labels] & box
    lab = first_voxels(S, connectivity)
    firsts, sizes = np.unique(lab[S], return_counts=True)
    face = np.zeros(labels.shape, dtype=bool)
    face[o[2], :, :] = face[e[2] - 1, :, :] = face[:, o[1], :] = face[:, e[1] - 1, :] = face[:, :, o[0]] = face[:, :, e[0] - 1] = True
    on_face = np.unique(lab[S & face & box])
    border = np.isin(firsts, on_face)
    return S, lab, firsts, sizes, border


def islands(labels, source, connectivity=6, max_islands=0, min_voxels=0, keep_label=-1, label_step=0, drop_label=-1, spare_border=False,
            measure=False, origin=None, extent=None, table=0):
    """Same arguments as Resources.label_islands, plus the label volume. -> (the result dict with every field of FIELDS, the label
    volume afterwards, per voxel the position of its island in the order: -1 outside the set, -2 in a spared island)"""
    nz, ny, nx = labels.shape
    S, lab, firsts, sizes, border = find(labels, source, connectivity, origin, extent)
    spared = border & bool(spare_border)
    order = [i for i in np.lexsort((firsts, -sizes)) if not spared[i]]   # size descending, first voxel ascending
    after = labels.copy()
    position = np.full(labels.shape, -1, dtype=np.int64)
    for i in np.nonzero(spared)[0]:
        position[lab == firsts[i]] = -2
    res = dict(set_voxels=int(S.sum()), islands=len(order), spared=int(spared.sum()), kept=0, dropped=0, kept_voxels=0, dropped_voxels=0,
               largest=int(sizes[order[0]]) if order else 0)
    kept_flags, acts = [], []
    lut_pos = np.full(S.size + 1, -1, dtype=np.int64)
    lut_act = np.full(S.size + 1, -1, dtype=np.int64)
    for pos, i in enumerate(order):
        size = int(sizes[i])
        kept = (max_islands == 0 or pos < max_islands) and size >= min_voxels
        act = (keep_label + pos * label_step if keep_label >= 0 else -1) if kept else drop_label
        res["kept" if kept else "dropped"] += 1
        res["kept_voxels" if kept else "dropped_voxels"] += size
        kept_flags.append(kept)
        acts.append(act)
        lut_pos[firsts[i]] = pos
        lut_act[firsts[i]] = act
    ordered = S & (position != -2)
    position[ordered] = lut_pos[lab[ordered]]
    if not measure:
        act_of = lut_act[lab]   # (lab is S.size outside S: -1)
        write = ordered & (act_of >= 0)
        after[write] = act_of[write].astype(np.uint8)
    changed = after != labels
    res["relabelled"] = int(changed.sum())
    if changed.any():
        z, y, x = np.nonzero(changed)
        res["bbox_min"], res["bbox_max"] = (int(x.min()), int(y.min()), int(z.min())), (int(x.max()), int(y.max()), int(z.max()))
    else:
        res["bbox_min"], res["bbox_max"] = (nx, ny, nz), (-1, -1, -1)
    entries = []
    for pos, i in enumerate(order[:table]):
        f = int(firsts[i])
        held = np.unique(after[lab == f])
        entries.append({"voxels": int(sizes[i]), "first": (f % nx, (f // nx) % ny, f // (nx * ny)), "label": int(held[0]) if len(held) == 1 else -1,
                        "kept": bool(kept_flags[pos]), "border": bool(border[i])})
    res["table_entries"], res["table"] = len(entries), entries
    return res, after, position


# ---- the four tools, as Resources names them ------------------------------------------------------------------------------------
def keep_largest(labels, label, n=1, erase_label=0, connectivity=6, **kw):
    return islands(labels, [label], connectivity, max_islands=n, keep_label=-1, drop_label=erase_label, **kw)


def remove_small(labels, label, min_voxels, erase_label=0, connectivity=6, **kw):
    return islands(labels, [label], connectivity, max_islands=0, min_voxels=min_voxels, keep_label=-1, drop_label=erase_label, **kw)


def split(labels, label, first_label, max_islands, drop_label=-1, connectivity=6, **kw):
    return islands(labels, [label], connectivity, max_islands=max_islands, keep_label=first_label, label_step=1, drop_label=drop_label, **kw)


def fill_holes(labels, label, max_voxels=None, connectivity=6, **kw):
    return islands(labels, [l for l in range(256) if l != label], connectivity, max_islands=0,
                   min_voxels=ANY_SIZE if max_voxels is None else max_voxels + 1, keep_label=-1, drop_label=label, spare_border=True, **kw)


# ---- the constructions of the tests ---------------------------------------------------------------------------------------------
def noise_mask(dims, q, seed=7):
    """the lowest fraction q of default_rng(seed).random(dims[::-1]) set, [z, y, x]"""
    r = np.random.default_rng(seed).random(dims[::-1])
    return r < np.quantile(r, q)


def checkerboard(n):
    z, y, x = np.indices((n, n, n))
    return (x + y + z) % 2 == 0


def diagonal_checkerboard(n):
    """voxels with x, y, z all even or all odd: no two share a face or an edge, each touches others at corners only"""
    z, y, x = np.indices((n, n, n))
    return (x % 2 == y % 2) & (y % 2 == z % 2)
