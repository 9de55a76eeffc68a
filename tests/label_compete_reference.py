"""Restatement of include/tbrm_compete.h's competitive growing from seed labels in numpy / Python (TEST INFRASTRUCTURE ONLY). Nothing
here is taken from the kernels: no bricks in the two statements of the answer, no activity words.

  dijkstra()  the reference: a heap Dijkstra over packed keys (cost << 8) | label, in 32 bits as the header packs them
  relax()     the second statement: a synchronous relaxation by shifted slices to the fixed point

Both start every word at 0xFFFFFFFF and lower it only by a strictly smaller key, so the one key 0xFFFFFFFF (cost 2^24 - 1 from label
255) claims nothing, as the header says. synchronous_brick_passes() is the pass count of a brick model in which every brick sees its
neighbours as they were before the pass: the device, whose bricks may see newer keys, needs at most that many.

Volumes and label volumes are indexed [z, y, x]; origins, extents and step costs are (x, y, z), as in the C-ABI."""
import heapq
import itertools

import numpy as np

UNREACHED = 0xFFFFFFFF
MAX_COST = 0xFFFFFF
FIELDS = ("seed_voxels", "claimable", "claimed", "relabelled", "claimed_per_label", "max_cost", "bbox_min", "bbox_max")   # all but "passes"
AXIS_OF = {0: 2, 1: 1, 2: 0}   # array axis -> (x, y, z) axis


def float_range(lo, hi):
    """tbrm_host_compete_float_range: origin and scale formed in double, narrowed to float32"""
    return float(np.float32(lo)), float(np.float32(65535.0 / (float(hi) - float(lo))))


def codes(vol, frange=None):
    """c(v) as int64; a NaN voxel's code is never used"""
    if vol.dtype != np.float32:
        return vol.astype(np.int64)
    o, s = np.float32(frange[0]), np.float32(frange[1])
    with np.errstate(invalid="ignore", over="ignore"):
        d = (vol - o).astype(np.float32)             # two float32 operations, each rounded
        m = (d * s).astype(np.float32)
        c = np.rint(np.fmin(np.fmax(m, np.float32(0.0)), np.float32(65535.0)))   # fmax / fmin: a NaN gives the other argument
    return np.nan_to_num(c, nan=0.0).astype(np.int64)


def box_mask(shape, origin=None, extent=None):
    box = np.zeros(shape, dtype=bool)
    if extent is None or tuple(extent) == (0, 0, 0):
        box[:] = True
    else:
        o = origin if origin is not None else (0, 0, 0)
        box[o[2]:o[2] + extent[2], o[1]:o[1] + extent[1], o[0]:o[0] + extent[0]] = True
    return box


def in_set(labels, values):
    ok = np.zeros(256, dtype=bool)
    ok[[int(v) for v in values]] = True
    return ok[labels]


def classify(vol, labels, seeds, lo, hi, origin=None, extent=None, writable=None):
    """(box, seed voxels, sources, claimable) as masks"""
    box = box_mask(vol.shape, origin, extent)
    seed = in_set(labels, seeds) & box
    if vol.dtype == np.float32:
        with np.errstate(invalid="ignore"):
            gate = (vol >= np.float32(lo)) & (vol <= np.float32(hi))   # a NaN fails both
        source = seed & ~np.isnan(vol)
    else:
        gate = (vol.astype(np.int64) >= int(lo)) & (vol.astype(np.int64) <= int(hi))
        source = seed
    may = np.ones_like(box) if writable is None else in_set(labels, writable)
    return box, seed, source, box & may & gate & ~seed


def limit_of(cost_limit):
    return MAX_COST if cost_limit == 0 else int(cost_limit)


def axis_weights(c, step_cost, shift):
    """per array axis a: the weights of the steps between [.., i, ..] and [.., i + 1, ..]"""
    return [int(step_cost[AXIS_OF[a]]) + (np.abs(np.diff(c, axis=a)) >> int(shift)) for a in range(3)]


def dijkstra(c, labels, source, claimable, step_cost, shift, cost_limit):
    """keys as uint32 [z, y, x]: a source's label at cost 0, a claimed voxel's key, UNREACHED elsewhere"""
    limit = limit_of(cost_limit)
    nz, ny, nx = c.shape
    keys = np.full(c.shape, UNREACHED, dtype=np.int64)
    keys[source] = labels[source]
    K, Cd, claim = keys.ravel(), c.ravel(), claimable.ravel()
    heap = [(int(K[i]), int(i)) for i in np.flatnonzero(source.ravel())]
    heapq.heapify(heap)
    strides = ((1, nx, 0), (nx, ny, 1), (nx * ny, nz, 2))   # (stride, size, (x, y, z) axis)
    while heap:
        key, i = heapq.heappop(heap)
        if key != K[i]:
            continue
        pos = (i % nx, (i // nx) % ny, i // (nx * ny))
        for stride, size, a in strides:
            for d in (-1, 1):
                if not 0 <= pos[a] + d < size:
                    continue
                j = i + d * stride
                if not claim[j]:
                    continue
                cost = (key >> 8) + int(step_cost[a]) + (abs(int(Cd[i]) - int(Cd[j])) >> int(shift))
                if cost > limit:
                    continue
                offer = ((cost << 8) | (key & 255)) & 0xFFFFFFFF
                if offer < K[j]:
                    K[j] = offer
                    heapq.heappush(heap, (offer, j))
    return keys.astype(np.uint32)


def relax(c, keys, mutable, step_cost, shift, cost_limit):
    """(keys at the fixed point, sweeps that lowered a key): every sweep offers each voxel of `mutable` its six neighbours' keys of the
    sweep before; the others keep theirs"""
    limit = limit_of(cost_limit)
    w = axis_weights(c, step_cost, shift)
    K = keys.astype(np.int64)
    sweeps = 0
    while True:
        best = K.copy()
        for a in range(3):
            lo_, hi_ = [slice(None)] * 3, [slice(None)] * 3
            lo_[a], hi_[a] = slice(0, -1), slice(1, None)
            lo_, hi_ = tuple(lo_), tuple(hi_)
            for src, dst in ((lo_, hi_), (hi_, lo_)):
                cost = (K[src] >> 8) + w[a]
                offer = np.where(cost <= limit, (cost << 8) | (K[src] & 255), UNREACHED)
                best[dst] = np.minimum(best[dst], offer)
        new = np.where(mutable, best, K)
        if (new == K).all():
            return K.astype(np.uint32), sweeps
        K = new
        sweeps += 1


def start_keys(labels, source):
    keys = np.full(labels.shape, UNREACHED, dtype=np.uint32)
    keys[source] = labels[source]
    return keys


def compete(vol, labels, seeds, lo, hi, step_cost=(1, 1, 1), value_shift=0, cost_limit=0, origin=None, extent=None, writable=None, measure_only=False,
            frange=None, solver="dijkstra"):
    """Same arguments as Resources.compete_labels, plus the label volume.
    -> (result dict without "passes", the label volume afterwards, the costs of the box as uint32 [ez, ey, ex], keys [z, y, x])"""
    box, seed, source, claimable = classify(vol, labels, seeds, lo, hi, origin, extent, writable)
    c = codes(vol, frange)
    if solver == "dijkstra":
        keys = dijkstra(c, labels, source, claimable, step_cost, value_shift, cost_limit)
    else:
        keys, _ = relax(c, start_keys(labels, source), claimable, step_cost, value_shift, cost_limit)
    claimed = claimable & (keys != UNREACHED)
    nz, ny, nx = vol.shape
    res = {"seed_voxels": int(seed.sum()), "claimable": int(claimable.sum()), "claimed": int(claimed.sum()), "relabelled": 0, "claimed_per_label": {},
           "max_cost": 0, "bbox_min": (nx, ny, nz), "bbox_max": (-1, -1, -1)}
    after = labels.copy()
    if res["claimed"]:
        z, y, x = np.nonzero(claimed)
        res["bbox_min"] = (int(x.min()), int(y.min()), int(z.min()))
        res["bbox_max"] = (int(x.max()), int(y.max()), int(z.max()))
        won = (keys[claimed] & 255).astype(np.uint8)
        res["claimed_per_label"] = {int(l): int(n) for l, n in zip(*np.unique(won, return_counts=True))}
        res["max_cost"] = int((keys[claimed] >> 8).max())
        if not measure_only:
            res["relabelled"] = int((labels[claimed] != won).sum())
            after[claimed] = won
    costs = np.full(vol.shape, UNREACHED, dtype=np.uint32)
    costs[claimed] = keys[claimed] >> 8
    costs[seed] = 0
    zs, ys, xs = np.nonzero(box)
    costs = costs[zs.min():zs.max() + 1, ys.min():ys.max() + 1, xs.min():xs.max() + 1]
    return res, after, costs, keys


def synchronous_brick_passes(vol, labels, seeds, lo, hi, step_cost=(1, 1, 1), value_shift=0, cost_limit=0, origin=None, extent=None, writable=None, frange=None):
    """(passes that lowered a key, keys): per pass every 8^3 brick of the volume's grid relaxes to its own fixed point from its keys and
    the facing keys of its neighbours as they were BEFORE the pass"""
    _, _, source, claimable = classify(vol, labels, seeds, lo, hi, origin, extent, writable)
    c = codes(vol, frange)
    K = start_keys(labels, source)
    nz, ny, nx = vol.shape
    passes = 0
    while True:
        new = K.copy()
        for bz, by, bx in itertools.product(range(0, nz, 8), range(0, ny, 8), range(0, nx, 8)):
            z0, y0, x0 = max(bz - 1, 0), max(by - 1, 0), max(bx - 1, 0)
            sub = (slice(z0, min(bz + 9, nz)), slice(y0, min(by + 9, ny)), slice(x0, min(bx + 9, nx)))
            own = np.zeros(K[sub].shape, dtype=bool)
            own[bz - z0:bz - z0 + 8, by - y0:by - y0 + 8, bx - x0:bx - x0 + 8] = True
            if not (claimable[sub] & own).any():
                continue
            k, _ = relax(c[sub], K[sub], claimable[sub] & own, step_cost, value_shift, cost_limit)
            new[sub] = np.where(own, k, new[sub])
        if (new == K).all():
            return passes, K
        K = new
        passes += 1


# ---- the constructions of the tests ---------------------------------------------------------------------------------------------
SHAPES = [(8, 8, 8), (17, 9, 10), (40, 24, 19)]                    # (x, y, z)
PARAMS = [((1, 1, 1), 0), ((0, 0, 0), 2), ((2, 2, 5), 1)]          # (step_cost, value_shift)
SEEDS, WALL = (1, 2, 3), 9


def noise_volume(dims, dtype, seed=7):
    rng = np.random.default_rng(seed)
    shape = tuple(dims[::-1])
    if np.dtype(dtype) == np.float32:
        vol = rng.uniform(-1000.0, 3000.0, size=shape).astype(np.float32)
        vol[rng.random(shape) < 0.03] = np.nan
        return vol
    return rng.integers(0, 256 if np.dtype(dtype) == np.uint8 else 65536, size=shape).astype(dtype)


def noise_labels(dims, vol=None, seed=7):
    """three seed labels as small strokes, a wall label as two barrier planes with holes; on float data the first voxel of label 1 is
    made a NaN seed by the caller's volume when `vol` is given"""
    rng = np.random.default_rng(seed + 100)
    nx, ny, nz = dims
    labels = np.zeros((nz, ny, nx), dtype=np.uint8)
    wall = rng.random((nz, ny)) < 0.8
    labels[:, :, nx // 2][wall] = WALL
    wall = rng.random((ny, nx)) < 0.7
    labels[nz // 2, :, :][wall] = WALL
    for k, l in enumerate(SEEDS):
        for _ in range(2):
            x, y, z = int(rng.integers(0, nx)), int(rng.integers(0, ny)), int(rng.integers(0, nz))
            labels[z, y, x:min(x + 2, nx)] = l
    if vol is not None and vol.dtype == np.float32:
        z, y, x = np.argwhere(labels == SEEDS[0])[0]
        vol[z, y, x] = np.nan   # a seed voxel that is no source
    return labels


def gate_of(dtype):
    """a gate that lets most of the noise pass"""
    if np.dtype(dtype) == np.float32:
        return -900.0, 2900.0
    top = 255 if np.dtype(dtype) == np.uint8 else 65535
    return top // 32, top - top // 32


def noise_case(dims, dtype, seed=7):
    """(vol, labels, keyword arguments common to the reference and the binding)"""
    vol = noise_volume(dims, dtype, seed)
    labels = noise_labels(dims, vol, seed)
    lo, hi = gate_of(dtype)
    return vol, labels, lo, hi, (float_range(-1000.0, 3000.0) if np.dtype(dtype) == np.float32 else None)


def binding_limit(costs):
    """a limit that binds: the median cost of the claimed voxels of an unlimited run (at least 1)"""
    c = np.sort(costs[(costs != UNREACHED) & (costs > 0)])
    return max(int(c[len(c) // 2]), 1) if len(c) else 1


def corridor_case(mask, dtype=np.uint8):
    """a corridor of claimable voxels between walls, one seed voxel (label 1) at its first voxel: (vol, labels)"""
    labels = np.where(mask, 0, WALL).astype(np.uint8)
    z, y, x = np.argwhere(mask)[0]
    labels[z, y, x] = 1
    return np.zeros(mask.shape, dtype=dtype), labels
