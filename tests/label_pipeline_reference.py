"""Random sequences of label edits on one running state (TEST INFRASTRUCTURE ONLY): a seeded generator of step lists and an interpreter that
runs a step list on numpy arrays. No algorithm lives here: the interpreter dispatches to the restatements of the single operators
(region_grow_reference.grow, label_morph_reference.morph, label_islands_reference.islands, label_margin_reference.margin) and to plain
slicing for the region writes, and keeps the running (data volume, label volume, colour table).

A step is a plain dict that prints in an assertion message; blocks of bytes and colour tables are rebuilt from the seeds it carries
(region_block, data_block, color_table). The kinds:
    region    update_label_region of a box with bytes of one label at a density (0: the block is all 0)
    grow, morph, islands, margin   the operator's call; "args" are the keyword arguments of the reference and of abi.Resources alike
    measure   one of the four with new_label -1 / measure=True: writes nothing
    colors    set_label_colors: every label a colour of its own; the present labels of "show" with alpha > 0, those of "clear" with alpha 0
    data      update_volume_region of a box of the data volume: zeros ("empty": its bricks fall below the window) or high values ("fill")
    reattach  release_label_volume, then attach_empty_labels: an all-zero label volume and the default colour table

Volumes are indexed [z, y, x]; origins, extents and seeds are (x, y, z), as in the C-ABI."""
import collections
import functools

import numpy as np

from tbraymarcherplugin_amd import synthetic as S
import label_islands_reference as IR
import label_margin_reference as GM
import label_morph_reference as MR
import label_reference as LR
import region_grow_reference as RG

SHAPES = [(40, 24, 19), (33, 17, 12), (24, 24, 24), (20, 17, 13)]   # the single-operator files' shapes: ragged last bricks
DTYPES = [np.uint8, np.uint16, np.float32]
SEEDS = tuple(range(12))
STEPS = 12
CHECKPOINTS = (3, 7, STEPS - 1)   # behind the fourth, the eighth and the last step: where the GPU test looks at the picture
KINDS = ("region", "grow", "morph", "islands", "margin", "measure", "colors", "data", "reattach")
WRITERS = ("region", "grow", "morph", "islands", "margin", "reattach")   # the kinds that may change a label byte
PALETTE = (1, 2, 3, 5, 7)
ISO, ANISO = (1, 1, 1), (256, 400, 1600)
ISLANDS_MODES = ("keep_largest", "remove_small", "split", "fill_holes")
GROW_FIELDS = ("voxels", "relabelled", "bbox_min", "bbox_max", "seeds_taken", "lo_used", "hi_used")   # grow's result but "passes"
FIELDS = {"grow": GROW_FIELDS, "morph": MR.FIELDS, "islands": IR.FIELDS, "margin": GM.FIELDS}
BRICK = 8

After = collections.namedtuple("After", "result labels vol colors")   # the state behind a step; the arrays are never written into again


# ---- the set-up of a seed -------------------------------------------------------------------------------------------------------
def setup(seed):
    """the shape, the data type and the first label volume of a seed: shapes and types spread over the seeds, empty and blob starts
    alternate; every fourth seed has a reattach"""
    return {"seed": seed, "dims": SHAPES[(seed + seed // 4) % 4], "dtype": np.dtype(DTYPES[seed % 3]).name, "vol_seed": 0x5EED0100 + seed,
            "start": "empty" if seed % 2 == 0 else "blobs", "reattach": seed % 4 == 3}


def initial(su):
    """(data volume, label volume, colour table) before the first step"""
    dims = su["dims"]
    vol = S.make_volume_numpy(dims, np.dtype(su["dtype"]), su["vol_seed"])
    labels = np.zeros(dims[::-1], dtype=np.uint8)
    if su["start"] == "blobs":
        labels[MR.blobs(dims, su["seed"] + 101)] = 7
        labels[MR.blobs(dims, su["seed"] + 100)] = 3
    return vol, labels, LR.default_label_colors()


# ---- what a step's seeds stand for ----------------------------------------------------------------------------------------------
def region_block(step):
    ex, ey, ez = step["extent"]
    r = np.random.default_rng(step["seed"]).random((ez, ey, ex))
    return np.where(r < step["density"], step["label"], 0).astype(np.uint8)


def data_block(step, dtype):
    ex, ey, ez = step["extent"]
    dtype = np.dtype(dtype)
    if step["mode"] == "empty":
        return np.zeros((ez, ey, ex), dtype=dtype)
    r = 0.6 + 0.4 * np.random.default_rng(step["seed"]).random((ez, ey, ex))   # "fill": well inside the window
    return r.astype(np.float32) if dtype == np.float32 else np.floor(r * RG.top_of(dtype)).astype(dtype)


def color_table(step):
    """every label but 0 in a colour of its own (the default table shows every label from 3 on as the same opaque black: an edit among
    them would not reach the picture), alpha 0.3 .. 0.9; the labels of "clear" keep their colour and lose their alpha"""
    rng = np.random.default_rng(step["seed"])
    c = np.zeros((256, 4), dtype=np.float32)
    c[1:, :3] = rng.uniform(0.0, 1.0, size=(255, 3))
    c[1:, 3] = rng.uniform(0.3, 0.9, size=255)
    for l in step["clear"]:
        c[l, 3] = 0.0
    return c


def call_of(step):
    """(which of "grow", "morph", "islands", "margin", its keyword arguments) of a grow, morph, islands, margin or measure step"""
    name = step["call"]
    args = dict(step["args"])
    if name == "islands" and "all_but" in args:   # fill holes: the set is everything but the label
        label = args.pop("all_but")
        args["source"] = [l for l in range(256) if l != label]
    return name, args


def box_bricks(dims, origin, extent):
    """bricks a box touches (no extent: the whole volume)"""
    if extent is None or tuple(extent) == (0, 0, 0):
        origin, extent = (0, 0, 0), dims
    n = 1
    for o, e in zip(origin, extent):
        n *= (o + e - 1) // BRICK - o // BRICK + 1
    return n


# ---- the interpreter ------------------------------------------------------------------------------------------------------------
def assigned(a, origin, block):
    out = a.copy()
    out[origin[2]:origin[2] + block.shape[0], origin[1]:origin[1] + block.shape[1], origin[0]:origin[0] + block.shape[2]] = block
    return out


def apply(step, vol, labels, colors):
    """one step on the state -> After(the reference's result dict (None where the call has none), labels, vol, colors)"""
    kind = step["kind"]
    if kind == "region":
        return After(None, assigned(labels, step["origin"], region_block(step)), vol, colors)
    if kind == "colors":
        return After(None, labels, vol, color_table(step))
    if kind == "data":
        return After(None, labels, assigned(vol, step["origin"], data_block(step, vol.dtype)), colors)
    if kind == "reattach":
        return After(None, np.zeros_like(labels), vol, LR.default_label_colors())
    name, args = call_of(step)
    if name == "grow":
        _, result, after = RG.grow(vol, labels=labels, **args)
    elif name == "morph":
        _, result, after = MR.morph(labels, **args)
    elif name == "margin":
        _, result, after = GM.margin(labels, **args)
    elif name == "islands":
        result, after, _ = IR.islands(labels, **args)
    else:
        raise ValueError(step)
    return After(result, after, vol, colors)


def run(su, steps):
    """the step list from the set-up's first state -> [After] per step"""
    vol, labels, colors = initial(su)
    out = []
    for step in steps:
        a = apply(step, vol, labels, colors)
        out.append(a)
        _, labels, vol, colors = a
    return out


# ---- the generator --------------------------------------------------------------------------------------------------------------
def pick(rng, seq):
    return seq[int(rng.integers(len(seq)))]


def draw_box(rng, dims, size):
    """(origin, extent): "brick": inside one brick; "large": all but a rim of 0 .. 3 voxels; "medium": a quarter to three quarters per axis"""
    origin, extent = [], []
    for n in dims:
        if size == "brick":
            b = int(rng.integers((n + BRICK - 1) // BRICK))
            lo, hi = b * BRICK, min(b * BRICK + BRICK, n)
            o = int(rng.integers(lo, max(lo + 1, hi - 3)))
            e = int(rng.integers(min(3, hi - o), hi - o + 1))
        elif size == "large":
            o = int(rng.integers(0, 4))
            e = n - o - int(rng.integers(0, 4))
        else:
            e = int(rng.integers(max(1, n // 4), max(2, 3 * n // 4)))
            o = int(rng.integers(0, n - e + 1))
        origin.append(o)
        extent.append(max(e, 1))
    return tuple(origin), tuple(extent)


def present(labels):
    return [int(l) for l in np.unique(labels) if l != 0]


def mask_args(rng, labels, args, boxed):
    """the optional box (drawn already: `boxed`) and the optional writable set of a morph or margin call"""
    if boxed is not None:
        args["origin"], args["extent"] = boxed
    if rng.random() < 0.35:
        args["writable"] = [0] if rng.random() < 0.5 else [0, pick(rng, PALETTE)]
    return args


def source_of(rng, labels):
    here = present(labels) or [pick(rng, PALETTE)]
    source = [pick(rng, here)]
    if len(here) > 1 and rng.random() < 0.4:
        source.append(pick(rng, [l for l in here if l != source[0]]))
    return source


def new_label_of(rng, source):
    """in the source, or out of it"""
    return source[0] if rng.random() < 0.6 else pick(rng, [l for l in PALETTE + (9,) if l not in source])


def gen_region(rng, vol, labels, plan):
    origin, extent = draw_box(rng, plan["dims"], "medium")
    return {"kind": "region", "origin": origin, "extent": extent, "label": pick(rng, PALETTE), "density": pick(rng, (0.0, 0.5, 0.8, 1.0, 0.7)),
            "seed": int(rng.integers(1 << 30))}


def gen_grow(rng, vol, labels, plan, measure=False):
    num = float if vol.dtype == np.float32 else int
    p1 = rng.uniform(30.0, 70.0)
    lo, hi = (num(v) for v in np.percentile(vol, [p1, p1 + rng.uniform(10.0, 30.0)]))
    args = {"seeds": [], "lo": lo, "hi": hi, "label": -1 if measure else pick(rng, PALETTE), "connectivity": pick(rng, (6, 26))}
    if rng.random() < 0.4:
        args["origin"], args["extent"] = draw_box(rng, plan["dims"], pick(rng, ("medium", "large")))
    if rng.random() < 0.3:
        args["writable"] = [0] if rng.random() < 0.5 else [0, pick(rng, PALETTE)]
    if rng.random() < 0.2:   # a range around the first seed's value
        in_range = np.argwhere((vol >= lo) & (vol <= hi))
        z, y, x = (int(v) for v in in_range[int(rng.integers(len(in_range)))])
        half = num((hi - lo) / 2)
        args.update(seeds=[(x, y, z)], lo=-half, hi=half, relative=True)
    n_seeds = 0 if (rng.random() < 0.15 and not args.get("relative")) else int(rng.integers(1, 4))   # none: plain thresholding
    cand, _, _ = RG.candidates(vol, args["lo"], args["hi"], labels, args.get("origin"), args.get("extent"), args.get("writable"),
                               np.asarray(args["seeds"], dtype=np.int64).reshape(-1, 3), args.get("relative", False))
    inside = np.argwhere(cand)
    while len(args["seeds"]) < n_seeds and len(inside):
        z, y, x = (int(v) for v in inside[int(rng.integers(len(inside)))])
        args["seeds"].append((x, y, z))
    if n_seeds and not args["seeds"]:   # no candidate at all: a seed that takes nothing, not a call that thresholds
        args["seeds"] = [(0, 0, 0)]
    return {"kind": "measure" if measure else "grow", "call": "grow", "args": args}


def gen_morph(rng, vol, labels, plan, measure=False):
    source = source_of(rng, labels)
    radius = int(rng.integers(1, 4))
    if plan.pop("long_morph", False):
        radius = int(rng.integers(9, 11))   # more than one launch of the step kernel
    args = {"op": pick(rng, MR.OPS), "radius": radius, "source": source, "new_label": -1 if measure else new_label_of(rng, source),
            "connectivity": pick(rng, (6, 26)), "erase_label": pick(rng, (0, 0, 4))}
    boxed = draw_box(rng, plan["dims"], pick(rng, ("medium", "large"))) if rng.random() < 0.4 else None
    return {"kind": "measure" if measure else "morph", "call": "morph", "args": mask_args(rng, labels, args, boxed)}


def staged_box(rng, plan, call):
    """the boxes of the islands and the margin calls of a sequence: the first inside one brick, the second large, later ones as they come
    — a later call needs more scratch than every call before it"""
    nth = plan["boxed"][call]
    plan["boxed"][call] += 1
    if nth == 0:
        return draw_box(rng, plan["dims"], "brick")
    if nth == 1:
        return draw_box(rng, plan["dims"], "large")
    return draw_box(rng, plan["dims"], "medium") if rng.random() < 0.5 else None


def gen_islands(rng, vol, labels, plan, measure=False):
    here = present(labels) or [pick(rng, PALETTE)]
    label = pick(rng, here)
    mode = pick(rng, ISLANDS_MODES)
    if plan["boxed"]["islands"] == 1 and plan["holes"] and plan["attempt"] < TRIES // 2:
        mode = "fill_holes"   # (holes are rare: the large box of some seeds looks for them first)
    args = {"source": [label], "connectivity": pick(rng, (6, 26)), "max_islands": 0, "min_voxels": 0, "keep_label": -1, "label_step": 0, "drop_label": -1,
            "spare_border": False, "measure": measure, "table": int(rng.integers(2, 6))}
    if mode == "keep_largest":
        args.update(max_islands=int(rng.integers(1, 3)), drop_label=pick(rng, (0, 0, 4)))
    elif mode == "remove_small":
        args.update(min_voxels=int(rng.integers(2, 25)), drop_label=pick(rng, (0, 0, 4)))
    elif mode == "split":
        args.update(max_islands=int(rng.integers(2, 5)), keep_label=int(rng.integers(10, 14)), label_step=1, drop_label=pick(rng, (-1, 0)))
    else:
        del args["source"]
        args.update(all_but=label, min_voxels=IR.ANY_SIZE if rng.random() < 0.5 else int(rng.integers(20, 200)), drop_label=label, spare_border=True)
    boxed = staged_box(rng, plan, "islands")
    if boxed is not None:
        args["origin"], args["extent"] = boxed
    return {"kind": "measure" if measure else "islands", "call": "islands", "mode": mode, "args": args}


def gen_margin(rng, vol, labels, plan, measure=False):
    source = source_of(rng, labels)
    weights = pick(rng, (ISO, ANISO))
    reach = int(rng.integers(1, 4))
    if plan.pop("long_margin", False):
        reach = 9   # two bricks either side
    args = {"op": pick(rng, GM.OPS), "weights": weights, "limit": (1 if weights == ISO else 256) * reach * reach, "source": source,
            "new_label": -1 if measure else new_label_of(rng, source), "erase_label": pick(rng, (0, 0, 4))}
    return {"kind": "measure" if measure else "margin", "call": "margin", "args": mask_args(rng, labels, args, staged_box(rng, plan, "margin"))}


def gen_measure(rng, vol, labels, plan):
    return pick(rng, (gen_grow, gen_morph, gen_islands, gen_margin))(rng, vol, labels, plan, measure=True)


def gen_colors(rng, vol, labels, plan):
    """some present labels get alpha 0, others become visible; one present label always shows"""
    here = present(labels) or [pick(rng, PALETTE)]
    order = [here[i] for i in rng.permutation(len(here))]
    n_show = max(1, int(rng.integers(1, len(order) + 1)) - (1 if len(order) > 1 else 0))
    return {"kind": "colors", "show": sorted(order[:n_show]), "clear": sorted(order[n_show:]), "seed": int(rng.integers(1 << 30))}


def gen_data(rng, vol, labels, plan):
    """"empty": zeros over whole bricks of the middle, where the data shows; "fill": high values in a corner, where it does not"""
    dims = plan["dims"]
    mode = plan["data_modes"].pop(0) if plan["data_modes"] else pick(rng, ("empty", "fill"))
    origin, extent = [], []
    for n in dims:
        nb = (n + BRICK - 1) // BRICK
        if mode == "empty":
            b = int(rng.integers(0, nb))
            o, e = b * BRICK, min(BRICK * int(rng.integers(1, 3)), n - b * BRICK)
        else:
            e = int(rng.integers(5, 12))
            o = 0 if rng.random() < 0.5 else n - e
        origin.append(o)
        extent.append(e)
    return {"kind": "data", "mode": mode, "origin": tuple(origin), "extent": tuple(extent), "seed": int(rng.integers(1 << 30))}


def gen_reattach(rng, vol, labels, plan):
    return {"kind": "reattach"}


GENERATORS = {"region": gen_region, "grow": gen_grow, "morph": gen_morph, "islands": gen_islands, "margin": gen_margin, "measure": gen_measure,
              "colors": gen_colors, "data": gen_data, "reattach": gen_reattach}
TRIES = 40


def schedule(rng, su):
    """the kinds of the twelve steps: nine writers, one measuring step, a colours step before the first checkpoint (behind a reattach:
    behind it) and a data step between two writers"""
    first = ["grow", "region"] if rng.random() < 0.5 else ["region", "grow"]
    if su["reattach"]:
        return [first[0], "morph", "reattach", first[1], "colors", "grow", "islands", "margin", "data", "islands", "margin", "measure"]
    last = ["margin", "morph", pick(rng, ("grow", "region", "morph"))]
    if rng.random() < 0.5:
        return first + ["colors", "islands", "morph", "data", "margin", "measure", "islands"] + last
    return first + ["colors", "islands", "margin", "morph", "measure", "islands", "data"] + last


def shown(labels, colors):
    """per voxel what its label adds to a ray: the premultiplied colour (colours of alpha 0 are all one)"""
    return np.concatenate([colors[:, :3] * colors[:, 3:], colors[:, 3:]], axis=1)[labels]


VISIBLE = 8   # voxels


def acceptable(kind, before, after, colors, attempt):
    """a writer's step is taken when it changes a byte and leaves the label volume neither empty nor full; in the first half of the
    draws only when VISIBLE voxels change what they show under the colour table in force, so that the edits reach the picture"""
    if kind not in WRITERS or kind == "reattach":
        return True
    if not ((after != before).any() and (after == 0).any() and (after != 0).any()):
        return False
    return attempt >= TRIES // 2 or int((shown(after, colors) != shown(before, colors)).any(axis=-1).sum()) >= VISIBLE


def generate(seed):
    """(the set-up, the step list, [After] per step) of a seed. A writer's step is drawn again, up to TRIES times, while the references
    say it would change nothing or would leave an empty or a full label volume."""
    su = setup(seed)
    rng = np.random.default_rng(0x1ABE1 + seed)
    vol, labels, colors = initial(su)
    plan = {"dims": su["dims"], "boxed": {"islands": 0, "margin": 0}, "long_morph": seed % 3 == 0, "long_margin": seed % 3 == 1,
            "data_modes": ["empty"] if seed % 2 == 0 else ["fill"], "holes": seed % 4 in (1, 2), "attempt": 0}
    steps, trace = [], []
    for kind in schedule(rng, su):
        for attempt in range(TRIES):
            trial = dict(plan, boxed=dict(plan["boxed"]), data_modes=list(plan["data_modes"]), attempt=attempt)   # a rejected draw leaves the plan as it was
            step = GENERATORS[kind](rng, vol, labels, trial)
            a = apply(step, vol, labels, colors)
            if acceptable(kind, labels, a.labels, colors, attempt):
                break
        plan = trial
        steps.append(step)
        trace.append(a)
        _, labels, vol, colors = a
    return su, steps, trace


@functools.lru_cache(maxsize=None)
def sequence(seed):
    """generate(seed), computed once a process: the references are the cost of every test that walks a sequence"""
    return generate(seed)


# ---- the fixed sequences of tests/test_gpu_label_pipeline.py --------------------------------------------------------------------
def grow_step(vol, share_lo, share_hi, label, seeds=(), **kw):
    """a grow step over the percentiles [share_lo, share_hi] of the data"""
    num = float if vol.dtype == np.float32 else int
    lo, hi = (num(v) for v in np.percentile(vol, [share_lo, share_hi]))
    return {"kind": "grow", "call": "grow", "args": dict(seeds=list(seeds), lo=lo, hi=hi, label=label, connectivity=6, **kw)}
