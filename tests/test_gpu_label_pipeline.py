"""The label edits as a pipeline on ONE handle (include/tbrm_labels.h, tbrm_segment.h, tbrm_morphology.h, tbrm_islands.h, tbrm_margin.h)
against the references, call after call without a fresh upload: the sequences of tests/label_pipeline_reference.py. What the writers
share per handle — the scratch they work in, the scratch that only ever grows, the per-brick label sets behind each call's bounding box,
the lazily merged skipping metadata — is where a sequence can go wrong while every single-call test stays green.

After every step: every field of the call's result, every byte of the label volume, and the light volume as it was. At the checkpoints
the handle that went through the edits must show what a fresh handle shows that was handed the same bytes: frames with and without
skipping, hit records, label statistics and a label-masked histogram, bit for bit. The results are integers and bytes: every comparison
with the references is exact equality."""
import collections

import numpy as np
import pytest
import torch

from tbraymarcherplugin_amd import abi, synthetic as S
import exact_reference as X
import label_islands_reference as IR
import label_margin_reference as GM
import label_morph_reference as MR
import label_pipeline_reference as P
import label_reference as LR
import region_grow_reference as RG

pytestmark = pytest.mark.gpu

WINDOW = (0.5, 0.9, True, False)
CAM = S.default_camera(64, 48)
TILE = abi.Tile(0, 0, 64, 48)
WORLD = S.default_world()
STEPS, JITTER = 100.0, 1
CHECKPOINTS = P.CHECKPOINTS
HOOKS = {"grow_batch": 1, "morph_steps": 1, "margin_skip": 0, "stats_groups": 3}

Run = collections.namedtuple("Run", "results bytes frames light")


def data_handle(dims, vol, light32=False):
    res = abi.Resources(dims, abi.DTYPE_FMT[vol.dtype], light32)
    res.upload_volume(vol)
    res.set_tf_lut(abi.color_curve_to_lut(S.tf_keys("A")))
    res.set_windowing(abi.WindowingParams(*WINDOW))
    return res


def edited_handle(su, light32=False):
    """the handle the sequence runs on: the data, two lights added once, then an empty or an uploaded label volume"""
    vol, labels, _ = P.initial(su)
    res = data_handle(su["dims"], vol, light32)
    for i in (0, 1):
        res.add_dir_light(S.light(i), True, WORLD)
    if su["start"] == "empty":
        res.attach_empty_labels()
    else:
        res.upload_label_volume(labels)
    return res


def fresh_handle(dims, after, light, light32=False):
    """a handle that never saw an edit: the state's bytes uploaded"""
    res = data_handle(dims, after.vol, light32)
    res.upload_label_volume(after.labels)
    res.set_label_colors(after.colors)
    res.upload_light_volume(light)
    return res


def on_handle(res, step, dtype):
    """the step on the handle -> the call's result dict (None where the call has none)"""
    kind = step["kind"]
    if kind == "region":
        return res.update_label_region(step["origin"], P.region_block(step))
    if kind == "colors":
        return res.set_label_colors(P.color_table(step))
    if kind == "data":
        return res.update_volume_region(step["origin"], P.data_block(step, dtype))
    if kind == "reattach":
        res.release_label_volume()
        assert not res.has_label_volume()
        return res.attach_empty_labels()
    name, args = P.call_of(step)
    return {"grow": res.grow_region, "morph": res.morph_labels, "islands": res.label_islands, "margin": res.margin_labels}[name](**args)


def same_step(res, i, step, want, dtype):
    """one step on the handle and what the reference says of it: every field of the result, every byte afterwards"""
    got = on_handle(res, step, dtype)
    if want.result is not None:
        for k in P.FIELDS[step["call"]]:
            assert got[k] == want.result[k], (i, step, k, got[k], want.result[k])
    down = res.download_label_volume()
    assert np.array_equal(down, want.labels), (i, step, int((down != want.labels).sum()),
                                                [(tuple(v[::-1]), int(down[tuple(v)]), int(want.labels[tuple(v)])) for v in np.argwhere(down != want.labels)[:5]])
    return got, down


def identical(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def views(res, labels, dims, dtype):
    """everything that reads the label bytes and the sets behind them"""
    top = 1.0 if np.dtype(dtype) == np.float32 else RG.top_of(dtype)
    two = [int(l) for l in np.unique(labels)[-2:]]
    box = ((3, 2, 1), (dims[0] // 2 + 1, dims[1] // 2 + 1, dims[2] // 2 + 1))
    counts, tally = res.volume_histogram(32, 0, top, labels=two)
    return {"skipping on": res.raymarch_lit(CAM, TILE, abi.RaymarchParams(STEPS, JITTER, True), WORLD),
            "skipping off": res.raymarch_lit(CAM, TILE, abi.RaymarchParams(STEPS, JITTER, False), WORLD),
            "hits": res.raymarch_hits(CAM, TILE, abi.RaymarchParams(STEPS, JITTER, True), WORLD, 0.5),
            "statistics": res.label_statistics(), "statistics of a box": res.label_statistics(*box),
            "histogram of %s" % two: counts, "histogram's tallies": np.array([tally[k] for k in abi.Resources.HISTOGRAM_TALLY], dtype=np.uint64)}


def checkpoint(res, after, light, dims, where):
    """the edited handle against a fresh one with the same bytes -> the edited handle's views"""
    seen = views(res, after.labels, dims, after.vol.dtype)
    with fresh_handle(dims, after, light) as fresh:
        want = views(fresh, after.labels, dims, after.vol.dtype)
    for k in want:
        assert identical(seen[k], want[k]), (where, k, int((seen[k].view(np.uint8) != want[k].view(np.uint8)).sum()) if seen[k].shape == want[k].shape else None)
    stats = seen["statistics"]
    assert np.array_equal(stats["count"], np.bincount(after.labels.ravel(), minlength=256)), where
    return seen


def walk(su, steps, trace, check=True, light32=False):
    """the sequence on one handle -> Run. Every step is held to the reference; check: the checkpoints against fresh handles"""
    dtype = np.dtype(su["dtype"])
    results, downs, frames = [], [], []
    with edited_handle(su, light32) as res:
        light = res.download_light_volume()
        assert light.any()
        for i, (step, want) in enumerate(zip(steps, trace)):
            got, down = same_step(res, i, step, want, dtype)
            results.append(got)
            downs.append(down)
            assert np.array_equal(res.download_light_volume(), light), (i, step)   # no edit of labels, colours or data moves the illumination
            if check and i in CHECKPOINTS:
                seen = checkpoint(res, want, light, su["dims"], (su, i, steps[:i + 1]))
                if frames:   # the edits reach the picture
                    assert not np.array_equal(seen["skipping on"], frames[-1]), (su, i, steps[:i + 1])
                frames.append(seen["skipping on"])
        final = res.raymarch_lit(CAM, TILE, abi.RaymarchParams(STEPS, JITTER, True), WORLD)
    return Run(results, downs, frames, light), final


DEFAULT_RUNS = {}


def default_run(seed):
    """the seed's sequence at the library's default tunables, walked once a process"""
    if seed not in DEFAULT_RUNS:
        DEFAULT_RUNS[seed] = walk(*P.sequence(seed))[0]
    return DEFAULT_RUNS[seed]


# ---- random sequences -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", P.SEEDS)
def test_random_sequences(gpu, seed):
    run = default_run(seed)
    assert len(run.results) == len(run.bytes) == P.STEPS and len(run.frames) == len(CHECKPOINTS)


# the bound and the taint cap of tests/test_gpu_labels.py::test_frame_matches_the_float64_restatement, and its floor for what must show
RESTATEMENT_BOUND, TAINT_CAP, SHOWN_FLOOR, SHOWN_BY = 5e-4, 0.2, 50, 1e-3


@pytest.mark.parametrize("seed", [1, 2], ids=["u16", "f32"])
def test_final_frame_matches_the_float64_restatement(gpu, seed):
    su, steps, trace = P.sequence(seed)
    assert su["dtype"] == {1: "uint16", 2: "float32"}[seed]
    (_, _, _, light), got = walk(su, steps, trace, check=False, light32=True)
    last = trace[-1]
    ex = X.Scene(last.vol, abi.host_bake_tf_lut(abi.color_curve_to_lut(S.tf_keys("A"))), abi.WindowingParams(*WINDOW), su["dims"], False)
    ex.set_light(light)
    ref, taint = LR.raymarch_lit(ex, last.labels, last.colors, CAM, TILE, STEPS, JITTER, WORLD)
    nolab, _ = X.raymarch_lit(ex, CAM, TILE, STEPS, JITTER, WORLD)
    d = np.abs(got.astype(np.float64) - ref)[~taint]
    shown = int((np.abs(ref - nolab).max(axis=-1)[~taint] > SHOWN_BY).sum())
    print(f"seed {seed}: taint {taint.mean():.4f}, max untainted |d| {d.max():.3e}, pixels that show the labels {shown}")
    assert taint.mean() < TAINT_CAP, taint.mean()
    assert d.max() <= RESTATEMENT_BOUND, f"max untainted |d| {d.max()}"
    assert shown >= SHOWN_FLOOR, shown   # the edits are in the picture


@pytest.mark.parametrize("seed", [3, 4])
def test_test_hooks_change_nothing(gpu, tunables, seed):
    """one pass a read-back, one step a launch, no brick classes, three workgroups of statistics: the same results, bytes and frames"""
    want = default_run(seed)
    for name, value in HOOKS.items():
        assert abi.get_tunable(name) != value, name
        tunables(name, value)
    su, steps, trace = P.sequence(seed)
    got, _ = walk(su, steps, trace)
    for i, step in enumerate(steps):
        if "call" in step:
            for k in P.FIELDS[step["call"]]:   # (the fields leave out the launch counts and grow's passes)
                assert got.results[i][k] == want.results[i][k], (i, step, k)
        assert np.array_equal(got.bytes[i], want.bytes[i]), (i, step)
    assert len(got.frames) == len(want.frames) == len(CHECKPOINTS)
    for a, b in zip(got.frames, want.frames):
        assert np.array_equal(a, b)
    morphs = [(i, s["args"]) for i, s in enumerate(steps) if s.get("call") == "morph"]
    assert morphs and any(a["radius"] > 1 for _, a in morphs)
    for i, a in morphs:   # the hooks were in force: a launch a step
        assert got.results[i]["launches"] == MR.launches(a["op"], a["radius"], 1) and want.results[i]["launches"] == MR.launches(a["op"], a["radius"], 8)


# ---- fixed sequences ------------------------------------------------------------------------------------------------------------
def islands_step(source, **kw):
    args = dict(source=source, connectivity=6, max_islands=0, min_voxels=0, keep_label=-1, label_step=0, drop_label=-1, spare_border=False,
                measure=False, table=4)
    args.update(kw)
    return {"kind": "islands", "call": "islands", "args": args}


def test_release_and_attach_in_mid_pipeline(gpu):
    """grow, close, release and attach, grow elsewhere, close, keep the largest: the first label volume leaves nothing behind"""
    su = {"seed": 0, "dims": (40, 24, 19), "dtype": "uint16", "vol_seed": 0x5EED0002, "start": "empty", "reattach": True}
    vol = P.initial(su)[0]
    z, y, x = (int(v) for v in np.argwhere(vol >= np.percentile(vol, 75))[0])
    close = lambda label, radius, connectivity: {"kind": "morph", "call": "morph", "args": dict(op=MR.CLOSE, radius=radius, source=[label], new_label=label,
                                                                                               connectivity=connectivity)}
    steps = [P.grow_step(vol, 75, 100, 1, [(x, y, z)]), close(1, 2, 26), {"kind": "reattach"},
             P.grow_step(vol, 60, 70, 2, origin=(4, 3, 2), extent=(30, 18, 14)), close(2, 1, 6), islands_step([2], max_islands=1, drop_label=0)]
    trace = P.run(su, steps)
    assert trace[1].labels.any() and not trace[2].labels.any() and trace[2].colors[3, 3] == 1.0
    assert (trace[5].labels == 2).any() and not (trace[5].labels == 1).any() and all(a.result["relabelled"] > 0 for a in trace if a.result)
    with edited_handle(su) as res:
        light = res.download_light_volume()
        for i, (step, want) in enumerate(zip(steps[:3], trace[:3])):
            same_step(res, i, step, want, np.uint16)
        assert not res.label_statistics()["count"][1:].any()
        allocs = res.path_counters()["operator_alloc_calls"]
        for i in (3, 4):
            same_step(res, i, steps[i], trace[i], np.uint16)
        assert res.path_counters()["operator_alloc_calls"] == allocs   # the scratch outlives the label volume it worked on
        same_step(res, 5, steps[5], trace[5], np.uint16)
        seen = checkpoint(res, trace[5], light, su["dims"], steps)
        assert seen["statistics"]["count"][2] == trace[5].result["kept_voxels"] and seen["statistics"]["count"][1] == 0
        res.release_label_volume()
        plain = res.raymarch_lit(CAM, TILE, abi.RaymarchParams(STEPS, JITTER, True), WORLD)
        assert not np.array_equal(plain, seen["skipping on"])   # label 2 did show
    with data_handle(su["dims"], vol) as never:   # and without labels the handle shows what one shows that never had any
        never.upload_light_volume(light)
        assert np.array_equal(never.raymarch_lit(CAM, TILE, abi.RaymarchParams(STEPS, JITTER, True), WORLD), plain)


SMALL_BOX = dict(origin=(8, 8, 8), extent=(8, 8, 8))   # one brick
NOISE_DIMS = (40, 24, 19)


def noise_labels():
    """label 3 on a third of the voxels, 7 on half of the rest: a checkerboard-like noise, hundreds of islands; label 1 on a few"""
    labels = np.where(IR.noise_mask(NOISE_DIMS, 0.5, 8), 7, 0).astype(np.uint8)
    labels[IR.noise_mask(NOISE_DIMS, 0.35, 7)] = 3
    labels[IR.noise_mask(NOISE_DIMS, 0.02, 9)] = 1
    return labels


def label_handle(labels):
    res = abi.Resources(NOISE_DIMS, abi.FMT_G8, False, False, 0)
    res.upload_volume(np.zeros(NOISE_DIMS[::-1], dtype=np.uint8))   # the calls never read the data
    res.upload_label_volume(labels)
    return res


def test_scratch_grows_between_calls(gpu):
    """a one-brick box, the whole volume, the one-brick box again: the second call frees and takes a larger scratch, the third finds it"""
    labels = noise_labels()
    # the islands: their counters tell
    steps = [islands_step([3], max_islands=1, drop_label=0, **SMALL_BOX), islands_step([3], max_islands=40, keep_label=100, label_step=1, drop_label=9, table=50),
             islands_step([7, 9], min_voxels=3, drop_label=0, connectivity=26, **SMALL_BOX)]
    with label_handle(labels) as res:
        seen, after = [res.islands_counters()], labels
        for i, step in enumerate(steps):
            want = P.apply(step, None, after, None)
            same_step(res, i, step, want, np.uint8)
            assert want.result["relabelled"] > 0, (i, want.result)
            after = want.labels
            seen.append(res.islands_counters())
        assert seen[0]["scratch_allocations"] == 0 and seen[1]["scratch_allocations"] == 3 and seen[1]["scratch_bytes"] > 0
        assert seen[2]["scratch_allocations"] == 6 and seen[2]["scratch_bytes"] > seen[1]["scratch_bytes"], seen
        assert seen[3]["scratch_allocations"] == 6 and seen[3]["scratch_bytes"] == seen[2]["scratch_bytes"], seen
        assert seen[2]["islands_found"] - seen[1]["islands_found"] >= 100
    # the margins: the results tell, and the free memory that the third call leaves as it was
    margin = lambda op, limit, label, **kw: {"kind": "margin", "call": "margin", "args": dict(op=op, weights=P.ISO, limit=limit, source=[label], new_label=label, **kw)}
    steps = [margin(GM.CLOSE, 4, 3, **SMALL_BOX), margin(GM.OPEN, 9, 3, erase_label=5), margin(GM.EXPAND, 1, 5, writable=[3], **SMALL_BOX)]
    with label_handle(labels) as res:
        after = labels
        for i, step in enumerate(steps):
            if i == 2:
                torch.cuda.synchronize()
                free = torch.cuda.mem_get_info()[0]
            want = P.apply(step, None, after, None)
            same_step(res, i, step, want, np.uint8)
            assert want.result["relabelled"] > 0, (i, want.result)
            after = want.labels
        torch.cuda.synchronize()
        assert torch.cuda.mem_get_info()[0] == free
        assert res.margin_counters()["margin_calls"] == 3
    # the distance map: the same scratch, and the staging of the map behind it
    with label_handle(labels) as res:
        whole = GM.distance(labels == 1, P.ISO, 9)                   # to the few voxels of label 1
        inner = GM.distance(labels != 0, P.ANISO, 256 * 9, inside=True)   # from inside everything that has a label to the rest
        o, e = SMALL_BOX["origin"], SMALL_BOX["extent"]
        cut = lambda d: d[o[2]:o[2] + e[2], o[1]:o[1] + e[1], o[0]:o[0] + e[0]]
        assert ((whole != GM.FAR) & (whole != 0)).any() and (whole == GM.FAR).any() and ((inner != GM.FAR) & (inner != 0)).any()
        got = res.label_distance([1], P.ISO, 9, **SMALL_BOX)
        assert np.array_equal(got, cut(whole)), np.argwhere(got != cut(whole))[:5]
        got = res.label_distance([1], P.ISO, 9)
        assert np.array_equal(got, whole), np.argwhere(got != whole)[:5]
        got = res.label_distance([1, 3, 7], P.ANISO, 256 * 9, inside=True)
        assert np.array_equal(got, inner), np.argwhere(got != inner)[:5]
        torch.cuda.synchronize()
        free = torch.cuda.mem_get_info()[0]
        got = res.label_distance([1, 3, 7], P.ANISO, 256 * 9, inside=True, **SMALL_BOX)
        assert np.array_equal(got, cut(inner)), np.argwhere(got != cut(inner))[:5]
        torch.cuda.synchronize()
        assert torch.cuda.mem_get_info()[0] == free
        assert np.array_equal(res.download_label_volume(), labels) and res.margin_counters()["margin_calls"] == 4   # a map writes no label
