"""Conditions on the generator of tests/label_pipeline_reference.py, checked with the references alone: the GPU test that walks these
sequences (tests/test_gpu_label_pipeline.py) cannot pass on trivial ones."""
import collections

import numpy as np
import pytest

from tbraymarcherplugin_amd import abi, synthetic as S
import exact_reference as X
import label_margin_reference as GM
import label_morph_reference as MR
import label_pipeline_reference as P
import label_reference as LR


def changed(seed):
    """per step: did a label byte change?"""
    su, steps, trace = P.sequence(seed)
    before = P.initial(su)[1]
    out = []
    for a in trace:
        out.append(bool((a.labels != before).any()))
        before = a.labels
    return out


def calls(kind=None):
    """(seed, index, step, its call's name and arguments) of every operator call of the seed set, measuring ones included"""
    for seed in P.SEEDS:
        for i, step in enumerate(P.sequence(seed)[1]):
            if "call" in step and (kind is None or step["call"] == kind):
                yield seed, i, step, P.call_of(step)[1]


def test_the_same_seed_gives_the_same_steps():
    for seed in (0, 3, 7):
        su, steps, trace = P.generate(seed)
        su2, steps2, trace2 = P.sequence(seed)
        assert su == su2 and steps == steps2 and repr(steps) == repr(steps2)
        assert all(np.array_equal(a.labels, b.labels) for a, b in zip(trace, trace2))
    assert P.sequence(0)[1] != P.sequence(4)[1]


def test_the_interpreter_alone_gives_the_generators_trace():
    for seed in (1, 6):
        su, steps, trace = P.sequence(seed)
        again = P.run(su, steps)
        assert len(again) == len(trace) == P.STEPS
        for a, b in zip(again, trace):
            assert a.result == b.result and np.array_equal(a.labels, b.labels) and np.array_equal(a.vol, b.vol) and np.array_equal(a.colors, b.colors)


@pytest.mark.parametrize("seed", P.SEEDS)
def test_every_sequence(seed):
    su, steps, trace = P.sequence(seed)
    assert len(steps) == P.STEPS and all(s["kind"] in P.KINDS for s in steps)
    assert su["dims"] in P.SHAPES and trace[0].vol.dtype == np.dtype(su["dtype"])
    moved = changed(seed)
    assert sum(moved) >= 8, (moved, steps)
    last = trace[-1].labels
    assert (last == 0).any() and (last != 0).any()   # neither empty nor full
    # a colours or a data step between two label-writing steps
    writes = [i for i, m in enumerate(moved) if m]
    assert any(s["kind"] in ("colors", "data") and writes[0] < i < writes[-1] for i, s in enumerate(steps)), steps
    # a measuring step leaves every byte
    before = P.initial(su)[1]
    for step, a in zip(steps, trace):
        if step["kind"] == "measure":
            assert np.array_equal(a.labels, before) and a.result.get("relabelled", 0) == 0, step
        before = a.labels
    # the steps are what the operators accept: seeds inside the volume, boxes inside it
    for step in steps:
        if "origin" in step.get("args", step):
            o, e = step.get("args", step)["origin"], step.get("args", step)["extent"]
            assert all(0 <= o[c] and e[c] >= 1 and o[c] + e[c] <= su["dims"][c] for c in range(3)), step


def test_kinds_operations_and_connectivities_over_the_seed_set():
    kinds = collections.Counter(s["kind"] for seed in P.SEEDS for s in P.sequence(seed)[1])
    assert all(kinds[k] >= 3 for k in P.KINDS), kinds
    assert {a["op"] for _, _, _, a in calls("morph")} == set(MR.OPS)
    assert {a["op"] for _, _, _, a in calls("margin")} == set(GM.OPS)
    assert {s["mode"] for _, _, s, _ in calls("islands")} == set(P.ISLANDS_MODES)
    for kind in ("grow", "morph", "islands"):
        assert {a["connectivity"] for _, _, _, a in calls(kind)} == {6, 26}, kind
    # the writing calls alone do as much: a measuring call is no edit
    written = [(s, a) for _, _, s, a in calls() if s["kind"] != "measure"]
    assert {a["op"] for s, a in written if s["call"] == "morph"} == set(MR.OPS)
    assert {a["op"] for s, a in written if s["call"] == "margin"} == set(GM.OPS)
    assert {s["mode"] for s, a in written if s["call"] == "islands"} == set(P.ISLANDS_MODES)
    # more than one launch of the step kernel; a reach of two bricks either side; both weightings; the masks
    assert any(a["radius"] >= 9 for s, a in written if s["call"] == "morph")
    assert any(max(GM.reaches(a["weights"], a["limit"])) >= 9 for s, a in written if s["call"] == "margin")
    assert {a["weights"] for s, a in written if s["call"] == "margin"} == {P.ISO, P.ANISO}
    for kind in ("grow", "morph", "margin"):
        assert any("writable" in a for s, a in written if s["call"] == kind), kind
        assert any("extent" in a for s, a in written if s["call"] == kind) and any("extent" not in a for s, a in written if s["call"] == kind), kind
    grows = [a for s, a in written if s["call"] == "grow"]
    assert any(a.get("relative") for a in grows) and any(len(a["seeds"]) == 0 for a in grows) and any(len(a["seeds"]) > 1 for a in grows)
    assert {len(a["source"]) for s, a in written if s["call"] in ("morph", "margin")} == {1, 2}
    assert any(a["new_label"] in a["source"] for s, a in written if s["call"] == "morph") and any(a["new_label"] not in a["source"] for s, a in written if s["call"] == "morph")
    regions = [s for seed in P.SEEDS for s in P.sequence(seed)[1] if s["kind"] == "region"]
    assert any(not P.region_block(s).any() for s in regions) and any(P.region_block(s).any() for s in regions)
    assert {s["mode"] for seed in P.SEEDS for s in P.sequence(seed)[1] if s["kind"] == "data"} == {"empty", "fill"}
    assert {np.dtype(P.sequence(seed)[0]["dtype"]) for seed in P.SEEDS} == {np.dtype(t) for t in P.DTYPES}
    assert {P.sequence(seed)[0]["dims"] for seed in P.SEEDS} == set(P.SHAPES)
    assert {P.sequence(seed)[0]["start"] for seed in P.SEEDS} == {"empty", "blobs"}


def test_a_later_boxed_call_covers_more_bricks():
    """the scratch of the islands and of the margins only ever grows: a small box first, a larger one later"""
    grew = 0
    for seed in P.SEEDS:
        su, steps, _ = P.sequence(seed)
        for kind in ("islands", "margin"):
            boxed = [P.box_bricks(su["dims"], s["args"]["origin"], s["args"]["extent"]) for s in steps if s.get("call") == kind and "extent" in s["args"]]
            most = [max(boxed[:i]) for i in range(1, len(boxed))]
            if any(b > m for b, m in zip(boxed[1:], most)):
                grew += 1
                break
    assert 2 * grew >= len(P.SEEDS), grew


def test_colour_steps_show_a_present_label_and_data_steps_move_the_data():
    for seed in P.SEEDS:
        su, steps, trace = P.sequence(seed)
        vol = P.initial(su)[0]
        for step, a in zip(steps, trace):
            if step["kind"] == "colors":
                assert any(a.colors[l, 3] > 0 for l in P.present(a.labels)) and all(a.colors[l, 3] == 0 for l in step["clear"]), step
                assert a.colors.dtype == np.float32 and a.colors.min() >= 0.0 and a.colors.max() <= 1.0
            if step["kind"] == "data":
                assert not np.array_equal(a.vol, vol), step
            vol = a.vol


def test_the_edits_between_two_checkpoints_can_reach_the_picture():
    """necessary for the GPU test's "each checkpoint's frame differs from the one before": voxels that show another colour"""
    for seed in P.SEEDS:
        su, steps, trace = P.sequence(seed)
        views = [P.shown(trace[i].labels, trace[i].colors) for i in P.CHECKPOINTS]
        for a, b in zip(views, views[1:]):
            assert int((a != b).any(axis=-1).sum()) >= 2 * P.VISIBLE, (seed, steps)


def test_the_restated_frames_of_two_checkpoints_differ():
    """... and sufficient, up to the illumination (the label step is unlit): in the float64 restatement of the GPU test's frame, under a
    constant light, ten untainted pixels move by more than 2e-3 — four times the bound the GPU's frame is held to the restatement by"""
    cam, tile, world = S.default_camera(64, 48), abi.Tile(0, 0, 64, 48), S.default_world()
    tf = abi.host_bake_tf_lut(abi.color_curve_to_lut(S.tf_keys("A")))
    for seed in P.SEEDS:
        su, steps, trace = P.sequence(seed)
        frames = []
        for i in P.CHECKPOINTS:
            ex = X.Scene(trace[i].vol, tf, abi.WindowingParams(0.5, 0.9, True, False), su["dims"], False)
            ex.set_light(np.full(su["dims"][::-1], 0.6))
            frames.append(LR.raymarch_lit(ex, trace[i].labels, trace[i].colors, cam, tile, 100.0, 1, world))
        for (a, ta), (b, tb) in zip(frames, frames[1:]):
            moved = int((np.abs(a - b).max(axis=-1)[~ta & ~tb] > 2e-3).sum())
            assert moved >= 10, (seed, moved, steps)
