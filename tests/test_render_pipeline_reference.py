"""The sequences of tests/render_pipeline_reference.py without a GPU: the generator is deterministic and keeps its promises, and the
oracle's trace of a sequence is worth comparing with — every light operator moves the light volume, every setter reaches a result,
every frame shows something — and is the float64 restatement's (tests/exact_reference.py) at the end of a whole sequence."""
import numpy as np
import pytest

from tbraymarcherplugin_amd import abi
import exact_reference as X
import render_pipeline_reference as P
import test_exact_reference as TX

# UNORM8 light volumes, the two smallest shapes: the flat volume, and ragged last bricks. (The third sequence of these shapes, seed 3,
# leaves 6.1 % of the restatement's light volume tainted, above the 5 % it may mask: the restatement cannot judge it.)
EXACT_SEEDS = (4, 9)


def test_generator_is_deterministic():
    for seed in P.SEEDS:
        for attempt in (0, 3):
            a, b = P.draw(seed, attempt), P.draw(seed, attempt)
            assert repr(a) == repr(b), (seed, attempt)
    assert repr(P.draw(0, 0)[1]) != repr(P.draw(0, 1)[1]) and repr(P.draw(0, 0)[1]) != repr(P.draw(1, 0)[1])


@pytest.mark.parametrize("seed", P.SEEDS)
def test_first_draws_are_the_first_acceptable_ones(oracle_mod, seed):
    """the table that spares every process the rejected draws: a search from draw 0 ends where the table says"""
    for attempt in range(P.FIRST_DRAW[seed]):
        su, steps = P.draw(seed, attempt)
        if set(P.motifs(steps)) != P.motifs_of(steps) or not P.every_frame_shows(su, steps, oracle_mod):
            continue
        _, facts = P.examine(su, steps, oracle_mod, quick=True)
        assert facts is None or not P.acceptable(steps, facts), (seed, attempt)
    assert P.sequence(seed)[3]["attempts"] == P.FIRST_DRAW[seed] + 1, seed


def test_setups_cover_what_the_issue_lists():
    sus = [P.setup(s) for s in P.SEEDS]
    assert len(sus) == 12 and [su["dtype"] for su in sus] == ["uint8", "uint16", "float32"] * 4
    assert sum(su["light32"] for su in sus) == 2 and sum(su["addr"] == abi.ADDRESS_CLAMP for su in sus) == 2
    assert sum(su["border"] == abi.BORDER_EXACT_FLOAT for su in sus) == 1 and sum(su["rgb"] for su in sus) == 1
    assert sum(su["reserve"] for su in sus) == 1 and sum(su["many"] for su in sus) == 1 and sum(su["half"] for su in sus) == 2
    assert sum(su["dims"] == (104, 88, 72) for su in sus) == 1
    assert {su["dims"] for su in sus} == {(72, 64, 56), (67, 45, 53), (45, 40, 37), (33, 40, 17), (40, 40, 5), (104, 88, 72)}


@pytest.mark.parametrize("seed", P.SEEDS)
def test_sequence_keeps_the_generators_promises(oracle_mod, seed):
    su, steps, trace, facts = P.sequence(seed)
    assert len(steps) == len(trace) == P.STEPS and steps[-1]["kind"] == "frames"
    m = P.motifs(steps)
    assert set(m) == P.motifs_of(steps) == set(P.MOTIFS) | (set() if su["rgb"] else {"labelled"}), m
    if not su["rgb"]:   # a label volume attached, a frame, a setter, frames x 2 at least, released: the only span with labels
        i = m["labelled"]
        assert [s["kind"] for s in steps].count("labels") == 2 and steps[i - 3]["attach"] and not steps[i + 1]["attach"]
        assert steps[i - 2] == {"kind": "frames", "k": 1} and steps[i - 1]["kind"] == P.L_SETTERS[seed % 3] and steps[i]["k"] >= 2
        assert steps[i - 1]["kind"] != "region" or steps[i - 1]["boxes"][0][2] == "fill"
    # frames x 4, a light operator, frames x 1 with no label volume attached and no checkpoint's other views in between; then a
    # setter and frames x 1
    i = m["relit"]
    assert steps[i - 1] == {"kind": "frames", "k": 4} and steps[i]["kind"] in P.LIGHT_OPS and steps[i + 1] == {"kind": "frames", "k": 1}
    assert steps[i + 2]["kind"] != "region" or steps[i + 2]["size"] == "brick"
    assert i - 1 not in P.CHECKPOINTS and i not in P.CHECKPOINTS
    assert m["marched"] == i + 2 and steps[i + 2]["kind"] == P.SETTERS[seed % 4] and steps[i + 3]["kind"] == "frames"
    # change A -> B, change B -> A, a setter, change A -> B again
    i = m["both_sides"]
    assert steps[i]["new"] == steps[i - 1]["old"] and steps[i]["old"] == steps[i - 1]["new"] and steps[i]["old"] != steps[i]["new"]
    assert steps[i + 1]["kind"] == P.SETTERS[(seed + 1) % 4] and steps[i + 1].get("how") != "same"
    assert steps[i + 2]["kind"] == "change" and (steps[i + 2]["old"], steps[i + 2]["new"]) == (steps[i - 1]["old"], steps[i - 1]["new"])
    # an invalidating setter directly in front of an operator on a light that was there before it
    i = m["stale"]
    assert steps[i - 1]["kind"] in P.SETTERS and steps[i]["kind"] in ("remove", "change")
    # the lights a step names are the lights that are there
    present, attached, since_reset = [], False, 0
    for i, s in enumerate(steps):
        k = s["kind"]
        if k == "add":
            present.append(s["light"])
        elif k == "remove":
            assert s["light"] in present, (i, s)
            present.remove(s["light"])
        elif k == "change":
            assert s["old"] in present, (i, s)
            present[present.index(s["old"])] = s["new"]
        elif k == "batch":
            assert len(s["lights"]) == 3 and not su["rgb"]
            present += s["lights"]
        elif k == "reset":
            assert s["lights"] == present and present, (i, s)
        elif k == "labels":
            assert s["attach"] != attached and not su["rgb"], (i, s)
            attached = s["attach"]
        elif k == "region":
            for (x, y, z), (ex, ey, ez), _, _ in s["boxes"]:
                assert min(x, y, z) >= 0 and min(ex, ey, ez) >= 1 and x + ex <= su["dims"][0] and y + ey <= su["dims"][1] and z + ez <= su["dims"][2], (i, s)
        if k in P.LIGHT_OPS:
            since_reset = 0 if k == "reset" else since_reset + 1
            assert not su["light32"] or since_reset < 7, (i, "a float light volume, seven operators in a row")
        assert present or i == 0
    assert not attached   # released again: the last frames are held to the oracle
    assert su["many"] == any(len(s["boxes"]) > 64 for s in steps if s["kind"] == "region")
    kinds = {s["kind"] for s in steps}
    every = {"add", "change", "reset", "window", "tf", "region", "upload", "world", "cache_clear", "view", "frames", "modes"}
    assert kinds >= every - (set() if su["rgb"] else set(P.LEFT_OUT[seed % 4])), kinds   # (a mono seed leaves two singles out, in turn)
    assert su["rgb"] or kinds >= {"batch", "labels"}


@pytest.mark.parametrize("seed", P.SEEDS)
def test_the_oracles_trace_is_worth_comparing_with(oracle_mod, seed):
    su, steps, trace, facts = P.sequence(seed)
    again, facts2 = P.examine(su, steps, oracle_mod)   # (not the cached verdict: the sequence as it stands)
    assert P.acceptable(steps, facts2), (facts2, facts["attempts"])
    for i, moved in facts2["moved"].items():
        assert moved, (i, steps[i], "a light operator that leaves the light volume as it was")
    for i, reached in facts2["reached"].items():
        if steps[i].get("how") == "same":
            assert not reached, (i, steps[i], "the same window again changed a result")
        else:
            assert reached, (i, steps[i], "neither the next light operator nor the next frame notices this step")
    stale = P.motifs(steps)["both_sides"] + 1
    assert facts2["reached_light"][stale], (stale, steps[stale], "the change behind this setter comes out as without it")
    assert facts2["relit"] and all(facts2["relit"].values()), facts2["relit"]   # frames either side of a light operator differ
    assert min(facts2["shown"].values()) >= P.SHOWN_FLOOR, facts2["shown"]
    assert su["rgb"] or (facts2["labels_shown"] and min(facts2["labels_shown"].values()) >= P.SHOWN_FLOOR), facts2["labels_shown"]
    for a, b in zip(trace, again):
        for k in a:
            if k == "light":
                assert P.same_lights(a[k], b[k])
            elif k != "kind":
                assert np.array_equal(a[k], b[k])


def test_windows_of_every_kind_are_drawn():
    hows = {s["how"] for seed in P.SEEDS for s in P.sequence(seed)[1] if s["kind"] == "window"}
    assert hows == {"new", "same", "ulp", "cutoffs"}
    changes = {s["how"] for seed in P.SEEDS for s in P.sequence(seed)[1] if s["kind"] == "change"}
    assert changes == {"small", "across", "back"}
    regions = {(s["size"], b[2]) for seed in P.SEEDS for s in P.sequence(seed)[1] if s["kind"] == "region" for b in s["boxes"][:1]}
    assert {r[0] for r in regions} == {"brick", "few", "half", "many"} and {r[1] for r in regions} == {"empty", "fill", "window"}
    kinds = {s["kind"] for seed in P.SEEDS for s in P.sequence(seed)[1]}
    assert kinds == {"add", "remove", "change", "batch", "reset", "window", "tf", "region", "upload", "world", "cache_clear", "view", "frames", "modes", "labels"}
    assert {s["device"] for seed in P.SEEDS for s in P.sequence(seed)[1] if s["kind"] == "region"} == {False, True}
    assert {s["tf"] for seed in P.SEEDS for s in P.sequence(seed)[1] if s["kind"] == "tf"} == set(P.TFS)
    assert {s["world"] for seed in P.SEEDS for s in P.sequence(seed)[1] if s["kind"] == "world"} == {"rot", "clip"}   # (from the default world)


@pytest.mark.parametrize("seed", EXACT_SEEDS)
def test_final_state_matches_the_float64_restatement(oracle_mod, seed):
    """the whole sequence on exact_reference.Scene — the data writes, transfer functions and windows in between included — against
    the oracle's last light volume and last lit frame, under tests/test_exact_reference.py's bounds and taint caps"""
    su, steps, trace, _ = P.sequence(seed)
    assert not su["light32"] and not su["rgb"]
    vol = P.volume_of(su["dims"], su["dtype"], su["vol_seed"]).copy()
    st = P.State(su, oracle_mod)
    light_dims = st.orcs[0].light_dims
    ex = X.Scene(vol, st.orcs[0].tf, abi.WindowingParams(*su["window"]), light_dims, True, su["addr"], su["border"])
    tf, window, world, view = su["tf"], tuple(su["window"]), "default", 0
    for i, s in enumerate(steps):
        k, w = s["kind"], P.WORLDS[world]
        if k in ("add", "remove"):
            ex.add_dir_light(s["light"][0], s["light"][1], k == "add", w)
        elif k == "change":
            ex.change_dir_light(s["old"][:2], s["new"][:2], w)
        elif k == "batch":
            for la, pa, _, _ in P.plain_schedule(s["lights"], w, light_dims, su["border"]):
                ex.add_dir_light(s["lights"][la][0], s["lights"][la][1], True, w, only_pass=pa)
        elif k == "reset":
            ex.clear_light_volume(0.0)
            for l in s["lights"]:
                ex.add_dir_light(l[0], l[1], True, w)
        elif k == "window":
            window = tuple(s["window"])
            ex.windowing = abi.WindowingParams(*window)
        elif k == "tf":
            tf = s["tf"]
            ex.tf = np.asarray(oracle_mod.bake_tf(P.tf_lut(tf)), dtype=np.float64)
        elif k == "region":
            for box in s["boxes"]:
                (x, y, z), (bx, by, bz) = box[0], box[1]
                vol[z:z + bz, y:y + by, x:x + bx] = P.box_block(box, vol.dtype, window)
            ex.data = X.decode(vol)
        elif k == "upload":
            vol[...] = P.volume_of(su["dims"], su["dtype"], s["vol_seed"])
            ex.data = X.decode(vol)
        elif k == "world":
            world = s["world"]
        elif k == "view":
            view = s["view"]
    last_light = [e for e in trace if "light" in e][-1]["light"][0]
    assert ex.taint.mean() < TX.TAINT_CAP, ex.taint.mean()
    ok, worst, exact = TX.prop_compare(False, last_light.astype(np.float64), ex.light.astype(np.float64), ex.taint)
    print(f"seed {seed}: light volume: max untainted |d| {worst} codes, exact {exact:.4f}, tainted {ex.taint.mean():.4f}")
    assert ok, (worst, exact)
    # the last frame: the restatement lit by the oracle's light volume (exact_scenes.run_exact_ray: a frame is compared on an uploaded light volume)
    ex.set_light(last_light)
    cam, tile, rp, w = P.view_args(view, world)
    ref, taint = X.raymarch_lit(ex, cam, tile, rp.steps, rp.jitter_frame, w)
    assert steps[-1]["kind"] == "frames" and taint.mean() < TX.TAINT_CAP, taint.mean()
    d = TX.frame_delta(trace[-1]["frame"].astype(np.float64), ref, taint)
    tol = TX.RGBA_TOL_STEEP if tf in TX.STEEP_TFS else TX.RGBA_TOL
    print(f"seed {seed}: last frame: max untainted |d| {d:.3e} (bound {tol}), tainted {taint.mean():.4f}")
    assert d <= tol, d
    assert (trace[-1]["frame"][..., 3] > 0.05).mean() > 0.02
