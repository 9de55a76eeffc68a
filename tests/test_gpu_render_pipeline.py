"""Everything that changes or reads the render state, as a pipeline on ONE handle against the CPU oracle, call after call: the
sequences of tests/render_pipeline_reference.py. What a handle carries between calls on this side — the factor cache and the block
lists behind the light operators, the lazily refreshed skipping metadata and its dirty boxes, the view cache behind the lit frames,
the label overlay's merged emptiness, the octree's validity — is where a sequence can go wrong while every single-call test stays
green: a stale cache entry, a block list of an old emptiness, a frame relit from the records of an old window.

After every light operator the light volume is the oracle's (UNORM8: bit for bit; float: TIGHT_TOL). After every frames or modes
step the pictures are the oracle's within TIGHT_TOL, every one of the k frames is the same bits, and those are the bits of the first
frame of a fresh handle that was handed the state's bytes — so a counted, a recording and a relit frame equal a plain march that
never saw the sequence — while tbrm_view_cache_stats moves as include/tbrm_view_cache.h says. At the checkpoints the edited handle
shows what the fresh one shows in every render mode, in the skipping metadata and in a histogram, bit for bit."""
import collections
import time

import numpy as np
import pytest
import torch

from tbraymarcherplugin_amd import abi
import render_pipeline_reference as P
from test_gpu_parity import TIGHT_TOL, assert_light_equal

pytestmark = pytest.mark.gpu

N_RESERVED = 8   # lights a sequence holds at the most: two adds, a batch of three, and what the single operators add
SWITCHES = [("light_cache_mb", 0), ("light_cache_mb", 4), ("view_cache_mb", 0), ("occ_dual", 0), ("sweep_chain", 1), ("light_sweep", 0),
            ("force_slice_kernel", 1), ("ray_lanes", 4), ("ray_lanes", 8), ("ray_tables", 0)]
SWITCH_SEEDS = (0, 3, 4)   # UNORM8 light volumes: whole brick layers (the sweep), ragged bricks under clamp, a pass the sweep declines

Run = collections.namedtuple("Run", "lights frames schedules view light_cache paths regions seconds peak_cache_bytes")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def identical(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def make_handle(su):
    return abi.Resources(su["dims"], abi.DTYPE_FMT[np.dtype(su["dtype"])], su["light32"], su["half"], 0, su["addr"], su["border"], rgb=su["rgb"])


def hand_over(res, st):
    """the state's data, transfer function and window (and label volume, if one is attached)"""
    res.upload_volume(st.vol)
    res.set_tf_lut(P.tf_lut(st.tf))
    res.set_windowing(abi.WindowingParams(*st.window))
    if st.labels is not None:
        res.upload_label_volume(st.labels)
        res.set_label_colors(st.colors)


def download_lights(res, su):
    return [res.download_light_channel(c) for c in range(3)] if su["rgb"] else [res.download_light_volume()]


def fresh_handle(su, st, lights):
    """a handle that never saw the sequence: the same creation arguments, the state's bytes, the downloaded light volume"""
    res = make_handle(su)
    hand_over(res, st)
    if su["rgb"]:
        for c in range(3):
            res.upload_light_channel(c, lights[c])
    else:
        res.upload_light_volume(lights[0])
    return res


def device_frame(res, st, skipping=True):
    cam, tile, rp, world = P.view_args(st.view, st.world)
    out = torch.full((tile.h, tile.w, 4), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    res.raymarch_lit_device(cam, tile, abi.RaymarchParams(rp.steps, rp.jitter_frame, skipping), world, out.data_ptr())
    res.flush()
    return out.cpu().numpy()


def handle_light(l, rgb):
    return abi.ColorDirLight(*l) if rgb else P.mono_light(l)


class Walk:
    """one handle and the oracle's State side by side; step() runs a step on both and holds the handle to the oracle"""

    def __init__(self, su, oracle_mod, check=True):
        self.su, self.check, self.rgb = su, check, su["rgb"]
        self.st = P.State(su, oracle_mod)
        self.res = make_handle(su)
        hand_over(self.res, self.st)
        self.res.clear_light_volume(0.0)
        if su["reserve"]:
            self.res.reserve(N_RESERVED, 1)   # (flags bit 0: the chunked chain's stores too, for the passes the sweep declines)
        # the view cache as include/tbrm_view_cache.h states it: which counter the next lit frame moves
        self.view_key, self.view_state = None, 0
        self.data_ver = self.tf_ver = 0
        self.octree_ok = False
        self.operator_moves = collections.Counter()   # of a reserved handle: allocations and stream waits inside light operators
        self.fallbacks = self.labelled_frames = 0
        self.peak_cache_bytes = 0
        self.lights, self.frames, self.schedules = {}, {}, {}
        self.i = -1

    def close(self):
        self.res.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- lit frames, and how the view cache must have served them
    def expected_counter(self, skipping):
        takes_part = not self.rgb and self.st.labels is None and abi.get_tunable("view_cache_mb") > 0
        key = (self.st.view, skipping, self.st.world, self.st.window, self.data_ver, self.tf_ver)
        if not takes_part:
            self.view_state = 0
            return "plain"
        if self.view_state == 0 or key != self.view_key:
            self.view_key, self.view_state = key, 1
            return "plain"
        self.view_state = min(self.view_state + 1, 4)
        return ("counted", "filled", "relit")[self.view_state - 2]

    def lit(self, skipping=True, host=False):
        """a lit frame of the view in force; the view cache's counters move as the header says"""
        s0 = self.res.view_cache_stats()
        want = self.expected_counter(skipping)
        if host:
            cam, tile, rp, world = P.view_args(self.st.view, self.st.world)
            frame = self.res.raymarch_lit(cam, tile, abi.RaymarchParams(rp.steps, rp.jitter_frame, skipping), world)
        else:
            frame = device_frame(self.res, self.st, skipping)
        s1 = self.res.view_cache_stats()
        moved = {k: s1[k] - s0[k] for k in ("plain", "counted", "filled", "relit", "dropped")}
        expected = dict(plain=0, counted=0, filled=0, relit=0, dropped=0)
        if not self.rgb:   # (a colour handle takes no part: its frames are not counted at all)
            expected[want] = 1
        assert moved == expected, (self.i, want, moved, self.view_state)
        return frame

    # ---- the steps
    def on_handle(self, step):
        """the step on the handle -> the pass order a batch reports (None otherwise)"""
        res, st, kind = self.res, self.st, step["kind"]
        world = P.WORLDS[st.world]
        if kind in ("add", "remove"):
            (res.add_color_dir_light if self.rgb else res.add_dir_light)(handle_light(step["light"], self.rgb), kind == "add", world)
        elif kind == "change":
            (res.change_color_dir_light if self.rgb else res.change_dir_light)(handle_light(step["old"], self.rgb), handle_light(step["new"], self.rgb), world)
        elif kind == "batch":
            return res.add_dir_lights([P.mono_light(l) for l in step["lights"]], True, world)
        elif kind == "reset":
            res.clear_light_volume(0.0)
            for l in step["lights"]:
                (res.add_color_dir_light if self.rgb else res.add_dir_light)(handle_light(l, self.rgb), True, world)
        elif kind == "window":
            res.set_windowing(abi.WindowingParams(*step["window"]))
        elif kind == "tf":
            res.set_tf_lut(P.tf_lut(step["tf"]))
            self.tf_ver += 1
        elif kind == "region":
            for box in step["boxes"]:
                block = P.box_block(box, st.vol.dtype, st.window)
                if step["device"]:
                    t = torch.from_numpy(np.ascontiguousarray(block).view(np.uint8).reshape(-1).copy()).cuda()
                    torch.cuda.synchronize()
                    res.update_volume_region_device(box[0], block.shape[::-1], t.data_ptr(), block.nbytes)
                    res.flush()
                else:
                    res.update_volume_region(box[0], block)
            self.data_ver += 1
            self.octree_ok = False
        elif kind == "upload":
            res.upload_volume(P.volume_of(self.su["dims"], self.su["dtype"], step["vol_seed"]))
            self.data_ver += 1
            self.octree_ok = False
        elif kind == "cache_clear":
            res.light_cache_clear()
            assert res.light_cache_stats()["entries"] == 0
        elif kind == "labels":
            if step["attach"]:
                res.upload_label_volume(P.label_volume(self.su["dims"], step["seed"]))
                res.set_label_colors(P.label_colors(step["seed"]))
            else:
                res.release_label_volume()
            assert res.has_label_volume() == step["attach"]
        return None

    def step(self, step):
        self.i += 1
        i, res, st, kind = self.i, self.res, self.st, step["kind"]
        where = (self.su["seed"], i, step)
        before = res.path_counters() if kind in P.LIGHT_OPS else None
        cache0 = res.light_cache_stats() if kind == "window" else None
        regions0 = res.volume_region_counters() if kind == "region" and len(step["boxes"]) > 64 else None
        schedule = self.on_handle(step)
        if before is not None:
            after = res.path_counters()
            for k in ("operator_alloc_calls", "operator_host_syncs"):
                self.operator_moves[k] += after[k] - before[k]
            self.peak_cache_bytes = max(self.peak_cache_bytes, res.light_cache_stats()["bytes"])
        entry = st.apply(step, schedule)
        if kind in P.LIGHT_OPS:
            if self.rgb:
                for c in range(3):   # every channel: an oracle scene of its own with intensity x colour
                    got = res.download_light_channel(c)
                    assert np.array_equal(got, entry["light"][c]), (where, c, int((got != entry["light"][c]).sum()))
            else:
                assert_light_equal(res, st.orcs[0])
            self.lights[i] = download_lights(res, self.su)
            self.schedules[i] = schedule
        elif kind == "window" and step["how"] == "same":   # the same window again: nothing cached is dropped
            cache1 = res.light_cache_stats()
            assert cache1["entries"] == cache0["entries"] and cache1["bytes"] == cache0["bytes"], (where, cache0, cache1)
        elif kind == "region" and regions0 is not None:   # more boxes than a handle tracks: the whole grid, once
            res.skipping_digest()
            regions1 = res.volume_region_counters()
            assert regions1["updates"] - regions0["updates"] == len(step["boxes"]), where
            assert regions1["minmax_rebuilds"] - regions0["minmax_rebuilds"] == 1 and regions1["bricks_refreshed"] == regions0["bricks_refreshed"], (where, regions0, regions1)
            self.fallbacks += 1
        elif kind == "frames":
            frames = [self.lit() for _ in range(step["k"])]
            for f in frames[1:]:
                assert np.array_equal(bits(f), bits(frames[0])), where
            cam, tile, rp, world = P.view_args(st.view, st.world)
            assert res.count_nominal_samples(cam, tile, rp, world) == entry["count"], where   # (nominal: labels or not)
            if st.labels is None:
                worst = float(np.abs(frames[0] - entry["frame"]).max())
                assert worst <= TIGHT_TOL, (where, worst)
            else:   # the attach was no empty gesture: the picture is not the one the oracle draws without labels
                shown = int((np.abs(frames[0] - entry["frame"]).max(axis=-1) > P.LABELS_SHOW_BY).sum())
                assert shown >= P.SHOWN_FLOOR, (where, shown)
                self.labelled_frames += step["k"]
            if self.check:
                with fresh_handle(self.su, st, download_lights(res, self.su)) as fresh:
                    want = device_frame(fresh, st)
                assert np.array_equal(bits(frames[0]), bits(want)), (where, int((bits(frames[0]) != bits(want)).sum()))
            self.frames[i] = frames[0]
        elif kind == "modes":
            cam, tile, rp, world = P.view_args(st.view, st.world)
            if not self.octree_ok:   # no level of an octree that a data write has outdated (or that nobody generated) is marched
                with pytest.raises(abi.TbrmError) as e:
                    res.raymarch_octree(cam, tile, rp, world, step["mip"])
                assert e.value.code == abi.ERR_NOT_INITIALIZED, where
            res.generate_octree()
            self.octree_ok = True
            got = {"intensity": res.raymarch_intensity(cam, tile, rp, world), "octree": res.raymarch_octree(cam, tile, rp, world, step["mip"])}
            got_hits = res.raymarch_hits(cam, tile, rp, world, P.HIT_THRESHOLD)
            assert got_hits.shape == (tile.h, tile.w)
            assert res.count_nominal_samples(cam, tile, rp, world) == entry["count"], where
            if st.labels is None:
                for k in got:
                    worst = float(np.abs(got[k] - entry[k]).max())
                    assert worst <= TIGHT_TOL, (where, k, worst)
            if self.check:   # labels or not: the modes and the hit records of a handle that never saw the sequence, bit for bit
                with fresh_handle(self.su, st, download_lights(res, self.su)) as fresh:
                    fresh.generate_octree()
                    want = {"intensity": fresh.raymarch_intensity(cam, tile, rp, world), "octree": fresh.raymarch_octree(cam, tile, rp, world, step["mip"])}
                    want_hits = fresh.raymarch_hits(cam, tile, rp, world, P.HIT_THRESHOLD)
                for k in got:
                    assert identical(got[k], want[k]), (where, k)
                assert identical(got_hits, want_hits), (where, "hits")
            self.frames[i] = got["octree"]
        if self.check and i in P.CHECKPOINTS:
            self.checkpoint(where)
        return entry

    def views(self, res, lit):
        """everything that reads the state: the four render modes, the skipping metadata, a histogram"""
        cam, tile, rp, world = P.view_args(self.st.view, self.st.world)
        out = {"skipping on": lit(True), "skipping off": lit(False)}
        out["hits"] = res.raymarch_hits(cam, tile, rp, world, P.HIT_THRESHOLD)
        out["intensity"] = res.raymarch_intensity(cam, tile, rp, world)
        res.generate_octree()
        out["octree"] = res.raymarch_octree(cam, tile, rp, world, 1)
        out["skipping digest"] = np.array(res.skipping_digest(), dtype=np.uint64)
        counts, tally = res.volume_histogram(32, 0, P.top_of(self.su["dtype"]))
        out["histogram"] = counts
        out["histogram's tallies"] = np.array([tally[k] for k in abi.Resources.HISTOGRAM_TALLY], dtype=np.uint64)
        return out

    def checkpoint(self, where):
        """the edited handle against a fresh one with the same bytes, bit for bit"""
        seen = self.views(self.res, lambda skipping: self.lit(skipping, host=True))
        self.octree_ok = True
        with fresh_handle(self.su, self.st, download_lights(self.res, self.su)) as fresh:
            cam, tile, rp, world = P.view_args(self.st.view, self.st.world)
            want = self.views(fresh, lambda skipping: fresh.raymarch_lit(cam, tile, abi.RaymarchParams(rp.steps, rp.jitter_frame, skipping), world))
        for k in want:
            assert identical(seen[k], want[k]), (where, k, int((seen[k].view(np.uint8) != want[k].view(np.uint8)).sum()) if seen[k].shape == want[k].shape else None)
        assert np.array_equal(bits(seen["skipping on"]), bits(seen["skipping off"])), where


def walk(su, steps, oracle_mod, check=True):
    """the sequence on one handle -> Run; every step is held to the oracle, check: and to fresh handles"""
    t0 = time.perf_counter()
    with Walk(su, oracle_mod, check) as w:
        for step in steps:
            w.step(step)
        res = w.res
        run = Run(w.lights, w.frames, w.schedules, res.view_cache_stats(), res.light_cache_stats(), res.path_counters(), res.volume_region_counters(),
                  time.perf_counter() - t0, w.peak_cache_bytes)
        if su["reserve"]:   # tests/test_gpu_reserve.py's promise, of every operator: nothing allocated, no stream waited for
            assert w.operator_moves["operator_alloc_calls"] == 0 and w.operator_moves["operator_host_syncs"] == 0, dict(w.operator_moves)
        assert su["rgb"] or w.labelled_frames >= 2   # a setter under an attached label volume, and frames behind it
        assert w.fallbacks == int(su["many"])
    return run


DEFAULT_RUNS = {}


def default_run(seed, oracle_mod):
    """the seed's sequence at the library's default tunables, walked once a process"""
    if seed not in DEFAULT_RUNS:
        su, steps, _, _ = P.sequence(seed)
        DEFAULT_RUNS[seed] = walk(su, steps, oracle_mod)
        r = DEFAULT_RUNS[seed]
        print(f"seed {seed}: {su['dims']} {su['dtype']} light {'f32' if su['light32'] else 'u8'}{' half' if su['half'] else ''}{' rgb' if su['rgb'] else ''}"
              f"{' reserved' if su['reserve'] else ''}: {' '.join(s['kind'] for s in steps)}: relit {r.view['relit']} hits {r.light_cache['hits']} "
              f"sweep {r.paths['passes_sweep']} chain {r.paths['passes_chain']} slice {r.paths['passes_slice']} bricks refreshed {r.regions['bricks_refreshed']} "
              f"whole-grid rebuilds {r.regions['minmax_rebuilds']}: {r.seconds:.2f} s")
    return DEFAULT_RUNS[seed]


# ---- random sequences -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", P.SEEDS)
def test_random_sequences(gpu, oracle_mod, seed):
    su, steps, _, _ = P.sequence(seed)
    run = default_run(seed, oracle_mod)
    assert len(run.lights) == sum(s["kind"] in P.LIGHT_OPS for s in steps) and len(run.frames) == sum(s["kind"] in ("frames", "modes") for s in steps)
    # the states were reached
    if su["rgb"]:
        assert run.view["relit"] == run.view["counted"] == run.view["filled"] == 0
    else:
        assert run.view["relit"] >= 1, run.view            # frames x 4, a light operator, frames x 1
    if not su["light32"]:
        assert run.light_cache["hits"] >= 2, run.light_cache   # change A -> B, change B -> A


def test_the_states_were_reached(gpu, oracle_mod):
    """over all seeds: the sweep and a path beside it, region updates refreshed brick by brick and once over the whole grid"""
    runs = [default_run(seed, oracle_mod) for seed in P.SEEDS]
    assert sum(r.paths["passes_sweep"] for r in runs) > 0
    assert sum(r.paths["passes_chain"] + r.paths["passes_slice"] for r in runs) > 0
    assert sum(r.regions["bricks_refreshed"] for r in runs) > 0
    many = [r for seed, r in zip(P.SEEDS, runs) if P.setup(seed)["many"]]
    assert len(many) == 1 and many[0].regions["updates"] > P.MANY_BOXES


@pytest.mark.parametrize("switch", SWITCHES, ids=["%s=%d" % s for s in SWITCHES])
@pytest.mark.parametrize("seed", SWITCH_SEEDS)
def test_switches_change_nothing(gpu, oracle_mod, tunables, seed, switch):
    """every step held to the oracle as before; UNORM8 light volumes and frames are the default walk's, bit for bit (a batch whose
    passes the switch pairs otherwise is the oracle's replay of its own order: pairing moves rounding ties by a code,
    test_batched_lights_match_oracle_replay — from there on the oracle alone holds the light volume)"""
    su, steps, _, _ = P.sequence(seed)
    assert not su["light32"] and not su["rgb"]
    want = default_run(seed, oracle_mod)
    name, value = switch
    assert abi.get_tunable(name) != value, name
    tunables(name, value)
    got = walk(su, steps, oracle_mod, check=False)
    same_order = True
    for i in sorted(want.lights):
        same_order = same_order and got.schedules[i] == want.schedules[i]
        if same_order:
            assert np.array_equal(got.lights[i][0], want.lights[i][0]), (seed, switch, i, steps[i])
    for i in sorted(want.frames):
        if same_order or i < min(j for j in want.schedules if got.schedules[j] != want.schedules[j]):
            assert np.array_equal(bits(got.frames[i]), bits(want.frames[i])), (seed, switch, i, steps[i])
    if name == "light_cache_mb" and value == 4 and seed == 0:   # the budget binds: what the default walk kept at once does not fit
        assert want.peak_cache_bytes > 4 << 20 >= got.peak_cache_bytes > 0, (want.peak_cache_bytes, got.peak_cache_bytes)
    if name == "light_cache_mb" and value == 0:
        assert got.light_cache["hits"] == 0 and got.light_cache["entries"] == 0
    if name == "view_cache_mb":
        assert got.view["relit"] == 0 and want.view["relit"] >= 1
    if name == "force_slice_kernel":
        assert got.paths["passes_slice"] > 0 and got.paths["passes_sweep"] == 0, got.paths
    if name == "light_sweep":
        assert got.paths["passes_sweep"] == 0, got.paths


# ---- a fixed sequence -----------------------------------------------------------------------------------------------------------
def moved(after, before):
    return {k: after[k] - before[k] for k in ("plain", "counted", "filled", "relit")}


def test_emptied_bricks_labels_and_a_window_in_mid_pipeline(gpu, oracle_mod):
    """two lights, four frames (the fourth relit); the bricks one light's occlusion was opaque in are emptied: the next frame is
    marched, not relit; a light turned there, back and there again (at last both sides kept); labels attached and a new window: two plain frames, the
    fresh handle's; labels released: four frames reach relit again"""
    su = dict(P.setup(0), seed=100, dims=(72, 64, 56), dtype="uint16", many=False)
    vol = P.volume_of(su["dims"], su["dtype"], su["vol_seed"])
    dense = np.argwhere(vol > 0.7 * 65535)
    assert len(dense) > 100
    lo, hi = dense.min(axis=0) // 8 * 8, np.minimum((dense.max(axis=0) // 8 + 1) * 8, vol.shape)   # (z, y, x): the bricks that hold the dense voxels
    origin, extent = tuple(int(v) for v in lo[::-1]), tuple(int(v) for v in (hi - lo)[::-1])
    a, b = ((1.0, .35, -.5), 0.5), ((-.4, 1.0, -.3), 0.4)
    b_turned = (tuple(float(v) for v in P.S.rotate_z(b[0], 5.0)), 0.4)
    steps = [{"kind": "view", "view": 1}, {"kind": "add", "light": a}, {"kind": "add", "light": b}, {"kind": "frames", "k": 4},
             {"kind": "region", "size": "few", "boxes": [(origin, extent, "empty", 0)], "device": False}, {"kind": "frames", "k": 1},
             {"kind": "change", "old": b, "new": b_turned, "how": "small"}, {"kind": "change", "old": b_turned, "new": b, "how": "back"},
             {"kind": "change", "old": b, "new": b_turned, "how": "back"}, {"kind": "labels", "attach": True, "seed": 5}, {"kind": "window", "window": P.WINDOWS[1], "how": "new"}, {"kind": "frames", "k": 2},
             {"kind": "labels", "attach": False, "seed": 5}, {"kind": "frames", "k": 4}]
    with Walk(su, oracle_mod) as w:
        stats = [w.res.view_cache_stats()]
        cache = []
        entries = []
        for step in steps:
            entries.append(w.step(step))
            stats.append(w.res.view_cache_stats())
            cache.append(w.res.light_cache_stats())
        at = lambda i: moved(stats[i + 1], stats[i])
        assert at(3) == dict(plain=1, counted=1, filled=1, relit=1)
        assert at(5) == dict(plain=1, counted=0, filled=0, relit=0)                     # new voxels: marched
        assert not np.array_equal(w.frames[3], w.frames[5])                              # (the emptied bricks did show)
        assert (entries[3]["frame"][..., 3] > 0).sum() >= 100 and (entries[5]["frame"][..., 3] > 0).sum() >= P.SHOWN_FLOOR
        n_b = abi.host_light_passes(P.mono_light(b), P.WORLDS["default"], su["dims"])[1]
        # there (new voxels: both lights' occlusion computed, the added light's kept), back (the removed light's at hand), there again
        # (both at hand: nothing computed)
        assert cache[6]["hits"] == cache[5]["hits"], (cache[5], cache[6])
        assert cache[7]["hits"] - cache[6]["hits"] == n_b, (cache[6], cache[7])
        assert cache[8]["hits"] - cache[7]["hits"] == 2 * n_b and cache[8]["propagated"] == cache[7]["propagated"], (cache[7], cache[8])
        assert at(11) == dict(plain=2, counted=0, filled=0, relit=0)                    # a label volume: every frame marched
        assert not np.array_equal(w.frames[11], w.frames[5])
        assert at(13) == dict(plain=1, counted=1, filled=1, relit=1)                    # released: relit again
        assert w.res.view_cache_stats()["relit"] == 2
