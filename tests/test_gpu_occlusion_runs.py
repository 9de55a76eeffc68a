"""The run form of the dual occlusion launch (k_light_occlusion_runs, tunable occ_run): a workgroup takes up to occ_run z-adjacent
live units of one column and sets up once what they share. Units, staging, ranks, factor layout and every voxel's arithmetic are
the per-unit form's, so the light volume must be the same BYTES for every occ_run (1 = the per-unit form) and the oracle's for the
default. tbrm_path_counters [15] counts the units that ran behind the first of their run: checked against the run list this file
cuts in numpy from the data (the flags of k_occ_flags / k_unit_flags, re-derived with their float32 sequence).

Shapes: 48 x 40 x 72 (9 unit layers, three tiles in x, a ragged last tile in y) and 48 x 40 x 68 (a last unit of four slices); the
data are zero (below the window's low cut-off: empty bricks) but for three boxes in the middle column. Units whose taps leave the
volume are never flagged, so the columns on the sides a light's taps lean to are live over all z (cut 4 + 4 + 1, or 2 + 2 + 2 + 2 + 1),
the others hold the boxes' stretches (2, 3, 5, 6, 7, 8 units, depending on the light) or nothing but the layer at the z border: under
that rule no column can be empty over all z, and slabs of zeros leave no stretch of one unit (a pass along x or y has blocks 16 deep in
z, so units come alive in pairs) — the run lengths 1 .. 4 come from cutting the stretches. A third shape, 16 x 16 x 600, has 75 unit
layers: the second 64-bit liveness word of k_occ_runs, and a stretch that is cut where it crosses unit layer 64."""
import math

import numpy as np
import pytest

from tbraymarcherplugin_amd import abi, synthetic as S

gpu_test = pytest.mark.gpu  # (test_the_data_leave_runs_of_every_length needs no device)

DIMS = [(48, 40, 72), (48, 40, 68)]
TALL = (16, 16, 600)  # one column of 75 unit layers
TALL_LIGHTS = [(1, 0.5, 0.01), (-0.5, 1, -0.01), (0.7, 1, 0.005)]  # (passes along x and y: both sweeps there, so one dual launch)
RUNS = (1, 2, 4, 64)
# both loop directions and every pair of pass axes
LIGHTS = [(0.3, 0.2, -1), (-0.3, 0.2, 1), (1, 0.35, -0.5), (-0.4, 1, -0.3), (-1, -0.6, 0.4)]
WINDOW = (0.5, 0.9, True, False)  # low cut-off at 0.05: a value of 0 is cut, a brick of zeros is empty
# live boxes, in voxels (x0, x1, y0, y1, z0, z1): all in the middle column of units, in single bricks of it, so that which of
# the neighbouring columns they reach depends on the side a light's taps lean to
BOXES = [
    (17, 23, 17, 31, 26, 29),
    (25, 31, 17, 23, 50, 53),
    (17, 31, 25, 31, 60, 62),
]


def make_volume(dims, dtype):
    nx, ny, nz = dims
    rng = np.random.default_rng(0x5EED0B00 + nz)
    v = np.zeros((nz, ny, nx), np.float32)
    for x0, x1, y0, y1, z0, z1 in BOXES if dims != TALL else [(3, 13, 3, 13, 20, 590)]:
        v[z0:z1, y0:y1, x0:x1] = 0.25 + 0.5 * rng.random((z1 - z0, y1 - y0, x1 - x0), dtype=np.float32)
    if dtype == np.float32:
        return v
    top = 255 if dtype == np.uint8 else 65535
    return np.round(v * top).astype(dtype)


# ---- the run list, in numpy ----------------------------------------------------------------------------------------------------

def _base_tap(pos, lv, off, dn):
    """texel_split's lower tap of light-volume position pos (k_occ_flags: float32, one operation at a time)"""
    cc = np.float32(np.float32(np.float32(pos) + np.float32(0.5)) / np.float32(lv)) + np.float32(off)
    x = np.float32(np.float32(cc * np.float32(dn)) - np.float32(0.5))
    return int(math.floor(float(x)))


def _empty_bricks(vol):
    """k_brick_minmax + k_brick_empty for data that are zero or well inside the window: a brick is empty when it and its +1 apron
    (wrap addressing) hold zeros only"""
    nz, ny, nx = vol.shape
    live = vol != 0
    out = np.zeros(((nz + 7) // 8, (ny + 7) // 8, (nx + 7) // 8), bool)
    for bz in range(out.shape[0]):
        for by in range(out.shape[1]):
            for bx in range(out.shape[2]):
                zi = [z % nz for z in range(8 * bz, min(8 * bz + 8, nz) + 1)]
                yi = [y % ny for y in range(8 * by, min(8 * by + 8, ny) + 1)]
                xi = [x % nx for x in range(8 * bx, min(8 * bx + 8, nx) + 1)]
                out[bz, by, bx] = not live[np.ix_(zi, yi, xi)].any()
    return out


def _pass_flags(p, dims, empty):
    """k_occ_flags of a sweep pass of an Add (one stream): flagged[slice group][block row][block column]"""
    a = p.axis
    du, dv = (1 if a == 0 else 0), (1 if a == 2 else 2)
    depth = (dims[a] + 7) // 8 * 8  # (the pass runs over whole brick layers)
    start = 0 if p.dir > 0 else depth - 1
    w, h = dims[du], dims[dv]
    flags = np.zeros((depth // 8, (h + 15) // 16, (w + 15) // 16), bool)
    for g in range(flags.shape[0]):
        for by in range(flags.shape[1]):
            for bx in range(flags.shape[2]):
                j0 = start + 8 * g * p.dir
                ends = {du: (16 * bx, min(16 * bx + 16, w) - 1), dv: (16 * by, min(16 * by + 16, h) - 1), a: (j0, j0 + 7 * p.dir)}
                ok, rng = True, [None] * 3
                for d in range(3):
                    taps = [_base_tap(e, dims[d], p.uvw_offset[d], dims[d]) for e in ends[d]]
                    lo, hi = min(taps), max(taps) + 1
                    ok = ok and lo >= 0 and hi < dims[d]  # (a block with taps outside the volume is never flagged)
                    rng[d] = (max(lo >> 3, 0), min(hi >> 3, empty.shape[2 - d] - 1))
                if ok:
                    flags[g, by, bx] = empty[rng[2][0]:rng[2][1] + 1, rng[1][0]:rng[1][1] + 1, rng[0][0]:rng[0][1] + 1].all()
    return flags


def live_units(vol, dims, light, world):
    """k_unit_flags of the dual launch of AddDirLight(light): live[unit layer][unit row][unit column]; None: no dual launch"""
    passes, n = abi.host_light_passes(light, world, dims)
    if n != 2:
        return None
    empty = _empty_bricks(vol)
    flags = [_pass_flags(p, dims, empty) for p in passes]
    live = np.zeros(((dims[2] + 7) // 8, (dims[1] + 15) // 16, (dims[0] + 15) // 16), bool)
    for gz, gy, gx in np.ndindex(live.shape):
        all_flagged = True
        for p, f in zip(passes, flags):
            depth = (dims[p.axis] + 7) // 8 * 8
            start = 0 if p.dir > 0 else depth - 1
            for half in range(1 if p.axis == 2 else 2):
                pos = [16 * gx, 16 * gy, 8 * gz]
                pos[p.axis] += 8 * half
                if pos[p.axis] >= dims[p.axis]:
                    continue
                pu, pv = (pos[1] if p.axis == 0 else pos[0]), (pos[1] if p.axis == 2 else pos[2])
                ks = (pos[p.axis] - start) * p.dir
                all_flagged = all_flagged and f[ks >> 3, pv >> 4, pu >> 4]
        live[gz, gy, gx] = not all_flagged
    return live


def stretches(live):
    """lengths of the stretches of z-adjacent live units, column by column (a stretch ends at every multiple of 64 unit layers: runs
    do not cross them)"""
    out = []
    for gy, gx in np.ndindex(live.shape[1:]):
        n = 0
        for gz in range(live.shape[0] + 1):
            if n and gz % 64 == 0:
                out.append(n)
                n = 0
            if gz < live.shape[0] and live[gz, gy, gx]:
                n += 1
            elif n:
                out.append(n)
                n = 0
    return out


def followers(live, r):
    """units that are not the first of their run when stretches are cut into runs of r: live units - runs"""
    return sum(n - -(-n // r) for n in stretches(live))


# ---- scenes ------------------------------------------------------------------------------------------------------------------

def open_scene(dims, dtype, vol, world, reserve=True):
    res = abi.Resources(dims, abi.DTYPE_FMT[np.dtype(dtype)], False)
    res.upload_volume(vol)
    res.set_tf_lut(abi.color_curve_to_lut(S.TF_A_KEYS))
    res.set_windowing(abi.WindowingParams(*WINDOW))
    if reserve:
        res.reserve(len(LIGHTS))
    res.clear_light_volume(0.0)
    return res


def run_operators(res, world, orc=None, check=None):
    """Adds of every light, a Change by 5 degrees of each, a Change across a major axis, a removal; after every operator
    check(name) (the light volume against the oracle's)"""
    def both(name, f):
        f(res)
        if orc is not None:
            f(orc)
            check(name)

    lights = [abi.DirLightParams(d, 0.35 + 0.05 * k) for k, d in enumerate(LIGHTS)]
    for k, l in enumerate(lights):
        both(f"add {k}", lambda t: t.add_dir_light(l, True, world))
    for k, l in enumerate(lights):
        new = abi.DirLightParams(S.rotate_z(LIGHTS[k], 5.0), l.light_intensity)
        both(f"change {k} by 5 degrees", lambda t: t.change_dir_light(l, new, world))
        lights[k] = new
    across = abi.DirLightParams((0.25, -0.3, 1), lights[0].light_intensity)  # light 0 leaves through the other z face: remove + add
    both("change across a major axis", lambda t: t.change_dir_light(lights[0], across, world))
    both("removal", lambda t: t.add_dir_light(lights[1], False, world))


COUNTERS_THAT_STAND = ("occlusion_single", "occlusion_dual", "occlusion_cached", "block_lists_built")


def test_the_data_leave_runs_of_every_length():
    """(no device: the numpy side alone) what this file's volumes are for"""
    world = S.default_world()
    for dims in DIMS:
        vol = make_volume(dims, np.uint16)
        seen, cut4 = set(), set()
        for d in LIGHTS:
            live = live_units(vol, dims, abi.DirLightParams(d, 0.4), world)
            assert live is not None, f"{d}: meant to have two passes"
            s = stretches(live)
            seen.update(s)
            cut4.update(min(4, n - o) for n in s for o in range(0, n, 4))
        assert live.shape[0] in seen, "a column that is live over all z"
        assert cut4 == {1, 2, 3, 4}, cut4
        assert len(seen) >= 5, seen


@gpu_test
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32])
@pytest.mark.parametrize("dims", DIMS)
def test_every_run_length_leaves_the_same_bytes_and_the_default_the_oracles(gpu, oracle_mod, tunables, dims, dtype):
    world = S.default_world()
    vol = make_volume(dims, dtype)
    orc = oracle_mod.OracleScene(vol, False)
    orc.set_tf_lut(abi.color_curve_to_lut(S.TF_A_KEYS))
    orc.set_windowing(abi.WindowingParams(*WINDOW))
    got, counters = {}, {}
    for r in RUNS:
        tunables("occ_run", r)
        with open_scene(dims, dtype, vol, world) as res:
            if r == 4:
                def check(name):
                    res.flush()
                    lv = res.download_light_volume()
                    assert np.array_equal(lv, orc.light), f"occ_run 4, {name}: {np.count_nonzero(lv != orc.light)} light voxels differ from the oracle"
                run_operators(res, world, orc, check)
            else:
                run_operators(res, world)
            res.flush()
            got[r] = res.download_light_volume()
            counters[r] = res.path_counters()
    for r in RUNS:
        assert got[r].tobytes() == got[1].tobytes(), f"occ_run {r}: {np.count_nonzero(got[r] != got[1])} light voxels differ from occ_run 1"
        for name in COUNTERS_THAT_STAND:
            assert counters[r][name] == counters[1][name], (r, name, counters[r], counters[1])
        assert (counters[r]["occlusion_units_in_runs"] > 0) == (r > 1), (r, counters[r])
    assert counters[1]["occlusion_dual"] > 0 and counters[1]["passes_chain"] == 0, counters[1]


@gpu_test
@pytest.mark.parametrize("dims", DIMS + [TALL])
@pytest.mark.parametrize("r", RUNS)
def test_units_in_runs_is_what_numpy_cuts_from_the_data(gpu, tunables, dims, r):
    world = S.default_world()
    vol = make_volume(dims, np.uint16)
    tunables("occ_run", r)
    with open_scene(dims, np.uint16, vol, world) as res:
        for d in (TALL_LIGHTS if dims == TALL else LIGHTS):
            light = abi.DirLightParams(d, 0.4)
            live = live_units(vol, dims, light, world)
            before = res.path_counters()
            res.add_dir_light(light, True, world)
            res.flush()  # (the counter never waits: exact once the run list has been cut on the device)
            after = res.path_counters()
            assert after["occlusion_dual"] - before["occlusion_dual"] == 1, (d, before, after)
            want = followers(live, r) if r > 1 else 0
            assert after["occlusion_units_in_runs"] - before["occlusion_units_in_runs"] == want, (d, r, stretches(live), before, after)
            if r > 1:
                assert want > 0


UNSTAGED_DIMS = (96, 80, 144)  # float32 data under a half-resolution light volume of 48 x 40 x 72: 3 x 3 x 9 units
UNSTAGED_BUDGET = 96 * 1024 // 2048  # bricks of 512 floats that the staging budget of 96 KiB holds


def unstaged_scene(world):
    """The first of LIGHTS whose two passes over the half-resolution light volume are both swept (one dual launch) and under which
    some unit of the middle column cannot be staged: its tap span crosses five bricks in x or y, which with three brick layers in z
    is 5 * 4 * 3 bricks of 2 KiB, more than the budget, while a unit of 4 * 4 * 3 bricks just fits. Returns (direction, brick
    counts of every unit [gz][gy][gx], widest x / y span of the middle column in bricks); None: no such light."""
    lv = tuple((d + 1) // 2 for d in UNSTAGED_DIMS)
    bn = [(d + 7) // 8 for d in UNSTAGED_DIMS]
    for d in LIGHTS:
        light = abi.DirLightParams(d, 0.4)
        plan = abi.host_plan_light(light, world, lv)
        if len(plan) != 2 or any(p[0] != 0 for p in plan):
            continue
        off = abi.host_light_passes(light, world, lv)[0][0].uvw_offset  # (the same for both passes of a light)

        def span(a, first, last):  # bricks the taps of positions first .. last touch along axis a, clamped to the grid
            taps = [_base_tap(e, lv[a], off[a], UNSTAGED_DIMS[a]) for e in (first, last)]
            return max(min((max(taps) + 1) >> 3, bn[a] - 1) - max(min(taps) >> 3, 0) + 1, 0)

        nx = [span(0, 16 * g, min(16 * g + 16, lv[0]) - 1) for g in range((lv[0] + 15) // 16)]
        ny = [span(1, 16 * g, min(16 * g + 16, lv[1]) - 1) for g in range((lv[1] + 15) // 16)]
        nz = [span(2, 8 * g, min(8 * g + 8, lv[2]) - 1) for g in range((lv[2] + 7) // 8)]
        counts = np.array([[[x * y * z for x in nx] for y in ny] for z in nz])
        if max(nx[1], ny[1]) >= 5 and counts[:, 1, 1].max() > UNSTAGED_BUDGET:
            return d, counts, max(nx[1], ny[1])
    return None


def test_the_unstaged_scene_holds_units_of_both_kinds():
    """(no device) the precondition of the "unstaged" case below"""
    found = unstaged_scene(S.default_world())
    assert found is not None, "no light of LIGHTS has two swept passes and a middle column that spans five bricks"
    _, counts, widest = found
    assert widest >= 5 and counts[:, 1, 1].max() >= 5 * 4 * 3 > UNSTAGED_BUDGET, (widest, counts[:, 1, 1])
    assert ((counts > 0) & (counts <= UNSTAGED_BUDGET)).any() and 4 * 4 * 3 <= UNSTAGED_BUDGET, counts


@gpu_test
@pytest.mark.parametrize("case", ["clip_plane", "cache_off", "not_reserved", "float_light_volume", "unstaged"])
def test_run_form_under_other_conditions(gpu, oracle_mod, tunables, case):
    """An active clip plane (the sample loop's other form), no factor cache (fused Changes: two streams per launch), a handle that
    was never reserved (its lists are allocated on the way), a float light volume (raw floats compared), units whose bricks do not fit
    the staging budget beside units whose bricks do (taps from global memory: unstaged_scene)."""
    if case == "unstaged":
        return run_form_with_unstaged_units(oracle_mod, tunables)
    dims, dtype = DIMS[0], np.uint16
    vol = make_volume(dims, dtype)
    world = S.default_world()
    if case == "clip_plane":
        tr = abi.identity_transform(scale=(100.0, 120.0, 80.0), translation=(10.0, -5.0, 3.0), rotation=(0.1305262, 0.0, 0.0, 0.9914449))
        world = abi.make_world(tr, clip_center=(12.0, -2.0, 5.0), clip_direction=(0.3, -0.2, 0.93))
    if case == "cache_off":
        tunables("light_cache_mb", 0)
    f32 = case == "float_light_volume"
    orc = oracle_mod.OracleScene(vol, f32)
    orc.set_tf_lut(abi.color_curve_to_lut(S.TF_A_KEYS))
    orc.set_windowing(abi.WindowingParams(*WINDOW))
    got = {}
    for r in RUNS:
        tunables("occ_run", r)
        with abi.Resources(dims, abi.FMT_G16, f32) as res:
            res.upload_volume(vol)
            res.set_tf_lut(abi.color_curve_to_lut(S.TF_A_KEYS))
            res.set_windowing(abi.WindowingParams(*WINDOW))
            if case != "not_reserved":
                res.reserve(len(LIGHTS))
            res.clear_light_volume(0.0)
            if r == 4 and not f32:
                def check(name):
                    res.flush()
                    lv = res.download_light_volume()
                    assert np.array_equal(lv, orc.light), f"{case}, occ_run 4, {name}: {np.count_nonzero(lv != orc.light)} light voxels differ from the oracle"
                run_operators(res, world, orc, check)
            else:
                run_operators(res, world)
            res.flush()
            got[r] = res.download_light_volume()
            c = res.path_counters()
            assert (c["occlusion_units_in_runs"] > 0) == (r > 1) and c["occlusion_dual"] > 0, (case, r, c)
    for r in RUNS:
        assert got[r].tobytes() == got[1].tobytes(), f"{case}, occ_run {r}: {np.count_nonzero(got[r] != got[1])} light voxels differ from occ_run 1"


def run_form_with_unstaged_units(oracle_mod, tunables):
    """An Add and a Change over dense float32 data of 96 x 80 x 144 under a half-resolution light volume: the same bytes for occ_run 1
    and 4, and the oracle's."""
    world = S.default_world()
    found = unstaged_scene(world)
    assert found is not None, "no light of LIGHTS has two swept passes and a middle column that spans five bricks"
    d, counts, widest = found
    assert widest >= 5 and counts[:, 1, 1].max() >= 5 * 4 * 3 > UNSTAGED_BUDGET, (widest, counts[:, 1, 1])
    assert ((counts > 0) & (counts <= UNSTAGED_BUDGET)).any(), counts
    vol = S.make_volume_numpy(UNSTAGED_DIMS, np.float32, 0x5EED0B14)
    light = abi.DirLightParams(d, 0.4)
    turned = abi.DirLightParams(S.rotate_z(d, 5.0), 0.4)
    orc = oracle_mod.OracleScene(vol, False, True)
    orc.set_tf_lut(abi.color_curve_to_lut(S.TF_A_KEYS))
    orc.set_windowing(abi.WindowingParams(*WINDOW))
    want = {}
    orc.add_dir_light(light, True, world)
    want["add"] = orc.light.copy()
    orc.change_dir_light(light, turned, world)
    want["change"] = orc.light.copy()
    got = {}
    for r in (1, 4):
        tunables("occ_run", r)
        with abi.Resources(UNSTAGED_DIMS, abi.DTYPE_FMT[np.dtype(np.float32)], False, True) as res:
            res.upload_volume(vol)
            res.set_tf_lut(abi.color_curve_to_lut(S.TF_A_KEYS))
            res.set_windowing(abi.WindowingParams(*WINDOW))
            res.reserve(2)
            res.clear_light_volume(0.0)
            res.add_dir_light(light, True, world)
            res.flush()
            got[r, "add"] = res.download_light_volume()
            res.change_dir_light(light, turned, world)
            res.flush()
            got[r, "change"] = res.download_light_volume()
            c = res.path_counters()
            assert c["occlusion_dual"] > 0 and (c["occlusion_units_in_runs"] > 0) == (r > 1), (r, c)
    for name in ("add", "change"):
        assert got[4, name].tobytes() == got[1, name].tobytes(), f"{name}: {np.count_nonzero(got[4, name] != got[1, name])} light voxels differ between occ_run 4 and 1"
        assert np.array_equal(got[4, name], want[name]), f"{name}: {np.count_nonzero(got[4, name] != want[name])} light voxels differ from the oracle"


@gpu_test
def test_a_reserved_handle_still_allocates_nothing_over_twenty_changes(gpu):
    dims = DIMS[0]
    vol = make_volume(dims, np.uint16)
    world = S.default_world()
    with open_scene(dims, np.uint16, vol, world) as res:
        lights = [abi.DirLightParams(d, 0.4) for d in LIGHTS[:4]]
        for l in lights:
            res.add_dir_light(l, True, world)
        res.flush()
        c0 = res.path_counters()
        angle = [0.0] * 4
        for k in range(20):
            i = k % 4
            angle[i] += 5.0
            new = abi.DirLightParams(S.rotate_z(LIGHTS[i], angle[i]), 0.4)
            res.change_dir_light(lights[i], new, world)
            lights[i] = new
        c1 = res.path_counters()  # (before the flush: what the operators themselves did)
        res.flush()
        c1["occlusion_units_in_runs"] = res.path_counters()["occlusion_units_in_runs"]
        assert c1["operator_alloc_calls"] == c0["operator_alloc_calls"] and c1["operator_host_syncs"] == c0["operator_host_syncs"], (c0, c1)
        assert c1["occlusion_units_in_runs"] > c0["occlusion_units_in_runs"], (c0, c1)


@gpu_test
def test_a_tall_volume_takes_the_second_liveness_word_and_cuts_runs_at_layer_64(gpu, oracle_mod, tunables):
    """16 x 16 x 600: 75 unit layers in one column, all live (its taps leave the volume in x and y) — k_occ_runs packs them into two
    64-bit words and a run ends at layer 64 whatever occ_run is. Same bytes for every occ_run, the oracle's for the default."""
    world = S.default_world()
    vol = make_volume(TALL, np.uint16)
    lights = [abi.DirLightParams(d, 0.4) for d in TALL_LIGHTS]
    orc = oracle_mod.OracleScene(vol, False)
    orc.set_tf_lut(abi.color_curve_to_lut(S.TF_A_KEYS))
    orc.set_windowing(abi.WindowingParams(*WINDOW))
    for l in lights:
        orc.add_dir_light(l, True, world)
    got = {}
    for r in RUNS:
        tunables("occ_run", r)
        with open_scene(TALL, np.uint16, vol, world) as res:
            for l in lights:
                res.add_dir_light(l, True, world)
            res.flush()
            got[r] = res.download_light_volume()
            c = res.path_counters()
            assert c["occlusion_dual"] == len(lights) and (c["occlusion_units_in_runs"] > 0) == (r > 1), (r, c)
    assert np.array_equal(got[4], orc.light), f"{np.count_nonzero(got[4] != orc.light)} light voxels differ from the oracle"
    for r in RUNS:
        assert got[r].tobytes() == got[1].tobytes(), f"occ_run {r}: {np.count_nonzero(got[r] != got[1])} light voxels differ from occ_run 1"
