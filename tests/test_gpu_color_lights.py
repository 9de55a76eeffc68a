"""Coloured directional lights (include/tbrm_color_lights.h) on the GPU. Both halves reduce bit for bit to what the library already
computes: channel c of a colour handle is the light volume of a mono handle that ran the same operators with the intensities
float32(I) * float32(color[c]); frame channel c is the mono frame lit by channel c. No oracle, no tolerance."""
import ctypes as C

import numpy as np
import pytest

from tbraymarcherplugin_amd import abi, synthetic as S
import exact_scenes as E

pytestmark = pytest.mark.gpu

WINDOW = (0.5, 0.9, True, False)
CAM = S.default_camera(96, 80)
TILE = abi.Tile(0, 0, 96, 80)
# the ragged volume's world: a cube mesh scaled unevenly, so that a float32 light volume's taps outgrow the sweep's hand-off wave
# and the planner falls back to the chunked chain (asserted through abi.host_plan_light below)
AXIS_WORLD = abi.make_world(abi.identity_transform(scale=(100.0, 130.0, 70.0)))

# lights from different faces: (direction, intensity, colour)
L1 = ((1.0, .35, -.5), 0.5, (1.0, 0.5, 0.0))
L2 = ((-.4, 1.0, -.3), 0.4, (0.2, 0.0, 1.0))
L3 = ((.2, -.3, -1.0), 0.4, (1.0, 1.0, 1.0))
L1_MOVED = ((.3, -1.0, .45), 0.5, (1.0, 0.5, 0.0))    # another major axis: remove + add
L2_RECOLORED = ((-.4, 1.0, -.3), 0.4, (0.7, 0.3, 0.0))  # colour only: G from 0, B to 0
# add, add, add (white), change across major axes, change of colour only, remove
SEQUENCE = [("add", L1), ("add", L2), ("add", L3), ("change", L1, L1_MOVED), ("change", L2, L2_RECOLORED), ("remove", L3)]


def color_light(l):
    return abi.ColorDirLight(*l)


def channel_light(l, c):
    """the mono light of channel c: one float32 product"""
    d, i, col = l
    return abi.DirLightParams(d, float(np.float32(i) * np.float32(col[c])))


def make_res(dims, dtype, light32, half=False, rgb=False, addr=abi.ADDRESS_WRAP, vol=None):
    res = abi.Resources(dims, abi.DTYPE_FMT[np.dtype(dtype)], light32, half, 0, addr, rgb=rgb)
    res.upload_volume(vol if vol is not None else S.make_volume_numpy(dims, dtype, 0x5EED0002))
    res.set_tf_lut(abi.color_curve_to_lut(S.tf_keys("A")))
    res.set_windowing(abi.WindowingParams(*WINDOW))
    return res


def apply_color(res, op, world):
    if op[0] == "change":
        res.change_color_dir_light(color_light(op[1]), color_light(op[2]), world)
    else:
        res.add_color_dir_light(color_light(op[1]), op[0] == "add", world)


def apply_mono(res, op, c, world):
    if op[0] == "change":
        res.change_dir_light(channel_light(op[1], c), channel_light(op[2], c), world)
    else:
        res.add_dir_light(channel_light(op[1], c), op[0] == "add", world)


def planned_paths(dims, light32, half, world):
    lv = tuple((d + 1) // 2 for d in dims) if half else dims
    paths = set()
    for l in (L1, L2, L3, L1_MOVED):
        paths |= {p[0] for p in abi.host_plan_light(abi.DirLightParams(l[0], l[1]), world, lv, light32)}
    return paths


def check_sequence(dims, dtype, light32, half, world):
    vol = S.make_volume_numpy(dims, dtype, 0x5EED0002)
    with make_res(dims, dtype, light32, half, rgb=True, vol=vol) as col:
        monos = [make_res(dims, dtype, light32, half, vol=vol) for _ in range(3)]
        try:
            assert col.light_channels() == 3 and monos[0].light_channels() == 1
            col.clear_light_volume(0.0)
            for m in monos:
                m.clear_light_volume(0.0)
            for k, op in enumerate(SEQUENCE):
                apply_color(col, op, world)
                for c in range(3):
                    apply_mono(monos[c], op, c, world)
                    assert np.array_equal(col.download_light_channel(c), monos[c].download_light_volume()), (k, op[0], c)
            lit = [int(np.count_nonzero(col.download_light_channel(c))) for c in range(3)]
            assert min(lit) > 0, lit   # every channel holds light at the end: nothing above compared empty volumes only
            col.flush()
        finally:
            for m in monos:
                m.close()


# (dims, data type, float32 light volume, half resolution, world, the paths the planner must take: 0 sweep, 1 chain, 2 slice)
CASES = [
    ("cube-u8", (64, 64, 64), np.uint16, False, False, None, {0}),
    ("cube-f32", (64, 64, 64), np.uint16, True, False, None, {0}),
    ("aniso-u8", (96, 72, 40), np.uint8, False, False, None, {0}),
    ("aniso-u8-half", (96, 72, 40), np.float32, False, True, None, {0}),
    ("ragged-u8", (67, 45, 53), np.uint16, False, False, AXIS_WORLD, {0}),
    ("ragged-f32-chain", (67, 45, 53), np.uint16, True, False, AXIS_WORLD, {0, 1}),
]


@pytest.mark.parametrize("cache_mb", [-1, 0], ids=["cache", "nocache"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_every_channel_is_the_mono_handle_with_the_scaled_intensity(gpu, tunables, case, cache_mb):
    _, dims, dtype, light32, half, world, want_paths = case
    world = world if world is not None else S.default_world()
    tunables("light_cache_mb", cache_mb)
    tunables("force_slice_kernel", 0)
    assert planned_paths(dims, light32, half, world) == want_paths   # both kinds of path occur over the cases: the sweep, and a fallback
    check_sequence(dims, dtype, light32, half, world)


@pytest.mark.parametrize("light32", [False, True], ids=["u8", "f32"])
def test_channels_match_on_the_slice_per_launch_path(gpu, tunables, light32):
    tunables("force_slice_kernel", 1)
    check_sequence((67, 45, 53), np.uint16, light32, False, AXIS_WORLD)


def test_white_is_mono(gpu):
    dims = (64, 64, 64)
    world = S.default_world()
    rp = abi.RaymarchParams(100.0, 3, True)
    vol = S.make_volume_numpy(dims, np.uint16, 0x5EED0002)
    with make_res(dims, np.uint16, False, rgb=True, vol=vol) as col, make_res(dims, np.uint16, False, vol=vol) as mono:
        for res in (col, mono):   # the mono entry points, on both handles
            res.clear_light_volume(0.0)
            res.add_dir_light(S.light(0), True, world)
            res.add_dir_light(S.light(1), True, world)
            res.change_dir_light(S.light(1), abi.DirLightParams(S.rotate_z(S.LIGHTS[1][0], 5.0), S.LIGHTS[1][1]), world)
        lv = mono.download_light_volume()
        assert lv.any()
        for c in range(3):
            assert np.array_equal(col.download_light_channel(c), lv), c
        frame = mono.raymarch_lit(CAM, TILE, rp, world)
        assert frame[..., 3].any()
        assert np.array_equal(col.raymarch_lit(CAM, TILE, rp, world), frame)
        assert col.count_nominal_samples(CAM, TILE, rp, world) == mono.count_nominal_samples(CAM, TILE, rp, world)
        assert np.array_equal(col.raymarch_intensity(CAM, TILE, rp, world), mono.raymarch_intensity(CAM, TILE, rp, world))
        col.clear_light_volume(0.25)
        mono.clear_light_volume(0.25)
        for c in range(3):
            assert np.array_equal(col.download_light_channel(c), mono.download_light_volume()), c


def channel_volumes(dims, unorm8):
    """three light volumes that differ everywhere: the seam field, its mirror image along x, and its complement"""
    base = E.seam_light_volume(dims, unorm8)
    flipped = np.ascontiguousarray(base[:, :, ::-1])
    comp = (255 - base) if unorm8 else (np.float32(1.0) - base)
    return [base, flipped, np.ascontiguousarray(comp)]


FRAME_CASES = [
    # (name, dims, data type, float32 light, half, address mode, world, tile, steps)
    ("u16-u8light-wrap", (48, 40, 44), np.uint16, False, False, abi.ADDRESS_WRAP, None, abi.Tile(0, 0, 96, 80), 100.0),
    ("u8-f32light-clamp", (45, 40, 37), np.uint8, True, False, abi.ADDRESS_CLAMP, None, abi.Tile(0, 0, 96, 80), 100.0),
    ("f32-f32light-clip", (40, 37, 44), np.float32, True, False, abi.ADDRESS_WRAP, E.CLIP_THROUGH, abi.Tile(0, 0, 96, 80), 100.0),
    ("u16-u8light-half-rowgroups", (48, 40, 44), np.uint16, False, True, abi.ADDRESS_WRAP, E.CLIP_THROUGH_NEAR, abi.Tile(8, 8, 80, 32, 2), 100.0),
]


@pytest.mark.parametrize("case", FRAME_CASES, ids=[c[0] for c in FRAME_CASES])
def test_frame_is_the_channel_wise_composition_of_three_mono_frames(gpu, tunables, case):
    _, dims, dtype, light32, half, addr, world, tile, steps = case
    world = world if world is not None else S.default_world()
    vol = S.make_volume_numpy(dims, dtype, 0x5EED0002)
    lv_dims = tuple((d + 1) // 2 for d in dims) if half else dims
    chans = channel_volumes(lv_dims, not light32)
    with make_res(dims, dtype, light32, half, rgb=True, addr=addr, vol=vol) as col, make_res(dims, dtype, light32, half, addr=addr, vol=vol) as mono:
        for a, b in ((0, 1), (0, 2), (1, 2)):
            assert (chans[a] != chans[b]).mean() > 0.9   # the three uploaded channels differ
        for c in range(3):
            col.upload_light_channel(c, chans[c])
            assert np.array_equal(col.download_light_channel(c), chans[c])   # round trip, and the channels are where they were put
        for skip in (True, False):
            for lanes in (4, 8):
                for tables in (0, 1):
                    tunables("ray_lanes", lanes)
                    tunables("ray_tables", tables)
                    rp = abi.RaymarchParams(steps, 3, skip)
                    frame = col.raymarch_lit(CAM, tile, rp, world)
                    want = np.empty_like(frame)
                    monos = []
                    for c in range(3):
                        mono.upload_light_volume(chans[c])
                        monos.append(mono.raymarch_lit(CAM, tile, rp, world))
                        want[..., c] = monos[c][..., c]
                    want[..., 3] = monos[0][..., 3]
                    assert np.array_equal(monos[1][..., 3], monos[0][..., 3]) and np.array_equal(monos[2][..., 3], monos[0][..., 3])
                    assert np.array_equal(frame, want), (skip, lanes, tables)
                    # a swapped or shared channel cannot pass: where the frame shows anything, the mono frames lit by two different
                    # channels differ in most pixels (any one differing pixel already fails the comparison above)
                    shown = frame[..., 3] > 0
                    assert shown.sum() > 200
                    for a, b in ((0, 1), (0, 2), (1, 2)):
                        for ch in range(3):
                            differs = monos[a][..., ch][shown] != monos[b][..., ch][shown]
                            assert differs.mean() > 0.5, (a, b, ch, float(differs.mean()))


def test_one_occlusion_per_light_and_a_reserved_handle_stands_still(gpu, tunables):
    tunables("light_cache_mb", -1)
    tunables("force_slice_kernel", 0)
    dims = (64, 64, 64)
    world = S.default_world()
    vol = S.make_volume_numpy(dims, np.uint16, 0x5EED0002)
    ops = [("add", L1), ("change", L1, (S.rotate_z(L1[0], 5.0), L1[1], L1[2])),
           ("change", (S.rotate_z(L1[0], 5.0), L1[1], L1[2]), (S.rotate_z(L1[0], 5.0), L1[1], (0.3, 1.0, 0.6)))]
    occ = []
    for rgb in (True, False):
        with make_res(dims, np.uint16, False, rgb=rgb, vol=vol) as res:
            res.clear_light_volume(0.0)
            before = res.path_counters()
            for op in ops:
                if rgb:
                    apply_color(res, op, world)
                else:   # the same operators on a mono handle (channel 0's intensities)
                    apply_mono(res, op, 0, world)
            res.flush()
            after = res.path_counters()
            occ.append((after["occlusion_single"] + after["occlusion_dual"]) - (before["occlusion_single"] + before["occlusion_dual"]))
            assert after["passes_sweep"] > before["passes_sweep"] and after["passes_chain"] == before["passes_chain"]
    assert occ[0] == occ[1] and occ[1] > 0, occ
    with make_res(dims, np.uint16, False, rgb=True, vol=vol) as res:
        res.reserve(4)
        res.clear_light_volume(0.0)
        apply_color(res, ("add", L1), world)
        apply_color(res, ("add", L2), world)
        res.flush()
        before = res.path_counters()
        cur = L1
        for k in range(50):
            nxt = (S.rotate_z(L1[0], 2.0 * (k + 1)), L1[1], (1.0, 0.5 + 0.01 * (k % 7), 0.02 * (k % 5)))
            apply_color(res, ("change", cur, nxt), world)
            cur = nxt
        after = res.path_counters()
        assert after["operator_alloc_calls"] == before["operator_alloc_calls"]
        assert after["operator_host_syncs"] == before["operator_host_syncs"]
        assert res.lib.tbrm_flush(res.handle) == abi.OK


def test_refusals(gpu):
    dims = (64, 64, 64)
    world = S.default_world()
    lib = abi.load()
    vol = S.make_volume_numpy(dims, np.uint16, 0x5EED0002)
    with make_res(dims, np.uint16, False, rgb=True, vol=vol) as col, make_res(dims, np.uint16, False, vol=vol) as mono:
        col.clear_light_volume(0.0)
        apply_color(col, ("add", L1), world)
        apply_color(col, ("add", L2), world)
        before = [col.download_light_channel(c) for c in range(3)]
        launches = col.launch_counters()
        h = col.handle
        buf = np.zeros(dims[::-1], dtype=np.uint8)
        lights = (abi.DirLightParams * 2)(S.light(0), S.light(1))
        sched, n = (C.c_int32 * 16)(), C.c_int32(0)
        slab, n_passes, sp, ptr, nb = abi.Slab(0, 32), C.c_int32(0), abi.SlabPass(), C.c_void_p(), C.c_size_t()
        d3, l3 = (C.c_int32 * 3)(), (C.c_int32 * 3)()
        rp = abi.RaymarchParams(100.0, -1, True)
        state = np.zeros((TILE.h, TILE.w, 4), dtype=np.float32)
        light = S.light(0)
        out_of_scope = {
            "tbrm_add_dir_lights": lambda: lib.tbrm_add_dir_lights(h, lights, 2, 1, C.byref(world), sched, C.byref(n)),
            "tbrm_slab_light_begin": lambda: lib.tbrm_slab_light_begin(h, None, C.byref(light), 1, C.byref(world), C.byref(slab), C.byref(n_passes)),
            "tbrm_slab_pass_begin": lambda: lib.tbrm_slab_pass_begin(h, 0, C.byref(sp)),
            "tbrm_slab_pass_chunk": lambda: lib.tbrm_slab_pass_chunk(h, 0),
            "tbrm_slab_pass_plane": lambda: lib.tbrm_slab_pass_plane(h, 0, 0, C.byref(ptr)),
            "tbrm_slab_resident_slices": lambda: lib.tbrm_slab_resident_slices(h, C.byref(d3), C.byref(l3)),
            "tbrm_slab_light_halo": lambda: lib.tbrm_slab_light_halo(h, 1, C.byref(ptr), C.byref(ptr), C.byref(nb)),
            "tbrm_raymarch_lit_slab_device": lambda: lib.tbrm_raymarch_lit_slab_device(h, C.byref(CAM), C.byref(TILE), C.byref(rp), C.byref(world), None,
                                                                                         state.ctypes.data, C.byref(slab), 0),
            "tbrm_upload_label_volume": lambda: lib.tbrm_upload_label_volume(h, buf.ctypes.data, buf.nbytes),
            "tbrm_download_light_volume": lambda: lib.tbrm_download_light_volume(h, buf.ctypes.data, buf.nbytes),
            "tbrm_upload_light_volume": lambda: lib.tbrm_upload_light_volume(h, buf.ctypes.data, buf.nbytes),
            "tbrm_light_volume_device_ptr": lambda: lib.tbrm_light_volume_device_ptr(h, C.byref(ptr), C.byref(nb)),
        }
        for name, call in out_of_scope.items():
            assert call() == abi.ERR_UNSUPPORTED, name
            assert b"colour handle" in lib.tbrm_last_error(), name
        assert col.launch_counters() == launches   # nothing was enqueued
        assert not col.has_label_volume()
        with pytest.raises(abi.TbrmError) as e:   # no colour form of a slab-resident handle
            abi.Resources(dims, abi.FMT_G16, owned=abi.Slab(0, 32), rgb=True)
        assert e.value.code == abi.ERR_UNSUPPORTED
        flag = C.c_int(0)
        for bad in (1.5, -0.1, float("nan")):
            for slot in range(3):
                colour = [0.5, 0.5, 0.5]
                colour[slot] = bad
                l = abi.ColorDirLight(L1[0], L1[1], colour)
                assert lib.tbrm_add_color_dir_light(h, C.byref(l), 1, C.byref(world), C.byref(flag)) == abi.ERR_INVALID_ARG, (bad, slot)
                good = color_light(L1)
                assert lib.tbrm_change_color_dir_light(h, C.byref(good), C.byref(l), C.byref(world), C.byref(flag)) == abi.ERR_INVALID_ARG
                assert lib.tbrm_change_color_dir_light(h, C.byref(l), C.byref(good), C.byref(world), C.byref(flag)) == abi.ERR_INVALID_ARG
        good = color_light(L1)
        assert lib.tbrm_add_color_dir_light(mono.handle, C.byref(good), 1, C.byref(world), C.byref(flag)) == abi.ERR_INVALID_ARG
        assert lib.tbrm_change_color_dir_light(mono.handle, C.byref(good), C.byref(good), C.byref(world), C.byref(flag)) == abi.ERR_INVALID_ARG
        assert lib.tbrm_download_light_channel(h, 3, buf.ctypes.data, buf.nbytes) == abi.ERR_INVALID_ARG
        assert lib.tbrm_download_light_channel(mono.handle, 1, buf.ctypes.data, buf.nbytes) == abi.ERR_INVALID_ARG
        assert lib.tbrm_download_light_channel(h, 0, buf.ctypes.data, buf.nbytes - 1) == abi.ERR_INVALID_ARG
        for c in range(3):
            assert np.array_equal(col.download_light_channel(c), before[c]), c   # the light channels are unchanged
        assert col.launch_counters() == launches
        # a zero direction follows tbrm_add_dir_light: accepted, nothing propagated
        assert col.add_color_dir_light(abi.ColorDirLight((0.0, 0.0, 0.0), 0.5, (1.0, 0.5, 0.0)), True, world)
        assert col.launch_counters() == launches
        # upload then download of a channel round-trips exactly, on both kinds of handle, and leaves the other channels alone
        pattern = np.random.default_rng(7).integers(0, 256, size=dims[::-1], dtype=np.uint8)
        col.upload_light_channel(1, pattern)
        assert np.array_equal(col.download_light_channel(1), pattern)
        assert np.array_equal(col.download_light_channel(0), before[0]) and np.array_equal(col.download_light_channel(2), before[2])
        mono.upload_light_channel(0, pattern)
        assert np.array_equal(mono.download_light_channel(0), pattern) and np.array_equal(mono.download_light_volume(), pattern)


@pytest.mark.parametrize("light32", [False, True], ids=["u8", "f32"])
def test_light_transfers_round_trip_on_a_ragged_volume(gpu, light32):
    """upload then download, exactly, where the bricked layout has something to get wrong: 3 x 2 x 2 bricks, no edge a multiple of 8"""
    dims = (20, 12, 9)
    rng = np.random.default_rng(20129)
    shape = dims[::-1]
    chans = [rng.random(shape, dtype=np.float32) if light32 else rng.integers(0, 256, size=shape, dtype=np.uint8) for _ in range(4)]
    with abi.Resources(dims, abi.FMT_G8, light32, rgb=True) as col, abi.Resources(dims, abi.FMT_G8, light32) as mono:
        for c in (2, 0, 1):
            col.upload_light_channel(c, chans[c])
        for c in range(3):
            assert np.array_equal(col.download_light_channel(c), chans[c]), c
        mono.upload_light_volume(chans[3])
        assert np.array_equal(mono.download_light_volume(), chans[3]) and np.array_equal(mono.download_light_channel(0), chans[3])
