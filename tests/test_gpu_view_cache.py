"""The view cache (include/tbrm_view_cache.h; DESIGN.md 4.1 "Relit frames"): a lit frame whose view has not changed is served by
k_relight from the records of an earlier march. Everything here is equality on the bits (float32 frames viewed as uint32) against
the plain march of the same handle with view_cache_mb = 0; tbrm_view_cache_stats says which kernel served a frame. res.flush()
between the calls makes the sequence plain / count / fill / relit deterministic."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tbraymarcherplugin_amd import abi, sharding, synthetic as S
import exact_reference as X

gpu_test = pytest.mark.gpu

DIMS = (40, 36, 44)                      # no dimension a multiple of 8
FB = (40, 28)
TILE = abi.Tile(3, 2, 29, 12, 2)         # non-zero origin, a width that is no multiple of 8, rows interleaved in groups
WINDOW = (0.5, 1.0, False, False)
JITTER = 3
CACHE_MB = 64                            # (the tests' arenas: the default's 1.5 GiB per handle is not needed for 40 x 28 pixels)
L0 = abi.DirLightParams((1.0, .35, -.5), 0.5)
L0_MOVED = abi.DirLightParams(S.rotate_z((1.0, .35, -.5), 5.0), 0.5)


def opaque_tf():
    """a thin haze from texel 1 (most rays through the cube run to their fractional last step), nothing below it (empty bricks to
    leap over), quickly opaque from texel 60 (rays that meet the blobs take the 0.95 exit a few samples in, most in mid-trip)"""
    lut = np.zeros((256, 4), dtype=np.float32)
    t = np.linspace(0.0, 1.0, 196, dtype=np.float32)
    lut[1:60] = (0.2, 0.5, 0.9, 0.02)
    lut[60:, 0] = 0.9 - 0.4 * t
    lut[60:, 1] = 0.3 + 0.6 * t
    lut[60:, 2] = 0.5
    lut[60:, 3] = 0.15 + 0.8 * t
    return lut


def volume(dtype, seed=2):
    return S.make_volume_numpy(DIMS, dtype, S.seed_for_config(seed))


def make_res(dtype=np.uint16, addr=abi.ADDRESS_WRAP, light32=False, half=False, tf=None):
    res = abi.Resources(DIMS, abi.DTYPE_FMT[np.dtype(dtype)], light32, half, 0, addr)
    res.upload_volume(volume(dtype))
    res.set_tf_lut(opaque_tf() if tf is None else tf)
    res.set_windowing(abi.WindowingParams(*WINDOW))
    res.clear_light_volume(0.0)
    assert res.add_dir_light(L0, True, S.default_world())
    return res


class View:
    """the arguments of a frame call, and the frame (device form, flushed)"""

    def __init__(self, steps=48.0, tile=TILE, fb=FB):
        self.cam = S.default_camera(*fb)
        self.tile = tile
        self.rp = abi.RaymarchParams(steps, JITTER, True)
        self.world = S.default_world()
        self.depth = None

    def frame(self, res):
        out = torch.full((self.tile.h, self.tile.w, 4), -7.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        res.raymarch_lit_device(self.cam, self.tile, self.rp, self.world, out.data_ptr(), None if self.depth is None else self.depth.data_ptr())
        res.flush()
        return out.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def moved(after, before):
    return {k: after[k] - before[k] for k in ("plain", "counted", "filled", "relit", "dropped")}


def to_relit(res, view):
    """four identical calls: marched plainly, counted, recorded, relit — returns the four frames"""
    s0 = res.view_cache_stats()
    frames = [view.frame(res) for _ in range(4)]
    assert moved(res.view_cache_stats(), s0) == dict(plain=1, counted=1, filled=1, relit=1, dropped=0)
    return frames


def plain_frame(res, view, tunables):
    """the march of the same handle, the cache off (forgets the view: the next cached frame starts over)"""
    tunables("view_cache_mb", 0)
    try:
        return view.frame(res)
    finally:
        tunables("view_cache_mb", CACHE_MB)


def random_light(res, seed):
    """seeded random codes straight into the bricked light volume"""
    res.flush()
    t = sharding.device_light_tensor(res)
    g = torch.Generator(device="cpu").manual_seed(seed)
    if t.dtype == torch.uint8:
        t.copy_(torch.randint(0, 256, t.shape, generator=g, dtype=torch.uint8))
    else:
        t.copy_(torch.rand(t.shape, generator=g, dtype=torch.float32))
    torch.cuda.synchronize()


# ---- the header (no GPU) ------------------------------------------------------------------------------------------------------
def test_header_symbols_are_exported_and_bound():
    lib = abi.load()
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tbrm_view_cache.h")
    text = open(header).read()
    declared = re.findall(r"TBRM_API\s+[\w\s\*]+?\b(tbrm_\w+)\s*\(", text)
    assert sorted(declared) == sorted(abi.VIEW_CACHE_SYMBOLS)
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.tbrm_view_cache_abi_version() == int(re.search(r"#define\s+TBRM_VIEW_CACHE_ABI_VERSION\s+(\d+)", text).group(1)) == abi.VIEW_CACHE_ABI_VERSION
    assert lib.tbrm_view_cache_stats(C.c_void_p(None), None) == abi.ERR_INVALID_ARG
    assert abi.get_tunable("view_cache_mb") >= 0


# ---- 1. relit equals marched ----------------------------------------------------------------------------------------------------
@gpu_test
@pytest.mark.parametrize("addr", [abi.ADDRESS_WRAP, abi.ADDRESS_CLAMP], ids=["wrap", "clamp"])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32], ids=["u8", "u16", "f32"])
def test_relit_equals_marched(gpu, tunables, dtype, addr):
    tunables("view_cache_mb", CACHE_MB)
    exits = contributing = fractional = 0
    for light32 in (False, True):
        for half in (False, True):  # the light volume on the data volume's grid (40 x 36 x 44), and on its own (20 x 18 x 22)
            with make_res(dtype, addr, light32, half) as res:
                assert res.light_dims == ((20, 18, 22) if half else DIMS)
                for steps in (48.0, 32.0):  # offset tables on (no dimension above 48) / off
                    for lanes in (4, 8):
                        tunables("ray_lanes", lanes)
                        view = View(steps)
                        res.clear_light_volume(0.0)
                        res.add_dir_light(L0, True, view.world)
                        first = to_relit(res, view)
                        for f in first[1:]:
                            assert np.array_equal(bits(f), bits(first[0])), (light32, half, steps, lanes)
                        random_light(res, 11)
                        lv1 = res.download_light_volume()
                        relit1 = view.frame(res)
                        res.change_dir_light(L0, L0_MOVED, view.world)
                        lv2 = res.download_light_volume()
                        relit2 = view.frame(res)
                        assert res.view_cache_stats()["relit"] >= 3 and res.view_cache_stats()["record_bytes"] > 0
                        res.upload_light_volume(lv1)
                        plain1 = plain_frame(res, view, tunables)
                        res.upload_light_volume(lv2)
                        plain2 = plain_frame(res, view, tunables)
                        assert np.array_equal(bits(relit1), bits(plain1)), (light32, half, steps, lanes)
                        assert np.array_equal(bits(relit2), bits(plain2)), (light32, half, steps, lanes)
                        assert not np.array_equal(bits(relit1), bits(first[0]))  # (the light did reach the frame)
                        exits += int(np.count_nonzero(plain1[..., 3] == 1.0))
                        contributing += int(np.count_nonzero(plain1[..., 3] > 0.0))
                        # rays that contribute, take no exit and end in a fractional step: steps x thickness (float64 here) at
                        # least 0.05 away from a whole number, far more than the kernel's fp32 thickness can be off
                        frac = np.mod(steps * X.cube_setup(view.cam, view.world, view.tile)[1], 1.0)
                        fractional += int(np.count_nonzero((plain1[..., 3] > 0.0) & (plain1[..., 3] < 1.0) & (frac > 0.05) & (frac < 0.95)))
    assert exits > 0 and contributing > exits and fractional > 0


@gpu_test
def test_empty_frames(gpu, tunables):
    """a frame no sample contributes to (a transfer function without opacity), and a tile that misses the volume: zeros, relit"""
    tunables("view_cache_mb", CACHE_MB)
    with make_res(tf=np.zeros((256, 4), dtype=np.float32)) as res:
        for f in to_relit(res, View()):
            assert not f.any()
    with make_res() as res:
        away = View(tile=abi.Tile(4000, 3000, 29, 12, 2))
        for f in to_relit(res, away):
            assert not f.any()
        random_light(res, 5)
        assert not away.frame(res).any()


# ---- 2. every input invalidates ------------------------------------------------------------------------------------------------
def _camera(view, res, tunables): view.cam = abi.look_at_camera(np.array([-1.2, -1.1, 0.7]) * S.VOLUME_SCALE, (0.0, 0.0, 0.0), (0.0, 0.0, 1.0), 60.0, *FB)
def _fov(view, res, tunables): view.cam = S.default_camera(*FB, vfov_deg=50.0)
def _tile_origin(view, res, tunables): view.tile = abi.Tile(4, 2, 29, 12, 2)
def _row_groups(view, res, tunables): view.tile = abi.Tile(3, 2, 29, 12, 1)
def _steps(view, res, tunables): view.rp = abi.RaymarchParams(50.0, JITTER, True)
def _skipping(view, res, tunables): view.rp = abi.RaymarchParams(48.0, JITTER, False)
def _jitter(view, res, tunables): view.rp = abi.RaymarchParams(48.0, JITTER + 1, True)
def _transform(view, res, tunables): view.world = abi.make_world(abi.identity_transform(S.VOLUME_SCALE, translation=(3.0, -2.0, 1.0)))
def _clip(view, res, tunables): view.world = abi.make_world(abi.identity_transform(S.VOLUME_SCALE), clip_center=(0.0, 0.0, 10.0), clip_direction=(0.0, 0.0, -1.0))
def _window(view, res, tunables): res.set_windowing(abi.WindowingParams(float(np.nextafter(np.float32(WINDOW[0]), np.float32(1.0))), *WINDOW[1:]))


def _tf(view, res, tunables):
    lut = opaque_tf()
    lut[180, 1] += 0.125
    res.set_tf_lut(lut)


def _upload(view, res, tunables): res.upload_volume(volume(np.uint16))
def _region(view, res, tunables): res.update_volume_region((8, 16, 24), np.full((8, 8, 8), 40000, dtype=np.uint16))
def _labels(view, res, tunables): res.upload_label_volume(np.zeros(DIMS[::-1], dtype=np.uint8))
def _lanes(view, res, tunables): tunables("ray_lanes", 4)
def _tables(view, res, tunables): tunables("ray_tables", 0)
def _xcd_rows(view, res, tunables): tunables("ray_xcd_rows", 0)
def _depth(view, res, tunables): view.depth = torch.full((FB[1], FB[0]), 120.0, dtype=torch.float32, device="cuda")


CHANGES = [_camera, _fov, _tile_origin, _row_groups, _steps, _skipping, _jitter, _transform, _clip, _window, _tf, _upload, _region,
           _labels, _lanes, _tables, _xcd_rows, _depth]


@gpu_test
@pytest.mark.parametrize("change", CHANGES, ids=[c.__name__[1:] for c in CHANGES])
def test_every_input_invalidates(gpu, tunables, change):
    tunables("view_cache_mb", CACHE_MB)
    with make_res() as res:
        view = View()
        to_relit(res, view)
        s0 = res.view_cache_stats()
        change(view, res, tunables)
        torch.cuda.synchronize()
        got = view.frame(res)
        d = moved(res.view_cache_stats(), s0)
        assert d["relit"] == 0 and d["plain"] + d["counted"] == 1, d
        assert np.array_equal(bits(got), bits(plain_frame(res, view, tunables)))


# ---- 3. does not fit --------------------------------------------------------------------------------------------------------------
@gpu_test
def test_a_view_too_large_is_marched(gpu, tunables):
    tunables("view_cache_mb", 1)  # (583 trips; this view records thousands)
    tunables("ray_lanes", 4)
    with make_res() as res:
        view = View(96.0, abi.Tile(0, 0, 96, 64, 1), (96, 64))
        frames = [view.frame(res) for _ in range(6)]
        s = res.view_cache_stats()
        assert (s["plain"], s["counted"], s["filled"], s["relit"], s["dropped"], s["record_bytes"]) == (4, 1, 1, 0, 1, 0), s
        tunables("view_cache_mb", 0)
        want = view.frame(res)
        tunables("view_cache_mb", 1)
        for f in frames:
            assert np.array_equal(bits(f), bits(want))
        s0 = res.view_cache_stats()
        view.rp = abi.RaymarchParams(96.0, JITTER + 1, True)  # another key: counted again
        view.frame(res), view.frame(res)
        assert moved(res.view_cache_stats(), s0) == dict(plain=1, counted=1, filled=0, relit=0, dropped=0)


@gpu_test
def test_a_view_with_more_waves_than_the_arena_has_words_for_is_marched(gpu, tunables):
    """131072 waves: their count and offset words alone are 16 bytes more than the arena (carve_view_arena fails): dropped at the
    second frame, never counted"""
    tunables("view_cache_mb", 1)
    tunables("ray_lanes", 4)
    with make_res() as res:
        view = View(32.0, abi.Tile(0, 0, 2048, 1024, 1), (2048, 1024))
        frames = [view.frame(res) for _ in range(3)]
        s = res.view_cache_stats()
        assert (s["plain"], s["counted"], s["filled"], s["relit"], s["dropped"], s["record_bytes"]) == (3, 0, 0, 0, 1, 0), s
        tunables("view_cache_mb", 0)
        want = view.frame(res)
        for f in frames:
            assert np.array_equal(bits(f), bits(want))


# ---- 4. two views alternating -----------------------------------------------------------------------------------------------------
@gpu_test
def test_two_alternating_views_only_march(gpu, tunables):
    tunables("view_cache_mb", CACHE_MB)
    with make_res() as res:
        a, b = View(), View()
        b.rp = abi.RaymarchParams(48.0, JITTER + 1, True)
        fa, fb = a.frame(res), b.frame(res)
        for _ in range(3):
            assert np.array_equal(bits(a.frame(res)), bits(fa)) and np.array_equal(bits(b.frame(res)), bits(fb))
        s = res.view_cache_stats()
        assert (s["plain"], s["counted"], s["filled"], s["relit"], s["dropped"]) == (8, 0, 0, 0, 0), s


# ---- 5. the host form ---------------------------------------------------------------------------------------------------------------
@gpu_test
def test_host_form_is_relit(gpu, tunables):
    tunables("view_cache_mb", CACHE_MB)
    with make_res() as res:
        view = View()
        for _ in range(4):
            res.raymarch_lit(view.cam, view.tile, view.rp, view.world)
        random_light(res, 23)
        s0 = res.view_cache_stats()
        got = res.raymarch_lit(view.cam, view.tile, view.rp, view.world)
        assert moved(res.view_cache_stats(), s0) == dict(plain=0, counted=0, filled=0, relit=1, dropped=0)
        assert np.array_equal(bits(got), bits(view.frame(res)))                      # (the device form, relit as well)
        assert np.array_equal(bits(got), bits(plain_frame(res, view, tunables)))
