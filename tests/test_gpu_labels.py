"""The label overlay of the lit march (include/tbrm_labels.h) on the GPU: bit-identity where nothing may change (no label shows,
skipping on / off, tiles, region updates, the illumination), the float64 restatement (tests/label_reference.py), the refusals."""
import numpy as np
import pytest

from tbraymarcherplugin_amd import abi, synthetic as S
import exact_reference as X
import exact_scenes as E
import label_reference as LR
from test_label_reference import SLAB_STEPS, slab_answer, slab_setup

pytestmark = pytest.mark.gpu

WINDOW = (0.5, 0.9, True, False)


def overlay_colors():
    """labels 1 .. 5 in distinct half-transparent colours, 6 fully opaque, 7 present but clear"""
    c = np.zeros((256, 4), dtype=np.float32)
    c[1:8] = [(1, 0, 0, 0.6), (0, 1, 0, 0.5), (0, 0, 1, 0.7), (1, 1, 0, 0.4), (0, 1, 1, 0.9), (1, 0, 1, 1.0), (0.5, 0.5, 0.5, 0.0)]
    return c


def clear_colors():
    c = np.zeros((256, 4), dtype=np.float32)
    c[:, :3] = 0.9   # colour without alpha: shows nothing
    return c


def sphere_labels(dims, centers, radii, values, rng=None, noise=0.0):
    nx, ny, nz = dims
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    lab = np.zeros((nz, ny, nx), dtype=np.uint8)
    for (cx, cy, cz), r, v in zip(centers, radii, values):
        lab[(x - cx * nx) ** 2 + (y - cy * ny) ** 2 + (z - cz * nz) ** 2 <= (r * min(dims)) ** 2] = v
    if noise:
        lab[rng.random(lab.shape) < noise] = 7
    return lab


def mostly_empty_volume(dims, dtype):
    """zero (cut off by the window: every brick empty) but for a blob in the middle"""
    nx, ny, nz = dims
    z, y, x = np.meshgrid((np.arange(nz) + 0.5) / nz, (np.arange(ny) + 0.5) / ny, (np.arange(nx) + 0.5) / nx, indexing="ij")
    v = np.clip(0.9 - 6.0 * np.sqrt((x - 0.5) ** 2 + (y - 0.5) ** 2 + (z - 0.5) ** 2), 0.0, 1.0)
    if dtype == np.uint8:
        return np.floor(v * 255 + 0.5).astype(np.uint8)
    if dtype == np.uint16:
        return np.floor(v * 65535 + 0.5).astype(np.uint16)
    return v.astype(np.float32)


def boundary_labels(dims):
    """single voxels on every corner, edge and face of the volume and on brick boundaries, in bricks the TF leaves empty"""
    nx, ny, nz = dims
    lab = np.zeros((nz, ny, nx), dtype=np.uint8)
    k = 0
    for x in (0, nx // 2, nx - 1):
        for y in (0, ny // 2, ny - 1):
            for z in (0, nz // 2, nz - 1):
                if (x, y, z) != (nx // 2, ny // 2, nz // 2):
                    lab[z, y, x] = 1 + k % 6
                    k += 1
    for v in (7, 8, 15, 16, 23, 24):   # both sides of brick boundaries, off the middle
        if v < nx and v < ny and v < nz:
            lab[v, 3, v] = 1 + v % 6
            lab[2, v, v] = 1 + (v + 1) % 6
    return lab


def make_res(dims, dtype, addr=abi.ADDRESS_WRAP, vol=None, light32=True):
    res = abi.Resources(dims, abi.DTYPE_FMT[np.dtype(dtype)], light32, False, 0, addr)
    res.upload_volume(vol if vol is not None else S.make_volume_numpy(dims, dtype, 0x5EED0002))
    res.set_tf_lut(abi.color_curve_to_lut(S.tf_keys("A")))
    res.set_windowing(abi.WindowingParams(*WINDOW))
    res.upload_light_volume(E.seam_light_volume(dims, not light32))
    return res


CAM = S.default_camera(96, 80)
TILE = abi.Tile(0, 0, 96, 80)


@pytest.mark.parametrize("lanes", [4, 8])
def test_all_clear_table_gives_the_frame_without_labels(gpu, tunables, lanes):
    tunables("ray_lanes", lanes)
    dims = (48, 40, 44)
    with make_res(dims, np.uint16) as res:
        for skip in (True, False):
            rp = abi.RaymarchParams(100.0, 3, skip)
            base = res.raymarch_lit(CAM, TILE, rp, S.default_world())
            res.upload_label_volume(np.random.default_rng(1).integers(0, 256, size=dims[::-1], dtype=np.uint8))
            res.set_label_colors(clear_colors())
            tunables("ray_labels", 0)   # no present label shows: the kernel without labels
            assert np.array_equal(res.raymarch_lit(CAM, TILE, rp, S.default_world()), base)
            tunables("ray_labels", 1)   # the label kernel all the same
            assert np.array_equal(res.raymarch_lit(CAM, TILE, rp, S.default_world()), base)
            tunables("ray_labels", 0)
            # a table that shows labels the volume does not hold: still nothing to show
            res.upload_label_volume(np.zeros(dims[::-1], dtype=np.uint8))
            res.set_label_colors(overlay_colors())
            assert np.array_equal(res.raymarch_lit(CAM, TILE, rp, S.default_world()), base)
            res.release_label_volume()
            assert not res.has_label_volume()
            assert np.array_equal(res.raymarch_lit(CAM, TILE, rp, S.default_world()), base)


@pytest.mark.parametrize("addr", [abi.ADDRESS_WRAP, abi.ADDRESS_CLAMP], ids=["wrap", "clamp"])
def test_skipping_is_exact_with_labels_on_faces_edges_corners(gpu, tunables, addr):
    dims = (40, 37, 44)   # ragged brick grid along y and z
    vol = mostly_empty_volume(dims, np.uint16)
    labels = boundary_labels(dims)
    cams = [S.default_camera(96, 80), abi.look_at_camera((-150.0, 120.0, -90.0), (0.0, 0.0, 0.0), (0.0, 0.0, 1.0), 45.0, 96, 80)]
    with make_res(dims, np.uint16, addr, vol) as res:
        res.upload_label_volume(labels)
        res.set_label_colors(overlay_colors())
        for cam in cams:
            no_label = None
            for lanes in (4, 8):
                for tables in (0, 1):
                    for wave_skip in (-1, 1):
                        tunables("ray_lanes", lanes)
                        tunables("ray_tables", tables)
                        tunables("ray_wave_skip", wave_skip)
                        for jitter in (-1, 5):
                            on = res.raymarch_lit(cam, TILE, abi.RaymarchParams(128.0, jitter, True), S.default_world())
                            off = res.raymarch_lit(cam, TILE, abi.RaymarchParams(128.0, jitter, False), S.default_world())
                            assert np.array_equal(on, off), (lanes, tables, wave_skip, jitter)
                            if jitter < 0 and no_label is None:
                                res.release_label_volume()
                                no_label = res.raymarch_lit(cam, TILE, abi.RaymarchParams(128.0, jitter, True), S.default_world())
                                res.upload_label_volume(labels)
                                res.set_label_colors(overlay_colors())
                                assert (np.abs(on - no_label).max(axis=-1) > 0).sum() >= 10   # the single voxels show
                                assert np.array_equal(res.raymarch_lit(cam, TILE, abi.RaymarchParams(128.0, jitter, True), S.default_world()), on)


def test_tiles_equal_the_whole_frame(gpu):
    dims = (48, 40, 44)
    labels = sphere_labels(dims, [(0.3, 0.4, 0.5), (0.7, 0.6, 0.4)], [0.2, 0.15], [1, 3])
    with make_res(dims, np.uint16) as res:
        res.upload_label_volume(labels)
        rp = abi.RaymarchParams(90.0, 2, True)
        whole = res.raymarch_lit(CAM, TILE, rp, S.default_world())
        parts = np.zeros_like(whole)
        for ty in (0, 40):
            for tx in (0, 48):
                parts[ty:ty + 40, tx:tx + 48] = res.raymarch_lit(CAM, abi.Tile(tx, ty, 48, 40), rp, S.default_world())
        assert np.array_equal(parts, whole)


def test_region_update_equals_full_upload(gpu):
    dims = (48, 40, 44)
    rng = np.random.default_rng(5)
    labels = sphere_labels(dims, [(0.3, 0.4, 0.5)], [0.2], [2])
    edited = labels.copy()
    boxes = [((5, 3, 7), (9, 6, 11), 4), ((0, 0, 0), (48, 40, 10), 0), ((30, 20, 25), (18, 20, 19), 5)]   # origin, extent (x, y, z)
    rp = abi.RaymarchParams(100.0, 1, True)
    with make_res(dims, np.uint16) as res:
        res.upload_label_volume(labels)
        res.set_label_colors(overlay_colors())
        for (ox, oy, oz), (ex, ey, ez), v in boxes:
            block = np.where(rng.random((ez, ey, ex)) < 0.6, v, 0).astype(np.uint8)
            edited[oz:oz + ez, oy:oy + ey, ox:ox + ex] = block
            res.update_label_region((ox, oy, oz), block)
        assert np.array_equal(res.download_label_volume(), edited)
        after_update = res.raymarch_lit(CAM, TILE, rp, S.default_world())
        res.upload_label_volume(edited)
        after_upload = res.raymarch_lit(CAM, TILE, rp, S.default_world())
        assert np.array_equal(after_update, after_upload)
        # erasing every shown label leaves the frame without labels
        res.update_label_region((0, 0, 0), np.zeros(dims[::-1], dtype=np.uint8))
        res.release_label_volume()
        base = res.raymarch_lit(CAM, TILE, rp, S.default_world())
        res.upload_label_volume(edited)
        res.update_label_region((0, 0, 0), np.zeros(dims[::-1], dtype=np.uint8))
        assert np.array_equal(res.raymarch_lit(CAM, TILE, rp, S.default_world()), base)
        with pytest.raises(abi.TbrmError) as e:
            res.update_label_region((40, 0, 0), np.zeros((1, 1, 9), dtype=np.uint8))
        assert e.value.code == abi.ERR_INVALID_ARG


def test_label_changes_leave_the_illumination_alone(gpu):
    dims = (48, 40, 44)
    world = S.default_world()
    new = abi.DirLightParams(S.rotate_z(S.LIGHTS[1][0], 5.0), S.LIGHTS[1][1])
    seen = []
    for with_labels in (False, True):
        with abi.Resources(dims, abi.FMT_G16) as res:
            res.upload_volume(S.make_volume_numpy(dims, np.uint16, 0x5EED0002))
            res.set_tf_lut(abi.color_curve_to_lut(S.tf_keys("A")))
            res.set_windowing(abi.WindowingParams(*WINDOW))
            for i in (0, 1):
                res.add_dir_light(S.light(i), True, world)
            before = res.download_light_volume()
            counters = res.path_counters()
            if with_labels:
                res.upload_label_volume(sphere_labels(dims, [(0.5, 0.5, 0.5)], [0.3], [1]))
                res.update_label_region((2, 2, 2), np.full((4, 5, 6), 3, dtype=np.uint8))
                res.set_label_colors(overlay_colors())
                assert np.array_equal(res.download_light_volume(), before)
                assert res.path_counters() == counters
            res.change_dir_light(S.light(1), new, world)
            seen.append((res.download_light_volume(), res.light_cache_stats(), res.path_counters()))
    assert np.array_equal(seen[0][0], seen[1][0])
    assert seen[0][1] == seen[1][1]
    assert seen[0][2] == seen[1][2]


def test_slab_of_one_label_known_answer_on_gpu(gpu):
    dims, vol, tf, labels, colors, cam, tile, world = slab_setup()
    with abi.Resources(dims, abi.FMT_G16, True) as res:
        res.upload_volume(vol)
        res.set_tf_lut(tf)
        res.set_windowing(abi.WindowingParams(0.5, 1.0, False, False))
        res.upload_light_volume(np.full(dims[::-1], 0.5, dtype=np.float32))
        res.upload_label_volume(labels)
        res.set_label_colors(colors)
        for skip in (True, False):
            got = res.raymarch_lit(cam, tile, abi.RaymarchParams(SLAB_STEPS, -1, skip), world)[0, 0]
            assert np.allclose(got, slab_answer(), rtol=0, atol=2e-6), (got, slab_answer())


def _random_camera(rng, w, h):
    d = rng.normal(size=3)
    d /= np.linalg.norm(d)
    target = rng.uniform(-15.0, 15.0, size=3)
    return abi.look_at_camera(tuple(target + d * rng.uniform(150.0, 230.0)), tuple(target), (0.0, 0.0, 1.0) if abs(d[2]) < 0.9 else (1.0, 0.0, 0.0),
                              rng.uniform(30.0, 50.0), w, h)


REF_CASES = [  # dims, data type, steps (fractional final steps), world, scene depth, seed
    ((64, 64, 64), np.uint8, 100.5, "plain", False, 11),
    ((96, 80, 72), np.uint16, 130.3, "clip", True, 12),
    ((128, 128, 128), np.float32, 151.7, "clip", False, 13),
]


@pytest.mark.parametrize("case", REF_CASES, ids=["64-u8", "96x80x72-u16-depth", "128-f32"])
def test_frame_matches_the_float64_restatement(gpu, case):
    import torch

    dims, dtype, steps, world_kind, with_depth, seed = case
    rng = np.random.default_rng(seed)
    world = E.ROT_WORLD if world_kind == "clip" else S.default_world()
    vol = S.make_volume_numpy(dims, dtype, 0x5EED0002)
    labels = sphere_labels(dims, [(0.35, 0.4, 0.5), (0.65, 0.55, 0.45), (0.5, 0.5, 0.2)], [0.18, 0.14, 0.1], [1, 3, 6], rng, noise=0.01)
    colors = overlay_colors()
    tf = abi.color_curve_to_lut(S.tf_keys("A"))
    baked = abi.host_bake_tf_lut(tf)
    light = E.seam_light_volume(dims, False)
    ex = X.Scene(vol, baked, abi.WindowingParams(*WINDOW), dims, False)
    ex.set_light(light)
    w, h = 48, 40
    tile = abi.Tile(0, 0, w, h)
    with make_res(dims, dtype, vol=vol) as res:
        res.upload_label_volume(labels)
        res.set_label_colors(colors)
        shown = 0
        for k in range(2):
            cam = _random_camera(rng, w, h)
            jitter = -1 if k == 0 else 4
            rp = abi.RaymarchParams(steps, jitter, True)
            depth = None
            if with_depth:
                depth = (190.0 + 30.0 * rng.random((h, w))).astype(np.float32)
                out = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
                d = torch.from_numpy(depth).cuda()
                res.raymarch_lit_device(cam, tile, rp, world, out.data_ptr(), d.data_ptr())
                res.flush()
                got = out.cpu().numpy().astype(np.float64)
            else:
                got = res.raymarch_lit(cam, tile, rp, world).astype(np.float64)
            ref, taint = LR.raymarch_lit(ex, labels, colors, cam, tile, steps, jitter, world, depth)
            nolab, _ = X.raymarch_lit(ex, cam, tile, steps, jitter, world, depth)
            assert taint.mean() < 0.2, taint.mean()
            d = np.abs(got - ref)[~taint]
            assert d.max() <= 5e-4, f"max untainted |d| {d.max()}"
            shown += int((np.abs(ref - nolab).max(axis=-1)[~taint] > 1e-3).sum())
        assert shown >= 50   # the labels are in the picture


def test_slab_stage_and_slab_resident_handles_refuse_labels(gpu):
    import torch

    dims = (32, 32, 64)
    with abi.Resources(dims, abi.FMT_G16, owned=abi.Slab(0, 32)) as part:
        with pytest.raises(abi.TbrmError) as e:
            part.upload_label_volume(np.zeros(dims[::-1], dtype=np.uint8))
        assert e.value.code == abi.ERR_UNSUPPORTED
        assert not part.has_label_volume()
    cam = S.default_camera(32, 32)
    tile = abi.Tile(0, 0, 32, 32)
    state = torch.zeros((32, 32, 4), dtype=torch.float32, device="cuda")
    with make_res(dims, np.uint16) as res:
        res.upload_label_volume(sphere_labels(dims, [(0.5, 0.5, 0.5)], [0.3], [1]))
        rp = abi.RaymarchParams(64.0, -1, True)
        with pytest.raises(abi.TbrmError) as e:
            res.raymarch_lit_slab_device(cam, tile, rp, S.default_world(), state.data_ptr(), abi.Slab(0, 64), 0)
        assert e.value.code == abi.ERR_UNSUPPORTED
        res.release_label_volume()
        res.raymarch_lit_slab_device(cam, tile, rp, S.default_world(), state.data_ptr(), abi.Slab(0, 64), 0)
        res.flush()
        assert np.allclose(state.cpu().numpy(), res.raymarch_lit(cam, tile, rp, S.default_world()), rtol=0, atol=1e-5)
