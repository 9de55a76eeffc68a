"""The HIP path against the independent float64 restatement (tests/exact_reference.py), through the C-ABI — directly,
not via the oracle. Scene matrix and runners: tests/exact_scenes.py; tolerances: tests/test_exact_reference.py (calibrated
there on the oracle, which the UNORM8 kernels match bit for bit).
"""
import numpy as np
import pytest

from tbraymarcherplugin_amd import abi
import exact_reference as X
import exact_scenes as E
from test_exact_reference import (TAINT_CAP, OCTREE_TAINT_CAP, PYRAMID_TAINT_CAP, RGBA_TOL, prop_compare, ray_tol, mode_tol, frame_delta,
                                  pyramid_compare, intensity_shows)

pytestmark = pytest.mark.gpu

BIG_TOL = 1e-4   # 256^3, 256-slice passes: per-slice fp32 error k * 2^-24 with k <= 2 measured at <= 65 slices
                 # (max 6e-6 over ~ 100 dependent slices) -> <= 256 * 4 * 2 * 2^-24 = 1.2e-4 worst case; asserted at the north star
BIG_RGBA_TOL = 5e-4  # 256 steps through 256^3 data: the fp32 position sum's error (<= 256 * 2^-24 UVW = 0.004 texel) times the
                     # data's texel-scale gradients reaches the colour through TF and opacity correction; measured 2.5e-4


@pytest.fixture(params=["sweep", "chunk", "slice"])
def kernel_variant(request, tunables):
    tunables("force_slice_kernel", 1 if request.param == "slice" else 0)
    tunables("light_sweep", 1 if request.param == "sweep" else 0)
    return request.param


@pytest.fixture(params=["4", "8"])
def ray_lanes(request, tunables):
    tunables("ray_lanes", int(request.param))
    return request.param


def _prop_check(scene):
    got, schedule = E.run_gpu(scene)
    baked = abi.host_bake_tf_lut(E.tf_lut(scene["tf"]))
    e, taint, _ = E.run_exact(scene, baked, schedule)
    assert taint.mean() < TAINT_CAP
    ok, worst, exact = prop_compare(scene["light32"], got, e, taint)
    assert ok, f"{scene['name']}: max untainted |d| {worst}, exact {exact}, tainted {taint.mean():.4f}"
    return got


def _ray_check(scene):
    got = E.run_gpu_ray(scene)
    baked = abi.host_bake_tf_lut(E.tf_lut(scene["tf"]))
    e, taint = E.run_exact_ray(scene, baked)
    assert taint.mean() < TAINT_CAP
    d = np.abs(got - e)[~taint]
    assert d.max() <= ray_tol(scene), f"{scene['name']}: max untainted |d| {d.max()}"
    return got


@pytest.mark.parametrize("scene", E.PROP_SCENES, ids=E.PROP_IDS)
def test_propagation_matches_float64_reference(gpu, scene, kernel_variant):
    _prop_check(scene)


@pytest.mark.parametrize("scene", E.RAY_SCENES, ids=E.RAY_IDS)
def test_raymarch_matches_float64_reference(gpu, scene, ray_lanes):
    _ray_check(scene)


# every A/B switch README calls result-neutral, at its non-default value: bit-identical to the default path, and within
# bound of the float64 reference
SWITCHES = [("ray_tables", 0), ("share_grid", 0), ("chain_fast_loop", 0), ("sweep_prefetch", 1), ("occ_slices", 8),
            ("fast_window_div", 0), ("chunk_steps", 4)]
SWITCH_PROP = [s for s in E.PROP_SCENES if s["name"] in ("brick-ragged-u16-u8", "half-res-rotated-clip-r32f",
                                                          "change-fused-fallback-u8", "step-tf-narrow-window-u8")]
SWITCH_RAY = [s for s in E.RAY_SCENES if s["name"] in ("outside-u16-jitter", "rotated-clip-bone", "depth-odd-tile-rowgroups")]


@pytest.mark.parametrize("switch,value", SWITCHES, ids=[s[0] for s in SWITCHES])
def test_switches_are_result_neutral(gpu, tunables, switch, value):
    default = abi.get_tunable(switch)
    assert default != value
    for scene in SWITCH_PROP:
        tunables(switch, default)
        base, _ = E.run_gpu(scene)
        tunables(switch, value)
        got = _prop_check(scene)
        assert np.array_equal(got, base), f"{switch}={value} changed {scene['name']}"
    for scene in SWITCH_RAY:
        tunables(switch, default)
        base = E.run_gpu_ray(scene)
        tunables(switch, value)
        got = _ray_check(scene)
        assert np.array_equal(got, base), f"{switch}={value} changed {scene['name']}"


def test_256_cube_two_oblique_lights_and_change(gpu):
    """A 256^3 R32F light volume, two oblique lights plus a Change, and a 256^2 frame of the result."""
    scene = E.prop("big-256", (256, 256, 256), np.uint16,
                   [("add",) + E.LIGHT_A, ("add",) + E.OBLIQUE_45[1],
                    ("change", E.LIGHT_A, (E.S.rotate_z(E.LIGHT_A[0], 5.0), 0.55))], light32=True)
    vol = E.volume(scene)
    baked = abi.host_bake_tf_lut(E.tf_lut(scene["tf"]))
    w = abi.WindowingParams(*scene["window"])
    res = abi.Resources(scene["dims"], abi.FMT_G16, True, False, 0, scene["addr"], scene["border"])
    cam = E.S.default_camera(256, 256)
    tile = abi.Tile(0, 0, 256, 256)
    with res:
        res.upload_volume(vol)
        res.set_tf_lut(E.tf_lut(scene["tf"]))
        res.set_windowing(w)
        for op in scene["ops"]:
            if op[0] == "add":
                res.add_dir_light(abi.DirLightParams(op[1], op[2]), True, scene["world"])
            else:
                res.change_dir_light(abi.DirLightParams(*op[1]), abi.DirLightParams(*op[2]), scene["world"])
        got = res.download_light_volume().astype(np.float64)
        frame = res.raymarch_lit(cam, tile, abi.RaymarchParams(256.0, 2, True), scene["world"]).astype(np.float64)
    e, taint, _ = E.run_exact(scene, baked)
    assert taint.mean() < TAINT_CAP
    d = np.abs(got - e)[~taint]
    assert d.max() <= BIG_TOL, f"256^3 light volume: max untainted |d| {d.max()}"
    ex = X.Scene(vol, baked, w, scene["dims"], False)
    ex.set_light(got)   # the frame is checked on the light volume the kernels produced
    ref, rtaint = X.raymarch_lit(ex, cam, tile, 256.0, 2, scene["world"])
    assert rtaint.mean() < TAINT_CAP
    assert np.abs(frame - ref)[~rtaint].max() <= BIG_RGBA_TOL


# ------------------------------------------------------------------------------------------------------------------
# Intensity and Octree render modes (tests/mode_reference.py). Each of the misreadings test_exact_reference proves the
# comparison catches on the oracle would be caught here too: the kernels are tied to the oracle bit for bit
# (tests/test_gpu_parity.py), and these tests hold them to the restatement with the same scenes, bounds and caps.

def _baked(scene):
    return abi.host_bake_tf_lut(E.tf_lut(scene["tf"]))


def _download_pyramid(res):
    return [res.download_octree_mip(m) for m in range(4)]


@pytest.mark.parametrize("scene", E.INTENSITY_SCENES, ids=E.INTENSITY_IDS)
def test_intensity_matches_float64_reference(gpu, scene):
    got = E.run_gpu_intensity(scene)
    e, taint = E.run_exact_intensity(scene, _baked(scene))
    worst = frame_delta(got, e, taint)
    print(f"intensity {scene['name']}: max untainted |d| {worst:.3g}, tainted {taint.mean():.4f}")
    assert taint.mean() < TAINT_CAP
    assert worst <= mode_tol(scene), f"{scene['name']}: max untainted |d| {worst}"
    assert intensity_shows(scene, got)


@pytest.mark.parametrize("scene", E.OCTREE_SCENES, ids=E.OCTREE_IDS)
def test_octree_march_matches_float64_reference(gpu, scene):
    got = E.run_gpu_octree(scene)
    e, taint = E.run_exact_octree(scene, _baked(scene))
    worst = frame_delta(got, e, taint)
    print(f"octree {scene['name']}: max untainted |d| {worst:.3g}, tainted {taint.mean():.4f}")
    assert taint.mean() < OCTREE_TAINT_CAP
    assert worst <= mode_tol(scene), f"{scene['name']}: max untainted |d| {worst}"
    assert (got[..., 3] > 0.05).mean() > 0.02


@pytest.mark.parametrize("entry", E.PYRAMID_VOLUMES, ids=E.PYRAMID_IDS)
def test_pyramid_matches_float64_reference(gpu, entry):
    vol = E.pyramid_volume(entry)
    with abi.Resources(entry[1], abi.DTYPE_FMT[np.dtype(entry[2])]) as res:
        res.upload_volume(vol)
        res.generate_octree()
        got = _download_pyramid(res)
    ok, why, share = pyramid_compare(got, vol)
    assert ok, f"{entry[0]}: {why}"
    assert share < PYRAMID_TAINT_CAP


def test_pyramid_regenerated_for_a_second_volume(gpu):
    """generate, upload other data, generate again: the second pyramid and a frame marched through it belong to the second
    volume"""
    scene = next(s for s in E.OCTREE_SCENES if s["name"] == "u16-ragged-mip1-cutoffs-off")
    second = dict(scene, seed=scene["seed"] + 17)
    first_vol, second_vol = E.mode_volume(scene), E.mode_volume(second)
    assert (first_vol != second_vol).mean() > 0.3
    rp = abi.RaymarchParams(scene["steps"], scene["jitter"], True)
    with abi.Resources(scene["dims"], abi.FMT_G16, True, False, 0, scene["addr"], scene["border"]) as res:
        res.set_tf_lut(E.tf_lut(scene["tf"]))
        res.set_windowing(abi.WindowingParams(*scene["window"]))
        res.upload_volume(first_vol)
        res.generate_octree()
        ok, why, _ = pyramid_compare(_download_pyramid(res), first_vol)
        assert ok, "first volume: " + why
        res.upload_volume(second_vol)
        res.generate_octree()
        got = _download_pyramid(res)
        frame = res.raymarch_octree(scene["cam"], scene["tile"], rp, scene["world"], scene["mip"]).astype(np.float64)
    ok, why, _ = pyramid_compare(got, second_vol)
    assert ok, "second volume: " + why
    assert not pyramid_compare(got, first_vol)[0]
    e, taint = E.run_exact_octree(second, _baked(scene))
    assert taint.mean() < OCTREE_TAINT_CAP
    assert frame_delta(frame, e, taint) <= mode_tol(scene)


BIG_MODE_DIMS = (256, 192, 160)


def test_256_class_intensity_and_octree(gpu):
    """256 x 192 x 160 u16: the pyramid, a 256^2 frame of 256 steps through each of its levels, and an intensity frame of the
    same size cut by a clip plane; bounds as for the small scenes."""
    cam, tile = E.S.default_camera(256, 256), abi.Tile(0, 0, 256, 256)
    oct_scene = E.mode("big-octree", BIG_MODE_DIMS, np.uint16, cam, tile, 256.0, 3, data="blocks", block=(19, 23, 17))
    int_scene = E.mode("big-intensity", BIG_MODE_DIMS, np.uint16, cam, tile, 256.0, 3, world=E.CLIP_THROUGH, shows="both")
    rp = abi.RaymarchParams(256.0, 3, True)
    vol = E.mode_volume(oct_scene)
    frames = []
    with E._gpu_resources(oct_scene) as res:
        res.generate_octree()
        pyramid = _download_pyramid(res)
        for mip in range(4):
            frames.append(res.raymarch_octree(cam, tile, rp, oct_scene["world"], mip).astype(np.float64))
    got_int = E.run_gpu_intensity(int_scene)
    ok, why, _ = pyramid_compare(pyramid, vol)
    assert ok, why
    for mip in range(4):
        e, taint = E.run_exact_octree(dict(oct_scene, mip=mip), _baked(oct_scene))
        worst = frame_delta(frames[mip], e, taint)
        print(f"256-class octree level {mip}: max untainted |d| {worst:.3g}, tainted {taint.mean():.4f}")
        assert taint.mean() < OCTREE_TAINT_CAP
        assert worst <= RGBA_TOL, f"level {mip}: max untainted |d| {worst}"
        assert (frames[mip][..., 3] > 0.05).mean() > 0.02
    e, taint = E.run_exact_intensity(int_scene, _baked(int_scene))
    worst = frame_delta(got_int, e, taint)
    print(f"256-class intensity: max untainted |d| {worst:.3g}, tainted {taint.mean():.4f}")
    assert taint.mean() < TAINT_CAP
    assert worst <= RGBA_TOL, f"intensity: max untainted |d| {worst}"
    assert intensity_shows(int_scene, got_int)
