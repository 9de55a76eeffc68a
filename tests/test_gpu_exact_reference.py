"""The HIP path against the independent float64 restatement (tests/exact_reference.py), through the C-ABI — directly,
not via the oracle. Scene matrix and runners: tests/exact_scenes.py; tolerances: tests/test_exact_reference.py (calibrated
there on the oracle, which the UNORM8 kernels match bit for bit).
"""
import numpy as np
import pytest

from tbraymarcherplugin_amd import abi
import exact_reference as X
import exact_scenes as E
from test_exact_reference import TAINT_CAP, prop_compare, ray_tol

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
