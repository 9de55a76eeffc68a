"""The float64 restatement of the label overlay (tests/label_reference.py) against exact_reference and a hand-computed answer."""
import numpy as np
import pytest

from tbraymarcherplugin_amd import abi
import exact_reference as X
import exact_scenes as E
import label_reference as LR

SLAB_STEPS = 15.5
SLAB_COLOR = (1.0, 0.5, 0.0, 0.01)
SLAB_Z = (4, 8)   # label 1 in voxel layers [4, 8) of a 16^3 volume


def slab_setup():
    """A 16^3 volume whose TF has alpha 0 everywhere, label 1 in the full x-y extent of z layers [4, 8), and the one-pixel camera
    whose ray runs down the volume's z axis (local z from 1 to 0, thickness exactly 1): with 15.5 steps, full sample k = 1 .. 15
    reads label layer rint(15 (1 - k / 15.5)) (k = 8 .. 11: layers 7 .. 4, none near a rounding boundary), the fractional one
    layer 0."""
    dims = (16, 16, 16)
    vol = E.S.make_volume_numpy(dims, np.uint16, 0x5EED0002)
    tf = np.zeros((256, 4), dtype=np.float32)
    tf[:, :3] = 0.7                                  # colour, but alpha 0: the data adds nothing
    labels = np.zeros(dims[::-1], dtype=np.uint8)
    labels[SLAB_Z[0]:SLAB_Z[1]] = 1
    colors = np.zeros((256, 4), dtype=np.float32)
    colors[1] = SLAB_COLOR
    cam = abi.Camera(abi.Vec3d(0.0, 0.0, 200.0), abi.Vec3d(0.0, 0.0, -1.0), abi.Vec3d(1.0, 0.0, 0.0), abi.Vec3d(0.0, 1.0, 0.0),
                     0.1, 0.1, 1, 1)
    return dims, vol, tf, labels, colors, cam, abi.Tile(0, 0, 1, 1), abi.make_world()


def slab_answer():
    """four full samples of colour c, each with a' = 1 - (1 - c.a)^(100 / steps): LE.a = 1 - (1 - c.a)^(4 * 100 / steps),
    LE.rgb = c.rgb LE.a"""
    n = SLAB_Z[1] - SLAB_Z[0]
    c = np.float32(SLAB_COLOR).astype(np.float64)   # (the table holds float32)
    a = 1.0 - (1.0 - c[3]) ** (n * 100.0 / SLAB_STEPS)
    return np.array([c[0] * a, c[1] * a, c[2] * a, a])


def _exact_scene(scene, baked):
    ex = X.Scene(E.volume(scene), baked, abi.WindowingParams(*scene["window"]), E.light_dims(scene), not scene["light32"],
                 scene["addr"], scene["border"])
    ex.set_light(E.ray_light(scene))
    return ex


@pytest.mark.parametrize("scene", [s for s in E.RAY_SCENES if s["name"] in ("outside-u16-jitter", "f32-u8-light-clamp",
                                                                           "depth-odd-tile-rowgroups", "rotated-clip-bone")],
                         ids=lambda s: s["name"])
def test_all_clear_table_equals_exact_reference(scene, abi_mod):
    baked = abi.host_bake_tf_lut(E.tf_lut(scene["tf"]))
    ex = _exact_scene(scene, baked)
    labels = np.random.default_rng(7).integers(0, 256, size=scene["dims"][::-1], dtype=np.uint8)
    clear = np.zeros((256, 4), dtype=np.float32)
    clear[:, :3] = 0.8                               # colour without alpha shows nothing
    args = (scene["cam"], scene["tile"], scene["steps"], scene["jitter"], scene["world"], scene["depth"])
    want, wtaint = X.raymarch_lit(ex, *args)
    got, gtaint = LR.raymarch_lit(ex, labels, clear, *args)
    assert np.array_equal(got, want) and np.array_equal(gtaint, wtaint)


def test_slab_of_one_label_known_answer(abi_mod):
    dims, vol, tf, labels, colors, cam, tile, world = slab_setup()
    ex = X.Scene(vol, tf, abi.WindowingParams(0.5, 1.0, False, False), dims, False)
    ex.set_light(np.full(dims[::-1], 0.5))
    got, taint = LR.raymarch_lit(ex, labels, colors, cam, tile, SLAB_STEPS, -1, world)
    assert not taint.any()
    assert np.allclose(got[0, 0], slab_answer(), rtol=0, atol=1e-12), (got[0, 0], slab_answer())
    # the same ray without the label step: nothing
    none, _ = X.raymarch_lit(ex, cam, tile, SLAB_STEPS, -1, world)
    assert not none.any()


def test_default_colors_and_rounding_reading():
    c = LR.default_label_colors()
    assert np.array_equal(c[:3], [[0, 0, 0, 0], [1, 0, 0, 0.5], [0, 1, 0, 0.5]]) and (c[3:] == [0, 0, 0, 1]).all()
    # HLSL round is round-half-to-even: (N - 1) * 0.5 = 7.5 of a 16-wide axis reads voxel 8, 6.5 reads 6
    labels = np.zeros((1, 1, 16), dtype=np.uint8)
    labels[0, 0, 8] = 1
    labels[0, 0, 6] = 2
    q = np.array([[0.5, 0.0, 0.0], [6.5 / 15.0, 0.0, 0.0]])
    col, _ = LR.label_lookup(labels, c, q, 0.0)
    assert np.array_equal(col[:, 3], [0.5, 0.5]) and col[0, 0] == 1.0 and col[1, 1] == 1.0
