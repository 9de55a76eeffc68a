"""The scene matrix shared by tests/test_exact_reference.py (oracle vs the float64 reference) and
tests/test_gpu_exact_reference.py (HIP path vs the float64 reference): where the kernels can go wrong.

A propagation scene is a dict: data dims / type, light-volume format and resolution, data addressing, border mode, TF,
window, world, and a list of operators. A raymarch scene uploads its own light volume (no propagation) and renders one
tile. An Intensity / Octree scene (tests/mode_reference.py) is a raymarch scene without a light volume, plus the kind of
data and the octree level. Runners drive the oracle, the float64 reference and the C-ABI with the same inputs.
"""
import numpy as np

from tbraymarcherplugin_amd import abi, synthetic as S
import exact_reference as X
import mode_reference as M


def _q(axis_deg, angle):
    """unit quaternion (x, y, z, w) of `angle` degrees about a unit axis"""
    a = np.asarray(axis_deg, dtype=np.float64)
    a = a / np.linalg.norm(a)
    h = np.deg2rad(angle) / 2.0
    return (*(a * np.sin(h)), np.cos(h))


def near_axis(weight, lateral=(0.6, 0.8)):
    """a light direction whose primary (-Z face) squared cosine is `weight`: just above / below the 0.99 snap"""
    c = np.sqrt(weight)
    s = np.sqrt(1.0 - weight)
    return (lateral[0] * s, lateral[1] * s, c)   # light shines +z -> light_pos -z -> face -Z


ROT_WORLD = abi.make_world(abi.identity_transform(scale=(100.0, 130.0, 70.0), translation=(10.0, -5.0, 3.0),
                                                  rotation=_q((0.3, 0.2, 0.9), 23.0)),
                           clip_center=(8.0, -2.0, 5.0), clip_direction=(0.3, -0.2, 0.93))


def _clip_outside(voxels, n=40):
    """a clip plane parallel to the x = 0 face, `voxels` light voxels outside it (the volume spans [-50, 50] in world x)"""
    return abi.make_world(abi.identity_transform(100.0), clip_center=(-50.0 - voxels * 100.0 / n, 0.0, 0.0),
                          clip_direction=(1.0, 0.0, 0.0))


# TF with a sharp alpha step at 0.5 and nonzero alpha at 0 (the data border maps to an opaque colour: Change's missing
# guard shows); piecewise-linear keys (t, r, g, b, a)
TF_STEP_KEYS = [(t, list(v)) for t, v in zip(
    [[0.0, 0.499, 0.501, 1.0]] * 4,
    [[0.2, 0.3, 0.9, 1.0], [0.3, 0.4, 0.8, 0.9], [0.6, 0.5, 0.3, 0.2], [0.05, 0.05, 0.6, 0.7]])]

LIGHT_A = ((1.0, .35, -.5), 0.5)
LIGHT_B = ((-.4, 1.0, -.3), 0.4)
LIGHT_C = ((.2, -.3, -1.0), 0.4)
SIX_FACES = [((1, .31, -.22), 0.5), ((-1, .2, .43), 0.6), ((.3, 1, -.21), 0.5), ((.26, -1, .5), 0.7),
             ((.11, .45, 1), 0.5), ((-.35, .2, -1), 0.9)]
OBLIQUE_45 = [((1.0, 0.93, -0.07), 0.6), ((-0.12, -1.0, 0.95), 0.5)]


def prop(name, dims, dtype, ops, light32=True, half=False, addr=abi.ADDRESS_WRAP, border=abi.BORDER_ENGINE_8BIT,
         tf="A", window=(0.5, 0.9, True, False), world=None, seed=0x5EED0002):
    return dict(name=name, dims=dims, dtype=dtype, ops=ops, light32=light32, half=half, addr=addr, border=border, tf=tf,
                window=window, world=world if world is not None else S.default_world(), seed=seed)


def _both(name, *a, **k):
    return [prop(name + "-r32f", *a, light32=True, **k), prop(name + "-u8", *a, light32=False, **k)]


PROP_SCENES = (
    _both("brick-ragged-u16", (33, 40, 17), np.uint16, [("add",) + LIGHT_A, ("add",) + LIGHT_B, ("remove",) + LIGHT_A])
    + _both("aniso-u8-six-faces", (65, 9, 24), np.uint8, [("add",) + l for l in SIX_FACES])
    + _both("flat-f32", (48, 48, 2), np.float32, [("add",) + LIGHT_C, ("add",) + OBLIQUE_45[0]], addr=abi.ADDRESS_CLAMP)
    + _both("one-wide-u16", (1, 30, 30), np.uint16, [("add",) + SIX_FACES[0], ("add",) + SIX_FACES[2], ("add",) + SIX_FACES[5]])
    + _both("half-res-rotated-clip", (45, 40, 37), np.uint16, [("add",) + LIGHT_A, ("add",) + LIGHT_C,
                                                               ("change", LIGHT_C, (S.rotate_z(LIGHT_C[0], -4.0), 0.35))],
            half=True, world=ROT_WORLD)
    + _both("near-axis-099", (24, 20, 28), np.uint16, [("add", near_axis(0.993), 0.8), ("add", near_axis(0.987), 0.7),
                                                       ("change", (near_axis(0.987), 0.7), (near_axis(0.985, (0.8, -0.6)), 0.7)),
                                                       ("change", (near_axis(0.985, (0.8, -0.6)), 0.7), (near_axis(0.983, (0.7, -0.5)), 0.6))])
    + _both("oblique-45-border-rows", (40, 36, 30), np.uint16, [("add",) + l for l in OBLIQUE_45] + [("add", (0.2, 1.0, 1.05), 0.6)],
            border=abi.BORDER_EXACT_FLOAT)
    + _both("intensities", (30, 26, 22), np.float32, [("add", LIGHT_A[0], 0.0), ("add", LIGHT_B[0], 0.3), ("add", LIGHT_C[0], 1.7),
                                                     ("add", SIX_FACES[4][0], 1.3)])
    + _both("clip-1.5-outside", (40, 40, 40), np.uint16, [("add", (1.0, 0.3, -0.2), 0.6), ("add",) + LIGHT_B],
            world=_clip_outside(1.5))
    + _both("clip-2.5-outside", (40, 40, 40), np.uint16, [("add", (1.0, 0.3, -0.2), 0.6), ("add",) + LIGHT_B],
            world=_clip_outside(2.5))
    + _both("step-tf-narrow-window", (36, 30, 34), np.uint16, [("add",) + LIGHT_A, ("add",) + SIX_FACES[3],
                                                               ("change", SIX_FACES[3], (S.rotate_z(SIX_FACES[3][0], 6.0), 0.7))],
            tf="step", window=(0.42, 0.3, True, True))
    + _both("change-fused-fallback", (32, 28, 36), np.uint16,
            [("add",) + LIGHT_A, ("add",) + LIGHT_B, ("change", LIGHT_A, (S.rotate_z(LIGHT_A[0], 5.0), 0.55)),
             ("change", LIGHT_B, ((1.0, 0.1, -0.2), 0.4)), ("remove", (1.0, 0.1, -0.2), 0.4)])
    + _both("batch", (28, 34, 26), np.uint8, [("batch", [LIGHT_A, LIGHT_B, LIGHT_C, SIX_FACES[4]])])
    + [prop("change-border-step-tf-r32f", (30, 30, 30), np.uint16,
            [("add",) + SIX_FACES[0], ("change", SIX_FACES[0], (S.rotate_z(SIX_FACES[0][0], 4.0), 0.5))],
            tf="step", window=(0.4, 0.6, False, False), light32=True)]
)
PROP_IDS = [s["name"] for s in PROP_SCENES]


def tf_lut(name):
    if name == "step":
        return abi.color_curve_to_lut(TF_STEP_KEYS)
    return abi.color_curve_to_lut(S.tf_keys(name))


def volume(scene):
    return S.make_volume_numpy(scene["dims"], scene["dtype"], scene["seed"])


def light_dims(scene):
    return tuple((d + 1) // 2 if scene["half"] else d for d in scene["dims"])


def run_exact(scene, baked_tf, schedule=None):
    """-> (light volume as float64 (UNORM8 as codes), taint, min face / border margins over all lights)"""
    w = abi.WindowingParams(*scene["window"])
    ex = X.Scene(volume(scene), baked_tf, w, light_dims(scene), not scene["light32"], scene["addr"], scene["border"])
    margins = []
    for op in scene["ops"]:
        if op[0] in ("add", "remove"):
            _, m = ex.add_dir_light(op[1], op[2], op[0] == "add", scene["world"])
            margins.append(m)
        elif op[0] == "change":
            _, m = ex.change_dir_light(op[1], op[2], scene["world"])
            margins.append(m)
        else:
            lights = op[1]
            order = schedule if schedule is not None else [(i, p, -1, -1) for i in range(len(lights)) for p in (0, 1)]
            for a, pa, b, pb in order:
                for li, pi in ((a, pa), (b, pb)):
                    if li >= 0:
                        _, m = ex.add_dir_light(lights[li][0], lights[li][1], True, scene["world"], only_pass=pi)
                        margins.append(m)
    return ex.light.astype(np.float64), ex.taint.copy(), margins


def run_oracle(oracle_mod, scene):
    orc = oracle_mod.OracleScene(volume(scene), scene["light32"], scene["half"], scene["addr"], scene["border"])
    orc.set_tf_lut(tf_lut(scene["tf"]))
    orc.set_windowing(abi.WindowingParams(*scene["window"]))
    for op in scene["ops"]:
        if op[0] in ("add", "remove"):
            orc.add_dir_light(abi.DirLightParams(op[1], op[2]), op[0] == "add", scene["world"])
        elif op[0] == "change":
            orc.change_dir_light(abi.DirLightParams(*op[1]), abi.DirLightParams(*op[2]), scene["world"])
        else:
            for l in op[1]:
                orc.add_dir_light(abi.DirLightParams(*l), True, scene["world"])
    return orc.light.astype(np.float64), orc.tf


def run_gpu(scene):
    """-> (light volume float64, the batch schedule the library reported or None)"""
    vol = volume(scene)
    res = abi.Resources(scene["dims"], abi.DTYPE_FMT[np.dtype(scene["dtype"])], scene["light32"], scene["half"], 0,
                        scene["addr"], scene["border"])
    schedule = None
    with res:
        res.upload_volume(vol)
        res.set_tf_lut(tf_lut(scene["tf"]))
        res.set_windowing(abi.WindowingParams(*scene["window"]))
        for op in scene["ops"]:
            if op[0] in ("add", "remove"):
                res.add_dir_light(abi.DirLightParams(op[1], op[2]), op[0] == "add", scene["world"])
            elif op[0] == "change":
                res.change_dir_light(abi.DirLightParams(*op[1]), abi.DirLightParams(*op[2]), scene["world"])
            else:
                schedule = res.add_dir_lights([abi.DirLightParams(*l) for l in op[1]], True, scene["world"])
        out = res.download_light_volume().astype(np.float64)
    return out, schedule


# ------------------------------------------------------------------------------------------------------------------
# raymarch scenes: an uploaded light volume, no propagation

def seam_light_volume(dims, unorm8):
    """smooth field with a strong gradient across the wrap seam on every axis: the far faces' last half texel blends with
    the opposite face's texels (WindowedRaymarchMaterials.usf:30)"""
    nx, ny, nz = dims
    z, y, x = np.meshgrid((np.arange(nz) + 0.5) / nz, (np.arange(ny) + 0.5) / ny, (np.arange(nx) + 0.5) / nx, indexing="ij")
    v = 0.15 + 0.8 * (0.4 * x + 0.35 * y + 0.25 * z) + 0.05 * np.sin(7 * x + 3 * y) * np.cos(5 * z)
    v = np.clip(v, 0.0, 1.0)
    if unorm8:
        return np.floor(v * 255.0 + 0.5).astype(np.uint8)
    return v.astype(np.float32)


def ray(name, dims, dtype, cam, tile, steps, jitter, light32=True, half=False, addr=abi.ADDRESS_WRAP, tf="A",
        window=(0.5, 0.9, True, False), world=None, depth=None):
    return dict(name=name, dims=dims, dtype=dtype, cam=cam, tile=tile, steps=steps, jitter=jitter, light32=light32, half=half,
                addr=addr, border=abi.BORDER_ENGINE_8BIT, tf=tf, window=window,
                world=world if world is not None else S.default_world(), depth=depth, seed=0x5EED0002)


def _inside_camera(w, h):
    return abi.look_at_camera((12.0, -8.0, 5.0), (60.0, 40.0, -30.0), (0.0, 0.0, 1.0), 70.0, w, h)


def _grazing_camera(w, h):
    """looks along the volume's top face: many rays cross only a sliver of the cube (thickness ~ 0)"""
    return abi.look_at_camera((-180.0, -20.0, 50.3), (0.0, 0.0, 49.0), (0.0, 0.0, 1.0), 40.0, w, h)


def _depth(w, h):
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    return (185.0 + 40.0 * np.sin(xx / 9.0) * np.cos(yy / 7.0)).astype(np.float32)


RAY_SCENES = [
    ray("outside-u16-wrap", (48, 40, 44), np.uint16, S.default_camera(96, 80), abi.Tile(0, 0, 96, 80), 64.0, -1),
    ray("outside-u16-jitter", (48, 40, 44), np.uint16, S.default_camera(96, 80), abi.Tile(0, 0, 96, 80), 100.0, 3),
    ray("f32-u8-light-clamp", (33, 40, 17), np.float32, S.default_camera(72, 64), abi.Tile(0, 0, 72, 64), 77.0, 5,
        light32=False, addr=abi.ADDRESS_CLAMP),
    ray("u8-half-res-light", (45, 40, 37), np.uint8, S.default_camera(80, 72), abi.Tile(0, 0, 80, 72), 90.0, 1, half=True),
    ray("inside-camera", (40, 40, 40), np.uint16, _inside_camera(64, 64), abi.Tile(0, 0, 64, 64), 128.0, 2),
    ray("grazing", (40, 40, 40), np.uint16, _grazing_camera(96, 64), abi.Tile(0, 0, 96, 64), 150.0, -1),
    ray("rotated-clip-bone", (48, 40, 44), np.uint16, S.default_camera(96, 80), abi.Tile(0, 0, 96, 80), 96.0, 4,
        tf="B", window=(0.5, 0.8, True, True), world=ROT_WORLD),
    ray("narrow-window-step-tf", (40, 36, 30), np.uint16, S.default_camera(80, 80), abi.Tile(0, 0, 80, 80), 64.0, -1,
        tf="step", window=(0.42, 0.3, True, True)),
    ray("depth-odd-tile-rowgroups", (48, 40, 44), np.uint16, S.default_camera(96, 96), abi.Tile(29, 27, 37, 19, 2), 80.0, 6,
        depth=_depth(96, 96)),
    ray("wrap-seam-opaque-faces", (36, 32, 40), np.uint16, S.default_camera(80, 80), abi.Tile(0, 0, 80, 80), 72.0, 7,
        tf="step", window=(0.4, 0.6, False, False)),
    ray("integer-step-counts", (32, 32, 32), np.uint16, S.default_camera(64, 64), abi.Tile(0, 0, 64, 64), 32.0, -1),
]
RAY_IDS = [s["name"] for s in RAY_SCENES]


def ray_light(scene):
    return seam_light_volume(light_dims(scene), not scene["light32"])


def run_exact_ray(scene, baked_tf):
    w = abi.WindowingParams(*scene["window"])
    ex = X.Scene(volume(scene), baked_tf, w, light_dims(scene), not scene["light32"], scene["addr"], scene["border"])
    ex.set_light(ray_light(scene))
    return X.raymarch_lit(ex, scene["cam"], scene["tile"], scene["steps"], scene["jitter"], scene["world"], scene["depth"])


def run_oracle_ray(oracle_mod, scene):
    orc = oracle_mod.OracleScene(volume(scene), scene["light32"], scene["half"], scene["addr"], scene["border"])
    orc.set_tf_lut(tf_lut(scene["tf"]))
    orc.set_windowing(abi.WindowingParams(*scene["window"]))
    orc.light[...] = ray_light(scene)
    out, _ = orc.raymarch_lit(scene["cam"], scene["tile"], abi.RaymarchParams(scene["steps"], scene["jitter"], True),
                              scene["world"], scene["depth"])
    return out.astype(np.float64), orc.tf


def run_gpu_ray(scene):
    vol = volume(scene)
    res = abi.Resources(scene["dims"], abi.DTYPE_FMT[np.dtype(scene["dtype"])], scene["light32"], scene["half"], 0,
                        scene["addr"], scene["border"])
    with res:
        res.upload_volume(vol)
        res.set_tf_lut(tf_lut(scene["tf"]))
        res.set_windowing(abi.WindowingParams(*scene["window"]))
        res.upload_light_volume(ray_light(scene))
        rp = abi.RaymarchParams(scene["steps"], scene["jitter"], True)
        if scene["depth"] is None:
            return res.raymarch_lit(scene["cam"], scene["tile"], rp, scene["world"]).astype(np.float64)
        import torch
        t = scene["tile"]
        out = torch.empty((t.h, t.w, 4), dtype=torch.float32, device="cuda")
        depth = torch.from_numpy(scene["depth"]).cuda()
        res.raymarch_lit_device(scene["cam"], t, rp, scene["world"], out.data_ptr(), depth.data_ptr())
        res.flush()
        return out.cpu().numpy().astype(np.float64)


# ------------------------------------------------------------------------------------------------------------------
# Intensity and Octree render modes (tests/mode_reference.py): no light volume, no propagation

def _clip_world(center, direction, transform=None):
    return abi.make_world(transform if transform is not None else abi.identity_transform(100.0),
                          clip_center=center, clip_direction=direction)


CLIP_THROUGH = _clip_world((6.0, -4.0, 3.0), (0.75, 0.5, -0.43))     # oblique, through the volume; keeps the far side
CLIP_THROUGH_NEAR = _clip_world((-20.0, -18.0, 12.0), (-0.6, -0.7, 0.4))  # keeps the corner nearest the default camera
CLIP_ALL = _clip_world((200.0, 0.0, 0.0), (1.0, 0.0, 0.0))            # every position lies on the clipped side
CLIP_FAR = _clip_world((-400.0, 0.0, 0.0), (1.0, 0.0, 0.0))           # clips nothing, far enough for the host's "never clips" path


def _opposite_camera(w, h):
    """from the +x +y +z side: rays leave through the volume's x = 0, y = 0 and z = 0 faces"""
    return abi.look_at_camera((150.0, 110.0, 95.0), (0.0, 0.0, 0.0), (0.0, 0.0, 1.0), 55.0, w, h)


def lifted_volume(dims, dtype, seed, wide=False):
    """the synthetic volume on top of a ramp, so that the cube's faces (where the synthetic volume is empty) show an intensity
    inside the window too; `wide` stretches f32 data to [-0.14, 1.3]: values below 0 and above 1"""
    nx, ny, nz = dims
    z, y, x = np.meshgrid((np.arange(nz) + 0.5) / nz, (np.arange(ny) + 0.5) / ny, (np.arange(nx) + 0.5) / nx, indexing="ij")
    v = 0.1 + 0.3 * (x + 2.0 * y + 3.0 * z) / 6.0 + 0.6 * S.make_volume_numpy(dims, np.float32, seed).astype(np.float64)
    if wide:
        v = v * 1.6 - 0.3
    if np.dtype(dtype) == np.float32:
        return v.astype(np.float32)
    scale = 255.0 if np.dtype(dtype) == np.uint8 else 65535.0
    return np.floor(np.clip(v, 0.0, 1.0) * scale + 0.5).astype(dtype)


def block_volume(dims, dtype, seed, block=(5, 6, 7), offset=(2, 3, 1), empty=0.45):
    """piecewise constant over blocks of a few voxels whose boundaries do not follow the pyramid's power-of-two grid; a share
    `empty` of the blocks holds a value the default window cuts off. f32 volumes span [-0.25, 1.3]."""
    rng = np.random.default_rng(seed)
    nx, ny, nz = dims
    nb = [(d + o) // b + 2 for d, b, o in zip((nx, ny, nz), block, offset)]
    palette = np.array([0.02, 0.2, 0.35, 0.5, 0.62, 0.75, 0.88, 1.0])
    pick = rng.integers(1, len(palette), size=(nb[2], nb[1], nb[0]))
    pick[rng.random(pick.shape) < empty] = 0
    z, y, x = np.meshgrid((np.arange(nz) + offset[2]) // block[2], (np.arange(ny) + offset[1]) // block[1],
                          (np.arange(nx) + offset[0]) // block[0], indexing="ij")
    v = palette[pick[z, y, x]]
    if np.dtype(dtype) == np.float32:
        return (v * 1.55 - 0.25).astype(np.float32)
    scale = 255.0 if np.dtype(dtype) == np.uint8 else 65535.0
    return np.floor(v * scale + 0.5).astype(dtype)


def mode_volume(scene):
    kind = scene.get("data", "synthetic")
    if kind == "blocks":
        return block_volume(scene["dims"], scene["dtype"], scene["seed"], block=scene.get("block", (5, 6, 7)),
                            empty=scene.get("empty", 0.45))
    if kind in ("lifted", "f32-wide"):
        return lifted_volume(scene["dims"], scene["dtype"], scene["seed"], wide=kind == "f32-wide")
    return volume(scene)


def mode(name, dims, dtype, cam, tile, steps, jitter, data="lifted", mip=0, block=(5, 6, 7), empty=0.45, shows="hit", **k):
    """shows (intensity): "both" hit and no-hit pixels where the clip plane cuts the volume, "none" where it removes all"""
    s = ray(name, dims, dtype, cam, tile, steps, jitter, **k)
    s.update(data=data, mip=mip, block=block, empty=empty, shows=shows)
    return s


def _full(w, h):
    return abi.Tile(0, 0, w, h)


INTENSITY_SCENES = [
    mode("outside-u16-wrap", (48, 40, 44), np.uint16, S.default_camera(96, 80), _full(96, 80), 64.0, -1),
    mode("clip-through-u8-jitter-fractional", (45, 40, 37), np.uint8, S.default_camera(80, 72), _full(80, 72), 90.5, 3,
         shows="both", world=CLIP_THROUGH),
    mode("clip-near-side-clamp", (48, 40, 44), np.uint16, S.default_camera(96, 80), _full(96, 80), 77.0, 1,
         addr=abi.ADDRESS_CLAMP, shows="both", world=CLIP_THROUGH_NEAR),
    mode("f32-out-of-range-rotated-clip", (33, 40, 17), np.float32, S.default_camera(72, 64), _full(72, 64), 77.0, 5,
         data="f32-wide", shows="both", world=ROT_WORLD),
    mode("inside-camera-pow2-integer-steps", (32, 32, 32), np.uint16, _inside_camera(64, 64), _full(64, 64), 32.0, -1),
    mode("grazing", (40, 40, 40), np.uint16, _grazing_camera(96, 64), _full(96, 64), 150.0, 2),
    mode("one-wide-axis", (1, 30, 30), np.uint16, S.default_camera(64, 64), _full(64, 64), 48.0, 6),
    mode("tiny-volume", (5, 6, 3), np.uint8, S.default_camera(64, 64), _full(64, 64), 40.0, -1),
    mode("clip-removes-everything", (40, 36, 30), np.uint16, S.default_camera(64, 64), _full(64, 64), 50.0, 4, shows="none", world=CLIP_ALL),
    mode("clip-far-outside", (40, 36, 30), np.uint16, S.default_camera(64, 64), _full(64, 64), 50.0, 4, world=CLIP_FAR),
    mode("steps-below-1-clip-jitter", (48, 40, 44), np.uint16, S.default_camera(96, 80), _full(96, 80), 0.5, 2,
         shows="both", world=CLIP_THROUGH_NEAR),
    mode("steps-below-1-no-jitter", (40, 36, 30), np.uint16, _opposite_camera(64, 64), _full(64, 64), 0.75, -1),
    mode("depth-sub-tile-rowgroups", (48, 40, 44), np.uint16, S.default_camera(96, 96), abi.Tile(29, 27, 37, 19, 2), 80.0, 6,
         depth=_depth(96, 96), shows="both", world=CLIP_THROUGH),
    mode("narrow-window", (40, 36, 30), np.uint16, S.default_camera(80, 80), _full(80, 80), 64.0, 7,
         window=(0.42, 0.3, True, True)),
]
INTENSITY_IDS = [s["name"] for s in INTENSITY_SCENES]

OCTREE_SCENES = [
    mode("u16-ragged-mip0", (44, 40, 37), np.uint16, S.default_camera(96, 80), _full(96, 80), 64.0, 3, data="blocks"),
    mode("u16-ragged-mip1-cutoffs-off", (44, 40, 37), np.uint16, S.default_camera(96, 80), _full(96, 80), 70.5, 1, data="blocks",
         mip=1, window=(0.5, 0.9, False, False)),
    mode("u8-mip2-rotated-clip", (45, 40, 37), np.uint8, S.default_camera(80, 72), _full(80, 72), 90.0, 5, data="blocks", mip=2,
         world=ROT_WORLD),
    mode("f32-out-of-range-mip3", (33, 40, 17), np.float32, S.default_camera(72, 64), _full(72, 64), 77.0, 2, data="blocks",
         mip=3, addr=abi.ADDRESS_CLAMP),
    mode("f32-mip0-clip-through", (33, 40, 17), np.float32, S.default_camera(72, 64), _full(72, 64), 60.0, 4, data="blocks",
         world=CLIP_THROUGH),
    mode("pow2-cube-no-jitter-exit-faces", (32, 32, 32), np.uint16, _opposite_camera(64, 64), _full(64, 64), 32.0, -1,
         data="blocks", empty=0.25),
    mode("pow2-cube-mip1-inside-camera", (32, 32, 32), np.uint16, _inside_camera(64, 64), _full(64, 64), 100.0, 2, data="blocks",
         mip=1),
    mode("grazing-mip0", (40, 40, 40), np.uint16, _grazing_camera(96, 64), _full(96, 64), 150.0, 6, data="blocks"),
    mode("one-wide-axis-mip1", (1, 30, 30), np.uint16, S.default_camera(64, 64), _full(64, 64), 48.0, 7, data="blocks", mip=1),
    mode("tiny-volume-mip2", (5, 6, 3), np.uint8, S.default_camera(64, 64), _full(64, 64), 40.0, 0, data="blocks", mip=2,
         block=(2, 3, 2)),
    mode("tiny-volume-mip3", (5, 6, 3), np.uint8, S.default_camera(64, 64), _full(64, 64), 40.5, -1, data="blocks", mip=3,
         block=(2, 3, 2)),
    mode("step-tf-narrow-window-mip0", (40, 36, 30), np.uint16, S.default_camera(80, 80), _full(80, 80), 64.0, 1, data="blocks",
         tf="step", window=(0.42, 0.3, True, True)),
    mode("steps-below-1-jitter-mip0", (44, 40, 37), np.uint16, S.default_camera(96, 80), _full(96, 80), 0.7, 2, data="blocks",
         empty=0.25),
    mode("steps-below-1-jitter-mip2-clip", (45, 40, 37), np.uint8, S.default_camera(80, 72), _full(80, 72), 0.9, 5, data="blocks",
         mip=2, world=CLIP_THROUGH_NEAR, empty=0.25),
    mode("clip-far-outside-mip1", (40, 36, 30), np.uint16, S.default_camera(64, 64), _full(64, 64), 50.0, 4, data="blocks",
         mip=1, world=CLIP_FAR),
    mode("depth-sub-tile-rowgroups-mip1", (48, 40, 44), np.uint16, S.default_camera(96, 96), abi.Tile(29, 27, 37, 19, 2), 80.0, 6,
         data="blocks", mip=1, depth=_depth(96, 96)),
]
OCTREE_IDS = [s["name"] for s in OCTREE_SCENES]

# volumes whose pyramid is compared texel by texel (the octree scenes' own volumes are compared too)
PYRAMID_VOLUMES = [
    ("synthetic-u8-ragged", (45, 40, 37), np.uint8, "synthetic"),
    ("synthetic-u16-ragged", (33, 40, 17), np.uint16, "synthetic"),
    ("synthetic-f32-out-of-range", (33, 40, 17), np.float32, "f32-wide"),
    ("synthetic-f32-pow2", (32, 32, 32), np.float32, "synthetic"),
    ("blocks-f32", (44, 40, 37), np.float32, "blocks"),
    ("one-wide-u16", (1, 30, 30), np.uint16, "synthetic"),
    ("tiny-u8", (5, 6, 3), np.uint8, "synthetic"),
    ("tiny-f32", (3, 2, 7), np.float32, "f32-wide"),
]
PYRAMID_IDS = [p[0] for p in PYRAMID_VOLUMES]


def pyramid_volume(entry):
    _, dims, dtype, kind = entry
    return mode_volume(dict(dims=dims, dtype=dtype, seed=0x5EED0002, data=kind))


def _exact_scene(scene, baked_tf):
    w = abi.WindowingParams(*scene["window"])
    return X.Scene(mode_volume(scene), baked_tf, w, light_dims(scene), not scene["light32"], scene["addr"], scene["border"])


def crossing_rays(scene):
    """the tile's pixels whose ray crosses the cube (before the depth limit)"""
    return X.cube_setup(scene["cam"], scene["world"], scene["tile"], scene["depth"])[1] > 0.0


def run_exact_intensity(scene, baked_tf):
    return M.raymarch_intensity(_exact_scene(scene, baked_tf), scene["cam"], scene["tile"], scene["steps"], scene["jitter"],
                                scene["world"], scene["depth"])


def run_exact_octree(scene, baked_tf):
    vol = mode_volume(scene)
    return M.raymarch_octree(_exact_scene(scene, baked_tf), M.generate_octree(vol), scene["mip"], scene["cam"], scene["tile"],
                             scene["steps"], scene["jitter"], scene["world"], scene["depth"], texel_taint=M.octree_taint(vol))


def _oracle_scene(oracle_mod, scene):
    orc = oracle_mod.OracleScene(mode_volume(scene), scene["light32"], scene["half"], scene["addr"], scene["border"])
    orc.set_tf_lut(tf_lut(scene["tf"]))
    orc.set_windowing(abi.WindowingParams(*scene["window"]))
    return orc


def run_oracle_intensity(oracle_mod, scene):
    orc = _oracle_scene(oracle_mod, scene)
    rp = abi.RaymarchParams(scene["steps"], scene["jitter"], True)
    return orc.raymarch_intensity(scene["cam"], scene["tile"], rp, scene["world"], scene["depth"]).astype(np.float64), orc.tf


def run_oracle_octree(oracle_mod, scene):
    orc = _oracle_scene(oracle_mod, scene)
    rp = abi.RaymarchParams(scene["steps"], scene["jitter"], True)
    out = orc.raymarch_octree(scene["cam"], scene["tile"], rp, scene["world"], scene["mip"], scene["depth"])
    return out.astype(np.float64), orc.tf


def _gpu_resources(scene):
    res = abi.Resources(scene["dims"], abi.DTYPE_FMT[np.dtype(scene["dtype"])], scene["light32"], scene["half"], 0,
                        scene["addr"], scene["border"])
    res.upload_volume(mode_volume(scene))
    res.set_tf_lut(tf_lut(scene["tf"]))
    res.set_windowing(abi.WindowingParams(*scene["window"]))
    return res


def _device_frame(scene, launch):
    """a frame through a `_device` entry point with the scene's depth buffer: launch(out pointer, depth pointer)"""
    import torch
    t = scene["tile"]
    out = torch.empty((t.h, t.w, 4), dtype=torch.float32, device="cuda")
    depth = torch.from_numpy(scene["depth"]).cuda()
    launch(out.data_ptr(), depth.data_ptr())
    return out, depth


def run_gpu_intensity(scene):
    rp = abi.RaymarchParams(scene["steps"], scene["jitter"], True)
    with _gpu_resources(scene) as res:
        if scene["depth"] is None:
            return res.raymarch_intensity(scene["cam"], scene["tile"], rp, scene["world"]).astype(np.float64)
        out, _depth_alive = _device_frame(scene, lambda o, d: res.raymarch_intensity_device(scene["cam"], scene["tile"], rp,
                                                                                           scene["world"], o, d))
        res.flush()
        return out.cpu().numpy().astype(np.float64)


def run_gpu_octree(scene):
    import ctypes as C
    rp = abi.RaymarchParams(scene["steps"], scene["jitter"], True)
    with _gpu_resources(scene) as res:
        res.generate_octree()
        if scene["depth"] is None:
            return res.raymarch_octree(scene["cam"], scene["tile"], rp, scene["world"], scene["mip"]).astype(np.float64)

        def launch(o, d):
            abi.check(res.lib.tbrm_raymarch_octree_device(res.handle, C.byref(scene["cam"]), C.byref(scene["tile"]), C.byref(rp),
                                                          C.byref(scene["world"]), int(scene["mip"]), C.c_void_p(d), C.c_void_p(o)))
        out, _depth_alive = _device_frame(scene, launch)
        res.flush()
        return out.cpu().numpy().astype(np.float64)
