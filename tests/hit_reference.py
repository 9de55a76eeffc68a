"""Float64 restatement of the hit march (TEST INFRASTRUCTURE ONLY), built on tests/exact_reference.py and tests/label_reference.py.

The semantics are include/tbrm_hit.h's: every ray is marched as exact_reference.raymarch_lit marches it — cube setup,
scene depth, jitter, step count, fractional last step, clip test, window, transfer function, opacity correction, and with a label
volume the unlit label step behind every data step — tracking the accumulated opacity alone. The hit is the first sample after whose
steps that opacity is > threshold, the fractional step included; the march ends there. Nothing here is taken from the kernels.

Decision taint: everything raymarch_lit taints on the way to the hit (MaxSteps / FinalStep near an integer, a sample near the clip
plane, a window position near a cut-off that decides something), with |alpha - threshold| < DELTA_EXIT in place of the 0.95 test,
and with a label volume label_reference's taint (a nearest-voxel index near a .5 boundary whose neighbour has another colour).
"""
import functools

import numpy as np

from tbraymarcherplugin_amd import abi
import exact_reference as X
import exact_scenes as E
import label_reference as LR


def unit_cube_to_world(world, uvw):
    """FTransform::TransformPosition of uvw - 0.5: scale, rotate, translate"""
    t = world.volume_transform
    return X._quat_rotate(t.rotation, (np.asarray(uvw, dtype=np.float64) - 0.5) * X._v(t.scale3d)) + X._v(t.translation)


def depth_along_forward(world, camera, uvw):
    return (unit_cube_to_world(world, uvw) - X._v(camera.position)) @ X._v(camera.forward)


def raymarch_hits(scene, camera, tile, steps, jitter_frame, world, threshold, scene_depth=None, labels=None, colors=None):
    """Per pixel of the tile: sample (-1: no hit), full_steps, uvw, alpha (no hit: the final opacity), value, depth (no hit: +inf),
    label (-1 without a label volume or a hit), taint, crossing (the ray has samples)."""
    threshold = float(np.float32(threshold))
    cc, cd = X.local_clipping(world)
    entry, thick, lcv, px, py, raw_thick = X.cube_setup(camera, world, tile, scene_depth)
    step_count = float(np.float32(steps))
    step_size = 1.0 / step_count
    actual = step_count * thick
    max_steps = np.floor(actual).astype(np.int64)
    final = actual - np.floor(actual)
    taint = ((final < X.DELTA_FRAC) | (final > 1.0 - X.DELTA_FRAC)) & (step_count * raw_thick > -X.DELTA_FRAC)
    vec = lcv * step_size
    step_world = X.VOLUME_DENSITY * step_size
    pos = entry.copy()
    if jitter_frame >= 0:
        r = X.rand3d_pcg16(px, py, np.full_like(px, jitter_frame & 7))[0].astype(np.float64) / 65535.0
        pos = pos - vec * r[..., None]
    shape = pos.shape[:-1]
    alpha = np.zeros(shape, dtype=np.float64)
    done = np.zeros(shape, dtype=bool)
    sample = np.full(shape, -1, dtype=np.int64)
    uvw = np.zeros(shape + (3,), dtype=np.float64)
    value = np.zeros(shape, dtype=np.float64)
    label = np.full(shape, -1, dtype=np.int64)
    dpos = X.delta_ray_pos(steps)
    data_mode = scene.data_address_mode
    if labels is not None:
        nz, ny, nx = labels.shape
        n_lab = np.array([nx, ny, nz], dtype=np.float64)

    def step(mask, p, stepw, index):
        """the data step, the label step behind it, then the hit test, on rays `mask`"""
        nonlocal taint
        if not mask.any():
            return
        q = p[mask]
        v = X.sample_3d(scene.data, q[:, 0], q[:, 1], q[:, 2], data_mode)
        sw = stepw[mask] if np.ndim(stepw) else stepw
        rgba, t = X.windowed_tf(v, sw, scene.tf, scene.windowing, X.DELTA_TF)
        a = alpha[mask]
        a = a + rgba[:, 3] * (1.0 - a)
        lab = np.full(len(q), -1, dtype=np.int64)
        if labels is not None:
            c, lt = LR.label_lookup(labels, colors, q, dpos)
            al = 1.0 - np.power(1.0 - c[:, 3], sw)
            a = a + al * (1.0 - a)
            t = t | lt
            idx = np.rint(np.clip(q, 0.0, 1.0) * (n_lab - 1.0)).astype(np.int64)
            lab = labels[idx[:, 2], idx[:, 1], idx[:, 0]].astype(np.int64)
        alpha[mask] = a
        taint[mask] = taint[mask] | t | (np.abs(a - threshold) < X.DELTA_EXIT)
        hit = a > threshold
        where = np.flatnonzero(mask.ravel())[hit]
        sample.ravel()[where] = np.broadcast_to(index, mask.shape).ravel()[where]
        uvw.reshape(-1, 3)[where] = q[hit]
        value.ravel()[where] = v[hit]
        label.ravel()[where] = lab[hit]
        done.ravel()[where] = True

    def clipped(p):
        dist = (p - cc) @ cd
        return dist <= 0.0, np.abs(dist) < dpos

    nmax = int(max_steps.max()) if max_steps.size else 0
    for i in range(nmax):
        active = (i < max_steps) & ~done
        if not active.any():
            break
        pos[active] += vec[active]
        cl, near = clipped(pos)
        taint |= active & near
        step(active & ~cl, pos, step_world, i)
    fin = ~done & (final > 0.0)
    pos[fin] += vec[fin] * final[fin][:, None]
    cl, near = clipped(pos)
    taint |= fin & near
    step(fin & ~cl, pos, X.VOLUME_DENSITY * final, max_steps)
    hit = sample >= 0
    depth = np.where(hit, depth_along_forward(world, camera, uvw), np.inf)
    return dict(sample=sample, full_steps=max_steps, uvw=uvw, alpha=alpha, value=value, depth=depth, label=label, taint=taint,
                crossing=(max_steps > 0) | (final > 0.0))


# ---- the scenes the hit tests share (tests/exact_scenes.py RAY_SCENES), each reference computed once ---------------------------------
HIT_SCENES = ("outside-u16-jitter", "f32-u8-light-clamp", "inside-camera", "grazing", "rotated-clip-bone", "depth-odd-tile-rowgroups")
THRESHOLDS = (0.05, 0.5, 0.95)


def scene_named(name):
    return next(s for s in E.RAY_SCENES if s["name"] == name)


def exact_scene(scene):
    """the float64 scene of a RAY_SCENES entry, with the baked transfer function the device holds"""
    baked = abi.host_bake_tf_lut(E.tf_lut(scene["tf"]))
    return X.Scene(E.volume(scene), baked, abi.WindowingParams(*scene["window"]), E.light_dims(scene), not scene["light32"], scene["addr"],
                   scene["border"])


@functools.lru_cache(maxsize=None)
def reference(name, threshold):
    s = scene_named(name)
    return raymarch_hits(exact_scene(s), s["cam"], s["tile"], s["steps"], s["jitter"], s["world"], threshold, s["depth"])


# a label scene: spheres of half-transparent labels (and one opaque, one clear) over the synthetic volume
LABEL_DIMS = (48, 40, 44)


def label_colors():
    c = np.zeros((256, 4), dtype=np.float32)
    c[1:8] = [(1, 0, 0, 0.6), (0, 1, 0, 0.5), (0, 0, 1, 0.7), (1, 1, 0, 0.4), (0, 1, 1, 0.9), (1, 0, 1, 1.0), (0.5, 0.5, 0.5, 0.0)]
    return c


def label_volume(dims=LABEL_DIMS):
    nx, ny, nz = dims
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    lab = np.zeros((nz, ny, nx), dtype=np.uint8)
    spheres = [((0.3, 0.3, 0.7), 0.22, 1), ((0.7, 0.35, 0.6), 0.2, 2), ((0.5, 0.7, 0.5), 0.25, 3), ((0.2, 0.75, 0.3), 0.15, 4),
               ((0.8, 0.8, 0.8), 0.15, 5), ((0.55, 0.2, 0.25), 0.12, 6), ((0.4, 0.5, 0.15), 0.12, 7)]
    for (cx, cy, cz), r, v in spheres:
        lab[(x - cx * nx) ** 2 + (y - cy * ny) ** 2 + (z - cz * nz) ** 2 <= (r * min(dims)) ** 2] = v
    return lab
