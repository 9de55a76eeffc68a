"""Float64 restatement of the lit march with the label overlay (TEST INFRASTRUCTURE ONLY), built on tests/exact_reference.py.

The semantics are include/tbrm_labels.h's (DESIGN.md "Label overlay"): at every sample the march takes — not clipped, inside
the depth limit, full steps and the fractional final step — the data sample's AccumulateWindowedRaymarchStep as
exact_reference.raymarch_lit restates it, THEN the unlit label step
    L = label[rint((N - 1) * saturate(pos))] per axis (HLSL round: half to even), c = colors[L],
    a' = 1 - (1 - c.a) ** step (step: the data sample's, 100 / steps or 100 * FinalStep),
    LE.rgb += c.rgb * a' * (1 - LE.a), LE.a += a' * (1 - LE.a),
THEN the 0.95 early-exit test of the full steps. Nothing here is taken from the kernels.

Decision taint, as exact_reference does for its own discontinuities: a sample whose (N - 1) * saturate(pos) lies within the
position-error margin of a .5 boundary on some axis may read the neighbouring voxel in fp32; the ray is tainted where a voxel
it may read instead has another colour.
"""
import numpy as np

import exact_reference as X


def default_label_colors():
    """GetColorFromLabelValue (RaymarchExperimental.usf): 0 clear, 1 half-transparent red, 2 half-transparent green, the rest
    opaque black"""
    c = np.zeros((256, 4), dtype=np.float32)
    c[3:, 3] = 1.0
    c[1] = (1.0, 0.0, 0.0, 0.5)
    c[2] = (0.0, 1.0, 0.0, 0.5)
    return c


def label_lookup(labels, colors, q, dpos):
    """SampleLabelVolume's voxel of positions q [n, 3] -> (colour [n, 4] float64, taint [n])"""
    nz, ny, nx = labels.shape
    n = np.array([nx, ny, nz], dtype=np.float64)
    u = np.clip(q, 0.0, 1.0) * (n - 1.0)
    idx = np.rint(u).astype(np.int64)                                  # round half to even
    # (an index near a .5 boundary may go to the other side: the neighbour it would be)
    near = np.abs(u - np.floor(u) - 0.5) < (n - 1.0) * dpos + 1e-9
    alt = np.where(u - np.floor(u) < 0.5, idx + 1, idx - 1)
    alt = np.clip(alt, 0, (n - 1).astype(np.int64))
    col = colors.astype(np.float64)
    eff = np.concatenate([col[:, :3] * col[:, 3:], col[:, 3:]], axis=1)   # what a label adds: colours of alpha 0 are all one
    lab = labels[idx[:, 2], idx[:, 1], idx[:, 0]]
    taint = np.zeros(len(q), dtype=bool)
    for k in range(1, 8):
        flip = np.array([(k >> a) & 1 for a in range(3)], dtype=bool)
        ok = np.all(near[:, flip], axis=1)
        if not ok.any():
            continue
        j = np.where(flip, alt, idx)
        other = labels[j[:, 2], j[:, 1], j[:, 0]]
        taint |= ok & np.any(eff[other] != eff[lab], axis=1)
    return col[lab], taint


def raymarch_lit(scene, labels, colors, camera, tile, steps, jitter_frame, world, scene_depth=None):
    """exact_reference.raymarch_lit with the label step after every data step. Returns (rgba [h, w, 4] float64, taint [h, w])."""
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
    le = np.zeros(pos.shape[:-1] + (4,), dtype=np.float64)
    done = np.zeros(pos.shape[:-1], dtype=bool)
    dpos = X.delta_ray_pos(steps)
    lv = scene.light_values()
    data_mode = scene.data_address_mode

    def accumulate(mask, p, stepw):
        nonlocal taint
        q = p[mask]
        v = X.sample_3d(scene.data, q[:, 0], q[:, 1], q[:, 2], data_mode)
        sw = stepw[mask] if np.ndim(stepw) else stepw
        rgba, t = X.windowed_tf(v, sw, scene.tf, scene.windowing, X.DELTA_TF)
        sq = np.clip(q, 0.0, 1.0)
        light = X.sample_3d(lv, sq[:, 0], sq[:, 1], sq[:, 2], X.ADDR_WRAP)
        rgba[:, :3] *= light[:, None]
        cur = le[mask]
        om = 1.0 - cur[:, 3]
        cur[:, :3] += rgba[:, :3] * rgba[:, 3:4] * om[:, None]
        cur[:, 3] += rgba[:, 3] * om
        # the label step (AccumulateOneRaymarchLabelStep): unlit, after the data step; a' = 0 adds nothing
        c, lt = label_lookup(labels, colors, q, dpos)
        a = 1.0 - np.power(1.0 - c[:, 3], sw)
        on = a != 0.0
        om = 1.0 - cur[:, 3]
        cur[on, :3] += c[on, :3] * a[on, None] * om[on, None]
        cur[on, 3] += a[on] * om[on]
        le[mask] = cur
        taint[mask] = taint[mask] | t | lt

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
        m = active & ~cl
        accumulate(m, pos, step_world)
        taint |= m & (np.abs(le[..., 3] - 0.95) < X.DELTA_EXIT)
        ex = m & (le[..., 3] > 0.95)
        le[ex, 3] = 1.0
        done |= ex
    fin = ~done & (final > 0.0)
    pos[fin] += vec[fin] * final[fin][:, None]
    cl, near = clipped(pos)
    taint |= fin & near
    m = fin & ~cl
    accumulate(m, pos, X.VOLUME_DENSITY * final)
    return le, taint
