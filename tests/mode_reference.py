"""Float64 restatement of the Intensity and Octree render modes (TEST INFRASTRUCTURE ONLY), built on tests/exact_reference.py.

Written from the reference's own lines, cited as `File.ext:line` (TBRaymarcherPlugin v0.9.2), reusing exact_reference's cube
setup, clipping parameters, D3D sampling, windowed TF, PCG16 jitter and position margin. Nothing here is taken from the
oracle or the kernels.

  * raymarch_intensity: PerformWindowedIntensityRaymarch (WindowedRaymarchMaterials.usf:187-242);
  * generate_octree:    GenerateOctreeShader.usf:28-107 on the render target of RaymarchVolume.cpp:873-877 (PF_G16, four mips,
                        base level at the data's dimensions rounded up to powers of two), MinMaxValues = (0, 1)
                        (OctreeShaders.h:49), dispatched one thread per 8^3 leaf (OctreeShaders.cpp:47-50);
  * raymarch_octree:    PerformWindowedRaymarchOctree (WindowedRaymarchMaterials.usf:99-183) with
                        SampleWindowedVolumeOctreeStep (WindowedSampling.usf:47-52).

Engine / hardware behaviour leaned on, restated from its definition: UNORM16 decode `c / 65535` and store
`trunc(clamp(x, 0, 1) * 65535 + 0.5)`; typed loads (Texture3D.Load, RWTexture3D reads) outside the level return 0 and typed
stores outside it are dropped; a texture's mip m has `max(1, d >> m)` texels per axis; float -> int conversion truncates
toward zero.

Where the march goes. Full step k of a ray samples entry + LocalCamVec * (k + 1 - r), r in [0, 1] the jitter, k + 1 <=
StepCount * Thickness: always inside the cube. The fractional step samples entry + dir * (Thickness - r / StepCount): with
jitter on and Thickness < r / StepCount — every ray when StepCount < 1, thin corner crossings otherwise — that is OUTSIDE
the cube, before the entry point. Only there can positions leave [0, 1]^3 by more than rounding; the scenes with
StepCount < 1 are the ones that exercise raw-versus-saturated positions, negative texel coordinates and out-of-level loads.

Decision taint, in exact_reference's sense (margins from there: delta_ray_pos, DELTA_FRAC, DELTA_TF, DELTA_EXIT):
  * intensity: the output is the first sample the clip plane leaves. Every clip test up to and including that sample's is a
    decision (plane distance within delta_ray_pos). `StepCount * Thickness` within DELTA_FRAC of an integer n may give n - 1
    or n full steps; the first n - 1 full steps are common to both readings, so the ray is tainted only when it did not hit
    within those (the last full step and the fractional step differ in their clip position; hit / no-hit may change);
  * octree march: a texel coordinate c = pos * W carries the position's error times W (W is a power of two: the product is
    exact in fp32; for z, `(pos * DataDepth / OctreeDepth0) * OctreeDepth` adds two roundings of relative size 2^-24, far
    below the position margin). The sample may read any texel that int(c +- margin) reaches, on each axis independently; the
    ray is tainted where one of those texels (or "outside the level": 0) would contribute something else than the texel read.
    A coordinate near an integer whose neighbours contribute the same taints nothing;
  * pyramid: `x * 65535 + 0.5` in fp32 rounds the product and the sum once each, each by <= half an ulp of a value below
    65536, i.e. <= 2^-9: a base texel of f32 data is tainted when x * 65535 lies within Q16_MARGIN = 2^-8 of a tie, and then
    carries the two codes it may hold. A reduced texel is tainted when the maximum over its children's lower codes differs
    from the maximum over their upper codes. u8 codes map to c * 257 and u16 codes to themselves, 0.5 away from any tie.

Dropped misreading: `intensity_full_step_unsaturated` (clip test and sample of the full steps at the raw CurPos). Full-step
positions never leave the cube (above), where saturate is the identity: no scene can observe it.
"""
import numpy as np

import exact_reference as X

Q16_MARGIN = 2.0 ** -8


def _pow2_at_least(n):
    """FMath::RoundUpToPowerOfTwo"""
    p = 1
    while p < n:
        p *= 2
    return p


# ------------------------------------------------------------------------------------------------------------------
# pyramid

def _halve(level, axis):
    """max over pairs along `axis`; an axis one texel wide has no second texel to read (it reads 0, and Max starts at 0)"""
    n = level.shape[axis]
    if n == 1:
        return level
    shape = list(level.shape)
    shape[axis:axis + 1] = [n // 2, 2]
    return level.reshape(shape).max(axis=axis + 1)


def _pyramid(volume):
    """-> (codes, lower codes, upper codes), four [z, y, x] int64 arrays each"""
    x = X.decode(volume)                                               # Volume.Load(...).r (GenerateOctreeShader.usf:45)
    x = np.nan_to_num(x, nan=0.0) * 1.0                                # * MinMaxValues.y (OctreeShaders.h:49)
    s = np.clip(x, 0.0, 1.0) * 65535.0                                 # exact in float64: 24 x 16 significant bits
    q = np.floor(s + 0.5).astype(np.int64)
    lo, hi = q.copy(), q.copy()
    if volume.dtype == np.float32:
        t = s - np.floor(s) - 0.5                                      # signed distance to the tie
        near = (np.abs(t) <= Q16_MARGIN) & (x > 0.0) & (x < 1.0)
        lo[near] = np.floor(s[near]).astype(np.int64)
        hi[near] = lo[near] + 1
    nz, ny, nx = volume.shape
    if "pyramid_no_pow2_padding" in X.MUTATIONS:
        shape0 = (nz, ny, nx)
    else:
        shape0 = (_pow2_at_least(nz), _pow2_at_least(ny), _pow2_at_least(nx))   # RaymarchVolume.cpp:876-877
    out = []
    for a in (q, lo, hi):
        base = np.zeros(shape0, dtype=np.int64)                        # loads outside the volume return 0
        base[:nz, :ny, :nx] = a
        levels = [base]
        for m in range(1, 4):                                          # GenerateOctreeShader.usf:59-105
            lower = levels[-1]
            want = tuple(max(1, d >> m) for d in shape0)               # a texture's mip m
            # (an odd width, possible only under the padding misreading, leaves its last texel to no parent)
            lower = lower[tuple(slice(0, 2 * w if d > 1 else 1) for d, w in zip(lower.shape, want))]
            for axis in range(3):
                lower = _halve(lower, axis)
            assert lower.shape == want
            levels.append(lower)
        out.append(levels)
    return out


def generate_octree(volume):
    """The four levels of the octree texture as UNORM16 codes [z, y, x]."""
    return [l.astype(np.uint16) for l in _pyramid(volume)[0]]


def octree_taint(volume):
    """Per-level masks of the texels an fp32 evaluation may store one code off; None for u8 / u16 data (exact)."""
    if volume.dtype != np.float32:
        return None
    _, lo, hi = _pyramid(volume)
    return [a != b for a, b in zip(lo, hi)]


# ------------------------------------------------------------------------------------------------------------------
# shared march set-up

def _march_setup(camera, tile, steps, jitter_frame, world, scene_depth):
    cc, cd = X.local_clipping(world)
    entry, thick, lcv, px, py, raw_thick = X.cube_setup(camera, world, tile, scene_depth)
    step_count = float(np.float32(steps))
    step_size = 1.0 / step_count                                       # :112 / :195
    actual = step_count * thick                                        # :114 / :197
    max_steps = np.floor(actual).astype(np.int64)                      # :116 / :199
    final = actual - np.floor(actual)                                  # :118 / :201
    near_int = ((final < X.DELTA_FRAC) | (final > 1.0 - X.DELTA_FRAC)) & (step_count * raw_thick > -X.DELTA_FRAC)
    vec = lcv * step_size                                              # :121 / :204
    pos = entry.copy()
    if jitter_frame >= 0:                                              # JitterEntryPos (RaymarchMaterialCommon.usf:73-78)
        r = X.rand3d_pcg16(px, py, np.full_like(px, jitter_frame & 7))[0].astype(np.float64) / 65535.0
        pos = pos - vec * r[..., None]
    return cc, cd, step_count, step_size, actual, max_steps, final, near_int, vec, pos


# ------------------------------------------------------------------------------------------------------------------
# intensity

def raymarch_intensity(scene, camera, tile, steps, jitter_frame, world, scene_depth=None):
    """PerformWindowedIntensityRaymarch (WindowedRaymarchMaterials.usf:187-242). Returns (rgba [h, w, 4], taint [h, w])."""
    cc, cd, step_count, step_size, actual, max_steps, final, near_int, vec, pos = _march_setup(
        camera, tile, steps, jitter_frame, world, scene_depth)
    dpos = X.delta_ray_pos(steps)
    out = np.zeros(pos.shape[:-1] + (4,), dtype=np.float64)            # :241 didn't hit anything
    hit = np.zeros(pos.shape[:-1], dtype=bool)
    hit_step = np.full(pos.shape[:-1], np.iinfo(np.int64).max)
    taint = np.zeros(pos.shape[:-1], dtype=bool)
    w = scene.windowing
    mode = scene.data_address_mode if "intensity_material_address_mode" in X.MUTATIONS else X.ADDR_CLAMP

    def shade(mask, p):
        q = p[mask]
        v = X.sample_3d(scene.data, q[:, 0], q[:, 1], q[:, 2], mode)  # Material.Clamp_WorldGroupSettings (:215, :231)
        tpos = (v - float(w.center) + float(w.width) / 2.0) / float(w.width)   # WindowedSampling.usf:14-17
        t = np.clip(tpos, 0.0, 1.0)                                    # :218
        rgba = np.stack([t, t, t, np.ones_like(t)], axis=-1)           # :220
        if "intensity_cutoffs" in X.MUTATIONS:                         # (the TF path's cut-offs, WindowedSampling.usf:28-31)
            cut = ((tpos < 0.0) & bool(w.low_cutoff)) | ((tpos > 1.0) & bool(w.high_cutoff))
            rgba[cut] = 0.0
        out[mask] = rgba

    def clip_test(p):
        dist = (p - cc) @ cd                                           # IsCurPosClipped (RaymarcherCommon.usf:22-25)
        return dist <= 0.0, np.abs(dist) < dpos

    nmax = int(max_steps.max()) if max_steps.size else 0
    for i in range(nmax):
        active = (i < max_steps) & ~hit
        if not active.any():
            break
        pos[active] += vec[active]                                     # :211
        sp = np.clip(pos, 0.0, 1.0)                                    # saturate(CurPos), test and sample (:213, :215)
        cl, near = clip_test(sp)
        taint |= active & near
        m = active & ~cl
        shade(m, sp)
        hit |= m
        hit_step[m] = i
    fin = ~hit & (final > 0.0)                                         # :225
    pos[fin] += vec[fin] * final[fin][:, None]                         # :227
    fp = np.clip(pos, 0.0, 1.0) if "intensity_final_step_saturated" in X.MUTATIONS else pos   # the raw CurPos (:229, :231)
    cl, near = clip_test(fp)
    taint |= fin & near
    shade(fin & ~cl, fp)
    # floor / frac of StepCount * Thickness: the first round(actual) - 1 full steps exist under either reading
    common = np.rint(actual).astype(np.int64) - 1
    taint |= near_int & (hit_step >= common)
    return out, taint


# ------------------------------------------------------------------------------------------------------------------
# octree march

def _to_int(c):
    """float3 -> int3 (WindowedRaymarchMaterials.usf:151; :174 builds a float3 that the int3 parameter of
    SampleWindowedVolumeOctreeStep converts the same way): truncation toward zero"""
    if "octree_round_nearest" in X.MUTATIONS:
        return np.rint(c).astype(np.int64)
    if "octree_floor_negative" in X.MUTATIONS:
        return np.floor(c).astype(np.int64)
    return np.trunc(c).astype(np.int64)


def _load(level, idx):
    """Texture3D.Load(int4(x, y, z, mip)) (WindowedSampling.usf:49-50) -> UNORM16 value; outside the level: 0"""
    nz, ny, nx = level.shape
    n = np.array([nx, ny, nz], dtype=np.int64)
    inside = np.all((idx >= 0) & (idx < n), axis=1)
    j = np.clip(idx, 0, n - 1)
    v = level[j[:, 2], j[:, 1], j[:, 0]].astype(np.float64) / 65535.0
    if "octree_load_clamps" in X.MUTATIONS:
        return v
    return np.where(inside, v, 0.0)


def raymarch_octree(scene, mips, mip, camera, tile, steps, jitter_frame, world, scene_depth=None, texel_taint=None):
    """PerformWindowedRaymarchOctree (WindowedRaymarchMaterials.usf:99-183) over level `mip` of `mips` (generate_octree's
    four levels). texel_taint: octree_taint's masks — a ray that reads a tainted texel is tainted.
    Returns (rgba [h, w, 4] float64, taint [h, w])."""
    cc, cd, step_count, step_size, actual, max_steps, final, near_int, vec, pos = _march_setup(
        camera, tile, steps, jitter_frame, world, scene_depth)
    taint = near_int.copy()
    step_world = X.VOLUME_DENSITY * step_size                          # :123
    level = mips[mip]
    od, oh, ow = (float(s) for s in level.shape)                       # GetDimensions(OctreeMip, ...) (:139)
    od0 = float(mips[0].shape[0])                                      # OctreeDepthConst (:134-136)
    nz, ny, nx = scene.data.shape                                      # DataVolume.GetDimensions (:131)
    if "octree_xy_data_dims" in X.MUTATIONS:
        ow, oh = nx / 2.0 ** mip, ny / 2.0 ** mip
    zscale = od if "octree_z_no_depth_ratio" in X.MUTATIONS else float(nz) / od0 * od
    scale = np.array([ow, oh, zscale], dtype=np.float64)
    dpos = X.delta_ray_pos(steps)
    margin = scale * dpos
    le = np.zeros(pos.shape[:-1] + (4,), dtype=np.float64)
    done = np.zeros(pos.shape[:-1], dtype=bool)
    ltaint = None if texel_taint is None else texel_taint[mip]

    def contribution(v, sw):
        rgba, t = X.windowed_tf(v, sw, scene.tf, scene.windowing, X.DELTA_TF)
        return rgba, t

    def accumulate(mask, p, sw):
        nonlocal taint
        q = p[mask]
        if not len(q):
            return
        c = q * scale                                                  # :151 / :174
        idx = _to_int(c)
        v = _load(level, idx)
        rgba, t = contribution(v, sw)                                  # SampleWindowedVolumeOctreeStep (WindowedSampling.usf:47-52)
        # the texels an fp32 evaluation of the coordinate may read instead
        lo, hi = _to_int(c - margin), _to_int(c + margin)
        near = lo != hi
        st = t.copy()
        if near.any():
            alt = np.where(lo != idx, lo, hi)
            eff = np.concatenate([rgba[:, :3] * rgba[:, 3:], rgba[:, 3:]], axis=1)
            for k in range(1, 8):
                flip = np.array([(k >> a) & 1 for a in range(3)], dtype=bool)
                ok = np.all(near[:, flip], axis=1)
                if not ok.any():
                    continue
                j = np.where(flip, alt[ok], idx[ok])
                o, _ = contribution(_load(level, j), sw[ok] if np.ndim(sw) else sw)
                oeff = np.concatenate([o[:, :3] * o[:, 3:], o[:, 3:]], axis=1)
                st[ok] |= np.any(oeff != eff[ok], axis=1)
        if ltaint is not None:
            n = np.array([ow, oh, od], dtype=np.int64)
            inside = np.all((idx >= 0) & (idx < n), axis=1)
            j = np.clip(idx, 0, n - 1)
            st |= inside & ltaint[j[:, 2], j[:, 1], j[:, 0]]
        cur = le[mask]
        om = 1.0 - cur[:, 3]                                           # AccumulateLightEnergy (RaymarchMaterialCommon.usf:82-88)
        cur[:, :3] += rgba[:, :3] * rgba[:, 3:4] * om[:, None]
        cur[:, 3] += rgba[:, 3] * om
        le[mask] = cur
        taint[mask] = taint[mask] | st

    def clipped(p):
        dist = (p - cc) @ cd                                           # IsCurPosClipped (RaymarcherCommon.usf:22-25)
        return dist <= 0.0, np.abs(dist) < dpos

    nmax = int(max_steps.max()) if max_steps.size else 0
    for i in range(nmax):
        active = (i < max_steps) & ~done
        if not active.any():
            break
        pos[active] += vec[active]                                     # :144
        cl, near = clipped(pos)
        taint |= active & near
        m = active & ~cl                                               # :147
        accumulate(m, pos, step_world)
        taint |= m & (np.abs(le[..., 3] - 0.95) < X.DELTA_EXIT)
        ex = m & (le[..., 3] > 0.95)                                   # :159-163, inside the full steps only
        le[ex, 3] = 1.0
        done |= ex
    fin = ~done & (final > 0.0)                                        # :168
    pos[fin] += vec[fin] * final[fin][:, None]                         # :170
    cl, near = clipped(pos)
    taint |= fin & near
    m = fin & ~cl
    if "octree_final_step_scaled" in X.MUTATIONS:
        sw = X.VOLUME_DENSITY * final[m]
    else:
        sw = step_world                                                # the fractional step keeps StepSizeWorld (:175)
    accumulate(m, pos, sw)
    if "octree_exit_on_final_step" in X.MUTATIONS:
        le[m & (le[..., 3] > 0.95), 3] = 1.0
    return le, taint
