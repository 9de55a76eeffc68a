"""Float64 NumPy restatement of the hot path, written from the reference plugin's own lines (TEST INFRASTRUCTURE ONLY).

This is the second, independent restatement of the operation the kernels compute. `oracle/tbrm_oracle.c` fixes ONE fp32
arithmetic definition that the kernels evaluate bit for bit; this module evaluates the operation itself, in float64,
with exact (unquantised) filter weights and `np.power` for the opacity correction. `Dir/File.ext:line` cites the reference
(TBRaymarcherPlugin v0.9.2) line each function restates. Nothing here is taken from the oracle or the kernels.

Engine / hardware behaviour the reference leans on, restated once each from its definition:
  * UNORM decode `c / (2^n - 1)` and the UNORM8 store `trunc(clamp(x, 0, 1) * 255 + 0.5)` (D3D11 format conversion rules);
  * the read buffer's border colour `FLinearColor(I * w).ToFColor(true)`: IEC 61966-2-1 sRGB encode, 8-bit round to nearest,
    decoded back to linear when the sampler is created; the data volume's `ToFColor(false)`: linear 8-bit round to nearest;
  * face-sort ties: `std::sort` is not stable, so a tie among the first two faces (or a tie at the 0.99 snap) is a coin toss.
    `light_passes` reports the margins (`sort_margin`, `snap_margin`, `border_margin`) and scenes must keep them open;
  * D3D sampling: texel split `x = u * N - 0.5`, the two taps `floor(x)`, `floor(x) + 1` addressed per tap (wrap / clamp /
    border), weights `frac(x)` — here exact;
  * Rand3DPCG16 (engine Random.ush): the published PCG3D recurrence, top 16 bits.

Decision taint. The operation is not continuous everywhere: an fp32 evaluation may legitimately take the other branch of a
comparison whose operand lies close to its threshold. Every function returns, next to its values, a boolean mask of the
outputs that depend on such a decision taken within a margin of its threshold. The margins (DELTA_*) come from the error
budget of an fp32 evaluation of the same quantities:
  * positions in UVW are sums of a handful of fp32 terms of magnitude <= 2: error <= ~8 ulp(2) = 2e-6 in propagation. The
    raymarch adds LocalCamVec once per step, so after S steps the error is <= S * ulp(1) ~ 6e-8 * S (3e-5 at 512 steps):
    DELTA_POS = 1e-5 for propagation, DELTA_RAY_POS = 2e-5 + 1.2e-7 * steps for the raymarch;
  * TF positions are (data - C + W/2) / W: a data value carries <= 1e-6 of filter error (plus the position error times the
    data gradient, <= 1e-3 per texel for the synthetic data times <= 2e-5 texel); divided by W >= 0.1: DELTA_TF = 1e-4
    (propagation 2e-5);
  * light alphas are products of <= 512 factors `1 - a` and convex bilinear mixes: relative error <= 512 * 4 * 2^-24 = 1.2e-4,
    absolute <= 1.2e-7 next to the 1e-3 write threshold: DELTA_WRITE = 2e-6, plus DELTA_WRITE_REL = 4 * 2^-24 per slice
    behind the operands times their magnitude (Change compares the difference of two O(1) alphas);
  * the accumulated opacity is a sum of <= 512 fp32 terms in [0, 1]: error <= 3e-5; DELTA_EXIT = 1e-4 around 0.95;
  * `StepCount * Thickness` is a product of an fp32 count with a thickness of error <= 4e-7 (cube setup): DELTA_FRAC = 2e-3
    around every integer (counts up to ~1000);
  * the UNORM8 light-volume read-modify-write store: x within DELTA_Q8 = 2e-6 (16 ulp of 1) of a rounding tie. The ping-pong
    buffers' own stores are NOT tainted: a one-code flip there spreads through every later slice's bilinear reads and would
    taint the whole volume; the UNORM8 comparison therefore allows one code everywhere and asserts an exact fraction instead.
Taint carries forward in propagation: a buffer texel that reads a tainted texel with nonzero bilinear weight is tainted.

`MUTATIONS` holds private switches, each one plausible misreading of the reference. They exist only so the tests can show
that the comparison against the oracle would catch such a misreading; the default set is empty.
"""
import numpy as np

VOLUME_DENSITY = 100.0                      # RaymarcherCommon.usf:18
ONE_OVER_SQRT_3 = 0.57735026919             # RaymarcherCommon.usf:13
FACE_NORMALS = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float64)  # LightingShaderUtils.h

ADDR_WRAP, ADDR_CLAMP, ADDR_BORDER = 0, 1, 2
BORDER_ENGINE_8BIT, BORDER_EXACT_FLOAT = 0, 1   # include/tbrm.h TBRM_BORDER_*

DELTA_POS = 1e-5
DELTA_TF_PROP = 2e-5
DELTA_TF = 1e-4
DELTA_WRITE = 2e-6
DELTA_WRITE_REL = 4.0 * 2.0 ** -24   # per slice behind the operand
DELTA_EXIT = 1e-4
DELTA_FRAC = 2e-3
DELTA_Q8 = 2e-6
DELTA_ALPHA_WEIGHT = 1e-5


def delta_ray_pos(steps):
    return 2e-5 + 1.2e-7 * float(steps)


MUTATIONS = set()
KNOWN_MUTATIONS = (
    "ppo_sign",            # PrevPixelOffset with the opposite sign
    "perm_x_transposed",   # axis-X permutation applied as M * v instead of v * M
    "uvw_not_normalised",  # UVWOffset left at GetStepSizeAndUVWOffset's length (no 1/min(TD) renormalisation)
    "no_099_clamp",        # the primary face weight not snapped to 1 above 0.99
    "no_write_threshold",  # every light change written, however small
    "add_no_guard",        # Add samples outside [0, 1] too
    "border_no_srgb",      # read-buffer border colour kept as the float I * w
    "final_step_stepsize", # final step's opacity exponent StepSize * FinalStep * VOLUME_DENSITY
    "light_clamp_addr",    # light volume read with clamp addressing
    "ppo_div_tdx",         # PrevPixelOffset divided by TD.x instead of TD.z
    "change_guard",        # Change given Add's uvw == saturate(uvw) guard
    # Intensity and Octree render modes (tests/mode_reference.py)
    "intensity_final_step_saturated",   # the fractional step clip-tested at saturate(CurPos) like the full steps
    "intensity_material_address_mode",  # data read with the lit material's address mode instead of clamp
    "intensity_cutoffs",                # the TF path's low / high cut-offs applied to the intensity
    "octree_round_nearest",             # int3 conversion rounding to nearest
    "octree_floor_negative",            # int3 conversion as floor: slightly negative coordinates leave the level
    "octree_z_no_depth_ratio",          # z scaled by the level's depth alone
    "octree_xy_data_dims",              # x, y scaled by the data's width instead of the pyramid's power of two
    "octree_load_clamps",               # Load outside the level clamped to the edge texel instead of reading 0
    "octree_final_step_scaled",         # the fractional step's opacity exponent scaled by FinalStep, as the lit march does
    "octree_exit_on_final_step",        # the 0.95 exit applied after the fractional step too
    "pyramid_no_pow2_padding",          # base level at the data's dimensions
)


# ------------------------------------------------------------------------------------------------------------------
# FTransform / FVector (engine math, double precision in UE5)

def _v(a):
    return np.array([a.x, a.y, a.z], dtype=np.float64)


def _normalize(v):
    """FVector::Normalize(SMALL_NUMBER): unchanged when |v|^2 <= 1e-8."""
    ss = float(np.dot(v, v))
    return v / np.sqrt(ss) if ss > 1e-8 else v


def _quat_rotate(q, v):
    """FQuat::RotateVector."""
    qv = np.array([q.x, q.y, q.z], dtype=np.float64)
    t = 2.0 * np.cross(qv, v)
    return v + q.w * t + np.cross(qv, t)


def _quat_unrotate(q, v):
    qv = np.array([-q.x, -q.y, -q.z], dtype=np.float64)
    t = 2.0 * np.cross(qv, v)
    return v + q.w * t + np.cross(qv, t)


def _scale_recip(t):
    s = _v(t.scale3d)
    return np.where(np.abs(s) <= 1e-8, 0.0, 1.0 / np.where(s == 0, 1.0, s))


def inverse_transform_vector(t, v):
    """FTransform::InverseTransformVector: unrotate, then divide by the scale."""
    return _quat_unrotate(t.rotation, np.asarray(v, dtype=np.float64)) * _scale_recip(t)


def inverse_transform_position(t, p):
    return _quat_unrotate(t.rotation, np.asarray(p, dtype=np.float64) - _v(t.translation)) * _scale_recip(t)


def local_clipping(world):
    """GetLocalClippingParameters (LightingShaderUtils.cpp:205-220)."""
    t = world.volume_transform
    center = inverse_transform_position(t, _v(world.clipping_plane.center)) + 0.5
    d = _quat_unrotate(t.rotation, _v(world.clipping_plane.direction)) * _v(t.scale3d)
    return center, _normalize(d)


# ------------------------------------------------------------------------------------------------------------------
# engine colour conversions

def _srgb_encode(x):
    return np.where(x <= 0.0031308, 12.92 * x, 1.055 * np.power(np.maximum(x, 0.0), 1.0 / 2.4) - 0.055)


def _srgb_decode(s):
    return np.where(s <= 0.04045, s / 12.92, np.power((s + 0.055) / 1.055, 2.4))


def border_light(linear, border_mode):
    """GetBorderColorIntSingle (LightingShaderUtils.cpp:197-203): FLinearColor(I*w).ToFColor(true) as the sampler border.
    Returns (value, margin): margin = distance in codes of the encoded value from a rounding tie."""
    if border_mode == BORDER_EXACT_FLOAT or "border_no_srgb" in MUTATIONS:
        return float(linear), 0.5
    x = min(max(float(linear), 0.0), 1.0)
    e = float(_srgb_encode(x)) * 255.0
    q = np.floor(e + 0.5)
    return float(_srgb_decode(q / 255.0)), abs((e - np.floor(e)) - 0.5)


def data_border(center, width, border_mode):
    """LightingShaders.h:82-89: ZeroTFValue = Center - 0.5 * Width as the data sampler's border, via ToFColor(false)."""
    z = float(center) - 0.5 * float(width)
    if border_mode == BORDER_EXACT_FLOAT:
        return z
    return float(np.floor(min(max(z, 0.0), 1.0) * 255.0 + 0.5) / 255.0)


def unorm8_store(x):
    """UNORM8 conversion: NaN -> 0, clamp, trunc(x * 255 + 0.5). Returns (codes, taint of a store near a rounding tie)."""
    x = np.nan_to_num(np.asarray(x, dtype=np.float64), nan=0.0)
    s = np.clip(x, 0.0, 1.0) * 255.0 + 0.5
    q = np.floor(s)
    near = (np.abs(s - np.round(s)) < DELTA_Q8 * 255.0) & (x > 0.0) & (x < 1.0)
    return q.astype(np.uint8), near


def decode(vol):
    """UNORM c / (2^n - 1); float data as stored."""
    if vol.dtype == np.uint8:
        return vol.astype(np.float64) / 255.0
    if vol.dtype == np.uint16:
        return vol.astype(np.float64) / 65535.0
    return vol.astype(np.float64)


# ------------------------------------------------------------------------------------------------------------------
# D3D sampling with exact weights

def _axis_taps(x, n, mode):
    """texel split of one axis: (index0, index1, valid0, valid1, frac)"""
    f0 = np.floor(x)
    fr = x - f0
    i0 = f0.astype(np.int64)
    i1 = i0 + 1
    if mode == ADDR_WRAP:
        return np.mod(i0, n), np.mod(i1, n), None, None, fr
    if mode == ADDR_CLAMP:
        return np.clip(i0, 0, n - 1), np.clip(i1, 0, n - 1), None, None, fr
    v0 = (i0 >= 0) & (i0 < n)
    v1 = (i1 >= 0) & (i1 < n)
    return np.clip(i0, 0, n - 1), np.clip(i1, 0, n - 1), v0, v1, fr


def sample_3d(vol, u, v, w, mode, border=0.0):
    """Texture3D.SampleLevel(linear, mode) of a decoded [z, y, x] float64 volume at UVW arrays u, v, w."""
    nz, ny, nx = vol.shape
    xs = _axis_taps(u * nx - 0.5, nx, mode)
    ys = _axis_taps(v * ny - 0.5, ny, mode)
    zs = _axis_taps(w * nz - 0.5, nz, mode)
    out = np.zeros(np.shape(u), dtype=np.float64)
    for dz in (0, 1):
        iz, wz = zs[dz], (zs[4] if dz else 1.0 - zs[4])
        for dy in (0, 1):
            iy, wy = ys[dy], (ys[4] if dy else 1.0 - ys[4])
            for dx in (0, 1):
                ix, wx = xs[dx], (xs[4] if dx else 1.0 - xs[4])
                t = vol[iz, iy, ix]
                if mode == ADDR_BORDER:
                    ok = xs[2 + dx] & ys[2 + dy] & zs[2 + dz]
                    t = np.where(ok, t, border)
                out += (wx * wy * wz) * t
    return out


def sample_2d_border(buf, u, v, border):
    """Texture2D.SampleLevel(bilinear, border) of an [h, w] float64 buffer. Returns (value, tap indices and weights)."""
    h, w = buf.shape
    xs = _axis_taps(u * w - 0.5, w, ADDR_BORDER)
    ys = _axis_taps(v * h - 0.5, h, ADDR_BORDER)
    out = np.zeros(np.shape(u), dtype=np.float64)
    taps = []
    for dy in (0, 1):
        iy, wy = ys[dy], (ys[4] if dy else 1.0 - ys[4])
        for dx in (0, 1):
            ix, wx = xs[dx], (xs[4] if dx else 1.0 - xs[4])
            ok = xs[2 + dx] & ys[2 + dy]
            out += (wx * wy) * np.where(ok, buf[iy, ix], border)
            taps.append((iy, ix, ok & ((wx * wy) > 0)))
    return out, taps


def sample_tf(tf, pos):
    """TF.SampleLevel(bilinear clamp, float2(TFPos, 0.5)) of the 256-texel RGBA table (WindowedSampling.usf:33)."""
    x = pos * 256.0 - 0.5
    f0 = np.floor(x)
    fr = (x - f0)[..., None]
    i0 = np.clip(f0.astype(np.int64), 0, 255)
    i1 = np.clip(f0.astype(np.int64) + 1, 0, 255)
    return tf[i0] * (1.0 - fr) + tf[i1] * fr


def windowed_tf(value, step_size, tf, windowing, delta_tf):
    """SampleWindowedTransferFunction (WindowedSampling.usf:14-37). Returns (rgba, taint)."""
    c, wd = float(windowing.center), float(windowing.width)
    pos = (value - c + wd / 2.0) / wd
    cut = np.zeros(np.shape(value), dtype=bool)
    taint = np.zeros(np.shape(value), dtype=bool)
    # a cut-off decides the output only where the TF's colour at the threshold is not already zero
    if windowing.low_cutoff:
        cut |= pos < 0.0
        if tf[0].any():
            taint |= np.abs(pos) < delta_tf
    if windowing.high_cutoff:
        cut |= pos > 1.0
        if tf[255].any():
            taint |= np.abs(pos - 1.0) < delta_tf
    rgba = sample_tf(tf, pos)
    a = np.clip(rgba[..., 3], 0.0, 1.0)
    rgba[..., 3] = 1.0 - np.power(1.0 - a, step_size)
    rgba[cut] = 0.0
    return rgba, taint


# ------------------------------------------------------------------------------------------------------------------
# pass parameters: GetLocalLightParamsAndAxes + AddDirLightToSingleLightVolume_RenderThread's per-axis block

def _transposed_dims(axis, d):
    """GetTransposedDimensions (LightingShaderUtils.cpp:48-64)."""
    return [(d[1], d[2], d[0]), (d[0], d[2], d[1]), (d[0], d[1], d[2])][axis]


def light_passes(direction, intensity, world, lv_dims, border_mode=BORDER_ENGINE_8BIT):
    """Returns (passes, n_passes, margins). direction: world light direction (3,), lv_dims (x, y, z).
    n_passes follows the loop break on FaceWeight == 0 (LightingShaders.cpp:62-68, 91-97)."""
    d = np.asarray(direction, dtype=np.float64)
    if not d.any():
        return [], 0, {}
    local = _normalize(inverse_transform_vector(world.volume_transform, d))   # LightingShaderUtils.cpp:167-169
    light_pos = -local                                                          # :177
    w = FACE_NORMALS @ light_pos                                                # GetMajorAxes :34-41
    w = np.where(w > 0, w * w, 0.0)
    order = sorted(range(6), key=lambda i: -w[i])                               # :44 (descending; ties asserted away)
    ws = [w[i] for i in order]
    margins = {"sort_margin": min(ws[0] - ws[1], ws[1] - ws[2]) if ws[1] > 0 else ws[0] - ws[1],
               "snap_margin": abs(ws[0] - 0.99)}
    weight = list(ws)
    if weight[0] > 0.99 and "no_099_clamp" not in MUTATIONS:                   # :181-184
        weight[0] = 1.0
    weight[1] = 1.0 - weight[0]                                                 # :187
    passes = []
    border_margin = 0.5
    for i in range(2):
        face = order[i]
        axis = face // 2
        td = _transposed_dims(axis, lv_dims)
        alpha = float(intensity) * weight[i]                                    # GetLightAlpha :222-225
        bl, bm = border_light(alpha, border_mode)
        if weight[i] > 0:
            border_margin = min(border_margin, bm)
        # GetUVOffset (:82-129)
        major = light_pos[axis] if face % 2 == 0 else -light_pos[axis]
        nlp = light_pos / major
        lateral = [a for a in range(3) if a != axis]
        ppo = np.array([nlp[lateral[0]], nlp[lateral[1]]]) / (td[0] if "ppo_div_tdx" in MUTATIONS else td[2])
        if "ppo_sign" in MUTATIONS:
            ppo = -ppo
        # GetStepSizeAndUVWOffset (:132-158)
        uvw = light_pos / (abs(light_pos[axis]) * td[2])
        step = float(np.linalg.norm(uvw))
        if "uvw_not_normalised" not in MUTATIONS:                               # LightingShaders.cpp:121-124
            uvw = _normalize(uvw) * (1.0 / min(td))
        direction_ = 1 if face % 2 else -1                                      # GetAxisDirection :66-70
        start, stop = (td[2] - 1, -1) if direction_ == -1 else (0, td[2])       # GetLoopStartStopIndexes :251-265
        passes.append(dict(face=face, axis=axis, weight=weight[i], light_alpha=alpha, border_light=bl,
                           prev_pixel_offset=ppo, uvw_offset=uvw, step_size=step, td=td, start=start, stop=stop,
                           dir=direction_))
    margins["border_margin"] = border_margin
    n = 0 if passes[0]["weight"] == 0 else (1 if passes[1]["weight"] == 0 else 2)
    return passes, n, margins


# ------------------------------------------------------------------------------------------------------------------
# propagation

class Scene:
    """What FBasicRaymarchRenderingResources holds for the propagation and the raymarch, in float64.
    volume: raw data [z, y, x] (uint8 / uint16 / float32); tf: the 256 x 4 table the texture holds (after the
    FFloat16 bake); light: float64 [z, y, x] (R32F) or uint8 codes (G8)."""

    def __init__(self, volume, tf, windowing, light_dims, light_unorm8, data_address_mode=ADDR_WRAP,
                 border_mode=BORDER_ENGINE_8BIT):
        self.data = decode(volume)
        self.tf = np.asarray(tf, dtype=np.float64).reshape(256, 4)
        self.windowing = windowing
        self.light_dims = tuple(int(x) for x in light_dims)     # (x, y, z)
        self.unorm8 = bool(light_unorm8)
        shape = self.light_dims[::-1]
        self.light = np.zeros(shape, dtype=np.uint8 if self.unorm8 else np.float64)
        self.taint = np.zeros(shape, dtype=bool)
        self.data_address_mode = data_address_mode
        self.border_mode = border_mode

    def light_values(self):
        return self.light.astype(np.float64) / 255.0 if self.unorm8 else self.light

    def set_light(self, lv):
        self.light = np.array(lv, dtype=np.uint8 if self.unorm8 else np.float64)
        self.taint[:] = False

    def clear_light_volume(self, value):
        """ClearVolumeTextureShader.usf:14-20"""
        if self.unorm8:
            q, _ = unorm8_store(np.full(self.light.shape, value))
            self.light = q
        else:
            self.light[:] = value
        self.taint[:] = False

    # -- buffers: stored in the light volume's format (R32F or UNORM8)
    def _store_buf(self, x):
        if self.unorm8:
            return unorm8_store(x)[0].astype(np.float64) / 255.0
        return np.asarray(x, dtype=np.float64)

    def _permute(self, axis, px, py, loop):
        """mul(int3(PixelLoc, Loop), PermutationMatrix) with GetPermutationMatrix (LightingShaderUtils.cpp:227-249):
        SetAxes puts the axes into the ROWS, so for X the row vector (px, py, Loop) maps to (Loop, px, py)."""
        L = np.full_like(px, loop)
        if axis == 0:
            if "perm_x_transposed" in MUTATIONS:
                return py, L, px
            return L, px, py
        if axis == 1:
            return px, L, py
        return px, py, L

    def _voxel_sample(self, p, x, y, z, cc, cd, dborder, guard):
        """CurrentSample of AddDirLightShader.usf:85-114 / ChangeDirLightShader.usf:87-140. Returns (sample, taint)."""
        res = np.array(self.light_dims, dtype=np.float64)
        uvw = [(c + 0.5) / res[k] + p["uvw_offset"][k] for k, c in enumerate((x, y, z))]   # GetUVW + UVWOffset
        dist = sum((uvw[k] - cc[k]) * cd[k] for k in range(3))                  # :87
        off = [(uvw[k] - (uvw[k] + cd[k] * dist)) * res[k] for k in range(3)]   # :90-93
        vd = np.sqrt(off[0] ** 2 + off[1] ** 2 + off[2] ** 2)                   # :95
        raw = 0.5 + ONE_OVER_SQRT_3 * vd * np.sign(dist)                        # :105
        aw = np.clip(raw, 0.0, 1.0)
        taint = np.abs(raw) < DELTA_ALPHA_WEIGHT
        ok = aw > 0.0
        if guard:                                                                # :110 all(SampleUVW == saturate(SampleUVW))
            for k in range(3):
                ok = ok & (uvw[k] >= 0.0) & (uvw[k] <= 1.0)
                taint |= (np.abs(uvw[k]) < DELTA_POS) | (np.abs(uvw[k] - 1.0) < DELTA_POS)
        v = sample_3d(self.data, uvw[0], uvw[1], uvw[2], ADDR_BORDER, dborder)
        rgba, t2 = windowed_tf(v, p["step_size"] * VOLUME_DENSITY, self.tf, self.windowing, DELTA_TF_PROP)
        cur = np.where(ok, rgba[..., 3] * aw, 0.0)
        taint |= ok & t2
        return cur, taint

    def _rmw(self, pos, delta, write, write_taint, dep_taint):
        """ALightVolume[pos] = ALightVolume[pos] + delta where `write` (AddDirLightShader.usf:123-127)."""
        x, y, z = pos
        valid = write & (x >= 0) & (x < self.light_dims[0]) & (y >= 0) & (y < self.light_dims[1]) & (z >= 0) & (z < self.light_dims[2])
        xi, yi, zi = x[valid], y[valid], z[valid]
        self.taint[zi, yi, xi] |= dep_taint[valid]
        tv = write_taint & (x >= 0) & (x < self.light_dims[0]) & (y >= 0) & (y < self.light_dims[1]) & (z >= 0) & (z < self.light_dims[2])
        self.taint[z[tv], y[tv], x[tv]] = True
        if self.unorm8:
            new = self.light[zi, yi, xi].astype(np.float64) / 255.0 + delta[valid]
            q, near = unorm8_store(new)
            self.light[zi, yi, xi] = q
            self.taint[zi, yi, xi] |= near
        else:
            self.light[zi, yi, xi] = self.light[zi, yi, xi] + delta[valid]

    def _streams_pass(self, streams, world, change):
        """One axis pass with one (Add / Remove) or two (Change: removed, added) streams sharing the face's geometry."""
        cc, cd = local_clipping(world)
        dborder = data_border(self.windowing.center, self.windowing.width, self.border_mode)
        p0 = streams[0][0]
        td = p0["td"]
        py, px = np.meshgrid(np.arange(td[1]), np.arange(td[0]), indexing="ij")
        state = []
        for p, _sign in streams:   # ping-pong buffers cleared to LightIntensity * weight (LightingShaders.cpp:62-80, 202-223)
            state.append([self._store_buf(np.full((td[1], td[0]), p["light_alpha"])), np.zeros((td[1], td[0]), dtype=bool)])
        guard = (not change) and "add_no_guard" not in MUTATIONS or (change and "change_guard" in MUTATIONS)
        for j in range(p0["start"], p0["stop"], p0["dir"]):
            x, y, z = self._permute(p0["axis"], px, py, j)
            lights, taints = [], []
            for k, (p, _sign) in enumerate(streams):
                buf, btaint = state[k]
                pu = (px + 0.5) / td[0] + p["prev_pixel_offset"][0]          # :81
                pv = (py + 0.5) / td[1] + p["prev_pixel_offset"][1]
                prev, taps = sample_2d_border(buf, pu, pv, p["border_light"])
                t = np.zeros(px.shape, dtype=bool)
                for iy, ix, live in taps:
                    t |= live & btaint[iy, ix]
                cur, st = self._voxel_sample(p, x, y, z, cc, cd, dborder, guard)
                l = prev * (1.0 - cur)                                          # :117
                t |= st
                lights.append(l)
                taints.append(t)
                state[k] = [self._store_buf(l), t]                              # :120 WriteBuffer[PixelLoc]
            if change:                                                          # ChangeDirLightShader.usf:152-155
                delta = lights[1] - lights[0]
            else:
                delta = lights[0] * streams[0][1]                               # AddDirLightShader.usf:126
            dep = taints[0] if not change else (taints[0] | taints[1])
            mag = np.abs(delta) if change else np.abs(lights[0])
            if "no_write_threshold" in MUTATIONS:
                write = np.ones(px.shape, dtype=bool)
                near = np.zeros(px.shape, dtype=bool)
            else:
                write = mag > 1e-3
                # the operands carry a relative error that grows with the slices behind them; Change's difference of two
                # O(1) alphas keeps their absolute error
                scale = np.abs(lights[0]) + (np.abs(lights[1]) if change else 0.0)
                near = np.abs(mag - 1e-3) < DELTA_WRITE + scale * DELTA_WRITE_REL * (abs(j - p0["start"]) + 1)
            self._rmw((x, y, z), delta, write, near, dep)

    def add_dir_light(self, direction, intensity, added, world, only_pass=None):
        """AddDirLightToSingleLightVolume_RenderThread (LightingShaders.cpp:35-166). Returns (n_passes, margins)."""
        passes, n, margins = light_passes(direction, intensity, world, self.light_dims, self.border_mode)
        for i in range(n):
            if only_pass is None or only_pass == i:
                self._streams_pass([(passes[i], 1.0 if added else -1.0)], world, change=False)
        return n, margins

    def change_dir_light(self, old, new, world):
        """ChangeDirLightInSingleLightVolume_RenderThread (LightingShaders.cpp:168-326); old / new = (direction, intensity).
        Returns (2 for the fused pass, -1 for the remove + add fallback, margins of both lights)."""
        rp, _, rm = light_passes(old[0], old[1], world, self.light_dims, self.border_mode)
        ap, _, am = light_passes(new[0], new[1], world, self.light_dims, self.border_mode)
        margins = {k: min(rm[k], am[k]) for k in rm}
        if rp[0]["face"] != ap[0]["face"] or rp[1]["face"] != ap[1]["face"]:   # :192-198
            self.add_dir_light(old[0], old[1], False, world)
            self.add_dir_light(new[0], new[1], True, world)
            return -1, margins
        for i in range(2):                                                      # no weight-0 break in Change (:238)
            self._streams_pass([(rp[i], -1.0), (ap[i], 1.0)], world, change=True)
        return 2, margins


# ------------------------------------------------------------------------------------------------------------------
# raymarch

def rand3d_pcg16(x, y, z):
    """Rand3DPCG16 (engine Random.ush): v = v * 1664525 + 1013904223, two rounds of v.x += v.y*v.z; ..., >> 16."""
    v = [np.asarray(a).astype(np.uint32) for a in (x, y, z)]
    with np.errstate(over="ignore"):
        v = [a * np.uint32(1664525) + np.uint32(1013904223) for a in v]
        for _ in range(2):
            v[0] = v[0] + v[1] * v[2]
            v[1] = v[1] + v[2] * v[0]
            v[2] = v[2] + v[0] * v[1]
    return [a >> np.uint32(16) for a in v]


def tile_rows(tile):
    step = tile.row_group_step if tile.row_group_step > 0 else 1
    j = np.arange(tile.h)
    return tile.y0 + (j // 8) * 8 * step + (j % 8)


def cube_setup(camera, world, tile, scene_depth=None):
    """PerformRaymarchCubeSetup (RaymarchMaterialCommon.usf:23-69) with the pinhole camera of include/tbrm.h.
    Returns (entry [h, w, 3], thickness [h, w], local unit cam vec [h, w, 3], px, py, t1 - t0 before the clamp)."""
    t = world.volume_transform
    rows = tile_rows(tile)
    py, px = np.meshgrid(rows, tile.x0 + np.arange(tile.w), indexing="ij")
    sx = (2.0 * (px + 0.5) / camera.width - 1.0) * camera.tan_half_fov_x
    sy = (1.0 - 2.0 * (py + 0.5) / camera.height) * camera.tan_half_fov_y
    fwd, right, up = _v(camera.forward), _v(camera.right), _v(camera.up)
    d = fwd + sx[..., None] * right + sy[..., None] * up
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    camvec = -d                                                       # CameraVector: pixel -> camera
    rr = _scale_recip(t)

    def inv_vec(v):
        q = t.rotation
        qv = np.array([-q.x, -q.y, -q.z])
        tt = 2.0 * np.cross(qv, v)
        return (v + q.w * tt + np.cross(qv, tt)) * rr

    lcp = inverse_transform_position(t, _v(camera.position)) + 0.5   # :47, :51
    lcv = inv_vec(camvec)
    lcv = -lcv / np.linalg.norm(lcv, axis=-1, keepdims=True)        # :48
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / lcv                                                # RayAABBIntersection (RaymarcherCommon.usf:66-88)
        tmin = (0.0 - lcp) * inv
        tmax = (1.0 - lcp) * inv
    t0 = np.max(np.minimum(tmin, tmax), axis=-1)
    t1 = np.min(np.maximum(tmin, tmax), axis=-1)
    t0 = np.maximum(0.0, t0)                                           # :57
    if scene_depth is not None:                                        # :26-44, :60
        depth = np.asarray(scene_depth, dtype=np.float64)[py, px]
        wdv = camvec * depth[..., None]
        lsd = np.linalg.norm(inv_vec(wdv), axis=-1)
        lsd = lsd / np.abs(camvec @ fwd)
        t1 = np.minimum(lsd, t1)
    thick = np.maximum(0.0, t1 - t0)                                   # :63
    entry = lcp + t0[..., None] * lcv                                  # :66
    return entry, thick, lcv, px, py, t1 - t0


def raymarch_lit(scene, camera, tile, steps, jitter_frame, world, scene_depth=None):
    """PerformWindowedLitRaymarch (WindowedRaymarchMaterials.usf:36-96) for every pixel of the tile.
    Returns (rgba [h, w, 4] float64, taint [h, w])."""
    cc, cd = local_clipping(world)
    entry, thick, lcv, px, py, raw_thick = cube_setup(camera, world, tile, scene_depth)
    step_count = float(np.float32(steps))
    step_size = 1.0 / step_count                                       # :47
    actual = step_count * thick                                        # :49
    max_steps = np.floor(actual).astype(np.int64)                      # :51
    final = actual - np.floor(actual)                                  # :53
    # MaxSteps / FinalStep flip where StepCount * Thickness is near an integer; a ray that misses the cube by more than
    # the margin has thickness 0 in any precision
    taint = ((final < DELTA_FRAC) | (final > 1.0 - DELTA_FRAC)) & (step_count * raw_thick > -DELTA_FRAC)
    vec = lcv * step_size                                              # :56
    step_world = VOLUME_DENSITY * step_size                            # :58
    pos = entry.copy()
    if jitter_frame >= 0:                                              # JitterEntryPos (RaymarchMaterialCommon.usf:73-78)
        r = rand3d_pcg16(px, py, np.full_like(px, jitter_frame & 7))[0].astype(np.float64) / 65535.0
        pos = pos - vec * r[..., None]
    le = np.zeros(pos.shape[:-1] + (4,), dtype=np.float64)
    done = np.zeros(pos.shape[:-1], dtype=bool)
    dpos = delta_ray_pos(steps)
    lv = scene.light_values()
    light_mode = ADDR_CLAMP if "light_clamp_addr" in MUTATIONS else ADDR_WRAP
    data_mode = scene.data_address_mode

    def accumulate(mask, p, stepw):
        """AccumulateWindowedRaymarchStep (:21-33) + AccumulateLightEnergy (RaymarchMaterialCommon.usf:82-88) on rays `mask`."""
        nonlocal taint
        q = p[mask]
        v = sample_3d(scene.data, q[:, 0], q[:, 1], q[:, 2], data_mode)
        sw = stepw[mask] if np.ndim(stepw) else stepw
        rgba, t = windowed_tf(v, sw, scene.tf, scene.windowing, DELTA_TF)
        sq = np.clip(q, 0.0, 1.0)                                     # saturate(CurPos), Wrap_WorldGroupSettings (:30)
        light = sample_3d(lv, sq[:, 0], sq[:, 1], sq[:, 2], light_mode)
        rgba[:, :3] *= light[:, None]
        cur = le[mask]
        om = 1.0 - cur[:, 3]
        cur[:, :3] += rgba[:, :3] * rgba[:, 3:4] * om[:, None]
        cur[:, 3] += rgba[:, 3] * om
        le[mask] = cur
        tt = taint[mask]
        taint[mask] = tt | t

    def clipped(p):
        dist = (p - cc) @ cd                                           # IsCurPosClipped (RaymarcherCommon.usf:22-25)
        return dist <= 0.0, np.abs(dist) < dpos

    nmax = int(max_steps.max()) if max_steps.size else 0
    for i in range(nmax):
        active = (i < max_steps) & ~done
        if not active.any():
            break
        pos[active] += vec[active]                                     # :67
        cl, near = clipped(pos)
        taint |= active & near
        m = active & ~cl
        accumulate(m, pos, step_world)
        taint |= m & (np.abs(le[..., 3] - 0.95) < DELTA_EXIT)
        ex = m & (le[..., 3] > 0.95)                                   # :75-79
        le[ex, 3] = 1.0
        done |= ex
    fin = ~done & (final > 0.0)                                        # :84
    pos[fin] += vec[fin] * final[fin][:, None]                         # :86
    cl, near = clipped(pos)
    taint |= fin & near
    m = fin & ~cl
    if "final_step_stepsize" in MUTATIONS:
        fs = step_size * final * VOLUME_DENSITY
    else:
        fs = VOLUME_DENSITY * final                                    # :91
    accumulate(m, pos, fs)
    return le, taint
