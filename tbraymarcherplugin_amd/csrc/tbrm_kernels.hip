// tbrm_kernels.hip — hand-written gfx950 (CDNA4, wave64) kernels of the raymarch + illumination hot path.
//
//   (the illumination kernels live in tbrm_light_kernels.hip)
//   k_raymarch_lit     : PerformRaymarchCubeSetup + PerformWindowedLitRaymarch
//                        (RaymarchMaterialCommon.usf:23-78, WindowedRaymarchMaterials.usf:21-96).
//   k_fill             : ClearTextureShader.usf:12-16 / ClearVolumeTextureShader.usf:14-20.
//   (skipping metadata, relayout, self-tests: tbrm_volume_kernels.hip)
//
// Compiled with -ffp-contract=off; see tbrm_device_math.h for the arithmetic contract.
#include "tbrm_device_sampling.h"

#include <algorithm>
#include <type_traits>

namespace tbrm {

// Compiled four times (build.py): as it stands, with -DTBRM_RAY_RGB_UNIT=1 for k_raymarch_lit's RGB-light form alone
// (launch_raymarch_rgb), with -DTBRM_RAY_REC_UNIT=1 for the view cache's kernels alone (the recording forms of k_raymarch_lit,
// k_view_scan, k_relight), and with -DTBRM_RAY_HIT_UNIT=1 for k_raymarch_hit alone (launch_raymarch_hit), so that the four sets of
// instantiations build side by side.
#if defined(TBRM_RAY_RGB_UNIT) || defined(TBRM_RAY_REC_UNIT) || defined(TBRM_RAY_HIT_UNIT)
#define TBRM_RAY_ONLY_UNIT 1
#undef TBRM_RAY_STATS // (the diagnostics build counts in the mono unit alone)
#endif
#ifndef TBRM_RAY_ONLY_UNIT
// ------------------------------------------------------------------------------------------------------------
// fill

template <int FMT>
__global__ void k_fill(void* dst, size_t n, float value)
{
    const size_t stride = (size_t) gridDim.x * blockDim.x;
    for (size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) store_voxel<FMT>(dst, i, value);
}

hipError_t launch_fill(void* dst, int fmt, size_t n, float value, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    if (fmt == FMT_U8) {
        // every byte gets the same UNORM8 code -> a plain memset (host replicates encode_u8)
        float x = value;
        if (x != x) x = 0.0f;
        x = x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x);
        const int code = (int) (x * 255.0f + 0.5f);
        return hipMemsetAsync(dst, code, n, s);
    }
    const int block = 256;
    const size_t want = (n + block - 1) / block;
    const int grid = (int) (want < 2048 ? want : 2048);
    hipLaunchKernelGGL(k_fill<FMT_F32>, dim3(grid), dim3(block), 0, s, dst, n, value);
    return hipGetLastError();
}
#endif // !TBRM_RAY_ONLY_UNIT

// ------------------------------------------------------------------------------------------------------------
// raymarch

__device__ __forceinline__ void rand3d_pcg16(int px, int py, int pz, uint32_t& ox)
{
    uint32_t x = (uint32_t) px, y = (uint32_t) py, z = (uint32_t) pz;
    x = x * 1664525u + 1013904223u;
    y = y * 1664525u + 1013904223u;
    z = z * 1664525u + 1013904223u;
    x += y * z; y += z * x; z += x * y;
    x += y * z; y += z * x; z += x * y;
    ox = x >> 16;
}

struct Ray {
    float pos[3];
    float lcv[3];
    float thickness;
};

__device__ __forceinline__ void normalize3(float* v)
{
    const float l = sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    v[0] = v[0] / l; v[1] = v[1] / l; v[2] = v[2] / l;
}

// PerformRaymarchCubeSetup (RaymarchMaterialCommon.usf:23-69) for framebuffer pixel (px,py).
__device__ __forceinline__ void cube_setup(const RayParams& p, int px, int py, Ray& ray)
{
    const float sx = (((2.0f * ((float) px + 0.5f)) / (float) p.width) - 1.0f) * p.thx;
    const float sy = (1.0f - ((2.0f * ((float) py + 0.5f)) / (float) p.height)) * p.thy;
    float d[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) d[c] = (p.fwd[c] + p.right[c] * sx) + p.up[c] * sy;
    normalize3(d);
    const float camvec[3] = {-d[0], -d[1], -d[2]};
    float lcp[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        lcp[c] = ((p.cam_pos[0] * p.m[0 + c] + p.cam_pos[1] * p.m[3 + c]) + p.cam_pos[2] * p.m[6 + c]) + p.m[9 + c];
        ray.lcv[c] = (camvec[0] * p.m[0 + c] + camvec[1] * p.m[3 + c]) + camvec[2] * p.m[6 + c];
    }
    normalize3(ray.lcv);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        ray.lcv[c] = -ray.lcv[c];
        lcp[c] = lcp[c] + 0.5f;
    }
    float t0 = 0.0f, t1 = 0.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) { // RayAABBIntersection (RaymarcherCommon.usf:66-88), box [0,1]^3
        const float inv = 1.0f / ray.lcv[c];
        const float tmin = (0.0f - lcp[c]) * inv, tmax = (1.0f - lcp[c]) * inv;
        const float lo = fminf(tmax, tmin), hi = fmaxf(tmax, tmin);
        if (c == 0) { t0 = lo; t1 = hi; }
        else { t0 = fmaxf(t0, lo); t1 = fminf(t1, hi); }
    }
    t0 = fmaxf(0.0f, t0);
    if (p.depth) {
        float nv[3] = {camvec[0], camvec[1], camvec[2]};
        normalize3(nv);
        const float depth = p.depth[(size_t) py * p.width + px];
        const float wdv[3] = {nv[0] * depth, nv[1] * depth, nv[2] * depth};
        float ldv[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) ldv[c] = (wdv[0] * p.m[0 + c] + wdv[1] * p.m[3 + c]) + wdv[2] * p.m[6 + c];
        float lsd = sqrtf((ldv[0] * ldv[0] + ldv[1] * ldv[1]) + ldv[2] * ldv[2]);
        lsd = lsd / fabsf((p.fwd[0] * camvec[0] + p.fwd[1] * camvec[1]) + p.fwd[2] * camvec[2]);
        t1 = fminf(lsd, t1);
    }
    ray.thickness = fmaxf(0.0f, t1 - t0);
#pragma unroll
    for (int c = 0; c < 3; ++c) ray.pos[c] = lcp[c] + (t0 * ray.lcv[c]);
}

// Pixel of the tile for ray (i, j) of a launch; rows interleave in groups of 8 across GPUs (tbrm_tile.row_group_step)
__device__ __forceinline__ bool tile_pixel_at(const RayParams& p, int i, int j, int& px, int& py)
{
    px = p.tile_x0 + i;
    py = p.tile_y0 + (j >> 3) * 8 * p.row_group_step + (j & 7);
    return i < p.tile_w && j < p.tile_h;
}

__device__ __forceinline__ bool tile_pixel(const RayParams& p, int& i, int& j, int& px, int& py)
{
    // 16x16 pixel block per workgroup, one 8x8 sub-tile per wave64 (the intensity, octree and count kernels: launch_pixel_blocks)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    i = blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7);
    j = blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
    return tile_pixel_at(p, i, j, px, py);
}

// The head of every march (PerformWindowedLitRaymarch, WindowedRaymarchMaterials.usf:46-62; the octree and intensity marches open the
// same way, :111-127 and :194-206) with JitterEntryPos (RaymarchMaterialCommon.usf:73-78): the ray's sample count and where it starts.
struct March {
    int max_steps;    // full steps: floor(Steps * thickness)
    float final_step; // the fraction of a step behind them
    int n_samples;    // the full steps, then the fractional one if there is any (:84-93)
    float sv[3];      // LocalCamVec * StepSize: what a full step adds to the position
    float pos[3];     // the (jittered) entry position
    float step_world; // a full step's length for the opacity correction
};
__device__ __forceinline__ March march_setup(const RayParams& p, const Ray& ray, int px, int py, bool valid) // !valid: a ray of no samples
{
    March m;
    const float step_size = 1 / p.steps;
    const float actual = p.steps * ray.thickness;
    const float fl = floorf(actual);
    m.max_steps = valid ? (int) fl : 0;
    m.final_step = valid ? actual - fl : 0.0f;
    m.n_samples = m.max_steps + (m.final_step > 0.0f ? 1 : 0);
    m.step_world = 100.0f * step_size;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        m.sv[c] = ray.lcv[c] * step_size;
        m.pos[c] = ray.pos[c];
    }
    if (p.jitter_frame >= 0) {
        uint32_t rr;
        rand3d_pcg16(px, py, p.jitter_frame & 7, rr);
        const float rnd = (float) rr / 65535.0f;
#pragma unroll
        for (int c = 0; c < 3; ++c) m.pos[c] = m.pos[c] - (m.sv[c] * rnd);
    }
    return m;
}

// AccumulateLightEnergy (RaymarchMaterialCommon.usf:82-88): c = (colour * alpha, alpha) of a sample, front to back
__device__ __forceinline__ void accumulate(float (&le)[4], const float4& c)
{
    const float om = 1.0f - le[3];
    le[0] = le[0] + (c.x * om);
    le[1] = le[1] + (c.y * om);
    le[2] = le[2] + (c.z * om);
    le[3] = le[3] + (c.w * om);
}
// The early exit (:75-79) belongs to the full steps only; the march that takes it leaves alpha at exactly 1.
__device__ __forceinline__ bool exit_reached(float le3, bool is_full_step) { return le3 > 0.95f && is_full_step; }

// The frame kernels' wave -> pixel mapping (k_raymarch_lit, k_relight): ray r of wave `wave` is ray (i, j) of the launch.
// Workgroups are dealt to the 8 XCDs round-robin by linear id: with the plain (x, y) order the eight horizontal neighbours of a
// pixel block — which march through the same bricks — sit behind eight different L2s. Bands of p.xcd_rows rows of blocks are dealt
// to the XCDs instead (band 8 m + x to XCD x: every XCD still gets an even share of the silhouette), walked column by column; an
// affinity for speed only.
template <int kRayLanes>
__device__ __forceinline__ void ray_of_wave(const RayParams& p, int wave, int r, int& i, int& j)
{
    constexpr int PW = 4, PH = kRayLanes == 4 ? 4 : 2; // rays of a wave: a PW x PH pixel patch
    constexpr int kRayBlockW = 2 * PW, kRayBlockH = 2 * PH;
    int bx = blockIdx.x, by = blockIdx.y;
    if (p.xcd_rows > 0 && (int) gridDim.y % (8 * p.xcd_rows) == 0) {
        const int id = by * (int) gridDim.x + bx, k = id >> 3, per_band = p.xcd_rows * (int) gridDim.x;
        const int band = k / per_band, kk = k - band * per_band;
        bx = kk / p.xcd_rows;
        by = (band * 8 + (id & 7)) * p.xcd_rows + (kk - bx * p.xcd_rows);
    }
    i = bx * kRayBlockW + (wave & 1) * PW + (r % PW);
    j = by * kRayBlockH + (wave >> 1) * PH + (r / PW);
}
// ... and the number a wave's records go by (RayRecord): from the launch id, which the mapping above does not change
__device__ __forceinline__ uint32_t ray_wave_number() { return ((uint32_t) blockIdx.y * gridDim.x + blockIdx.x) * 4u + (threadIdx.x >> 6); }

// ---- k_raymarch_lit ---------------------------------------------------------------------------------------------
// A ray is a serial loop in the reference (positions by repeated addition, front-to-back accumulation with early
// exit). One ray per lane makes a frame as slow as its longest ray: a 512-step ray is 512 dependent memory round trips
// while most of the chip has long run out of work (measured: 1.5 resident waves per SIMD on average, 14 % VALU issue).
// Here a wave marches 16 rays with 4 lanes each (or 8 with 8; a 4x4 / 4x2 pixel patch): per trip lane b of a ray evaluates
// sample L*trip + b
// — position, clip / empty-brick test, 16 taps, transfer function, opacity correction, light — so the expensive part of
// L consecutive samples runs side by side, and only the cheap part stays serial: the L lanes exchange their
// (colour*alpha, alpha) through LDS and each replays AccumulateLightEnergy over the L samples in ray order, which also
// decides the early exit exactly where the reference takes it. Arithmetic per sample and per accumulation step is the
// reference's; a lane reaches its sample position by performing every addition of the ray up to it.
//
// SLAB: one stage of a frame marched slab by slab (tbrm_raymarch_lit_slab_device). The handle owns light-volume slices
// [slab_z0, slab_z1); a sample belongs to the slab its (saturated) z position falls in, and along a ray those slabs come
// in order. The stage takes the ray's LightEnergy as the slabs before it left it (p.out, in place), accumulates the
// samples it owns exactly where the unpartitioned loop would, and hands the state on. Positions are still reached by
// performing every addition of the ray, so every sample, and the early exit, are bit for bit those of the whole march.
#ifdef TBRM_RAY_STATS // diagnostics build (tools/ray_stats.sh): how full the waves of the lit march are
__device__ unsigned long long g_ray_stats[6]; // trips of a wave through the loop, lanes not done, lanes sampling, trips in which any lane samples,
                                              // trips in which any lane has something to accumulate (alpha != 0), such lanes
extern "C" __attribute__((visibility("default"))) int tbrm_debug_ray_stats(unsigned long long* out, int reset)
{
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_ray_stats), sizeof(g_ray_stats)) != hipSuccess) return 1;
    if (reset) {
        const unsigned long long z[6] = {0, 0, 0, 0, 0, 0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_ray_stats), z, sizeof(z)) != hipSuccess) return 1;
    }
    return 0;
}
#endif

// TAB: the data volume's texel -> voxel-offset arithmetic (address mode, +1 tap, bricked offset, brick index of the leap-distance
// look-up: ~45 integer instructions per sample, more than the filter itself) comes out of three small tables the workgroup copies
// into LDS, one {voxel offset, brick-index part} pair per texel index and axis (tbrm_internal.h ray_tab_*; tbrm_resources_create builds
// them); a sample's base and +1 entries of an axis arrive with one 16-byte LDS read. The host picks it when no sample position can lie
// more than two texels outside the volume (a step of at most one texel: positions stay within one step of the unit cube) and the
// tables are small.
//
// LABELS: the label overlay (include/tbrm_labels.h). The lane that takes sample idx also loads the label byte of the sample's
// nearest voxel, beside the data taps; the replay then applies, per sample and in ray order, the data step, the unlit label step
// and the early-exit test. The full step's (rgb * a', a') of every colour-table entry is computed once per workgroup into LDS
// (dynamic, behind the tables: LABELS = false keeps the static layout); the fractional step computes its own. The host passes the
// skipping distance field that has the label occupancy merged in (tbrm_api_labels.cpp), so skipped samples stay exact no-ops.
//
// RGB: the light volume of a colour handle (include/tbrm_color_lights.h): three channels p.light / p.light_g / p.light_b of one
// layout, so one set of tap offsets and one set of weights serves all three (the data taps' where same_grid holds). The light is
// needed only behind a_sat != 0: the channels are fetched and filtered there, one after the other — three sets of raw taps beside
// the data taps do not fit the 80 registers of six waves per SIMD. The sample is ((cs.r l_r) a, (cs.g l_g) a, (cs.b l_b) a, a);
// nothing else of the march sees the light.
//
// REC: the view cache's recording forms (DESIGN.md 4.1 "Relit frames"; compiled in the recording unit alone). Both deliver the
// normal frame. REC_COUNT also writes, per wave, the number of its trips that had something to accumulate (any_x); REC_FILL writes
// those trips' records (RayRecord: the sample's colour, corrected opacity and saturated position — everything of x but the light)
// from the wave's offset on, when the scan before it found that they fit. REC_OFF is the march itself.
constexpr int REC_OFF = 0, REC_COUNT = 1, REC_FILL = 2;
template <int DFMT, int LFMT, int DMODE, int kRayLanes, bool SLAB = false, bool TAB = false, bool LABELS = false, bool RGB = false, int REC = REC_OFF>
__global__ __launch_bounds__(256, 6) void k_raymarch_lit(const RayParams p) // 6 waves per SIMD (80 VGPRs): measured 3-8 % faster than 5 or 8
{
    static_assert(REC == REC_OFF || (!SLAB && !LABELS && !RGB), "only the plain mono march has recording forms");
    static_assert(!(RGB && (SLAB || LABELS)), "colour handles have no slab stage and no label step");
    static_assert(kRayLanes == 4 || kRayLanes == 8, "instantiated for 4 and 8 lanes per ray");
    static_assert(!(TAB && SLAB), "slab stages keep the arithmetic path (relocated layers)");
    static_assert(!(LABELS && SLAB), "slab stages have no label step");
    extern __shared__ __attribute__((aligned(16))) uint2 s_tab[]; // TAB: [x | y | z] (ray_tab_*); LABELS: then s_lab, s_lb
    const uint2* const tab_x = s_tab;
    const uint2* const tab_y = tab_x + (TAB ? ray_tab_axis_entries(p.data.nx) : 0);
    const uint2* const tab_z = tab_y + (TAB ? ray_tab_axis_entries(p.data.ny) : 0);
    constexpr int LSH = kRayLanes == 4 ? 2 : 3;
    __shared__ float4 s_tf[256];
    __shared__ float4 s_x[256]; // per lane: (colour * alpha, alpha) of its sample; alpha < 0: nothing to accumulate
    s_tf[threadIdx.x] = p.tf[threadIdx.x];
    // LABELS: per colour-table entry its full-step (rgb * a', a'); per lane the label of its sample (-1: no label step)
    float4* const s_lab = reinterpret_cast<float4*>(s_tab + (TAB ? ray_tab_entries(p.data.nx, p.data.ny, p.data.nz) : 0));
    short* const s_lb = reinterpret_cast<short*>(s_lab + 256);
    if constexpr (LABELS) {
        const float4 c = p.lab_colors[threadIdx.x];
        const float a = c.w != 0.0f ? one_minus_pow01_(1.0f - c.w, 100.0f * (1 / p.steps)) : 0.0f; // (the data path's step_world)
        s_lab[threadIdx.x] = make_float4(c.x * a, c.y * a, c.z * a, a);
    }
    if constexpr (!TAB) __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = lane & (kRayLanes - 1), r = lane >> LSH; // sample slot, ray within the wave
    int i, j, px, py;
    ray_of_wave<kRayLanes>(p, wave, r, i, j);
    const bool valid = tile_pixel_at(p, i, j, px, py);

    Ray ray;
    cube_setup(p, valid ? px : p.tile_x0, valid ? py : p.tile_y0, ray);

    // PerformWindowedLitRaymarch (WindowedRaymarchMaterials.usf:36-96)
    const March m = march_setup(p, ray, px, py, valid);
    const int max_steps = m.max_steps, n_samples = m.n_samples;
    const float final_step = m.final_step, step_world = m.step_world, sv0 = m.sv[0], sv1 = m.sv[1], sv2 = m.sv[2];
    float pos0 = m.pos[0], pos1 = m.pos[1], pos2 = m.pos[2];
    if constexpr (TAB) { // the tables (the handle built them once: tbrm_resources::d_ray_tab), unless no ray of the workgroup meets the volume
        if (__syncthreads_or(n_samples > 0)) {
            const int n16 = ray_tab_entries(p.data.nx, p.data.ny, p.data.nz) >> 1;
            for (int i = threadIdx.x; i < n16; i += 256) reinterpret_cast<uint4*>(s_tab)[i] = reinterpret_cast<const uint4*>(p.tab)[i];
            __syncthreads();
        }
    }

    const float nx = (float) p.data.nx, ny = (float) p.data.ny, nz = (float) p.data.nz;
    const float lnx = (float) p.lv_dims[0], lny = (float) p.lv_dims[1], lnz = (float) p.lv_dims[2];
    const VolumeDev lightv{p.light, p.lv_dims[0], p.lv_dims[1], p.lv_dims[2], LFMT, p.lv_bnx, p.lv_bnxy, p.lv_wrap_layer, p.lv_wrap_shift};
    // the light volume shares the data volume's footprint when it has the same size and the position is inside the
    // cube (saturate(CurPos) == CurPos): same texel split, same wrapped indices, same brick offsets
    const bool same_grid = DMODE == ADDR_WRAP && p.share_grid;

    // empty-space leaping: texels the position moves per full step along its fastest axis
    const float inv_texels_per_step = 1.0f / fmaxf(fmaxf(fabsf(sv0) * nx, fabsf(sv1) * ny), fabsf(sv2) * nz);
    int safe_until = -1; // this lane's samples with index <= safe_until are known to be based in empty bricks
    const bool wave_skip = p.wave_skip != 0 && p.skip_dist != nullptr;
    bool eager = false;  // the wave's last trip sampled nothing: this trip's lanes renew their ranges (wave-uniform)
    int renew_wait = 0;  // empty trips to let pass before the next renewal (a renewal that bought no blind trip is not repeated at once)

    float le[4] = {0.0f, 0.0f, 0.0f, 0.0f}; // LightEnergy, replicated in the kRayLanes lanes of the ray
    bool done = n_samples == 0;
    bool mine = valid; // SLAB: this stage's sweep direction handles the ray (rays with local dz >= 0 go up through the slabs)
    if constexpr (SLAB) {
        mine = valid && (p.slab_dir == 0 || (p.slab_dir > 0) == (ray.lcv[2] >= 0.0f));
        if (mine) {
            const float4 in = reinterpret_cast<const float4*>(p.out)[(size_t) j * p.tile_w + i];
            le[0] = in.x; le[1] = in.y; le[2] = in.z; le[3] = in.w;
            done = done || le[3] == 1.0f; // the early exit was taken in a slab before this one (it leaves alpha at exactly 1)
        } else done = true;
    }
    int adds = 0; // full-step additions this lane has applied to its position
    // REC: trips recorded so far; REC_FILL: where the wave's records go, if it may write them (the count form counted as many)
    [[maybe_unused]] uint32_t n_rec = 0, rec_first = 0, rec_room = 0;
    if constexpr (REC == REC_FILL) {
        rec_first = p.rec.offsets[ray_wave_number()];
        rec_room = p.rec.meta[1] != 0 ? p.rec.counts[ray_wave_number()] : 0;
    }
    float4* const xs = s_x + (threadIdx.x & ~(kRayLanes - 1)); // the ray's kRayLanes exchange slots

    // A trip is five stages: advance the position, locate the sample, shade it, exchange and replay, the wave-wide leap. They stay one
    // body, each stage a headed block: at 80 registers the allocation does not survive cutting them out (any one of them as a by-reference
    // lambda or an inlined function gave some instantiation scratch it had not had). The stages another kernel runs as well are text
    // included here: 1 and 2 (tbrm_ray_locate.inc) and 5 (tbrm_ray_leap.inc) with k_raymarch_hit, 4 (tbrm_ray_replay.inc) with k_relight.
    for (int base = 0; __builtin_amdgcn_ballot_w64(!done) != 0; base += kRayLanes) {
        float4 x = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
        [[maybe_unused]] float4 rec_x = x;                                // REC_FILL: (cs.rgb, a) of x
        [[maybe_unused]] float rec_sp0 = 0.0f, rec_sp1 = 0.0f, rec_sp2 = 0.0f; // ... and where its light is sampled
#include "tbrm_ray_locate.inc"
#ifdef TBRM_RAY_STATS
        {
            const unsigned long long nd = __builtin_popcountll(__builtin_amdgcn_ballot_w64(!done)), nl = __builtin_popcountll(__builtin_amdgcn_ballot_w64(live));
            if (lane == 0) { atomicAdd(&g_ray_stats[0], 1ull); atomicAdd(&g_ray_stats[1], nd); atomicAdd(&g_ray_stats[2], nl); if (nl) atomicAdd(&g_ray_stats[3], 1ull); }
        }
#endif
        // ---- 3. shade: everything of the reference's loop body up to AccumulateLightEnergy -> x = (colour * alpha, alpha)
        if (live) {
            RawTaps<DFMT> dtaps;
            RawTaps<LFMT> ltaps;
            [[maybe_unused]] TapOffsets lt{}; // RGB: the light taps' offsets, shared by the three channels
            float gx, gy, gz;
            TapOffsets dt;
            if constexpr (TAB) dt = tab_dt;
            else dt = tap_offsets<DMODE, SLAB>(p.data, ix, iy, iz);
            dtaps.issue(p.data.data, dt);
            if constexpr (LABELS) { // the nearest label voxel (SampleLabelVolume): rint((N - 1) * saturate(pos)) per axis, in [0, N - 1]
                const int lx = (int) __builtin_rintf((float) (p.data.nx - 1) * saturate_(q0));
                const int ly = (int) __builtin_rintf((float) (p.data.ny - 1) * saturate_(q1));
                const int lz = (int) __builtin_rintf((float) (p.data.nz - 1) * saturate_(q2));
                lab = p.labels[brick_off(lx, ly, lz, p.data.bnx, p.data.bnxy)];
            }
            // LightVolume.SampleLevel(Wrap, saturate(CurPos)) (WindowedRaymarchMaterials.usf:30)
            const float sp0 = saturate_(q0), sp1 = saturate_(q1), sp2 = saturate_(q2);
            if (same_grid && sp0 == q0 && sp1 == q1 && sp2 == q2) {
                gx = fx; gy = fy; gz = fz;
                if constexpr (RGB) lt = dt;
                else ltaps.issue(p.light, dt);
            } else {
                int lx, ly, lz; // (saturated coordinates: in [0, 1], or NaN -> 0)
                texel_split_bounded(sp0, lnx, lx, gx);
                texel_split_bounded(sp1, lny, ly, gy);
                texel_split_bounded(sp2, lnz, lz, gz);
                if constexpr (RGB) lt = tap_offsets<ADDR_WRAP, SLAB>(lightv, lx, ly, lz);
                else ltaps.issue(p.light, tap_offsets<ADDR_WRAP, SLAB>(lightv, lx, ly, lz));
            }
            const float v = dtaps.filter(fx, fy, fz);
            // SampleWindowedTransferFunction (WindowedSampling.usf:20-37)
            const float tpos = window_position<DFMT != FMT_F32>(v, p.win);
            if (!((tpos < 0.0f && p.win.low_cutoff > 0.0f) || (tpos > 1.0f && p.win.high_cutoff > 0.0f))) {
                const float4 cs = sample_tf(s_tf, tpos);
                const float a_sat = saturate_(cs.w);
                if (a_sat != 0.0f) { // else 1 - pow(1, s) = 0: the sample contributes exactly nothing
                    // (a_sat in (0, 1]; the step is 100 / steps or 100 x a fraction in (0, 1): >= 0 unless the host passed a negative
                    // step count, which build_ray_params rejects — pow01_ is pow_ on that domain, bit for bit)
                    const float a = one_minus_pow01_(1.0f - a_sat, step);
                    if constexpr (RGB) {
                        ltaps.issue(p.light, lt);
                        const float lr = ltaps.filter(gx, gy, gz);
                        ltaps.issue(p.light_g, lt);
                        const float lg = ltaps.filter(gx, gy, gz);
                        ltaps.issue(p.light_b, lt);
                        const float lb = ltaps.filter(gx, gy, gz);
                        x = make_float4((cs.x * lr) * a, (cs.y * lg) * a, (cs.z * lb) * a, a);
                    } else {
                        const float l = ltaps.filter(gx, gy, gz);
                        x = make_float4((cs.x * l) * a, (cs.y * l) * a, (cs.z * l) * a, a);
                        if constexpr (REC == REC_FILL) { rec_x = make_float4(cs.x, cs.y, cs.z, a); rec_sp0 = sp0; rec_sp1 = sp1; rec_sp2 = sp2; }
                    }
                }
            }
            if constexpr (LABELS) {
                if (is_full && s_lab[lab].w == 0.0f) lab = -1; // adds exactly nothing
            }
        }

        // ---- 4. exchange and replay: accumulate() over the ray's kRayLanes samples of the trip, in order, in every lane of
        // the ray; the early exit belongs to the full steps only (:75-79). A trip in which no lane of the wave has
        // anything to accumulate (empty space, windowed-out values) needs no exchange.
        bool to_accumulate = x.w >= 0.0f || x.w != x.w;
        if constexpr (LABELS) to_accumulate = to_accumulate || lab >= 0;
        const bool any_x = __builtin_amdgcn_ballot_w64(to_accumulate) != 0;
#ifdef TBRM_RAY_STATS
        {
            const unsigned long long nx = __builtin_popcountll(__builtin_amdgcn_ballot_w64(x.w >= 0.0f || x.w != x.w));
            if (lane == 0 && nx) { atomicAdd(&g_ray_stats[4], 1ull); atomicAdd(&g_ray_stats[5], nx); }
        }
#endif
        if (any_x) {
            if constexpr (REC == REC_FILL) {
                if (n_rec < rec_room) {
                    const size_t trip = (size_t) rec_first + n_rec;
                    char* const row = p.rec.rows + trip * kRayRecordRowBytes;
                    if (lane == 0) p.rec.base[trip] = base;
                    reinterpret_cast<float4*>(row)[lane] = rec_x;
                    float* const sp = reinterpret_cast<float*>(row + 64 * sizeof(float4));
                    sp[lane] = rec_sp0; sp[64 + lane] = rec_sp1; sp[128 + lane] = rec_sp2;
                }
            }
            if constexpr (REC != REC_OFF) ++n_rec;
#include "tbrm_ray_replay.inc"
        }
        if (base + kRayLanes >= n_samples) done = true;
#include "tbrm_ray_leap.inc"
    }
    if ((SLAB ? mine : valid) && b == 0) reinterpret_cast<float4*>(p.out)[(size_t) j * p.tile_w + i] = make_float4(le[0], le[1], le[2], le[3]);
    if constexpr (REC == REC_COUNT) {
        if (lane == 0) p.rec.counts[ray_wave_number()] = n_rec;
    }
}

// The frame kernels' grid (k_raymarch_lit, k_relight): workgroups of 4 waves of 4x4 / 4x2 rays
template <int RL> static dim3 ray_grid(const RayParams& p)
{
    constexpr int BW = 8, BH = RL == 4 ? 8 : 4;
    return dim3((p.tile_w + BW - 1) / BW, (p.tile_h + BH - 1) / BH);
}
template <int DFMT, int LFMT, int RL, bool SLAB, bool TAB, bool LABELS, bool RGB, int REC>
static hipError_t launch_lit(const RayParams& p, size_t lds_bytes, hipStream_t s)
{
    const dim3 grid = ray_grid<RL>(p), block(256);
    if (p.data_addr_mode == ADDR_CLAMP) hipLaunchKernelGGL((k_raymarch_lit<DFMT, LFMT, ADDR_CLAMP, RL, SLAB, TAB, LABELS, RGB, REC>), grid, block, lds_bytes, s, p);
    else hipLaunchKernelGGL((k_raymarch_lit<DFMT, LFMT, ADDR_WRAP, RL, SLAB, TAB, LABELS, RGB, REC>), grid, block, lds_bytes, s, p);
    return hipGetLastError();
}
#ifndef TBRM_RAY_ONLY_UNIT
// the offset tables (k_raymarch_lit TAB): a step of at most one texel along every axis — then no sample's base tap lies below
// -2 or above n — and tables of at most 16 KiB (six workgroups per CU keep their place)
bool ray_tables_for(const RayParams& p)
{
    const size_t tab_bytes = (size_t) ray_tab_entries(p.data.nx, p.data.ny, p.data.nz) * sizeof(uint2);
    return !p.slab_on && p.tab != nullptr && tune(TUNE_RAY_TABLES) != 0 && (float) std::max(p.data.nx, std::max(p.data.ny, p.data.nz)) <= p.steps && tab_bytes <= 16 * 1024;
}
#endif
template <int DFMT, int LFMT, int RL, bool LABELS, bool RGB, int REC>
static hipError_t launch_ray3(const RayParams& p, hipStream_t s)
{
    // LABELS: the colour-table contributions and the exchanged label bytes, behind the tables (4.5 KiB)
    constexpr size_t lab_bytes = LABELS ? 256 * sizeof(float4) + 256 * sizeof(short) : 0;
    if (p.slab_on) {
        if constexpr (LABELS || RGB || REC != REC_OFF) return hipErrorInvalidValue; // (the host refuses slab stages while labels are attached, and on colour handles)
        else return launch_lit<DFMT, LFMT, RL, true, false, false, false, REC_OFF>(p, 0, s);
    }
    const size_t tab_bytes = (size_t) ray_tab_entries(p.data.nx, p.data.ny, p.data.nz) * sizeof(uint2);
    if (ray_tables_for(p)) return launch_lit<DFMT, LFMT, RL, false, true, LABELS, RGB, REC>(p, tab_bytes + lab_bytes, s);
    return launch_lit<DFMT, LFMT, RL, false, false, LABELS, RGB, REC>(p, lab_bytes, s);
}
#ifndef TBRM_RAY_ONLY_UNIT
int ray_lanes_for(const RayParams& p)
{
    // Lanes per ray, measured on MI355X (ms per frame; 2 lanes: 0.85 / 0.64 / 0.27, 16 lanes: 0.80 / 1.50 / 0.15):
    //                     config 3 (1024^2 rays,   config 5 (2048^2,   config 2 (512^2,   config 4 (1024^2,
    //                               512 steps)              512 steps)         256 steps)        1024 steps)
    //   4 lanes per ray          0.57                    0.68                0.18               1.28
    //   8 lanes per ray          0.61                    0.95                0.14               1.17
    // More lanes per ray shorten the serial chain, fewer keep more rays (and their setup) per wave: few rays or long rays
    // want 8. The rule: rays x (512 / steps) <= 700 k.
    const double load = (double) p.tile_w * (double) p.tile_h * 512.0 / (double) (p.steps > 1.0f ? p.steps : 1.0f);
    const int forced = tune(TUNE_RAY_LANES);
    return (forced ? forced : (load <= 700000.0 ? 8 : 4)) == 8 ? 8 : 4;
}
#endif
template <int DFMT, int LFMT, bool RGB, int REC>
static hipError_t launch_ray2(const RayParams& p, hipStream_t s)
{
    const int rl = ray_lanes_for(p);
    if constexpr (RGB) {
        if (p.labels || !p.light_g || !p.light_b) return hipErrorInvalidValue; // (the host refuses label volumes on colour handles)
        return rl == 8 ? launch_ray3<DFMT, LFMT, 8, false, true, REC>(p, s) : launch_ray3<DFMT, LFMT, 4, false, true, REC>(p, s);
    } else if constexpr (REC != REC_OFF) {
        if (p.labels) return hipErrorInvalidValue; // (frames with a label step are not recorded)
        return rl == 8 ? launch_ray3<DFMT, LFMT, 8, false, false, REC>(p, s) : launch_ray3<DFMT, LFMT, 4, false, false, REC>(p, s);
    } else {
        if (p.labels) return rl == 8 ? launch_ray3<DFMT, LFMT, 8, true, false, REC>(p, s) : launch_ray3<DFMT, LFMT, 4, true, false, REC>(p, s);
        return rl == 8 ? launch_ray3<DFMT, LFMT, 8, false, false, REC>(p, s) : launch_ray3<DFMT, LFMT, 4, false, false, REC>(p, s);
    }
}
template <int DFMT, bool RGB, int REC>
static hipError_t launch_ray1(const RayParams& p, hipStream_t s)
{
    return p.lv_fmt == FMT_U8 ? launch_ray2<DFMT, FMT_U8, RGB, REC>(p, s) : launch_ray2<DFMT, FMT_F32, RGB, REC>(p, s);
}
template <bool RGB, int REC = REC_OFF>
static hipError_t launch_ray0(const RayParams& p, hipStream_t s)
{
    if (p.tile_w <= 0 || p.tile_h <= 0) return hipSuccess;
    switch (p.data.fmt) {
        case FMT_U8: return launch_ray1<FMT_U8, RGB, REC>(p, s);
        case FMT_U16: return launch_ray1<FMT_U16, RGB, REC>(p, s);
        default: return launch_ray1<FMT_F32, RGB, REC>(p, s);
    }
}
#if defined(TBRM_RAY_RGB_UNIT)
hipError_t launch_raymarch_rgb(const RayParams& p, hipStream_t s) { return launch_ray0<true>(p, s); }
#elif defined(TBRM_RAY_HIT_UNIT)
// ---- k_raymarch_hit: where each ray of a tile first gets opaque (include/tbrm_hit.h) ---------------------------------
// The accumulated opacity of a ray never sees the light volume, so this is k_raymarch_lit without its light taps, light filter and
// colour channels: the same prologue (ray_of_wave, cube_setup, march_setup), the same trip — stages 1, 2 and 5 are the lit march's
// own text — and the same replay of accumulate() over the ray's samples in ray order, with one float (the corrected opacity) per
// lane through LDS instead of a float4. The hit test `LightEnergy.a > threshold` stands where exit_reached() stands in the lit
// march, on the fractional step as well; a threshold of at most 0.95 is passed no later than 0.95 is, so the march needs no second
// exit. The lane that evaluated the hit sample still holds its position, filtered value and label and writes the record; lane 0 of
// a ray that ends without a hit writes the no-hit record. Records go out as two 16-byte words.
//
// Waves per SIMD (TBRM_HIT_WAVES, a build-time switch for tools/hit_map_time.py): 6, the lit march's bound, under which the allocator
// is left alone — the instantiations take 58 - 74 registers, none spills, all reach 6 - 8 waves. Builds with 4, 5 and 7 are this code;
// 8 caps the registers at 64 (six instantiations then spill two to scratch, ten keep scalars in vector lanes) and measured the same
// frame time (profiles/r09_hit_map.txt).
#ifndef TBRM_HIT_WAVES
#define TBRM_HIT_WAVES 6
#endif
template <int DFMT, int DMODE, int kRayLanes, bool TAB, bool LABELS>
__global__ __launch_bounds__(256, TBRM_HIT_WAVES) void k_raymarch_hit(const RayParams p, const HitParams h)
{
    static_assert(kRayLanes == 4 || kRayLanes == 8, "instantiated for 4 and 8 lanes per ray");
    constexpr bool SLAB = false; // (what the shared stages name for the slab stage, which a hit map never is)
    extern __shared__ __attribute__((aligned(16))) uint2 s_tab[]; // TAB: [x | y | z] (ray_tab_*); LABELS: then s_lab, s_lb
    const uint2* const tab_x = s_tab;
    const uint2* const tab_y = tab_x + (TAB ? ray_tab_axis_entries(p.data.nx) : 0);
    const uint2* const tab_z = tab_y + (TAB ? ray_tab_axis_entries(p.data.ny) : 0);
    constexpr int LSH = kRayLanes == 4 ? 2 : 3;
    __shared__ float s_tfa[256]; // the transfer function's alpha channel
    __shared__ float s_a[256];   // per lane: the corrected opacity of its sample; < 0: nothing to accumulate
    s_tfa[threadIdx.x] = p.tf[threadIdx.x].w;
    // LABELS: per colour-table entry its full-step a'; per lane the label of its sample (-1: no label step)
    float* const s_lab = reinterpret_cast<float*>(s_tab + (TAB ? ray_tab_entries(p.data.nx, p.data.ny, p.data.nz) : 0));
    short* const s_lb = reinterpret_cast<short*>(s_lab + 256);
    if constexpr (LABELS) {
        const float cw = p.lab_colors[threadIdx.x].w;
        s_lab[threadIdx.x] = cw != 0.0f ? one_minus_pow01_(1.0f - cw, 100.0f * (1 / p.steps)) : 0.0f; // (the data path's step_world)
    }
    if constexpr (!TAB) __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = lane & (kRayLanes - 1), r = lane >> LSH; // sample slot, ray within the wave
    int i, j, px, py;
    ray_of_wave<kRayLanes>(p, wave, r, i, j);
    const bool valid = tile_pixel_at(p, i, j, px, py);

    Ray ray;
    cube_setup(p, valid ? px : p.tile_x0, valid ? py : p.tile_y0, ray);
    const March m = march_setup(p, ray, px, py, valid);
    const int max_steps = m.max_steps, n_samples = m.n_samples;
    const float final_step = m.final_step, step_world = m.step_world, sv0 = m.sv[0], sv1 = m.sv[1], sv2 = m.sv[2];
    float pos0 = m.pos[0], pos1 = m.pos[1], pos2 = m.pos[2];
    if constexpr (TAB) { // the tables, unless no ray of the workgroup meets the volume
        if (__syncthreads_or(n_samples > 0)) {
            const int n16 = ray_tab_entries(p.data.nx, p.data.ny, p.data.nz) >> 1;
            for (int k = threadIdx.x; k < n16; k += 256) reinterpret_cast<uint4*>(s_tab)[k] = reinterpret_cast<const uint4*>(p.tab)[k];
            __syncthreads();
        }
    }

    const float nx = (float) p.data.nx, ny = (float) p.data.ny, nz = (float) p.data.nz;
    [[maybe_unused]] const float lnz = 0.0f; // (named by the slab stage's test in the shared text)
    const float inv_texels_per_step = 1.0f / fmaxf(fmaxf(fabsf(sv0) * nx, fabsf(sv1) * ny), fabsf(sv2) * nz);
    int safe_until = -1;
    const bool wave_skip = p.wave_skip != 0 && p.skip_dist != nullptr;
    bool eager = false;
    int renew_wait = 0;

    float le[4] = {0.0f, 0.0f, 0.0f, 0.0f}; // LightEnergy: only .a is ever read, so only .a is computed
    bool done = n_samples == 0;
    bool found = false; // the ray's hit record has been written
    int adds = 0;
    float* const xs = s_a + (threadIdx.x & ~(kRayLanes - 1)); // the ray's kRayLanes exchange slots
    const size_t out_at = (size_t) j * p.tile_w + i;

    for (int base = 0; __builtin_amdgcn_ballot_w64(!done) != 0; base += kRayLanes) {
#include "tbrm_ray_locate.inc"
        // ---- 3. shade: the reference's loop body up to AccumulateLightEnergy, alpha alone -> xa
        float xa = -1.0f, v = 0.0f;
        [[maybe_unused]] int lab_at = -1; // LABELS: the label byte of the sample's nearest voxel, whether or not it has a step to take
        if (live) {
            RawTaps<DFMT> dtaps;
            TapOffsets dt;
            if constexpr (TAB) dt = tab_dt;
            else dt = tap_offsets<DMODE, false>(p.data, ix, iy, iz);
            dtaps.issue(p.data.data, dt);
            if constexpr (LABELS) { // the nearest label voxel (SampleLabelVolume): rint((N - 1) * saturate(pos)) per axis, in [0, N - 1]
                const int lx = (int) __builtin_rintf((float) (p.data.nx - 1) * saturate_(q0));
                const int ly = (int) __builtin_rintf((float) (p.data.ny - 1) * saturate_(q1));
                const int lz = (int) __builtin_rintf((float) (p.data.nz - 1) * saturate_(q2));
                lab = p.labels[brick_off(lx, ly, lz, p.data.bnx, p.data.bnxy)];
                lab_at = lab;
            }
            v = dtaps.filter(fx, fy, fz);
            // SampleWindowedTransferFunction (WindowedSampling.usf:20-37), its alpha
            const float tpos = window_position<DFMT != FMT_F32>(v, p.win);
            if (!((tpos < 0.0f && p.win.low_cutoff > 0.0f) || (tpos > 1.0f && p.win.high_cutoff > 0.0f))) {
                const float a_sat = saturate_(sample_tf_alpha(s_tfa, tpos));
                if (a_sat != 0.0f) xa = one_minus_pow01_(1.0f - a_sat, step); // (the lit march's domain: a_sat in (0, 1], step >= 0)
            }
            if constexpr (LABELS) {
                if (is_full && s_lab[lab] == 0.0f) lab = -1; // adds exactly nothing
            }
        }

        // ---- 4. exchange and replay, as the lit march's stage 4 (tbrm_ray_replay.inc) with the hit test for its exit test
        bool to_accumulate = xa >= 0.0f || xa != xa;
        if constexpr (LABELS) to_accumulate = to_accumulate || lab >= 0;
        int hit_slot = -1; // the slot of the trip whose sample is the ray's hit (the same in every lane of the ray)
        if (__builtin_amdgcn_ballot_w64(to_accumulate) != 0) {
            s_a[threadIdx.x] = xa;
            if constexpr (LABELS) s_lb[threadIdx.x] = (short) lab;
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int t = 0; t < kRayLanes; ++t) {
                const float cw = xs[t];
                const bool data_step = !(cw < 0.0f);
                if (done || (!LABELS && !data_step)) continue;
                if (data_step) accumulate(le, make_float4(0.0f, 0.0f, 0.0f, cw));
                if constexpr (LABELS) { // then the label step (AccumulateOneRaymarchLabelStep: unlit)
                    const int lb = s_lb[(threadIdx.x & ~(kRayLanes - 1)) + t];
                    if (lb >= 0) {
                        float a;
                        if (base + t < max_steps) a = s_lab[lb];
                        else { // the fractional step (once per ray): its own a' with the step 100 * FinalStep
                            const float raw = p.lab_colors[lb].w;
                            a = raw != 0.0f ? one_minus_pow01_(1.0f - raw, 100.0f * final_step) : 0.0f;
                        }
                        accumulate(le, make_float4(0.0f, 0.0f, 0.0f, a));
                    }
                }
                if (le[3] > h.threshold) { hit_slot = t; done = true; }
            }
            __builtin_amdgcn_wave_barrier();
        }
        if (hit_slot >= 0) { // (a slot with a step to take: its lane evaluated the sample)
            found = true;
            if (b == hit_slot) {
                h.hits[2 * out_at] = make_uint4(__float_as_uint(q0), __float_as_uint(q1), __float_as_uint(q2), (uint32_t) idx);
                h.hits[2 * out_at + 1] = make_uint4(__float_as_uint(le[3]), __float_as_uint(v), (uint32_t) (LABELS ? lab_at : -1), (uint32_t) max_steps);
                if (h.depth) h.depth[out_at] = (((q0 - 0.5f) * h.dg[0] + (q1 - 0.5f) * h.dg[1]) + (q2 - 0.5f) * h.dg[2]) + h.d0;
            }
        }
        if (base + kRayLanes >= n_samples) done = true;
#include "tbrm_ray_leap.inc"
    }
    if (valid && b == 0 && !found) {
        h.hits[2 * out_at] = make_uint4(0u, 0u, 0u, (uint32_t) -1);
        h.hits[2 * out_at + 1] = make_uint4(__float_as_uint(le[3]), 0u, (uint32_t) -1, (uint32_t) max_steps);
        if (h.depth) h.depth[out_at] = __builtin_inff();
    }
}

template <int DFMT, int RL, bool TAB, bool LABELS>
static hipError_t launch_hit3(const RayParams& p, const HitParams& h, size_t lds_bytes, hipStream_t s)
{
    const dim3 grid = ray_grid<RL>(p), block(256);
    if (p.data_addr_mode == ADDR_CLAMP) hipLaunchKernelGGL((k_raymarch_hit<DFMT, ADDR_CLAMP, RL, TAB, LABELS>), grid, block, lds_bytes, s, p, h);
    else hipLaunchKernelGGL((k_raymarch_hit<DFMT, ADDR_WRAP, RL, TAB, LABELS>), grid, block, lds_bytes, s, p, h);
    return hipGetLastError();
}
template <int DFMT, int RL, bool LABELS>
static hipError_t launch_hit2(const RayParams& p, const HitParams& h, hipStream_t s)
{
    // LABELS: the colour table's full-step a' and the exchanged label bytes, behind the tables (1.5 KiB)
    constexpr size_t lab_bytes = LABELS ? 256 * sizeof(float) + 256 * sizeof(short) : 0;
    const size_t tab_bytes = (size_t) ray_tab_entries(p.data.nx, p.data.ny, p.data.nz) * sizeof(uint2);
    if (ray_tables_for(p)) return launch_hit3<DFMT, RL, true, LABELS>(p, h, tab_bytes + lab_bytes, s); // (the lit march's rule)
    return launch_hit3<DFMT, RL, false, LABELS>(p, h, lab_bytes, s);
}
template <int DFMT>
static hipError_t launch_hit1(const RayParams& p, const HitParams& h, hipStream_t s)
{
    const bool eight = ray_lanes_for(p) == 8; // (the lit march's rule)
    if (p.labels) return eight ? launch_hit2<DFMT, 8, true>(p, h, s) : launch_hit2<DFMT, 4, true>(p, h, s);
    return eight ? launch_hit2<DFMT, 8, false>(p, h, s) : launch_hit2<DFMT, 4, false>(p, h, s);
}
hipError_t launch_raymarch_hit(const RayParams& p, const HitParams& h, hipStream_t s)
{
    if (p.tile_w <= 0 || p.tile_h <= 0) return hipSuccess;
    if (p.slab_on) return hipErrorInvalidValue; // (the host refuses slab-resident handles)
    switch (p.data.fmt) {
        case FMT_U8: return launch_hit1<FMT_U8>(p, h, s);
        case FMT_U16: return launch_hit1<FMT_U16>(p, h, s);
        default: return launch_hit1<FMT_F32>(p, h, s);
    }
}
#elif defined(TBRM_RAY_REC_UNIT)
hipError_t launch_raymarch_recording(const RayParams& p, bool fill, hipStream_t s)
{
    return fill ? launch_ray0<false, REC_FILL>(p, s) : launch_ray0<false, REC_COUNT>(p, s);
}

// ---- k_view_scan: the count form's per-wave trip counts -> each wave's first trip, the total, and whether the arena holds it -------
__global__ __launch_bounds__(1024) void k_view_scan(const RayRecord rec, uint32_t n_waves, uint32_t cap_trips)
{
    // (64-bit sums: a total beyond 2^32 trips must read as "does not fit", not wrap; the offsets of such a view are never used.
    // Each thread walks a contiguous run of counts: uncoalesced, and run once per view)
    __shared__ unsigned long long s_sum[1024];
    const uint32_t per = (n_waves + 1023u) / 1024u;
    const uint32_t w0 = (uint32_t) min((unsigned long long) threadIdx.x * per, (unsigned long long) n_waves), w1 = (uint32_t) min((unsigned long long) w0 + per, (unsigned long long) n_waves);
    unsigned long long sum = 0;
    for (uint32_t w = w0; w < w1; ++w) sum += rec.counts[w];
    s_sum[threadIdx.x] = sum;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) { // inclusive scan of the threads' sums
        const unsigned long long v = (int) threadIdx.x >= d ? s_sum[threadIdx.x - d] : 0ull;
        __syncthreads();
        s_sum[threadIdx.x] += v;
        __syncthreads();
    }
    unsigned long long at = s_sum[threadIdx.x] - sum;
    for (uint32_t w = w0; w < w1; ++w) { rec.offsets[w] = (uint32_t) at; at += rec.counts[w]; }
    if (threadIdx.x == 1023) {
        const unsigned long long total = s_sum[1023];
        rec.meta[0] = (uint32_t) min(total, 0xffffffffull);
        rec.meta[1] = total <= cap_trips ? 1u : 0u;
    }
}
hipError_t launch_view_scan(const RayRecord& rec, uint32_t n_waves, uint32_t cap_trips, hipStream_t s)
{
    hipLaunchKernelGGL(k_view_scan, dim3(1), dim3(1024), 0, s, rec, n_waves, cap_trips);
    return hipGetLastError();
}

// ---- k_relight: the frame of an unchanged view from its records ------------------------------------------------------------------
// Everything of a sample but its light is a function of the view (camera, tile, steps, volume, window, transfer function, clip plane):
// the recording forms of k_raymarch_lit kept, for every trip of a wave that had something to accumulate, each lane's (colour, corrected
// opacity) and the saturated position its light is sampled at. A wave here is the march's wave (same grid, same ray_of_wave, same
// ray_wave_number): it walks its records in order, fetches and filters the 8 light taps of the lanes that have a step to take (the
// general path of the march's light look-up: texel_split_bounded + tap_offsets<ADDR_WRAP>, which the shared-grid shortcut equals bit
// for bit), forms x = ((cs.rgb l) a, a) and runs the march's own stage 4. The alpha channel and the early exit never see the light,
// so the steps taken and the exits are the march's. Trip t + 1's record is requested before trip t is worked on.
struct RelightTrip { int base; float4 c; float sp0, sp1, sp2; };
__device__ __forceinline__ RelightTrip relight_load(const RayRecord& rec, size_t trip, int lane)
{
    const char* const row = rec.rows + trip * kRayRecordRowBytes;
    const float* const sp = reinterpret_cast<const float*>(row + 64 * sizeof(float4));
    return RelightTrip{rec.base[trip], reinterpret_cast<const float4*>(row)[lane], sp[lane], sp[64 + lane], sp[128 + lane]};
}
template <int LFMT, int kRayLanes>
__global__ __launch_bounds__(256) void k_relight(const RayParams p)
{
    constexpr int LSH = kRayLanes == 4 ? 2 : 3;
    __shared__ float4 s_x[256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = lane & (kRayLanes - 1), r = lane >> LSH;
    int i, j, px, py;
    ray_of_wave<kRayLanes>(p, wave, r, i, j);
    const bool valid = tile_pixel_at(p, i, j, px, py);
    Ray ray;
    cube_setup(p, valid ? px : p.tile_x0, valid ? py : p.tile_y0, ray);
    const March m = march_setup(p, ray, px, py, valid);
    const int max_steps = m.max_steps, n_samples = m.n_samples;

    const float lnx = (float) p.lv_dims[0], lny = (float) p.lv_dims[1], lnz = (float) p.lv_dims[2];
    const VolumeDev lightv{p.light, p.lv_dims[0], p.lv_dims[1], p.lv_dims[2], LFMT, p.lv_bnx, p.lv_bnxy, p.lv_wrap_layer, p.lv_wrap_shift};
    float le[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    bool done = n_samples == 0;
    float4* const xs = s_x + (threadIdx.x & ~(kRayLanes - 1));
    // (what the shared stage 4 names for the label step, which a relit frame never has)
    constexpr bool LABELS = false;
    [[maybe_unused]] short* const s_lb = nullptr;
    [[maybe_unused]] const float4* const s_lab = nullptr;
    [[maybe_unused]] const int lab = -1;
    [[maybe_unused]] const float final_step = 0.0f;

    const uint32_t w = ray_wave_number();
    const uint32_t n = p.rec.counts[w];
    const size_t first = p.rec.offsets[w];
    RelightTrip next{};
    if (n > 0) next = relight_load(p.rec, first, lane);
    for (uint32_t trip = 0; trip < n; ++trip) { // (the included stage 4 has a loop variable t of its own)
        const RelightTrip cur = next;
        if (trip + 1 < n) next = relight_load(p.rec, first + trip + 1, lane);
        float4 x = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
        if (cur.c.w >= 0.0f || cur.c.w != cur.c.w) {
            int lx, ly, lz;
            float gx, gy, gz;
            texel_split_bounded(cur.sp0, lnx, lx, gx);
            texel_split_bounded(cur.sp1, lny, ly, gy);
            texel_split_bounded(cur.sp2, lnz, lz, gz);
            RawTaps<LFMT> ltaps;
            ltaps.issue(p.light, tap_offsets<ADDR_WRAP, false>(lightv, lx, ly, lz));
            const float l = ltaps.filter(gx, gy, gz);
            x = make_float4((cur.c.x * l) * cur.c.w, (cur.c.y * l) * cur.c.w, (cur.c.z * l) * cur.c.w, cur.c.w);
        }
        const int base = cur.base;
        {
#include "tbrm_ray_replay.inc"
        }
        if (base + kRayLanes >= n_samples) done = true;
    }
    if (valid && b == 0) reinterpret_cast<float4*>(p.out)[(size_t) j * p.tile_w + i] = make_float4(le[0], le[1], le[2], le[3]);
}
template <int LFMT, int RL> static hipError_t launch_relight2(const RayParams& p, hipStream_t s)
{
    hipLaunchKernelGGL((k_relight<LFMT, RL>), ray_grid<RL>(p), dim3(256), 0, s, p);
    return hipGetLastError();
}
hipError_t launch_relight(const RayParams& p, hipStream_t s) // (the lanes per ray the records were written with: the key holds them)
{
    if (p.tile_w <= 0 || p.tile_h <= 0) return hipSuccess;
    const bool eight = ray_lanes_for(p) == 8;
    if (p.lv_fmt == FMT_U8) return eight ? launch_relight2<FMT_U8, 8>(p, s) : launch_relight2<FMT_U8, 4>(p, s);
    return eight ? launch_relight2<FMT_F32, 8>(p, s) : launch_relight2<FMT_F32, 4>(p, s);
}
#else
hipError_t launch_raymarch(const RayParams& p, hipStream_t s) { return launch_ray0<false>(p, s); }

// ---- self-test of the division-free window position (tf_position_fast against the IEEE quotient, every float in [0, 1]) --------------
__global__ __launch_bounds__(256) void k_selftest_window_division(WindowDev w, unsigned long long* mismatches)
{
    const uint32_t last = 0x3f800000u; // 1.0f
    unsigned long long bad = 0;
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i <= last; i += (uint64_t) gridDim.x * blockDim.x) {
        const float v = __uint_as_float((uint32_t) i);
        const float a = tf_position(v, w.center, w.width), b = tf_position_fast(v, w.center, w.width, w.inv_width);
        if (__float_as_uint(a) != __float_as_uint(b)) ++bad;
    }
    if (bad) atomicAdd(mismatches, bad);
}
hipError_t launch_selftest_window_division(const WindowDev& w, unsigned long long* d_mismatches, hipStream_t s)
{
    hipLaunchKernelGGL(k_selftest_window_division, dim3(256 * 64), dim3(256), 0, s, w, d_mismatches);
    return hipGetLastError();
}

// ---- self-test of the opacity correction's short form (one_minus_pow01_ against 1 - pow01_, every float in [0, 1]) --------------------
__global__ __launch_bounds__(256) void k_selftest_opacity_correction(float step0, float step1, unsigned long long* mismatches)
{
    const uint32_t last = 0x3f800000u; // 1.0f
    unsigned long long bad = 0;
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i <= last; i += (uint64_t) gridDim.x * blockDim.x) {
        const float x = __uint_as_float((uint32_t) i);
        float p0, p1, s0, s1;
        pow01_2_(x, step0, step1, p0, p1);
        one_minus_pow01_2_(x, step0, step1, s0, s1);
        const float a = 1.0f - pow01_(x, step0), b = one_minus_pow01_(x, step0);
        if (__float_as_uint(1.0f - p0) != __float_as_uint(s0) || __float_as_uint(1.0f - p1) != __float_as_uint(s1) || __float_as_uint(a) != __float_as_uint(b)) ++bad;
    }
    if (bad) atomicAdd(mismatches, bad);
}
hipError_t launch_selftest_opacity_correction(float step0, float step1, unsigned long long* d_mismatches, hipStream_t s)
{
    hipLaunchKernelGGL(k_selftest_opacity_correction, dim3(256 * 64), dim3(256), 0, s, step0, step1, d_mismatches);
    return hipGetLastError();
}

// One ray per lane, 16x16 pixel blocks (tile_pixel): the launch of the intensity, octree and count kernels; an empty tile launches nothing
static hipError_t launch_pixel_blocks(void (*kernel)(const RayParams), const RayParams& p, hipStream_t s)
{
    if (p.tile_w <= 0 || p.tile_h <= 0) return hipSuccess;
    hipLaunchKernelGGL(kernel, dim3((p.tile_w + 15) / 16, (p.tile_h + 15) / 16), dim3(256), 0, s, p);
    return hipGetLastError();
}

// ---- k_raymarch_intensity: PerformWindowedIntensityRaymarch (WindowedRaymarchMaterials.usf:187-242) ----------------
// The slice view: the windowed intensity of the first sample the clipping plane leaves. Without a clipping plane that is
// every ray's first sample, so one ray per lane is the right shape here (no long serial loop to split up).
template <int DFMT>
__global__ __launch_bounds__(256) void k_raymarch_intensity(const RayParams p)
{
    int i, j, px, py;
    if (!tile_pixel(p, i, j, px, py)) return;
    Ray ray;
    cube_setup(p, px, py, ray);
    const March m = march_setup(p, ray, px, py, true);
    const float sv0 = m.sv[0], sv1 = m.sv[1], sv2 = m.sv[2];
    float pos0 = m.pos[0], pos1 = m.pos[1], pos2 = m.pos[2];
    const float nx = (float) p.data.nx, ny = (float) p.data.ny, nz = (float) p.data.nz;
    auto intensity = [&](float u, float v, float w) -> float { // DataVolume.SampleLevel(Clamp, uvw).r -> clamp(TFPos, 0, 1)
        int ix, iy, iz;
        float fx, fy, fz;
        texel_split(u, nx, ix, fx);
        texel_split(v, ny, iy, fy);
        texel_split(w, nz, iz, fz);
        const float val = sample_trilinear_at<DFMT>(p.data.data, tap_offsets<ADDR_CLAMP>(p.data, ix, iy, iz), fx, fy, fz);
        return __builtin_amdgcn_fmed3f(tf_position(val, p.win.center, p.win.width), 0.0f, 1.0f);
    };
    float4 out = make_float4(0.0f, 0.0f, 0.0f, 0.0f); // didn't hit anything (:241)
    bool hit = false;
    for (int k = 0; k < m.max_steps; ++k) {
        pos0 = pos0 + sv0; pos1 = pos1 + sv1; pos2 = pos2 + sv2;
        const float s0 = saturate_(pos0), s1 = saturate_(pos1), s2 = saturate_(pos2);
        if (!(p.clip_mode && is_clipped(s0, s1, s2, p.cc, p.cd))) {
            const float t = intensity(s0, s1, s2);
            out = make_float4(t, t, t, 1.0f);
            hit = true;
            break;
        }
    }
    if (!hit && m.final_step > 0.0f) {
        pos0 = pos0 + (sv0 * m.final_step); pos1 = pos1 + (sv1 * m.final_step); pos2 = pos2 + (sv2 * m.final_step);
        if (!(p.clip_mode && is_clipped(pos0, pos1, pos2, p.cc, p.cd))) {
            const float t = intensity(pos0, pos1, pos2);
            out = make_float4(t, t, t, 1.0f);
        }
    }
    reinterpret_cast<float4*>(p.out)[(size_t) j * p.tile_w + i] = out;
}

hipError_t launch_raymarch_intensity(const RayParams& p, hipStream_t s)
{
    switch (p.data.fmt) {
        case FMT_U8: return launch_pixel_blocks(k_raymarch_intensity<FMT_U8>, p, s);
        case FMT_U16: return launch_pixel_blocks(k_raymarch_intensity<FMT_U16>, p, s);
        default: return launch_pixel_blocks(k_raymarch_intensity<FMT_F32>, p, s);
    }
}

// ---- Octree render mode (experimental in the reference) -------------------------------------------------------------
// GenerateOctreeShader.usf:28-107: level 0 = the volume (x MinMaxValues.y = 1, OctreeShaders.h:49) as UNORM16, 0 outside the
// volume; level m = max over the 2x2x2 texels of level m-1. One thread per output texel (the reference runs one thread
// per 8^3 leaf, [numthreads(1,1,1)]).
template <int DFMT>
__global__ __launch_bounds__(256) void k_octree_base(const OctreeParams p)
{
    const size_t n = (size_t) p.dims[0] * p.dims[1] * p.dims[2];
    const size_t i = (size_t) blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int x = (int) (i % p.dims[0]), y = (int) ((i / p.dims[0]) % p.dims[1]), z = (int) (i / ((size_t) p.dims[0] * p.dims[1]));
    float v = 0.0f;
    if (x < p.data.nx && y < p.data.ny && z < p.data.nz) v = load_voxel<DFMT>(p.data.data, brick_off(x, y, z, p.data.bnx, p.data.bnxy)) * 1.0f;
    p.out[i] = (uint16_t) __builtin_floorf(__builtin_amdgcn_fmed3f(v, 0.0f, 1.0f) * 65535.0f + 0.5f); // UNORM16 store, NaN -> 0
}
__global__ __launch_bounds__(256) void k_octree_reduce(const OctreeParams p)
{
    const size_t n = (size_t) p.dims[0] * p.dims[1] * p.dims[2];
    const size_t i = (size_t) blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int x = (int) (i % p.dims[0]), y = (int) ((i / p.dims[0]) % p.dims[1]), z = (int) (i / ((size_t) p.dims[0] * p.dims[1]));
    uint32_t mx = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int sx = 2 * x + (k & 1), sy = 2 * y + ((k >> 1) & 1), sz = 2 * z + (k >> 2);
        if (sx < p.lower_dims[0] && sy < p.lower_dims[1] && sz < p.lower_dims[2])
            mx = max(mx, (uint32_t) p.lower[((size_t) sz * p.lower_dims[1] + sy) * p.lower_dims[0] + sx]);
    }
    p.out[i] = (uint16_t) mx;
}
hipError_t launch_octree_level(const OctreeParams& p, bool base, hipStream_t s)
{
    const size_t n = (size_t) p.dims[0] * p.dims[1] * p.dims[2];
    const dim3 grid((unsigned) ((n + 255) / 256)), block(256);
    if (!base) hipLaunchKernelGGL(k_octree_reduce, grid, block, 0, s, p);
    else if (p.data.fmt == FMT_U8) hipLaunchKernelGGL(k_octree_base<FMT_U8>, grid, block, 0, s, p);
    else if (p.data.fmt == FMT_U16) hipLaunchKernelGGL(k_octree_base<FMT_U16>, grid, block, 0, s, p);
    else hipLaunchKernelGGL(k_octree_base<FMT_F32>, grid, block, 0, s, p);
    return hipGetLastError();
}

// PerformWindowedRaymarchOctree (WindowedRaymarchMaterials.usf:99-183): unlit, point-sampled march over one octree level.
__global__ __launch_bounds__(256) void k_raymarch_octree(const RayParams p)
{
    __shared__ float4 s_tf[256];
    s_tf[threadIdx.x] = p.tf[threadIdx.x];
    __syncthreads();
    int i, j, px, py;
    if (!tile_pixel(p, i, j, px, py)) return;
    Ray ray;
    cube_setup(p, px, py, ray);
    const March m = march_setup(p, ray, px, py, true);
    const float sv0 = m.sv[0], sv1 = m.sv[1], sv2 = m.sv[2];
    float pos0 = m.pos[0], pos1 = m.pos[1], pos2 = m.pos[2];
    const float ow = (float) p.oct_dims[0], oh = (float) p.oct_dims[1], od = (float) p.oct_dims[2], data_depth = (float) p.data.nz;
    float le[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int k = 0; k <= m.max_steps; ++k) {
        if (k < m.max_steps) { pos0 = pos0 + sv0; pos1 = pos1 + sv1; pos2 = pos2 + sv2; }
        else {
            if (!(m.final_step > 0.0f)) break;
            pos0 = pos0 + (sv0 * m.final_step); pos1 = pos1 + (sv1 * m.final_step); pos2 = pos2 + (sv2 * m.final_step);
        }
        if (p.clip_mode && is_clipped(pos0, pos1, pos2, p.cc, p.cd)) continue;
        // int3 VoxelPos = float3(x * W, y * H, (z * DataDepth / OctreeDepth0) * OctreeDepth) (:150): truncation; Load outside -> 0
        const float fx = pos0 * ow, fy = pos1 * oh, fz = ((pos2 * data_depth) / p.oct_depth0) * od;
        float v = 0.0f;
        if (fx == fx && fy == fy && fz == fz && fx > -1.0f && fy > -1.0f && fz > -1.0f && fx < ow && fy < oh && fz < od) {
            const int vx = (int) fx, vy = (int) fy, vz = (int) fz;
            v = decode_u16(p.octree[((size_t) vz * p.oct_dims[1] + vy) * p.oct_dims[0] + vx]);
        }
        // SampleWindowedTransferFunction with StepSizeWorld — also in the fractional step (:176), unlike the lit march
        const float tpos = tf_position(v, p.win.center, p.win.width);
        if ((tpos < 0.0f && p.win.low_cutoff > 0.0f) || (tpos > 1.0f && p.win.high_cutoff > 0.0f)) continue;
        const float4 cs = sample_tf(s_tf, tpos);
        const float a_sat = saturate_(cs.w);
        const float a = 1.0f - pow_(1.0f - a_sat, m.step_world);
        accumulate(le, make_float4(cs.x * a, cs.y * a, cs.z * a, a)); // ((cs * a) * om, as the lit march's samples)
        if (exit_reached(le[3], k < m.max_steps)) { le[3] = 1.0f; break; }
    }
    reinterpret_cast<float4*>(p.out)[(size_t) j * p.tile_w + i] = make_float4(le[0], le[1], le[2], le[3]);
}
hipError_t launch_raymarch_octree(const RayParams& p, hipStream_t s) { return launch_pixel_blocks(k_raymarch_octree, p, s); }

// Nominal samples: sum over rays of floor(Steps*thickness) + [frac > 0].
__global__ __launch_bounds__(256) void k_count_samples(const RayParams p)
{
    int i, j, px, py;
    const bool valid = tile_pixel(p, i, j, px, py);
    unsigned long long n = 0;
    if (valid) {
        Ray ray;
        cube_setup(p, px, py, ray);
        n = (unsigned long long) march_setup(p, ray, px, py, true).n_samples;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_down(n, o, 64);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(p.sample_counter, n);
}

hipError_t launch_count_samples(const RayParams& p, hipStream_t s) { return launch_pixel_blocks(k_count_samples, p, s); }

#endif // the unit

} // namespace tbrm
