// tbrm_api_render.cpp — the C-ABI's render entry points (include/tbrm.h): the lit raymarch (PerformWindowedLitRaymarch,
// WindowedRaymarchMaterials.usf:36-96, with its cube setup RaymarchMaterialCommon.usf:23-69), its slab stage, the Intensity
// slice view (:187-242), the Octree mode's pyramid and march (GenerateOctreeShader.usf:28-107, :99-183) and the nominal-sample
// count of the benchmark's metric. Handle life cycle, inputs and light operators: tbrm_api.cpp.
#include "tbrm_resources.h"
#include "../../include/tbrm_view_cache.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace tbrm;
using namespace tbrm_host;

namespace tbrm_host {

int build_ray_params(tbrm_resources* r, const tbrm_camera* cam, const tbrm_tile* tile, const tbrm_raymarch_params* rp,
                     const tbrm_world_params* world, RayParams& p)
{
    if (!(rp->steps > 0.0f)) return fail(TBRM_ERR_INVALID_ARG, "steps must be > 0");
    if (tile->w < 0 || tile->h < 0 || cam->width <= 0 || cam->height <= 0) return fail(TBRM_ERR_INVALID_ARG, "bad tile/camera size");
    std::memset(&p, 0, sizeof(p)); // (padding too: the view cache compares the block)
    p.data = data_view(r);
    p.data_addr_mode = r->desc.data_address_mode == TBRM_ADDRESS_CLAMP ? ADDR_CLAMP : ADDR_WRAP;
    p.tf = r->d_tf;
    p.win = window_dev(r);
    p.xcd_rows = tune(TUNE_RAY_XCD_ROWS);
    p.light = r->d_light;
    for (int c = 0; c < 3; ++c) p.lv_dims[c] = r->lv_dims[c];
    p.lv_bnx = r->lbn[0];
    p.lv_bnxy = r->lbn[0] * r->lbn[1];
    p.lv_fmt = r->lv_fmt;
    p.lv_wrap_layer = r->res_light.wrap_src;
    p.lv_wrap_shift = (r->res_light.hi - r->res_light.wrap_src) * 8;
    const tbrm_vec3d* v[4] = {&cam->position, &cam->forward, &cam->right, &cam->up};
    float* dst[4] = {p.cam_pos, p.fwd, p.right, p.up};
    for (int k = 0; k < 4; ++k) {
        dst[k][0] = (float) v[k]->x; dst[k][1] = (float) v[k]->y; dst[k][2] = (float) v[k]->z;
    }
    p.thx = (float) cam->tan_half_fov_x;
    p.thy = (float) cam->tan_half_fov_y;
    p.width = cam->width;
    p.height = cam->height;
    host_world_to_local(world->volume_transform, p.m);
    host_local_clipping(*world, p.cc, p.cd);
    p.clip_mode = raymarch_clip_mode(p.cc, p.cd);
    {   // (measured: frames of 128^3 / 256^3 volumes lose 15 % to the bookkeeping, 512^3 is even, 2048^2 rays through 512^3 gain 12 %)
        const int ws = tune(TUNE_RAY_WAVE_SKIP);
        p.wave_skip = ws > 0 || (ws < 0 && std::min(r->desc.dim_x, std::min(r->desc.dim_y, r->desc.dim_z)) >= 384) ? 1 : 0;
    }
    p.share_grid = (r->lv_dims[0] == r->desc.dim_x && r->lv_dims[1] == r->desc.dim_y && r->lv_dims[2] == r->desc.dim_z &&
                    !r->resident && tune(TUNE_SHARE_GRID)) ? 1 : 0; // (the two volumes of a slab-resident handle relocate different layers)
    p.tile_x0 = tile->x0; p.tile_y0 = tile->y0; p.tile_w = tile->w; p.tile_h = tile->h;
    p.row_group_step = tile->row_group_step > 0 ? tile->row_group_step : 1;
    p.steps = rp->steps;
    p.jitter_frame = rp->jitter_frame;
    p.bnx = r->bn[0]; p.bny = r->bn[1]; p.bnz = r->bn[2];
    p.tab = r->d_ray_tab;
    return TBRM_OK;
}

// the skipping metadata of a lit frame that asks for it, brought up to date
int attach_skipping(tbrm_resources* r, const tbrm_raymarch_params* rp, RayParams& p)
{
    if (!rp->enable_skipping) return TBRM_OK;
    if (int e = ensure_skipping(r)) return e;
    p.empty_bits = r->d_empty;
    p.skip_dist = r->d_dist[0];
    return TBRM_OK;
}

} // namespace tbrm_host

namespace {

// The host-pointer form of a frame call: checks the tile, has `march` (the call's _device form, which makes every other argument
// check) render it into the handle's own device buffer, grown to the largest tile seen, and copies that to the caller's, complete
// on return. *delivered: a frame went out (an empty tile is TBRM_OK with nothing done).
template <class March> int deliver_frame(tbrm_resources* r, const tbrm_tile* tile, float* host_out_rgba, March&& march, bool* delivered = nullptr)
{
    if (!r || !tile || !host_out_rgba) return fail(TBRM_ERR_INVALID_ARG, "null argument");
    if (tile->w < 0 || tile->h < 0) return fail(TBRM_ERR_INVALID_ARG, "bad tile size");
    const size_t bytes = (size_t) tile->w * tile->h * 4 * sizeof(float);
    if (bytes == 0) return TBRM_OK;
    if (int e = bind(r)) return e;
    if (bytes > r->out_bytes) {
        HIP_TRY(hipStreamSynchronize(r->stream));
        (void) hipFree(r->d_out);
        r->d_out = nullptr;
        r->out_bytes = 0;
        HIP_TRY(hipMalloc((void**) &r->d_out, bytes));
        r->out_bytes = bytes;
    }
    if (int e = march(r->d_out)) return e;
    HIP_TRY(hipMemcpyAsync(host_out_rgba, r->d_out, bytes, hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    if (delivered) *delivered = true;
    return TBRM_OK;
}

// ---- the view cache (tbrm_resources.h ViewCache; DESIGN.md 4.1 "Relit frames") -----------------------------------------------------

// The current view's share of the arena: [counts | offsets | meta] for its waves, then as many trips' base words and rows as fit.
// false: no arena, or not even the per-wave words fit.
bool carve_view_arena(ViewCache& v, const RayParams& p)
{
    const size_t bw = 8, bh = v.lanes == 4 ? 8 : 4; // (launch_lit's grid: 4 waves per workgroup)
    const size_t waves = ((size_t) p.tile_w + bw - 1) / bw * (((size_t) p.tile_h + bh - 1) / bh) * 4;
    const size_t align = 256, header = (2 * waves * sizeof(uint32_t) + 16 + align - 1) / align * align;
    if (!v.arena || waves > 0xffffffffu || header + 2 * align + kRayRecordTripBytes > v.arena_bytes) return false;
    const size_t cap = std::min<size_t>((v.arena_bytes - header - align) / kRayRecordTripBytes, 0xffffffffu);
    v.n_waves = (uint32_t) waves;
    v.cap_trips = (uint32_t) cap;
    v.rec.counts = reinterpret_cast<uint32_t*>(v.arena);
    v.rec.offsets = v.rec.counts + waves;
    v.rec.meta = v.rec.offsets + waves;
    v.rec.base = reinterpret_cast<int32_t*>(v.arena + header);
    v.rec.rows = v.arena + header + (cap * sizeof(int32_t) + align - 1) / align * align;
    return true;
}

// The frame of a mono handle: the march, or — for a view this handle has marched, counted and recorded — k_relight.
int march_or_relight(tbrm_resources* r, RayParams& p)
{
    ViewCache& v = r->view;
    const auto plain = [&]() -> int {
        HIP_TRY(launch_raymarch(p, r->stream));
        ++v.stats[0];
        return TBRM_OK;
    };
    // frames that never take part: the feature off, a scene depth, an attached label volume, slab stages and slab-resident handles
    if (tune(TUNE_VIEW_CACHE_MB) <= 0 || p.depth || r->d_labels || p.slab_on || r->resident || p.tile_w <= 0 || p.tile_h <= 0) {
        v.state = ViewCache::kNone;
        v.stats[5] = 0;
        return plain();
    }
    RayParams key;
    std::memcpy(&key, &p, sizeof(key));
    key.out = nullptr;
    const int lanes = ray_lanes_for(p), tables = ray_tables_for(p) ? 1 : 0;
    if (v.state == ViewCache::kNone || v.lanes != lanes || v.tables != tables || v.data_gen != r->data_gen || v.tf_gen != r->tf_gen ||
        std::memcmp(&v.key, &key, sizeof(key)) != 0) { // another view (a moving camera stays here: the march it always ran)
        std::memcpy(&v.key, &key, sizeof(key));
        v.lanes = lanes;
        v.tables = tables;
        v.data_gen = r->data_gen;
        v.tf_gen = r->tf_gen;
        v.state = ViewCache::kPlain;
        v.stats[5] = 0;
        return plain();
    }
    switch (v.state) {
    case ViewCache::kPlain: // the second frame of the view: the march, counting its recorded trips per wave
        ensure_view_arena(r, false);
        if (!carve_view_arena(v, p)) {
            v.state = ViewCache::kTooLarge;
            ++v.stats[4];
            return plain();
        }
        p.rec = v.rec;
        HIP_TRY(launch_raymarch_recording(p, false, r->stream));
        v.state = ViewCache::kCounted;
        ++v.stats[1];
        return TBRM_OK;
    case ViewCache::kCounted: // the third: offsets, the march writing the records (if they fit), and the verdict on its way to the host
        p.rec = v.rec;
        HIP_TRY(launch_view_scan(v.rec, v.n_waves, v.cap_trips, r->stream));
        HIP_TRY(launch_raymarch_recording(p, true, r->stream));
        HIP_TRY(hipMemcpyAsync(v.meta_host, v.rec.meta, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, r->stream));
        HIP_TRY(hipEventRecord(v.ev_meta, r->stream));
        v.state = ViewCache::kFilled;
        ++v.stats[2];
        return TBRM_OK;
    case ViewCache::kFilled: { // asked, never waited for
        const hipError_t q = hipEventQuery(v.ev_meta);
        if (q == hipErrorNotReady) {
            (void) hipGetLastError();
            return plain();
        }
        HIP_TRY(q);
        if (!v.meta_host[1]) {
            v.state = ViewCache::kTooLarge;
            ++v.stats[4];
            return plain();
        }
        v.state = ViewCache::kReady;
        v.stats[5] = (uint64_t) v.meta_host[0] * kRayRecordTripBytes + 2 * (uint64_t) v.n_waves * sizeof(uint32_t);
        [[fallthrough]];
    }
    case ViewCache::kReady:
        p.rec = v.rec;
        HIP_TRY(launch_relight(p, r->stream));
        ++v.stats[3];
        return TBRM_OK;
    default: // kTooLarge: the march, until the key changes
        return plain();
    }
}

} // namespace

namespace tbrm_host {

void ensure_view_arena(tbrm_resources* r, bool eager)
{
    ViewCache& v = r->view;
    const int mb = tune(TUNE_VIEW_CACHE_MB);
    if (v.arena_tried || mb <= 0 || r->resident || r->light_channels != 1) return;
    v.arena_tried = true;
    size_t want = (size_t) mb << 20, free_b = 0, total_b = 0;
    // (the factor-cache arena's rule, reserve_resources: never the last of the device's memory)
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
        const size_t spare = free_b > ((size_t) 8 << 30) ? free_b - ((size_t) 8 << 30) : 0;
        want = std::min(want, eager ? spare / 2 : spare / 8);
    } else (void) hipGetLastError();
    void* a = nullptr;
    void* h = nullptr;
    hipEvent_t ev = nullptr;
    if (want >= ((size_t) 64 << 10) && hipMalloc(&a, want) == hipSuccess && hipHostMalloc(&h, 4 * sizeof(uint32_t), hipHostMallocDefault) == hipSuccess &&
        hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess) {
        v.arena = (char*) a;
        v.arena_bytes = want;
        v.meta_host = (uint32_t*) h;
        v.ev_meta = ev;
        return;
    }
    (void) hipGetLastError(); // (no arena: no relit frames — every frame still marches)
    if (a) (void) hipFree(a);
    if (h) (void) hipHostFree(h);
}

void release_view_cache(tbrm_resources* r)
{
    ViewCache& v = r->view;
    if (v.arena) (void) hipFree(v.arena);
    if (v.meta_host) (void) hipHostFree(v.meta_host);
    if (v.ev_meta) (void) hipEventDestroy(v.ev_meta);
    v = ViewCache{};
}

} // namespace tbrm_host

extern "C" {

int tbrm_view_cache_abi_version(void) { return TBRM_VIEW_CACHE_ABI_VERSION; }

int tbrm_view_cache_stats(const tbrm_resources* r, uint64_t out[6])
{
    if (!r || !out) return fail(TBRM_ERR_INVALID_ARG, "null argument");
    for (int k = 0; k < 6; ++k) out[k] = r->view.stats[k];
    return TBRM_OK;
}

int tbrm_raymarch_lit_device(tbrm_resources* r, const tbrm_camera* cam, const tbrm_tile* tile, const tbrm_raymarch_params* rp,
                             const tbrm_world_params* world, const float* device_scene_depth, float* device_out_rgba)
{
    if (r && r->resident) return fail(TBRM_ERR_UNSUPPORTED, "slab-resident handle: frames are marched with tbrm_raymarch_lit_slab_device");
    if (!r || !cam || !tile || !rp || !world || !device_out_rgba) return fail(TBRM_ERR_INVALID_ARG, "null argument");
    if (!initialized(r)) return fail(TBRM_ERR_NOT_INITIALIZED, "resources have no volume or transfer function");
    if (int e = bind(r)) return e;
    RayParams p;
    if (int e = build_ray_params(r, cam, tile, rp, world, p)) return e;
    p.depth = device_scene_depth;
    p.out = device_out_rgba;
    if (int e = attach_skipping(r, rp, p)) return e;
    if (int e = label_ray_params(r, p)) return e; // (tbrm_labels.h: the label step, when a label volume shows something)
    if (int e = begin_timed(r, 1)) return e;
    if (r->light_channels == 3) { // (tbrm_color_lights.h: ColorSample.rgb x LightVolume.rgb; a colour handle has no label volume)
        p.light = r->light_channel(0);
        p.light_g = r->light_channel(1);
        p.light_b = r->light_channel(2);
        HIP_TRY(launch_raymarch_rgb(p, r->stream));
    } else if (int e = march_or_relight(r, p)) return e;
    ++r->launches[2];
    return end_timed(r, 1);
}

int tbrm_raymarch_lit_slab_device(tbrm_resources* r, const tbrm_camera* cam, const tbrm_tile* tile, const tbrm_raymarch_params* rp,
                                  const tbrm_world_params* world, const float* device_scene_depth, float* device_state_rgba,
                                  const tbrm_slab* slab, int direction)
{
    if (int e = refuse_color(r, "tbrm_raymarch_lit_slab_device")) return e;
    if (!r || !cam || !tile || !rp || !world || !device_state_rgba || !slab) return fail(TBRM_ERR_INVALID_ARG, "null argument");
    if (r->d_labels) return fail(TBRM_ERR_UNSUPPORTED, "the slab stage of the lit march has no label step: release the label volume first");
    if (!initialized(r)) return fail(TBRM_ERR_NOT_INITIALIZED, "resources have no volume or transfer function");
    if (slab->z_begin < 0 || slab->z_end > r->lv_dims[2] || slab->z_begin >= slab->z_end)
        return fail(TBRM_ERR_INVALID_ARG, "slab [%d, %d) of a light volume %d deep", slab->z_begin, slab->z_end, r->lv_dims[2]);
    if (int e = bind(r)) return e;
    RayParams p;
    if (int e = build_ray_params(r, cam, tile, rp, world, p)) return e;
    p.depth = device_scene_depth;
    p.out = device_state_rgba;
    p.slab_on = 1;
    p.slab_z0 = slab->z_begin;
    p.slab_z1 = slab->z_end;
    p.slab_dir = direction > 0 ? 1 : (direction < 0 ? -1 : 0);
    if (r->resident && (slab->z_begin != r->owned.z_begin || slab->z_end != r->owned.z_end))
        return fail(TBRM_ERR_INVALID_ARG, "a slab-resident handle marches its own slab [%d, %d) only", r->owned.z_begin, r->owned.z_end);
    if (int e = attach_skipping(r, rp, p)) return e;
    if (int e = begin_timed(r, 1)) return e;
    HIP_TRY(launch_raymarch(p, r->stream));
    ++r->launches[2];
    return end_timed(r, 1);
}

int tbrm_raymarch_lit(tbrm_resources* r, const tbrm_camera* cam, const tbrm_tile* tile, const tbrm_raymarch_params* rp,
                      const tbrm_world_params* world, float* host_out_rgba)
{
    bool delivered = false;
    if (int e = deliver_frame(r, tile, host_out_rgba, [&](float* d_out) { return tbrm_raymarch_lit_device(r, cam, tile, rp, world, nullptr, d_out); }, &delivered)) return e;
    return delivered ? sweep_failed(r) : TBRM_OK; // (a frame lit by a light volume that a failed sweep left undefined is not handed out as good)
}

int tbrm_raymarch_intensity_device(tbrm_resources* r, const tbrm_camera* cam, const tbrm_tile* tile, const tbrm_raymarch_params* rp,
                                   const tbrm_world_params* world, const float* device_scene_depth, float* device_out_rgba)
{
    if (r && r->resident) return fail(TBRM_ERR_UNSUPPORTED, "slab-resident handle: only the lit march has a slab form");
    if (!r || !cam || !tile || !rp || !world || !device_out_rgba) return fail(TBRM_ERR_INVALID_ARG, "null argument");
    if (!r->has_volume) return fail(TBRM_ERR_NOT_INITIALIZED, "resources have no volume");
    if (int e = bind(r)) return e;
    RayParams p;
    if (int e = build_ray_params(r, cam, tile, rp, world, p)) return e;
    p.depth = device_scene_depth;
    p.out = device_out_rgba;
    if (int e = begin_timed(r, 1)) return e;
    HIP_TRY(launch_raymarch_intensity(p, r->stream));
    ++r->launches[2];
    return end_timed(r, 1);
}

int tbrm_raymarch_intensity(tbrm_resources* r, const tbrm_camera* cam, const tbrm_tile* tile, const tbrm_raymarch_params* rp,
                            const tbrm_world_params* world, float* host_out_rgba)
{
    return deliver_frame(r, tile, host_out_rgba, [&](float* d_out) { return tbrm_raymarch_intensity_device(r, cam, tile, rp, world, nullptr, d_out); });
}

int tbrm_octree_mip_dims(const tbrm_resources* r, int mip, int32_t out_dims[3])
{
    if (!r || !out_dims || mip < 0 || mip > 3) return fail(TBRM_ERR_INVALID_ARG, "bad argument");
    const tbrm_resources::Dims d = r->data_dims();
    for (int c = 0; c < 3; ++c) {
        int p2 = 1;
        while (p2 < d[c]) p2 <<= 1; // FMath::RoundUpToPowerOfTwo (RaymarchVolume.cpp:876-877)
        out_dims[c] = std::max(p2 >> mip, 1);
    }
    return TBRM_OK;
}

int tbrm_generate_octree(tbrm_resources* r)
{
    if (r && r->resident) return fail(TBRM_ERR_UNSUPPORTED, "slab-resident handle: only the lit march has a slab form");
    if (!r) return fail(TBRM_ERR_INVALID_ARG, "null argument");
    if (!r->has_volume) return fail(TBRM_ERR_NOT_INITIALIZED, "resources have no volume");
    if (int e = bind(r)) return e;
    for (int m = 0; m < 4; ++m) {
        int32_t d[3];
        (void) tbrm_octree_mip_dims(r, m, d);
        for (int c = 0; c < 3; ++c) r->oct_dims[m][c] = d[c];
        if (!r->d_octree[m]) HIP_TRY(hipMalloc((void**) &r->d_octree[m], (size_t) d[0] * d[1] * d[2] * sizeof(uint16_t)));
        OctreeParams op{};
        op.data = data_view(r);
        op.lower = m ? r->d_octree[m - 1] : nullptr;
        for (int c = 0; c < 3; ++c) { op.dims[c] = d[c]; op.lower_dims[c] = m ? r->oct_dims[m - 1][c] : 0; }
        op.out = r->d_octree[m];
        HIP_TRY(launch_octree_level(op, m == 0, r->stream));
    }
    r->octree_valid = true;
    return TBRM_OK;
}

int tbrm_download_octree_mip(tbrm_resources* r, int mip, uint16_t* host_out, size_t bytes)
{
    if (!r || !host_out || mip < 0 || mip > 3) return fail(TBRM_ERR_INVALID_ARG, "bad argument");
    if (!r->octree_valid) return fail(TBRM_ERR_NOT_INITIALIZED, "no octree: call tbrm_generate_octree after uploading the volume");
    if (int e = bind(r)) return e;
    const size_t need = (size_t) r->oct_dims[mip][0] * r->oct_dims[mip][1] * r->oct_dims[mip][2] * sizeof(uint16_t);
    if (bytes != need) return fail(TBRM_ERR_INVALID_ARG, "octree level %d is %zu bytes, got %zu", mip, need, bytes);
    HIP_TRY(hipMemcpyAsync(host_out, r->d_octree[mip], need, hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    return TBRM_OK;
}

int tbrm_raymarch_octree_device(tbrm_resources* r, const tbrm_camera* cam, const tbrm_tile* tile, const tbrm_raymarch_params* rp,
                                const tbrm_world_params* world, int octree_mip, const float* device_scene_depth, float* device_out_rgba)
{
    if (!r || !cam || !tile || !rp || !world || !device_out_rgba || octree_mip < 0 || octree_mip > 3) return fail(TBRM_ERR_INVALID_ARG, "bad argument");
    if (!r->has_volume || !r->has_tf) return fail(TBRM_ERR_NOT_INITIALIZED, "resources have no volume or transfer function");
    if (!r->octree_valid) return fail(TBRM_ERR_NOT_INITIALIZED, "no octree: call tbrm_generate_octree after uploading the volume");
    if (int e = bind(r)) return e;
    RayParams p;
    if (int e = build_ray_params(r, cam, tile, rp, world, p)) return e;
    p.depth = device_scene_depth;
    p.out = device_out_rgba;
    p.octree = r->d_octree[octree_mip];
    for (int c = 0; c < 3; ++c) p.oct_dims[c] = r->oct_dims[octree_mip][c];
    p.oct_depth0 = (float) r->oct_dims[0][2];
    if (int e = begin_timed(r, 1)) return e;
    HIP_TRY(launch_raymarch_octree(p, r->stream));
    ++r->launches[2];
    return end_timed(r, 1);
}

int tbrm_raymarch_octree(tbrm_resources* r, const tbrm_camera* cam, const tbrm_tile* tile, const tbrm_raymarch_params* rp,
                         const tbrm_world_params* world, int octree_mip, float* host_out_rgba)
{
    return deliver_frame(r, tile, host_out_rgba, [&](float* d_out) { return tbrm_raymarch_octree_device(r, cam, tile, rp, world, octree_mip, nullptr, d_out); });
}

int tbrm_count_nominal_samples(tbrm_resources* r, const tbrm_camera* cam, const tbrm_tile* tile, const tbrm_raymarch_params* rp,
                               const tbrm_world_params* world, uint64_t* out_samples)
{
    if (!r || !cam || !tile || !rp || !world || !out_samples) return fail(TBRM_ERR_INVALID_ARG, "null argument");
    if (int e = bind(r)) return e;
    RayParams p;
    if (int e = build_ray_params(r, cam, tile, rp, world, p)) return e;
    p.sample_counter = r->d_counter;
    HIP_TRY(hipMemsetAsync(r->d_counter, 0, sizeof(unsigned long long), r->stream));
    HIP_TRY(launch_count_samples(p, r->stream));
    unsigned long long v = 0;
    HIP_TRY(hipMemcpyAsync(&v, r->d_counter, sizeof(v), hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    *out_samples = v;
    return TBRM_OK;
}

} // extern "C"
