// tbrm_api_hit.cpp — surface-hit maps and ray picking (include/tbrm_hit.h): the argument checks, the view of the handle the frame calls
// build (build_ray_params, attach_skipping, label_ray_params: tbrm_api_render.cpp, tbrm_api_labels.cpp), the launch of k_raymarch_hit
// (tbrm_kernels.hip compiled as the hit unit) and the counters. The world position and depth of a record are host arithmetic
// (tbrm_host_math.cpp).
//
// The calls read the data volume, the label volume, the transfer function and the skipping metadata, and write the caller's buffers
// (the host forms: the handle's hit staging) only: no generation moves, the view cache is neither consulted nor told (a hit map is
// no frame of the view), launches[] and the frame's timing events are left alone.
#include "tbrm_resources.h"
#include "../../include/tbrm_hit.h"

#include <cmath>
#include <cstring>

using namespace tbrm;
using namespace tbrm_host;

static_assert(sizeof(tbrm_hit) == 32 && sizeof(tbrm_hit) == 2 * sizeof(uint4), "k_raymarch_hit writes a record as two 16-byte words");

namespace {

// what every device-touching hit call checks; the pointers and the threshold before the handle is looked at
int hit_arguments(const tbrm_resources* r, const void* cam, const void* rp, const void* world, const void* out, float threshold)
{
    if (!r || !cam || !rp || !world || !out) return fail(TBRM_ERR_INVALID_ARG, "null argument");
    if (!(threshold >= 0.0f && threshold <= 0.95f)) return fail(TBRM_ERR_INVALID_ARG, "hit threshold %g: must be in [0, 0.95]", (double) threshold);
    if (r->resident) return fail(TBRM_ERR_UNSUPPORTED, "slab-resident handle: it holds only some layers of the volume");
    if (!initialized(r)) return fail(TBRM_ERR_NOT_INITIALIZED, "resources have no volume or transfer function");
    return TBRM_OK;
}

// the hit kernel over a tile, on the handle's stream
int enqueue_hits(tbrm_resources* r, const tbrm_camera* cam, const tbrm_tile* tile, const tbrm_raymarch_params* rp, const tbrm_world_params* world,
                 float threshold, const float* d_scene_depth, tbrm_hit* d_hits, float* d_depth)
{
    RayParams p;
    if (int e = build_ray_params(r, cam, tile, rp, world, p)) return e;
    p.depth = d_scene_depth;
    if (int e = attach_skipping(r, rp, p)) return e;
    if (int e = label_ray_params(r, p)) return e;
    // (a label volume none of whose labels shows: the frame marches without the label step; the record still names the label, and the
    // steps its kernel form takes add exactly nothing)
    if (r->d_labels && !p.labels) { p.labels = r->d_labels; p.lab_colors = r->d_lab_colors; }
    HitParams h{};
    h.hits = reinterpret_cast<uint4*>(d_hits);
    h.depth = d_depth;
    h.threshold = threshold;
    host_hit_depth_form(world->volume_transform, *cam, h.dg, &h.d0);
    HIP_TRY(launch_raymarch_hit(p, h, r->stream));
    if (p.tile_w > 0 && p.tile_h > 0) ++r->hit_counters[2];
    return TBRM_OK;
}

// The host form of a tile: the kernel into the handle's staging (grown to the largest tile seen), one copy back, one wait.
int hits_to_host(tbrm_resources* r, const tbrm_camera* cam, const tbrm_tile* tile, const tbrm_raymarch_params* rp, const tbrm_world_params* world,
                 float threshold, tbrm_hit* host_hits, float* host_depth)
{
    if (tile->w < 0 || tile->h < 0) return fail(TBRM_ERR_INVALID_ARG, "bad tile size");
    const size_t n = (size_t) tile->w * tile->h, rec_bytes = n * sizeof(tbrm_hit), bytes = rec_bytes + n * sizeof(float);
    if (n == 0) return TBRM_OK;
    if (int e = bind(r)) return e;
    if (bytes > r->hit_bytes) {
        HIP_TRY(hipStreamSynchronize(r->stream));
        (void) hipFree(r->d_hit);
        r->d_hit = nullptr;
        r->hit_bytes = 0;
        HIP_TRY(hipMalloc((void**) &r->d_hit, bytes));
        r->hit_bytes = bytes;
    }
    tbrm_hit* const d_hits = reinterpret_cast<tbrm_hit*>(r->d_hit);
    float* const d_depth = host_depth ? reinterpret_cast<float*>(r->d_hit + rec_bytes) : nullptr;
    if (int e = enqueue_hits(r, cam, tile, rp, world, threshold, nullptr, d_hits, d_depth)) return e;
    HIP_TRY(hipMemcpyAsync(host_hits, d_hits, rec_bytes, hipMemcpyDeviceToHost, r->stream));
    if (host_depth) HIP_TRY(hipMemcpyAsync(host_depth, d_depth, n * sizeof(float), hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    return TBRM_OK;
}

} // namespace

extern "C" {

int tbrm_hit_abi_version(void) { return TBRM_HIT_ABI_VERSION; }

int tbrm_raymarch_hits_device(tbrm_resources* r, const tbrm_camera* cam, const tbrm_tile* tile, const tbrm_raymarch_params* rp,
                              const tbrm_world_params* world, float threshold, const float* device_scene_depth, tbrm_hit* device_out_hits,
                              float* device_out_depth)
{
    if (!tile) return fail(TBRM_ERR_INVALID_ARG, "null argument");
    if (int e = hit_arguments(r, cam, rp, world, device_out_hits, threshold)) return e;
    if (int e = bind(r)) return e;
    if (int e = enqueue_hits(r, cam, tile, rp, world, threshold, device_scene_depth, device_out_hits, device_out_depth)) return e;
    ++r->hit_counters[0];
    return TBRM_OK;
}

int tbrm_raymarch_hits(tbrm_resources* r, const tbrm_camera* cam, const tbrm_tile* tile, const tbrm_raymarch_params* rp,
                       const tbrm_world_params* world, float threshold, tbrm_hit* host_out_hits, float* host_out_depth)
{
    if (!tile) return fail(TBRM_ERR_INVALID_ARG, "null argument");
    if (int e = hit_arguments(r, cam, rp, world, host_out_hits, threshold)) return e;
    if (int e = hits_to_host(r, cam, tile, rp, world, threshold, host_out_hits, host_out_depth)) return e;
    ++r->hit_counters[0];
    return TBRM_OK;
}

int tbrm_pick(tbrm_resources* r, const tbrm_camera* cam, int32_t px, int32_t py, const tbrm_raymarch_params* rp, const tbrm_world_params* world,
              float threshold, tbrm_hit* out_hit, double out_world_position[3], double* out_depth)
{
    if (!cam) return fail(TBRM_ERR_INVALID_ARG, "null argument");
    if (px < 0 || py < 0 || px >= cam->width || py >= cam->height)
        return fail(TBRM_ERR_INVALID_ARG, "pixel (%d, %d) outside the %d x %d framebuffer", (int) px, (int) py, (int) cam->width, (int) cam->height);
    if (int e = hit_arguments(r, cam, rp, world, out_hit, threshold)) return e;
    const tbrm_tile one{px, py, 1, 1, 1, 0};
    if (int e = hits_to_host(r, cam, &one, rp, world, threshold, out_hit, nullptr)) return e;
    host_hits_to_world(*world, *cam, out_hit, 1, out_world_position, out_depth);
    ++r->hit_counters[1];
    return TBRM_OK;
}

int tbrm_host_hits_to_world(const tbrm_world_params* world, const tbrm_camera* cam, const tbrm_hit* hits, size_t n, double* out_xyz,
                            double* out_depth)
{
    if (!world || !cam || (!hits && n > 0)) return fail(TBRM_ERR_INVALID_ARG, "null argument");
    host_hits_to_world(*world, *cam, hits, n, out_xyz, out_depth);
    return TBRM_OK;
}

int tbrm_hit_counters(const tbrm_resources* r, uint64_t out[3])
{
    if (!r || !out) return fail(TBRM_ERR_INVALID_ARG, "null argument");
    for (int k = 0; k < 3; ++k) out[k] = r->hit_counters[k];
    return TBRM_OK;
}

} // extern "C"
