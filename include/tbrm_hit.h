/* tbrm_hit.h — surface-hit maps and ray picking (C-ABI, libtbrm.so): where each ray of the lit raymarch first gets opaque, as a record
 * per pixel (position in the volume, sample index, accumulated opacity, data value, label) and as a depth buffer in the convention of
 * the raymarch's own scene_depth input. "What is under this pixel?" — a label to hand to tbrm_label_statistics, a data value under the
 * cursor, a spot for a clip plane or a region edit — and "how deep is the visible surface here?" — scene geometry composited against
 * the volume — are answered where the volume lives; the only other way to them is to download the volume and march it on the host.
 *
 * Semantics (tests hold them against a float64 restatement, and bit for bit against the lit frame's alpha channel):
 *   For every pixel of the tile the ray is marched exactly as tbrm_raymarch_lit marches it (PerformWindowedLitRaymarch): cube setup,
 *   the optional scene depth, jitter, step count, the fractional last step, the clip test, window, transfer function and opacity
 *   correction; positions are reached by performing every addition; on handles with a label volume the unlit label step follows each
 *   data step. Only the accumulated opacity LightEnergy.a is tracked: it never sees the light volume.
 *   The HIT of a ray is the first sample after whose steps (the data step and, on label handles, the label step behind it) the
 *   accumulated opacity is > threshold, 0 <= threshold <= 0.95. The test is the 0.95 early exit's comparison in the early exit's
 *   place, and it applies to the fractional step as well. The march of a ray ends at its hit.
 *   So at threshold 0.95 a ray has a hit in its full steps exactly where the lit frame's alpha is 1, and otherwise the record's alpha
 *   IS the lit frame's alpha; at threshold 0 a ray has a hit exactly where the lit frame's alpha is not 0.
 *
 * State. A hit call reads the volumes, the transfer function, the window and the skipping metadata (brought up to date as a frame
 * with enable_skipping would) and changes nothing of the handle: not the light volume, the generations, the factor cache or the view
 * cache's state — a lit frame after it is bit-identical to the frame before it, and a view that was being relit still is.
 * tbrm_launch_counters, tbrm_path_counters and tbrm_last_gpu_time_ms do not see hit calls; tbrm_hit_counters counts them. The host
 * forms wait for the stream once, as a download does (not counted by tbrm_path_counters [12] / [13]); their staging buffer is the
 * handle's, grown to the largest tile seen. The device form allocates nothing and waits for nothing.
 * Mono handles, colour handles and handles with a label volume accept the calls. Slab-resident handles: TBRM_ERR_UNSUPPORTED. No
 * volume or no transfer function: TBRM_ERR_NOT_INITIALIZED. A null argument, a threshold outside [0, 0.95] or NaN, a pixel outside
 * the framebuffer: TBRM_ERR_INVALID_ARG. */
#ifndef TBRM_HIT_H
#define TBRM_HIT_H

#include "tbrm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TBRM_HIT_ABI_VERSION 1

typedef struct tbrm_hit {
    float   uvw[3];      /* the hit sample's position in the volume's unit cube exactly as the march holds it (not saturated); no hit: 0,0,0 */
    int32_t sample;      /* index of the hit sample along the ray, 0 .. full_steps (== full_steps: the fractional step); -1: no hit */
    float   alpha;       /* accumulated opacity right after the hit sample (> threshold); no hit: the ray's final accumulated opacity */
    float   value;       /* the filtered data value at the hit sample, in the units the window sees (UNORM: code/(2^n-1)); no hit: 0 */
    int32_t label;       /* label handles: the nearest-voxel label byte at the hit sample (SampleLabelVolume's voxel), else -1; no hit: -1 */
    int32_t full_steps;  /* the ray's floor(Steps * thickness); 0 for a ray that misses the cube */
} tbrm_hit;

TBRM_API int tbrm_hit_abi_version(void);
/* The hit map of a tile, enqueued on the handle's stream like tbrm_raymarch_lit_device: tile.w * tile.h records, row-major, in the row
 * order of the frame calls (16-byte aligned device memory). device_scene_depth: as tbrm_raymarch_lit_device's, or NULL.
 * device_out_depth: NULL, or one float per pixel in the convention of scene_depth — the distance of the hit along camera.forward in
 * world units, (P - camera.position) . forward with P = the volume transform applied to uvw - 0.5; +inf where the ray has no hit. */
TBRM_API int tbrm_raymarch_hits_device(tbrm_resources* res, const tbrm_camera* camera, const tbrm_tile* tile,
                                       const tbrm_raymarch_params* params, const tbrm_world_params* world, float threshold,
                                       const float* device_scene_depth, tbrm_hit* device_out_hits, float* device_out_depth);
/* The same into host memory, complete on return (host_out_depth may be NULL; no scene depth). */
TBRM_API int tbrm_raymarch_hits(tbrm_resources* res, const tbrm_camera* camera, const tbrm_tile* tile,
                                const tbrm_raymarch_params* params, const tbrm_world_params* world, float threshold,
                                tbrm_hit* host_out_hits, float* host_out_depth);
/* One framebuffer pixel (px, py), marched as a 1 x 1 tile by the same kernel: the record, and from it in double precision
 * (tbrm_host_hits_to_world) the world position and depth, each of which may be NULL. No hit: position 0,0,0 and depth +inf. */
TBRM_API int tbrm_pick(tbrm_resources* res, const tbrm_camera* camera, int32_t px, int32_t py, const tbrm_raymarch_params* params,
                       const tbrm_world_params* world, float threshold, tbrm_hit* out_hit, double out_world_position[3],
                       double* out_depth);
/* Pure host code, double precision, no device: for n records the world position P = volume transform applied to uvw - 0.5 (out_xyz,
 * 3 n doubles, or NULL) and the depth (P - camera.position) . camera.forward (out_depth, n doubles, or NULL). Records without a hit
 * (sample < 0) give 0,0,0 and +inf. */
TBRM_API int tbrm_host_hits_to_world(const tbrm_world_params* world, const tbrm_camera* camera, const tbrm_hit* hits, size_t n,
                                     double* out_xyz, double* out_depth);
/* Cumulative per handle: [0] hit-map calls (device and host form), [1] tbrm_pick calls, [2] launches of the hit kernel. */
TBRM_API int tbrm_hit_counters(const tbrm_resources* res, uint64_t out[3]);

#ifdef __cplusplus
}
#endif
#endif /* TBRM_HIT_H */
