/* tbrm_volume_region.h — region updates of the data volume (C-ABI, libtbrm.so): a host that sculpts, streams a volume in tile by
 * tile or refreshes part of a simulation field writes a sub-box instead of uploading the whole volume again.
 *
 * A box is dense, x fastest, in the handle's data_format, and covers the voxels [origin, origin + extent) of a volume that
 * tbrm_upload_volume[_device] has already put in place. After a successful update every entry point behaves, bit for bit, as on a
 * fresh handle that uploaded the whole edited volume:
 *   - no occlusion computed from the old data is served again (the factor cache is treated as by tbrm_upload_volume);
 *   - the octree is invalid until the next tbrm_generate_octree, as after an upload;
 *   - the empty-space-skipping metadata follows incrementally: the per-brick value ranges are recomputed for the bricks a box can
 *     reach only (DESIGN.md §11 has the rule), the emptiness bits and the distance field, which are small, as a whole. More than
 *     64 boxes pending before the metadata is next needed, or boxes that reach as many bricks as the volume has, rebuild the
 *     ranges as a whole instead.
 * The light volume is not touched: the host re-propagates its lights (tbrm_clear_light_volume and the Add operators), which is
 * what the reference does on every change of the volume.
 *
 * Colour handles and handles with a label volume accept region updates (the data volume exists once on them); slab-resident
 * handles refuse them (TBRM_ERR_UNSUPPORTED). The calls enqueue on the handle's stream behind everything issued before and return
 * when the transfer is done: the caller's buffer is free on return. */
#ifndef TBRM_VOLUME_REGION_H
#define TBRM_VOLUME_REGION_H

#include "tbrm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TBRM_VOLUME_REGION_ABI_VERSION 1

TBRM_API int tbrm_volume_region_abi_version(void);
/* Writes the box; n_bytes = the box's voxels x the format's bytes per voxel. TBRM_ERR_INVALID_ARG: a null argument, an extent
 * <= 0, a box that leaves the volume, another n_bytes. TBRM_ERR_NOT_INITIALIZED: no volume has been uploaded yet. */
TBRM_API int tbrm_update_volume_region(tbrm_resources* res, const int32_t origin[3], const int32_t extent[3],
                                       const void* host_voxels, size_t n_bytes);
/* The same from device memory (aligned to the voxel size); nothing is allocated. */
TBRM_API int tbrm_update_volume_region_device(tbrm_resources* res, const int32_t origin[3], const int32_t extent[3],
                                              const void* device_voxels, size_t n_bytes);
/* Reads the box back, in the same form. */
TBRM_API int tbrm_download_volume_region(tbrm_resources* res, const int32_t origin[3], const int32_t extent[3],
                                         void* host_out, size_t n_bytes);
/* Cumulative per handle: [0] region updates accepted, [1] voxels they wrote, [2] bricks whose value range was recomputed
 * incrementally — per pending box the bricks it reaches, so a brick that two boxes reach counts twice —, [3] rebuilds of every
 * brick's range, whatever caused them (an upload, the first frame, the fall-back above). */
TBRM_API int tbrm_volume_region_counters(const tbrm_resources* res, uint64_t out[4]);
/* A test hook: brings the skipping metadata up to date (needs a volume and a transfer function), reads it back and hashes it on
 * the host (64-bit FNV-1a over the raw bytes): [0] bricks, [1] empty bricks, [2] hash of the per-brick value ranges, [3] hash of
 * the final distance field. Equal metadata gives equal words. */
TBRM_API int tbrm_volume_skipping_digest(tbrm_resources* res, uint64_t out[4]);

#ifdef __cplusplus
}
#endif
#endif /* TBRM_VOLUME_REGION_H */
