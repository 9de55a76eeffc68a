/* tbrm_segment.h — seeded region growing into the label volume (C-ABI, libtbrm.so): connected threshold growing from seed voxels,
 * computed where the voxels, the label volume and its skipping metadata live. It is the step between a click (tbrm_pick,
 * tbrm_hit.h) and a label that the overlay shows (tbrm_labels.h) and the statistics measure (tbrm_volume_stats.h); the only other
 * way to it is to download the volume, flood-fill it on the host and upload a box of labels.
 *
 * Candidates. A voxel is a candidate when
 *   - it lies inside the volume (the zero padding of ragged edge bricks never is) and inside the box [origin, origin + extent); an
 *     all-zero extent is the whole volume, as in tbrm_histogram_desc;
 *   - its stored value v has lo <= v <= hi, in the STORED units of tbrm_volume_stats.h: integral codes with
 *     0 <= lo <= hi <= 255 | 65535 for UNORM8 / UNORM16; for R32_FLOAT lo <= hi, both finite after narrowing to float32 (done on the
 *     host). A NaN voxel is never a candidate;
 *   - its current label L has its bit set in writable: (writable[L >> 5] >> (L & 31)) & 1, the label-mask convention of
 *     tbrm_histogram_desc. Without a label volume every voxel has label 0.
 * Region. The candidates connected to a seed through candidates; connectivity 6 (faces) or 26 (faces, edges, corners). Paths never
 * leave the box and never wrap across a volume face, whatever data_address_mode says.
 * Seeds. n_seeds triples (x, y, z), 0 <= n_seeds <= TBRM_GROW_MAX_SEEDS. A seed inside the volume that is not a candidate
 * contributes nothing. n_seeds == 0 is plain thresholding: every candidate joins, connectivity is not consulted (it must still be
 * 6 or 26).
 * relative_to_seed. lo and hi are offsets from the first seed's stored value v0 (read whether or not that seed is a candidate): the
 * range used is [v0 + lo, v0 + hi] — the "magic wand" tolerance. UNORM data: lo <= hi integral offsets of magnitude <= 255 | 65535, the
 * range clamped to the format's; a range that misses the format's range altogether is empty (the region is empty, lo_used = hi_used =
 * the nearer end of the format's range). R32_FLOAT: the sums are formed in double and narrowed to float32; v0 NaN: the region is
 * empty. The result reports the range that was used.
 * new_label. 0 .. 255: every region voxel's label byte becomes new_label. -1: measure only, nothing is written.
 *
 * State (the contract tbrm_volume_region.h set for edits). After a writing call everything behaves bit for bit as if the same bytes
 * had been written with tbrm_update_label_region: the per-brick label sets of the bricks the region's bounding box touches are
 * recomputed, the live bits refreshed, the merged skipping metadata goes stale. Nothing on the data side moves: generations,
 * emptiness bits, distance field, block lists, factor cache, light volume. A measure-only call changes nothing at all: the frame after
 * it is the frame before it. Ordering is that of the statistics calls: enqueued behind everything issued before on the handle's
 * stream, complete on return; the call's waits are its own (tbrm_path_counters [12] / [13] do not count them).
 * Scratch: two bits per voxel in brick order (128 bytes per brick, 32 MiB at 512^3) and a few words per brick, taken by the handle's
 * first tbrm_grow_region and freed with the handle; later calls allocate nothing. tbrm_resources_reserve does not take it.
 * Handles. Mono handles with a label volume accept every mode; a writing call without a label volume is TBRM_ERR_NOT_INITIALIZED
 * (tbrm_attach_empty_label_volume). Colour handles have no label volume: they, and mono handles without one, accept measure-only
 * calls. Slab-resident handles: TBRM_ERR_UNSUPPORTED. No volume uploaded: TBRM_ERR_NOT_INITIALIZED. TBRM_ERR_INVALID_ARG: a null
 * argument, a connectivity other than 6 / 26, a box that leaves the volume, a bad lo / hi, new_label outside -1 .. 255, n_seeds out of
 * range, a seed outside the volume, relative_to_seed without a seed. */
#ifndef TBRM_SEGMENT_H
#define TBRM_SEGMENT_H

#include "tbrm.h"
#include "tbrm_hit.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TBRM_SEGMENT_ABI_VERSION 1
#define TBRM_GROW_MAX_SEEDS 4096

typedef struct tbrm_grow_desc {
    int32_t origin[3], extent[3];   /* the box; extent = {0,0,0}: the whole volume (origin is then ignored) */
    int32_t connectivity;           /* 6 or 26 */
    int32_t new_label;              /* 0 .. 255, or -1: measure only */
    int32_t relative_to_seed;       /* 0: lo / hi are stored values; 1: offsets from the first seed's stored value */
    int32_t reserved;               /* 0 */
    double  lo, hi;
    uint32_t writable[8];           /* labels that may be grown over (all ones: every label) */
} tbrm_grow_desc;

typedef struct tbrm_grow_result {
    uint64_t voxels;                /* the region's size, voxels that already held new_label included */
    uint64_t relabelled;            /* voxels whose label byte changed; 0 in measure-only mode */
    int32_t  bbox_min[3], bbox_max[3]; /* inclusive; an empty region: bbox_min = the volume's dims, bbox_max = -1 */
    int32_t  passes;                /* propagation passes that moved the region (0 when n_seeds == 0) */
    int32_t  seeds_taken;           /* seeds that were candidates */
    double   lo_used, hi_used;      /* the range that was applied, in stored units */
} tbrm_grow_result;

TBRM_API int tbrm_segment_abi_version(void);
/* seeds_xyz: 3 * n_seeds int32 (may be NULL when n_seeds == 0). */
TBRM_API int tbrm_grow_region(tbrm_resources* res, const tbrm_grow_desc* desc, const int32_t* seeds_xyz, int32_t n_seeds,
                              tbrm_grow_result* out);
/* Attaches an all-zero label volume without a host transfer: the allocations and the default colours of the first
 * tbrm_upload_label_volume. A no-op when a label volume is attached. Colour handles and slab-resident handles refuse as
 * tbrm_upload_label_volume does. */
TBRM_API int tbrm_attach_empty_label_volume(tbrm_resources* res);
/* Pure host code: the voxel the label step (tbrm_labels.h) reads at a hit, rint((N - 1) * saturate(uvw)) per axis in float32, round
 * half to even. A record without a hit (sample < 0), a dim < 1: TBRM_ERR_INVALID_ARG. */
TBRM_API int tbrm_host_hit_voxel(const int32_t dims[3], const tbrm_hit* hit, int32_t out_xyz[3]);
/* Cumulative per handle: [0] tbrm_grow_region calls, [1] propagation passes (the sum of tbrm_grow_result::passes), [2] brick visits
 * (one per brick per pass in which it was processed), [3] bricks holding region voxels whose label bytes were written. */
TBRM_API int tbrm_segment_counters(const tbrm_resources* res, uint64_t out[4]);

#ifdef __cplusplus
}
#endif
#endif /* TBRM_SEGMENT_H */
