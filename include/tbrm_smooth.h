/* tbrm_smooth.h — smoothing of labels (C-ABI, libtbrm.so): a majority (rank) filter over a box, computed where the label volume
 * lives. Open and close (tbrm_morphology.h, tbrm_margin.h) move a label's surface one way only: open cuts, close fills. A median
 * moves it both ways at once: a voxel takes the value of the majority of a small box round it, so spurs go, pits fill and the volume
 * stays roughly what it was — the "Smoothing -> Median" of the usual segmentation editors. The only other way to it is to download
 * the label volume, run a median filter on the host and upload a box.
 *
 * Integers only; every result is exact. S is the source set exactly as in tbrm_morphology.h: the voxels of the whole volume whose
 * label has its bit in source; the zero padding of ragged edge bricks is never in it. A call carries radius[3] = (r_x, r_y, r_z),
 * rank_num, rank_den and iterations. The window of a voxel v is the box [v - r, v + r] per axis, CLIPPED TO THE VOLUME:
 *   n(v) = the number of voxels of that clipped window,
 *   c(v) = the number of them in S — counted over the WHOLE volume, not the call's box.
 * One pass is
 *   rank(S) = { v in the volume : c(v) * rank_den > n(v) * rank_num }.
 * The median is rank_num / rank_den = 1 / 2: a strict majority of the voxels that exist; a tie leaves the voxel unset. What lies
 * outside the volume has no vote (the face rule of tbrm_morphology.h restated): a label on a volume face is neither eaten nor grown
 * from outside, and a full volume stays full. Nothing wraps. iterations = k applies the pass k times, S_{i+1} = rank(S_i), every
 * intermediate taken over the whole volume, the way open and close chain their transforms.
 * rank_num = 0 is the dilation by the box; rank_den above the window's size with rank_num = rank_den - 1 is the erosion by the box
 * (27 / 28 at radius 1): both fall out of the one comparison.
 * The box, writable, new_label (-1 measures only), erase_label, added, removed, relabelled, the bounding box, the state contract, the
 * ordering contract and the errors are those of tbrm_morph_labels, word for word.
 *
 * TBRM_ERR_INVALID_ARG, besides tbrm_morph_labels' own, with a message that names the field: a radius outside
 * 0 .. TBRM_SMOOTH_MAX_RADIUS; every radius 0; iterations outside 1 .. TBRM_SMOOTH_MAX_ITERATIONS, or iterations * r_a above
 * TBRM_SMOOTH_MAX_REACH for an axis (the reach limit of tbrm_morph_labels and tbrm_margin_labels); rank_den outside
 * 1 .. TBRM_SMOOTH_MAX_RANK_DEN; rank_num outside 0 .. rank_den - 1; a non-zero reserved. Under these bounds
 * c * rank_den <= 33^3 * 256 < 2^31: every product the kernel forms fits 32 bits.
 *
 * Physical units are host arithmetic: tbrm_host_smooth_radii turns a voxel spacing and a radius (same unit) into radii,
 * r_a = floor(radius / spacing_a + 0.5). It refuses (TBRM_ERR_INVALID_ARG) non-finite or non-positive input, radii that are all 0 and
 * a radius above TBRM_SMOOTH_MAX_RADIUS.
 *
 * Cost and scratch. A pass is one launch, a workgroup per brick of the range: the bricks that the box grown by the reach
 * iterations * r_a, clamped to the volume, touches. It works in the scratch of tbrm_grow_region and takes none of its own: a call
 * allocates nothing once that scratch is there. Bricks whose result the board classes give are not computed (tunable smooth_skip,
 * default 1; 0 computes every brick of the range: the test hook and the A/B switch; the result is the same): a brick that is full
 * with every brick of the volume within ceil(r_a / 8) bricks per axis full stays full, one that is empty among empty bricks stays
 * empty, whatever the rank. */
#ifndef TBRM_SMOOTH_H
#define TBRM_SMOOTH_H

#include "tbrm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TBRM_SMOOTH_ABI_VERSION 1
#define TBRM_SMOOTH_MAX_RADIUS 16
#define TBRM_SMOOTH_MAX_ITERATIONS 64
#define TBRM_SMOOTH_MAX_REACH 64
#define TBRM_SMOOTH_MAX_RANK_DEN 256

typedef struct tbrm_smooth_desc {
    int32_t origin[3], extent[3];   /* the box that may change; extent = {0,0,0}: the whole volume */
    int32_t radius[3];              /* r_x, r_y, r_z: each 0 .. TBRM_SMOOTH_MAX_RADIUS, not all 0 */
    int32_t rank_num, rank_den;     /* set where c * rank_den > n * rank_num; the median is 1 / 2 */
    int32_t iterations;             /* passes, 1 .. TBRM_SMOOTH_MAX_ITERATIONS */
    int32_t new_label;              /* 0 .. 255 for voxels that join; -1: measure only */
    int32_t erase_label;            /* 0 .. 255 for voxels that leave */
    int32_t reserved;               /* 0 */
    uint32_t source[8];             /* the set S: voxels whose label has its bit here */
    uint32_t writable[8];           /* labels a joining voxel may overwrite (all ones: every label) */
} tbrm_smooth_desc;

typedef struct tbrm_smooth_result {
    uint64_t source_voxels, result_voxels; /* |S in the box|, |R in the box| */
    uint64_t added, removed, relabelled;   /* as in tbrm_morph_result */
    int32_t  bbox_min[3], bbox_max[3];     /* of added and removed together, inclusive; none: bbox_min = the volume's dims, bbox_max = -1 */
    int32_t  reach[3];                     /* iterations * r_a */
    int32_t  launches;                     /* launches of the counting kernel: one per pass */
} tbrm_smooth_result;

TBRM_API int tbrm_smooth_abi_version(void);
TBRM_API int tbrm_smooth_labels(tbrm_resources* res, const tbrm_smooth_desc* desc, tbrm_smooth_result* out);
/* no handle, no device: spacing and radius -> radii (above) */
TBRM_API int tbrm_host_smooth_radii(const double spacing[3], double radius, int32_t radii[3]);
/* Cumulative per handle: [0] tbrm_smooth_labels calls, [1] launches of the counting kernel, [2] bricks computed (a brick in a pass
 * whose result its neighbourhood's classes did not give), [3] bricks whose label bytes were written. */
TBRM_API int tbrm_smooth_counters(const tbrm_resources* res, uint64_t out[4]);

#ifdef __cplusplus
}
#endif
#endif /* TBRM_SMOOTH_H */
