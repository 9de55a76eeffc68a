/* tbrm_morphology.h — binary morphology of the label volume (C-ABI, libtbrm.so): dilate, erode, open and close a set of labels by a
 * radius, computed where the label volume and its skipping metadata live. It is the step after tbrm_grow_region (tbrm_segment.h): a
 * grown region leaks through one-voxel bridges (open), has pinholes (close) and wants a margin (dilate, erode). The only other way
 * to it is to download the label volume, filter it on the host and upload a box of labels.
 *
 * The set. S is every voxel of the WHOLE volume (not of the box) whose label L has its bit in source:
 * (source[L >> 5] >> (L & 31)) & 1, the mask convention of tbrm_grow_desc::writable. The zero padding of ragged edge bricks is
 * never in it and never a neighbour.
 * The operators. A unit step is the 6-neighbour cross (connectivity 6) or the 3 x 3 x 3 cube (26); radius r, 1 .. TBRM_MORPH_MAX_RADIUS,
 * is r unit steps (so the structuring element is the octahedron or the cube of that radius, not a sphere).
 *   dilate(S, r): r steps; everything outside the volume counts as unset.
 *   erode(S, r) = ~dilate(~S, r) with the complement taken inside the volume: outside the volume counts as SET, a label that touches
 *                 a volume face is not eaten from outside.
 *   open = dilate(erode(S, r), r), close = erode(dilate(S, r), r).
 * Nothing wraps across a volume face, whatever data_address_mode says. R is the operator's result over the whole volume.
 * The box. Voxels inside [origin, origin + extent) may change; an all-zero extent is the whole volume (origin is then ignored).
 * Voxels outside it are read as they are — S outside the box acts on the result inside — and never written. Inside the box
 *   added   = the voxels of R \ S whose current label has its bit in writable: they get new_label;
 *   removed = the voxels of S \ R: they get erase_label (writable is not consulted: they are the source's own voxels).
 * new_label -1 measures only: added and removed are counted, nothing is written, relabelled is 0.
 *
 * State and ordering: the contract of tbrm_grow_region, word for word. After a writing call everything behaves bit for bit as if the
 * same bytes had been written with tbrm_update_label_region: the per-brick label sets of the bricks the bounding box touches are
 * recomputed, the live bits refreshed, the merged skipping metadata goes stale. Nothing on the data side moves. A measure-only call
 * changes nothing at all. The call is enqueued behind everything issued before on the handle's stream and complete on return; its
 * waits are its own (tbrm_path_counters [12] / [13] do not count them). It works in the scratch of tbrm_grow_region (two bit boards
 * per brick and a few words), taken by whichever of the two calls comes first: a handle that has grown a region allocates nothing.
 * Cost: a launch of the step kernel iterates up to 8 unit steps, so an operator costs ceil(r / 8) step launches, twice that for
 * open and close (tunable morph_steps, 1 .. 8, default 8; the result is the same for every value).
 * Errors. No volume or no label volume (colour handles have none): TBRM_ERR_NOT_INITIALIZED. Slab-resident handles:
 * TBRM_ERR_UNSUPPORTED. TBRM_ERR_INVALID_ARG: a null argument, an op, radius or connectivity out of range, new_label outside
 * -1 .. 255, erase_label outside 0 .. 255, a box that leaves the volume, a non-zero reserved. */
#ifndef TBRM_MORPHOLOGY_H
#define TBRM_MORPHOLOGY_H

#include "tbrm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TBRM_MORPH_ABI_VERSION 1
#define TBRM_MORPH_MAX_RADIUS 64

enum { TBRM_MORPH_DILATE = 0, TBRM_MORPH_ERODE = 1, TBRM_MORPH_OPEN = 2, TBRM_MORPH_CLOSE = 3 };

typedef struct tbrm_morph_desc {
    int32_t origin[3], extent[3];   /* the box that may change; extent = {0,0,0}: the whole volume */
    int32_t op, radius;             /* TBRM_MORPH_*; radius 1 .. TBRM_MORPH_MAX_RADIUS: that many unit steps */
    int32_t connectivity;           /* 6: a unit step is the 6-neighbour cross; 26: the 3 x 3 x 3 cube */
    int32_t new_label;              /* 0 .. 255 for voxels that join; -1: measure only */
    int32_t erase_label;            /* 0 .. 255 for voxels that leave */
    int32_t reserved;               /* 0 */
    uint32_t source[8];             /* the set S: voxels whose label has its bit here */
    uint32_t writable[8];           /* labels a joining voxel may overwrite (all ones: every label) */
} tbrm_morph_desc;

typedef struct tbrm_morph_result {
    uint64_t source_voxels, result_voxels; /* |S in the box|, |R in the box| */
    uint64_t added, removed, relabelled;   /* as above; relabelled: label bytes that changed (0 when measuring) */
    int32_t  bbox_min[3], bbox_max[3];     /* of added and removed together, inclusive; none: bbox_min = the volume's dims, bbox_max = -1 */
    int32_t  launches, reserved;           /* launches of the step kernel */
} tbrm_morph_result;

TBRM_API int tbrm_morph_abi_version(void);
TBRM_API int tbrm_morph_labels(tbrm_resources* res, const tbrm_morph_desc* desc, tbrm_morph_result* out);
/* Cumulative per handle: [0] tbrm_morph_labels calls, [1] launches of the step kernel, [2] brick windows computed (a brick in a
 * launch whose output the board classes did not give), [3] bricks whose label bytes were written. */
TBRM_API int tbrm_morph_counters(const tbrm_resources* res, uint64_t out[4]);

#ifdef __cplusplus
}
#endif
#endif /* TBRM_MORPHOLOGY_H */
