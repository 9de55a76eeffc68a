/* tbrm_islands.h — the islands of a label (C-ABI, libtbrm.so): connected-component labelling of a set of labels, computed where the
 * label volume and its skipping metadata live, and one rule over the components that is keep the largest n, remove the small ones,
 * split them into labels of their own and fill the holes. It is the step after tbrm_grow_region (tbrm_segment.h) and
 * tbrm_morph_labels (tbrm_morphology.h): after a threshold or an opening a label is one large body plus hundreds of specks. The only
 * other way to it is to download the label volume, label the components on the host and upload a box of labels.
 *
 * The set. S is every voxel inside the box [origin, origin + extent) whose label L has its bit in source:
 * (source[L >> 5] >> (L & 31)) & 1, the mask convention of tbrm_morph_desc::source. An all-zero extent is the whole volume (origin is
 * then ignored). The zero padding of ragged edge bricks is never in it and never a neighbour. Voxels outside the box are not in the
 * set: a connection that leaves the box is cut, as in tbrm_grow_region (and unlike tbrm_morph_labels).
 * The islands are the connected components of S, 6-connected (faces) or 26-connected (faces, edges, corners). Nothing wraps across
 * a volume face, whatever data_address_mode says. An island has
 *   a size in voxels,
 *   a first voxel: the one with the smallest linear index x + X * (y + Y * z) (X, Y: the volume's width and height),
 *   a border bit: some voxel of it lies on a face of the box.
 * The order. Islands are ordered by size descending, equal sizes by first voxel ascending: a total order that does not depend on how
 * the components were found. With spare_border = 1 the border islands are spared: taken out of the order, never changed, only
 * counted.
 * The rule. The island at position i of the order, counting from 0, is kept when (max_islands == 0 || i < max_islands) &&
 * size >= min_voxels, otherwise dropped. Kept islands get keep_label + i * label_step (keep_label -1: their bytes stay as they are;
 * label_step is 0 or 1, and 1 requires keep_label >= 0, max_islands >= 1 and keep_label + max_islands - 1 <= 255), dropped islands
 * get drop_label (-1: their bytes stay). Only voxels of S are ever written and each belongs to exactly one island, so there is no
 * writable mask. flags & TBRM_ISLANDS_MEASURE counts everything and writes nothing.
 *   keep the largest n:  max_islands = n, keep_label = -1, drop_label = erase
 *   remove the small:    max_islands = 0, min_voxels = n, keep_label = -1, drop_label = erase
 *   split:               max_islands = k, keep_label = first, label_step = 1; drop_label is the caller's choice
 *   fill the holes of label a, enclosed background islands of up to n voxels:
 *                        source = ~bit(a), spare_border = 1, min_voxels = n + 1 (UINT64_MAX: of any size), keep_label = -1,
 *                        drop_label = a
 * The table. With table != NULL the first min(capacity, islands) islands of the order come back: voxels, first (a valid seed for
 * tbrm_grow_region), label — the label its voxels hold after the call, -1 when they were left as they are and are of several labels
 * — and flags.
 *
 * State and ordering: the contract of tbrm_grow_region, word for word. After a writing call that changed a byte everything behaves
 * bit for bit as if the same bytes had been written with tbrm_update_label_region: the per-brick label sets of the bricks the
 * bounding box touches are recomputed, the live bits refreshed, the merged skipping metadata goes stale. Nothing on the data side
 * moves. A measuring call changes nothing at all. The call is enqueued behind everything issued before on the handle's stream and
 * complete on return; its waits are its own (tbrm_path_counters [12] / [13] do not count them).
 * Memory. The call works in a scratch of its own that the handle keeps, taken on demand and only ever grown: a call that needs no
 * more than an earlier one allocates nothing. It is three buffers: 584 bytes per brick of the box (a bit board, a local component id
 * per voxel, a count and a base); 40 bytes per local component — a component of S inside one 8^3 brick: at most half the box's
 * voxels, in practice a few per set brick; 12 bytes per island plus the temporary storage of the sort and 24 bytes per table entry.
 * tbrm_islands_counters [4] says how many bytes the handle holds.
 * Errors. No volume or no label volume (colour handles have none): TBRM_ERR_NOT_INITIALIZED. Slab-resident handles and volumes of
 * 2^32 voxels or more (an island's size and first voxel are 32-bit sort keys): TBRM_ERR_UNSUPPORTED. TBRM_ERR_INVALID_ARG: a null
 * desc or out, a table with negative capacity or null with capacity > 0, connectivity other than 6 / 26, a box that leaves the
 * volume, keep_label or drop_label outside -1 .. 255, label_step outside 0 / 1 or the step conditions above, a negative
 * max_islands, spare_border outside 0 / 1, unknown flag bits, a non-zero reserved. */
#ifndef TBRM_ISLANDS_H
#define TBRM_ISLANDS_H

#include "tbrm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TBRM_ISLANDS_ABI_VERSION 1
#define TBRM_ISLANDS_MEASURE 1u      /* tbrm_islands_desc::flags: count everything, write nothing */
#define TBRM_ISLAND_KEPT 1u          /* tbrm_island::flags */
#define TBRM_ISLAND_BORDER 2u

typedef struct tbrm_islands_desc {
    int32_t origin[3], extent[3];   /* the box the set is taken in; extent = {0,0,0}: the whole volume */
    int32_t connectivity;           /* 6 or 26 */
    int32_t max_islands;            /* 0: no limit by position */
    uint64_t min_voxels;            /* kept islands have at least this many voxels */
    int32_t keep_label;             /* 0 .. 255 for kept islands (plus position * label_step); -1: leave their bytes */
    int32_t label_step;             /* 0 or 1 */
    int32_t drop_label;             /* 0 .. 255 for dropped islands; -1: leave their bytes */
    int32_t spare_border;           /* 1: islands on a face of the box are out of the order and never change */
    uint32_t flags;                 /* TBRM_ISLANDS_MEASURE */
    uint32_t reserved;              /* 0 */
    uint32_t source[8];             /* the set S: voxels whose label has its bit here */
} tbrm_islands_desc;

typedef struct tbrm_islands_result {
    uint64_t set_voxels;                  /* |S| */
    uint64_t islands, spared;             /* islands in the order; border islands spared (0 without spare_border) */
    uint64_t kept, dropped;               /* of the ordered islands */
    uint64_t kept_voxels, dropped_voxels;
    uint64_t largest;                     /* the size of the order's first island, 0 when there is none */
    uint64_t relabelled;                  /* label bytes that changed (0 when measuring) */
    int32_t  bbox_min[3], bbox_max[3];    /* of the changed bytes, inclusive; none: bbox_min = the volume's dims, bbox_max = -1 */
    int32_t  table_entries, reserved;     /* entries written to the table */
} tbrm_islands_result;

typedef struct tbrm_island {
    uint64_t voxels;
    int32_t  first[3];                    /* (x, y, z) of the first voxel */
    int32_t  label;                       /* what its voxels hold after the call; -1: left as they are and of several labels */
    uint32_t flags;                       /* TBRM_ISLAND_KEPT, TBRM_ISLAND_BORDER */
    uint32_t reserved;
} tbrm_island;

TBRM_API int tbrm_islands_abi_version(void);
TBRM_API int tbrm_label_islands(tbrm_resources* res, const tbrm_islands_desc* desc, tbrm_island* table, int32_t capacity, tbrm_islands_result* out);
/* Cumulative per handle: [0] tbrm_label_islands calls, [1] islands found (ordered and spared), [2] bricks whose label bytes were
 * written, [3] local components (components of the set inside one brick: the slots the merge unites), [4] bytes of scratch the
 * handle holds now (not cumulative), [5] times the scratch was taken or grown. */
TBRM_API int tbrm_islands_counters(const tbrm_resources* res, uint64_t out[6]);

#ifdef __cplusplus
}
#endif
#endif /* TBRM_ISLANDS_H */
