/* tbrm_compete.h — competitive growing from seed labels (C-ABI, libtbrm.so): the "grow from seeds" of a segmentation editor. A few
 * painted strokes of several labels compete for the rest of a box: every claimable voxel goes to the seed label that reaches it at
 * the least cost along a path of face steps, computed where the voxels and the label volume live. The only other way to it is to
 * download the volume and the labels, run a shortest-path solver on the host and upload a box of labels.
 *
 * Voxels. The box is [origin, origin + extent); an all-zero extent is the whole volume, as in tbrm_grow_desc.
 *   - Seed voxels: the voxels of the box whose current label L has its bit in seeds, (seeds[L >> 5] >> (L & 31)) & 1.
 *   - Claimable voxels: the voxels of the box that lie inside the volume (the zero padding of ragged edge bricks never does), whose
 *     label has its bit in writable and not in seeds, and whose stored value v passes the gate lo <= v <= hi: the units and rules
 *     of tbrm_grow_desc without relative_to_seed (integral codes with 0 <= lo <= hi <= 255 | 65535 for UNORM8 / UNORM16; R32_FLOAT:
 *     lo <= hi, both finite after narrowing to float32). A NaN voxel is never claimable.
 *   - Every other voxel is a wall.
 * Codes. c(v) is the stored code for UNORM8 / UNORM16. For R32_FLOAT
 *     c(v) = (uint32) rintf(fminf(fmaxf((v - float_origin) * float_scale, 0.0f), 65535.0f)),
 * the subtraction and the multiplication two separate float32 operations (never one fused multiply-add), rintf to nearest, ties to
 * even. tbrm_host_compete_float_range makes float_origin / float_scale of a value range. A NaN seed voxel is a seed voxel (it never
 * changes, its cost is 0) but no source: no path starts there.
 * Cost. The neighbourhood is the 6 face neighbours; 26-connectivity is not offered, connectivity must be 6. A step between face
 * neighbours u, v along axis a costs
 *     w = step_cost[a] + (|c(u) - c(v)| >> value_shift),    step_cost[a] in 0 .. 65535 (per axis: the voxel spacing), value_shift in 0 .. 16.
 * A path starts at a seed voxel and continues through claimable voxels only: it never leaves the box, never wraps across a volume
 * face whatever data_address_mode says, never passes through a second seed voxel. Its key is (cost << 8) | label_of_its_seed. A
 * claimable voxel's key is the minimum over all paths to it whose cost is at most cost_limit (1 .. 2^24 - 1; 0 means 2^24 - 1): the
 * cheapest seed, ties to the smaller label. Costs never decrease along a path, so pruning a partial path above the limit loses
 * nothing. A voxel with a key is claimed and takes that label; the others keep theirs. Seed voxels never change.
 * The 24-bit limit is deliberate: key and label fit one 32-bit word, which halves the traffic of the pass kernel and makes a racy
 * read of a neighbour's word whole. The one word 0xFFFFFFFF — cost 2^24 - 1 reached from label 255 — is the word of a voxel nothing
 * has reached, so that one path is never taken: for label 255 the largest cost that claims is 2^24 - 2.
 * The answer is a unique set of integers: it does not depend on how the device schedules the work. Only `passes` may.
 *
 * costs_out (optional, host memory): extent[0] * extent[1] * extent[2] uint32 of the box in use, x fastest: the cost of claimed
 * voxels, 0 for seed voxels, TBRM_COMPETE_NO_COST everywhere else. It is filled in measuring calls too.
 *
 * State (the contract of tbrm_grow_region). After a writing call everything behaves bit for bit as if the same bytes had been
 * written with tbrm_update_label_region: the per-brick label sets of the bricks the claimed voxels' bounding box touches are
 * recomputed, the live bits refreshed, the merged skipping metadata goes stale. Nothing on the data side moves. A measuring call
 * (measure_only = 1) changes nothing at all. The call is enqueued behind everything issued before on the handle's stream and is
 * complete on return; its waits are its own (tbrm_path_counters [12] / [13] do not count them).
 * Scratch: one 32-bit key per voxel of the bricks the box touches (2 KiB per brick), one claimable bit per voxel (64 bytes per
 * brick), two activity words per brick and a few hundred control words: 512 MiB + 18 MiB for a whole 512^3 volume. With costs_out a
 * second buffer of 4 bytes per voxel of the box. Both are taken by the first call that needs them at that call's size, grown when a
 * later call needs more, never shrunk, freed with the handle: from the second call of the same size on a call allocates nothing.
 * tbrm_resources_reserve does not take them.
 * Handles. Mono handles with a label volume. No volume, or no label volume (colour handles never have one): TBRM_ERR_NOT_INITIALIZED.
 * Slab-resident handles: TBRM_ERR_UNSUPPORTED. TBRM_ERR_INVALID_ARG: a null res, desc or out, a box that is empty or leaves the
 * volume, a bad lo / hi, step_cost, value_shift or cost_limit out of range, a connectivity other than 6, measure_only other than
 * 0 / 1, reserved non-zero, on a float handle a float_scale that is not finite or not positive or a float_origin that is not finite.
 * No seed voxel in the box is not an error: nothing is claimed. */
#ifndef TBRM_COMPETE_H
#define TBRM_COMPETE_H

#include "tbrm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TBRM_COMPETE_ABI_VERSION 1
#define TBRM_COMPETE_MAX_COST 0xFFFFFFu      /* 2^24 - 1 */
#define TBRM_COMPETE_MAX_STEP_COST 65535
#define TBRM_COMPETE_MAX_SHIFT 16
#define TBRM_COMPETE_NO_COST 0xFFFFFFFFu

typedef struct tbrm_compete_desc {
    int32_t origin[3], extent[3];   /* the box; extent = {0,0,0}: the whole volume (origin is then ignored) */
    int32_t connectivity;           /* 6 */
    int32_t measure_only;           /* 0: claimed voxels take their label; 1: nothing is written */
    int32_t step_cost[3];           /* 0 .. 65535 per axis */
    int32_t value_shift;            /* 0 .. 16 */
    uint32_t cost_limit;            /* 1 .. 2^24 - 1; 0: 2^24 - 1 */
    int32_t reserved;               /* 0 */
    double  lo, hi;                 /* the gate, in stored units */
    float   float_origin, float_scale; /* R32_FLOAT handles: the code rule above; ignored otherwise */
    uint32_t seeds[8];              /* the labels that grow */
    uint32_t writable[8];           /* the labels that may be claimed (all ones: every label that is no seed) */
} tbrm_compete_desc;

typedef struct tbrm_compete_result {
    uint64_t seed_voxels;           /* seed voxels in the box */
    uint64_t claimable;             /* claimable voxels in the box */
    uint64_t claimed;               /* of those, the ones with a key */
    uint64_t relabelled;            /* voxels whose label byte changed; 0 in a measuring call */
    uint64_t claimed_per_label[256];
    uint32_t max_cost;              /* the largest cost of a claimed voxel; 0 when nothing was claimed */
    int32_t  passes;                /* passes that changed a brick */
    int32_t  bbox_min[3], bbox_max[3]; /* of the claimed voxels, inclusive; none: bbox_min = the volume's dims, bbox_max = -1 */
} tbrm_compete_result;

TBRM_API int tbrm_compete_abi_version(void);
TBRM_API int tbrm_compete_labels(tbrm_resources* res, const tbrm_compete_desc* desc, uint32_t* costs_out, tbrm_compete_result* out);
/* Pure host code: the float_origin / float_scale that map [lo, hi] onto the codes 0 .. 65535, origin = lo and scale = 65535 / (hi - lo),
 * formed in double and narrowed to float32. lo / hi not finite, hi <= lo, or a result that is not finite and positive as float32:
 * TBRM_ERR_INVALID_ARG. */
TBRM_API int tbrm_host_compete_float_range(double lo, double hi, float* float_origin, float* float_scale);
/* Cumulative per handle: [0] tbrm_compete_labels calls, [1] passes (the sum of tbrm_compete_result::passes), [2] brick visits (one
 * per brick per pass in which it was relaxed), [3] bricks whose label bytes were written. */
TBRM_API int tbrm_compete_counters(const tbrm_resources* res, uint64_t out[4]);

#ifdef __cplusplus
}
#endif
#endif /* TBRM_COMPETE_H */
