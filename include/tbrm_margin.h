/* tbrm_margin.h — Euclidean margins of labels (C-ABI, libtbrm.so): grow, shrink, open and close a set of labels by a DISTANCE, on
 * anisotropic voxels, computed where the label volume lives. tbrm_morph_labels (tbrm_morphology.h) counts unit steps: its structuring
 * element is an octahedron or a cube in voxels. "A 5 mm margin round this label" on 0.7 x 0.7 x 2.5 mm voxels is a ball in
 * millimetres; the only other way to it is to download the label volume, run a distance transform on the host and upload a box.
 *
 * Integers only; every result is exact. A call carries weights[3] and limit. The weighted squared distance of the voxels u and v is
 *   w_x dx^2 + w_y dy^2 + w_z dz^2,
 * and D_T(v), for a set T of voxels of the volume, is its minimum over u in T — over the WHOLE volume, not the box; infinite when T
 * is empty. S is the source set exactly as in tbrm_morphology.h: the voxels of the whole volume whose label has its bit in source;
 * the zero padding of ragged edge bricks is never in it.
 *   expand(S) = { v in the volume : D_S(v) <= limit }
 *   shrink(S) = { v in S : D_{V \ S}(v) > limit }, the complement taken inside the volume V: what lies outside the volume is not in
 *               it, a label on a volume face is not eaten from outside (the erosion rule of tbrm_morphology.h)
 *   open = expand(shrink(S)), close = shrink(expand(S)).
 * Nothing wraps. The box, writable, new_label (-1 measures only), erase_label, added, removed, relabelled, the bounding box, the state
 * contract, the ordering contract and the errors are those of tbrm_morph_labels, word for word.
 *
 * The reach along axis a is n_a = isqrt(limit / w_a) (integer division first): the largest n with w_a n^2 <= limit.
 * TBRM_ERR_INVALID_ARG, besides tbrm_morph_labels' own: a weight of 0; limit 0 or >= 2^31; a reach above TBRM_MARGIN_MAX_REACH;
 * every reach 0 (nothing is within reach). Under these bounds every sum the kernels form fits 32 bits.
 *
 * Physical units are host arithmetic: tbrm_host_margin_weights turns a voxel spacing and a radius (same unit) into weights and limit:
 * with s the smallest spacing, w_a = llround((spacing_a / s)^2 * 256) and limit = floor((radius / s)^2 * 256). Isotropic spacing gives
 * w = 256 each and exactly the discrete ball d^2 <= r^2; otherwise a weight is off by at most half a unit in 256 or more: 1 part in
 * 512 of the squared spacing ratio. It refuses (TBRM_ERR_INVALID_ARG) non-finite or non-positive input and whatever breaks the bounds above.
 *
 * The distance map is the same transform made visible: tbrm_label_distance writes D_S(v) for the voxels of a box into a host buffer,
 * dense uint32 [ez][ey][ex], capped: every value <= limit is exact, every other voxel holds TBRM_MARGIN_FAR. With inside
 * non-zero it is D_{V \ S}. It reads origin, extent, weights, limit and source of the desc; the other fields must be valid and are ignored.
 *
 * Cost and scratch. A transform is three launches (the bricks' states from the board classes, the x and y axes from the bits, the z
 * axis and the threshold); expand and shrink are one transform, open and close two. It works on the bricks the box grown by the
 * reach (twice the reach for open and close) touches — the range — in the scratch of tbrm_grow_region plus a scratch of its own,
 * kept with the handle, only ever grown, freed with it: 4 bytes per voxel of the largest range a call has needed so far (2 bytes:
 * the intermediate field after the first two axes; 2 bytes: staging of a distance map, which leaves in chunks of z slices) plus one
 * byte per brick (4 1/512 bytes per voxel). A repeated call on the same or a smaller range allocates nothing.
 * Bricks whose result the board classes give are not computed (tunable margin_skip, default 1; 0 computes every brick of the range:
 * the test hook and the A/B switch; the result is the same): a brick that is full stays full under an expand, a brick with nothing
 * set within ceil(n_a / 8) bricks per axis stays empty (shrink: the same on the complement). */
#ifndef TBRM_MARGIN_H
#define TBRM_MARGIN_H

#include "tbrm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TBRM_MARGIN_ABI_VERSION 1
#define TBRM_MARGIN_MAX_REACH 64
#define TBRM_MARGIN_FAR 0xFFFFFFFFu

enum { TBRM_MARGIN_EXPAND = 0, TBRM_MARGIN_SHRINK = 1, TBRM_MARGIN_OPEN = 2, TBRM_MARGIN_CLOSE = 3 };

typedef struct tbrm_margin_desc {
    int32_t origin[3], extent[3];   /* the box that may change (tbrm_label_distance: that is written); extent = {0,0,0}: the whole volume */
    int32_t op;                     /* TBRM_MARGIN_* */
    int32_t new_label;              /* 0 .. 255 for voxels that join; -1: measure only */
    int32_t erase_label;            /* 0 .. 255 for voxels that leave */
    int32_t reserved;               /* 0 */
    uint32_t weights[3];            /* w_x, w_y, w_z: each >= 1 */
    uint32_t limit;                 /* 1 .. 2^31 - 1 */
    uint32_t source[8];             /* the set S: voxels whose label has its bit here */
    uint32_t writable[8];           /* labels a joining voxel may overwrite (all ones: every label) */
} tbrm_margin_desc;

typedef struct tbrm_margin_result {
    uint64_t source_voxels, result_voxels; /* |S in the box|, |R in the box| */
    uint64_t added, removed, relabelled;   /* as in tbrm_morph_result */
    int32_t  bbox_min[3], bbox_max[3];     /* of added and removed together, inclusive; none: bbox_min = the volume's dims, bbox_max = -1 */
    int32_t  reach[3];                     /* n_x, n_y, n_z */
    int32_t  launches;                     /* launches of the distance kernels: 3 per transform */
} tbrm_margin_result;

TBRM_API int tbrm_margin_abi_version(void);
TBRM_API int tbrm_margin_labels(tbrm_resources* res, const tbrm_margin_desc* desc, tbrm_margin_result* out);
/* out_bytes must be 4 * ex * ey * ez of the resolved box */
TBRM_API int tbrm_label_distance(tbrm_resources* res, const tbrm_margin_desc* desc, int32_t inside, void* out_host, size_t out_bytes);
/* no handle, no device: spacing and radius -> weights and limit (above) */
TBRM_API int tbrm_host_margin_weights(const double spacing[3], double radius, uint32_t weights[3], uint32_t* limit);
/* Cumulative per handle: [0] tbrm_margin_labels and tbrm_label_distance calls, [1] launches of the distance kernels, [2] bricks
 * computed (a brick in a transform whose result its neighbourhood's classes did not give), [3] bricks whose label bytes were written. */
TBRM_API int tbrm_margin_counters(const tbrm_resources* res, uint64_t out[4]);

#ifdef __cplusplus
}
#endif
#endif /* TBRM_MARGIN_H */
