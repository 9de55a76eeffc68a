/* tbrm_scissors.h — view-space scissors (C-ABI, libtbrm.so): cut or fill labels under a lasso drawn on the rendered image, computed
 * where the label volume lives. Every other label edit is volumetric: the caller says which labels and which box. Scissors take the
 * camera the frame was rendered with and a mask of its pixels: "erase what is under it", "keep only what is under it", "fill it".
 * The only other way to it is to download the label volume, project every voxel centre on the host and upload a box.
 *
 * Integers only; every result is exact.
 *
 * The projection is three integer rows u[4], v[4], w[4] with w_min, w_max, width, height. For the voxel (x, y, z) of the volume
 *   U = u[0] x + u[1] y + u[2] z + u[3], and V and W likewise;
 *   the voxel is IN VIEW when W > 0 and w_min <= W <= w_max;
 *   its pixel is px = floor(U / W), py = floor(V / W) — floor division: a negative U gives a negative pixel.
 * The half-voxel offset of the voxel's centre lives in the constant column; the device never sees a float.
 * tbrm_host_scissors_projection makes the rows from a tbrm_camera; hand-made rows are as good.
 *
 * The mask is height rows of ceil(width / 32) words of 32 bits in host memory: pixel px of a row is bit px & 31 of its word
 * px >> 5. Bits at or beyond width must be 0. tbrm_host_scissors_polygon makes one from a lasso's points.
 *
 * M is the set of voxels OF THE VOLUME that are in view, whose pixel lies inside [0, width) x [0, height) and whose mask bit is set;
 * the padding of ragged edge bricks is never in it. S is the source set exactly as in tbrm_morphology.h: the voxels of the whole
 * volume whose label has its bit in source. op gives the result R:
 *   TBRM_SCISSORS_ERASE_INSIDE    S \ M
 *   TBRM_SCISSORS_ERASE_OUTSIDE   S & M
 *   TBRM_SCISSORS_FILL_INSIDE     S | M
 *   TBRM_SCISSORS_FILL_OUTSIDE    S | (volume \ M)
 * The box, writable, new_label (-1 measures only), erase_label, added, removed, relabelled, the bounding box, the state contract, the
 * ordering contract and the errors are those of tbrm_morph_labels, word for word. Nothing outside the box is consulted: there is no
 * reach, the call works on the bricks the box touches.
 *
 * TBRM_ERR_INVALID_ARG, besides tbrm_morph_labels' own, with a message that names the field: width or height outside
 * 1 .. TBRM_SCISSORS_MAX_IMAGE; a row r with |r[0]| (dim_x - 1) + |r[1]| (dim_y - 1) + |r[2]| (dim_z - 1) + |r[3]| at or above
 * 2^TBRM_SCISSORS_COORD_BITS; w_min < 1 or w_max < w_min; op out of range; n_words other than height * ceil(width / 32); a mask bit at
 * or beyond width; a non-zero reserved. Under these bounds |U|, |V|, W < 2^46 and width * W < 2^60: every quantity the kernel forms
 * fits a signed 64-bit integer.
 *
 * tbrm_host_scissors_projection restates tbrm_camera's own pixel rule (tbrm.h) for the centre of voxel i, in double precision:
 *   uvw = (i + 0.5) / dims - 0.5, P = the volume transform applied to uvw, c = ((P - position) . right, . up, . forward),
 *   U = (c_r / tan_half_fov_x + c_f) width / 2, V = (c_f - c_u / tan_half_fov_y) height / 2, W = c_f,
 * all three affine in i. The rows are scaled by ONE power of two 2^k and rounded to nearest, floor(x 2^k + 0.5); k (scale_log2) is the
 * largest value that keeps the bound above. The coefficient of an axis of one voxel multiplies nothing and is 0. depth_min and
 * depth_max are world units along forward — the out_depth of tbrm_hit.h and the frame's scene_depth, so "cut down to the visible
 * surface" is depth_max = a picked depth: w_min = max(1, ceil(depth_min 2^k)), w_max = floor(depth_max 2^k), INT64_MAX for +inf
 * (both clamped to it). It refuses (TBRM_ERR_INVALID_ARG) non-finite camera or transform values, non-positive tangents, a width or
 * height outside 1 .. TBRM_SCISSORS_MAX_IMAGE, dims below 1, depth_max < depth_min or a NaN depth, and a degenerate scale (rows that
 * are all zero, or that no k of -1000 .. 1000 brings under the bound).
 *
 * tbrm_host_scissors_polygon fills mask_words (all of it: it is cleared first) by the even-odd rule at the pixel centres
 * (px + 0.5, py + 0.5); edges are half-open in y (an edge from a to b crosses the row yc when a.y <= yc < b.y or b.y <= yc < a.y);
 * which side of an edge a centre lies on is the SIGN OF A CROSS PRODUCT, never a quotient, so vertices that are multiples of 2^-8 below
 * 2^15 in magnitude give products exact in double, and the mask is exact. Pixels outside the frame are dropped. It refuses
 * n_points < 3, non-finite points, a width or height out of range and an n_words other than height * ceil(width / 32).
 *
 * Cost and scratch. A call uploads the mask into a staging buffer of the handle that only grows (a second call with a mask no larger
 * allocates nothing), builds a summary of it on the device (a summed-area table over cells of 32 x 8 pixels), and runs one kernel, a
 * wave per brick of the box. A brick whose result S alone gives (empty under an erase, full under a fill) and a brick whose eight
 * corner voxels put it wholly inside or outside M are written as a whole; only the others are projected voxel by voxel (tunable
 * scissors_skip, default 1; 0 projects every brick of the range: the test hook and the A/B switch; the result is the same). */
#ifndef TBRM_SCISSORS_H
#define TBRM_SCISSORS_H

#include "tbrm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TBRM_SCISSORS_ABI_VERSION 1
#define TBRM_SCISSORS_MAX_IMAGE 16384
#define TBRM_SCISSORS_COORD_BITS 46

enum {
    TBRM_SCISSORS_ERASE_INSIDE = 0,
    TBRM_SCISSORS_ERASE_OUTSIDE = 1,
    TBRM_SCISSORS_FILL_INSIDE = 2,
    TBRM_SCISSORS_FILL_OUTSIDE = 3
};

typedef struct tbrm_scissors_projection {
    int64_t u[4], v[4], w[4];   /* U, V, W of the voxel (x, y, z): r[0] x + r[1] y + r[2] z + r[3] */
    int64_t w_min, w_max;       /* in view: W > 0 and w_min <= W <= w_max */
    int32_t width, height;      /* of the mask, 1 .. TBRM_SCISSORS_MAX_IMAGE */
    int32_t scale_log2;         /* written by tbrm_host_scissors_projection (k: a world depth d is W = d 2^k); not read by any call */
    int32_t reserved;           /* not read */
} tbrm_scissors_projection;

typedef struct tbrm_scissors_desc {
    int32_t origin[3], extent[3];   /* the box that may change; extent = {0,0,0}: the whole volume */
    int32_t op;                     /* TBRM_SCISSORS_* */
    int32_t new_label;              /* 0 .. 255 for voxels that join; -1: measure only */
    int32_t erase_label;            /* 0 .. 255 for voxels that leave */
    int32_t reserved;               /* 0 */
    uint32_t source[8];             /* the set S: voxels whose label has its bit here */
    uint32_t writable[8];           /* labels a joining voxel may overwrite (all ones: every label) */
    tbrm_scissors_projection projection;
} tbrm_scissors_desc;

typedef struct tbrm_scissors_result {
    uint64_t source_voxels, result_voxels; /* |S in the box|, |R in the box| */
    uint64_t added, removed, relabelled;   /* as in tbrm_morph_result */
    int32_t  bbox_min[3], bbox_max[3];     /* of added and removed together, inclusive; none: bbox_min = the volume's dims, bbox_max = -1 */
    int32_t  bricks_inside, bricks_outside;/* bricks whose corners put them wholly inside / outside M */
    int32_t  bricks_projected;             /* bricks projected voxel by voxel */
    int32_t  launches;                     /* kernel launches of the call's own: the mask summary's and the scissors kernel's */
} tbrm_scissors_result;

TBRM_API int tbrm_scissors_abi_version(void);
TBRM_API int tbrm_scissors_labels(tbrm_resources* res, const tbrm_scissors_desc* desc, const uint32_t* mask_words, size_t n_words,
                                  tbrm_scissors_result* out);
/* Cumulative per handle: [0] tbrm_scissors_labels calls, [1] kernel launches (as in the result), [2] bricks projected voxel by voxel,
 * [3] bricks whose label bytes were written. */
TBRM_API int tbrm_scissors_counters(const tbrm_resources* res, uint64_t out[4]);
/* host only, no handle, no device (above) */
TBRM_API int tbrm_host_scissors_projection(const int32_t dims[3], const tbrm_world_params* world, const tbrm_camera* camera,
                                           double depth_min, double depth_max, tbrm_scissors_projection* out);
TBRM_API int tbrm_host_scissors_polygon(const double* xy, size_t n_points, int32_t width, int32_t height, uint32_t* mask_words, size_t n_words);

#ifdef __cplusplus
}
#endif
#endif /* TBRM_SCISSORS_H */
