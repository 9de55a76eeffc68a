/* tbrm_paint.h — the 3D paint brush (C-ABI, libtbrm.so): a stroke of capsules painted into, or erased from, a set of labels,
 * computed where the label volume lives. The other label edits grow, clean up and cut what is there; the brush stroke itself was the
 * one step left to the host: paint into a host copy and upload a box (tbrm_update_label_region). A brush that respects label masks or
 * paints only voxels inside an intensity range has to read the current labels and voxels, and the only way to them is a download of
 * the whole volume. Here a stroke costs what the stroke touches, not what the volume holds.
 *
 * Integers only; every result is exact.
 *
 * Stroke. n_points points, 1 .. TBRM_PAINT_MAX_POINTS, each three int32 in EIGHTHS OF A VOXEL: the centre of voxel i is at 8 i on
 * its axis. Points may lie outside the volume; every coordinate c has |c| <= TBRM_PAINT_MAX_COORD (2^18). A volume with a dimension
 * above TBRM_PAINT_MAX_DIM (16384) is refused with TBRM_ERR_UNSUPPORTED. One point is one ball. The points k and k + 1 form the
 * segment k; a segment with a == b is a ball.
 *
 * Metric. That of tbrm_margin.h: weights[3], each 1 .. 65535, and <p, q> = w_x p_x q_x + w_y p_y q_y + w_z p_z q_z on vectors in
 * eighths. limit is in the same units, 1 .. 2^30 - 1. A segment's squared length dd = <b - a, b - a> must be below 2^30
 * (TBRM_ERR_INVALID_ARG names the segment; tbrm_host_paint_stroke splits such segments). The reach along axis a in eighths is
 * n_a = isqrt(limit / w_a) (integer division first: the largest n with w_a n^2 <= limit); in voxels, ceil(n_a / 8), which must be at
 * most TBRM_PAINT_MAX_REACH (64).
 *
 * Distance rule. For a voxel centre v and a segment a -> b take d = b - a, e = v - a, dd = <d, d>, de = <d, e>, ee = <e, e>. The
 * voxel is WITHIN the segment when
 *   de <= 0   and  ee <= limit;                       (nearest to a)
 *   de >= dd  and  <v - b, v - b> <= limit;           (nearest to b; <v - b, v - b> = ee - 2 de + dd)
 *   otherwise ee dd - de^2 <= limit dd.               (nearest to the inside: the squared distance is ee - de^2 / dd)
 * No quotient is ever formed. The bound: with |c| <= 2^18 and voxel centres in 0 .. 8 * 16383, |e_a| < 2^19 and |d_a| <= 2^19, so ee
 * and |de| stay below 3 * 2^16 * 2^38 < 2^56. A voxel within the segment lies within sqrt(limit) of a point of it, which lies within
 * sqrt(dd) of a: ee <= (sqrt(limit) + sqrt(dd))^2 <= 2 (dd + limit) < 2^32. A voxel with ee > 2 (dd + limit) is rejected on that
 * first; for the others ee dd < 2^62, de^2 <= ee dd (Cauchy-Schwarz) and limit dd < 2^60: every quantity fits a signed 64-bit integer.
 *
 * Gate. With gate = 1 a voxel also needs its stored value v in lo <= v <= hi: the units, the validation and the NaN rule of
 * tbrm_grow_desc without relative_to_seed (integral codes with 0 <= lo <= hi <= 255 | 65535 for UNORM8 / UNORM16; R32_FLOAT: lo <= hi,
 * both finite after narrowing to float32; a NaN voxel never passes). With gate = 0, lo and hi are not read.
 *
 * M is the set of voxels OF THE VOLUME (never the padding of ragged edge bricks) that are within some segment and pass the gate.
 * S is the source set exactly as in tbrm_morphology.h. op gives the result R:
 *   TBRM_PAINT_PAINT   S | M
 *   TBRM_PAINT_ERASE   S \ M
 * The box, writable, new_label (-1 measures only), erase_label, added, removed, relabelled, the bounding box, the state contract, the
 * ordering contract and the handle errors are those of tbrm_morph_labels, word for word. Nothing wraps.
 *
 * TBRM_ERR_INVALID_ARG, besides tbrm_morph_labels' own, with a message that names the field: n_points outside 1 .. 4096; op or gate
 * out of range; a weight outside 1 .. 65535; limit outside 1 .. 2^30 - 1; a reach above 64 voxels; a coordinate beyond 2^18; a
 * segment with dd >= 2^30; with the gate a bad lo / hi.
 *
 * Cost. The stroke's bounding box grown by the reach, cut to the box, is the WORK BOX: only the bricks it touches are loaded, painted
 * and written, and a stroke that misses the box launches nothing. The stroke is cut into runs of at most 64 consecutive segments, each
 * with its own grown bounding box; a brick tests the runs' boxes, then the segments' boxes of the runs it meets, and only the voxels
 * of bricks that meet a segment are tested against those segments. A brick whose eight corner voxels (of its in-volume part) are
 * within one and the same segment is in the stamp as a whole: the set of points within a segment is convex. With the tunable
 * paint_skip = 0 (default 1) there are no verdicts and no culling: every brick of the work box tests every voxel against every
 * segment — the test hook and the A/B switch; the result is the same. The points and runs are staged in a buffer of the handle that
 * only grows: a second call with a stroke no longer allocates nothing.
 *
 * tbrm_host_paint_brush: spacing and radius (same unit) -> weights and limit. The weights are tbrm_host_margin_weights', the limit is
 * that function's limit x 64 (eighths squared). It refuses what that function refuses and whatever breaks the bounds above.
 * tbrm_host_paint_stroke: positions in the volume's unit cube (tbrm_hit::uvw; 3 floats each) -> points. Per axis
 * nearbyint(8.0 * (N_a - 1) * clamp(uvw_a, 0, 1)) in double (a NaN goes to 0), the voxel convention of tbrm_host_hit_voxel. A point
 * equal to the one before it is dropped. A segment whose dd would reach 2^30 under `weights` is split into the fewest equal parts
 * that all stay below it, the inserted points a + floor(j (b - a) / k) per axis. n_out receives the number of points; with a
 * capacity below it nothing is written and the call fails with TBRM_ERR_INVALID_ARG (n_out is still set). */
#ifndef TBRM_PAINT_H
#define TBRM_PAINT_H

#include "tbrm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TBRM_PAINT_ABI_VERSION 1
#define TBRM_PAINT_MAX_POINTS 4096
#define TBRM_PAINT_MAX_COORD (1 << 18)
#define TBRM_PAINT_MAX_DIM 16384
#define TBRM_PAINT_MAX_WEIGHT 65535
#define TBRM_PAINT_MAX_LIMIT ((1u << 30) - 1u)
#define TBRM_PAINT_MAX_REACH 64

enum { TBRM_PAINT_PAINT = 0, TBRM_PAINT_ERASE = 1 };

typedef struct tbrm_paint_desc {
    int32_t origin[3], extent[3];   /* the box that may change; extent = {0,0,0}: the whole volume */
    int32_t op;                     /* TBRM_PAINT_* */
    int32_t new_label;              /* 0 .. 255 for voxels that join; -1: measure only */
    int32_t erase_label;            /* 0 .. 255 for voxels that leave */
    int32_t gate;                   /* 0: every voxel passes; 1: lo <= stored value <= hi */
    uint32_t weights[3];            /* w_x, w_y, w_z: each 1 .. 65535 */
    uint32_t limit;                 /* 1 .. 2^30 - 1 */
    double  lo, hi;                 /* the gate, in stored units (read with gate = 1) */
    uint32_t source[8];             /* the set S: voxels whose label has its bit here */
    uint32_t writable[8];           /* labels a joining voxel may overwrite (all ones: every label) */
} tbrm_paint_desc;

typedef struct tbrm_paint_result {
    uint64_t stamp_voxels;                 /* |M in the box| */
    uint64_t added, removed, relabelled;   /* as in tbrm_morph_result */
    int32_t  bbox_min[3], bbox_max[3];     /* of added and removed together, inclusive; none: bbox_min = the volume's dims, bbox_max = -1 */
    int32_t  segments;                     /* max(n_points - 1, 1) */
    int32_t  bricks_whole;                 /* bricks whose corners put them in the stamp as a whole */
    int32_t  bricks_untouched;             /* bricks of the work box that meet no segment's box */
    int32_t  bricks_evaluated;             /* bricks tested voxel by voxel */
    int32_t  launches;                     /* kernel launches of the call: 3, or 0 when the stroke misses the box */
    int32_t  reserved;                     /* 0 */
} tbrm_paint_result;

TBRM_API int tbrm_paint_abi_version(void);
TBRM_API int tbrm_paint_labels(tbrm_resources* res, const tbrm_paint_desc* desc, const int32_t* points_xyz, size_t n_points, tbrm_paint_result* out);
/* Cumulative per handle: [0] tbrm_paint_labels calls, [1] kernel launches (as in the result), [2] bricks tested voxel by voxel,
 * [3] bricks whose label bytes were written. */
TBRM_API int tbrm_paint_counters(const tbrm_resources* res, uint64_t out[4]);
/* host only, no handle, no device (above) */
TBRM_API int tbrm_host_paint_brush(const double spacing[3], double radius, uint32_t weights[3], uint32_t* limit);
TBRM_API int tbrm_host_paint_stroke(const int32_t dims[3], const float* uvw, size_t n, const uint32_t weights[3], int32_t* out_points, size_t capacity, size_t* n_out);

#ifdef __cplusplus
}
#endif
#endif /* TBRM_PAINT_H */
