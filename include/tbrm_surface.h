/* tbrm_surface.h — the surface of a set of labels as an indexed mesh (C-ABI, libtbrm.so), extracted where the label volume lives:
 * surface nets on the binary label map. Every segmentation workflow ends in geometry — a static mesh, a file for printing or
 * measuring, a proxy for collision or picking — and the only other way to it is a download of the whole label volume followed by a
 * host mesher. The method needs no case table, its topology is decided by bits alone and a vertex is a ratio of two small integers:
 *
 * Integers only; every result is exact, the optional float32 positions included (three IEEE operations, stated below).
 *
 * Set. S is every voxel inside the box [origin, origin + extent) whose label has its bit in source[8]. An all-zero extent is the
 * whole volume. Voxels outside the box, outside the volume and in the padding of ragged edge bricks are not in S: the surface is
 * closed at the box's faces, cut as tbrm_label_islands cuts. Nothing wraps. The box is resolved and refused as every label call's.
 *
 * Cells. A cell is named by its high corner voxel h, o_a <= h_a <= e_a per axis (o = origin, e = origin + extent): extent + 1 cells
 * per axis. Its eight corners are the voxels h - 1 + (i & 1, i >> 1 & 1, i >> 2 & 1), i = 0 .. 7; `corners` has bit i set when
 * corner i is in S. A cell is ACTIVE when corners is neither 0 nor 255. There is one vertex per active cell.
 *
 * Vertex record (tbrm_surface_vertex, 20 bytes). cell = h - 1 is the low corner voxel (-1 on a face at 0). edges is the number of
 * the cell's 12 edges whose two corners differ (3 .. 12). sum[a] is the sum over those edges of their midpoint's coordinate along
 * a, in half voxels from the low corner (each 0, 1 or 2). normal[a] is the number of corners in S on the low side along a minus
 * the number on the high side (-4 .. 4): it points from S outwards and may be (0, 0, 0) in ambiguous cells. The vertex lies at
 * cell_a + sum_a / (2 edges) in voxel-index units (voxel i's centre is at i) — always inside its cell.
 *
 * Quads. An active cell h owns the three lattice edges h - e_a -> h, a = x, y, z. An end that is not a voxel of the box counts as
 * outside S. An owned edge whose ends differ gives one quad: with (b, c) the cyclic successors of a, its vertices are those of the
 * cells k0 = h, k1 = h + e_b, k2 = h + e_b + e_c, k3 = h + e_c (all four active by construction). The index order is
 * (k0, k1, k2, k3) when the low end h - e_a is in S (outward normal +a), else (k0, k3, k2, k1): counter-clockwise seen from
 * outside. With every vertex at its cell's centre the signed volume of the mesh is |S|, and every mesh edge is shared by 2 or 4
 * quads. Indices are uint32_t: a quad is 4 indices, or with TBRM_SURFACE_TRIANGLES the two triangles (q0, q1, q2), (q0, q2, q3),
 * 6 indices.
 *
 * Order. Cells are grouped in 8^3 blocks by h >> 3 (the volume's brick grid, which the cells of a face at a multiple of 8 leave by
 * one block). Blocks run x fastest over the block range of the cell box, cells within a block run x fastest (x, then y, then z).
 * Vertices follow that order; quads follow their owner's order, then the axis x, y, z.
 *
 * Positions (optional: written when the pointer is not null), float[3 * vertices]. num = 2 edges cell_a + sum_a, |num| < 2^24, so
 * its conversion to float32 is exact (a volume with a dimension above TBRM_SURFACE_MAX_DIM is refused with TBRM_ERR_UNSUPPORTED);
 * q = num / (2 edges) as one IEEE float32 division, round to nearest; p_a = scale_a q + offset_a as one float32 multiplication
 * followed by one float32 addition, NOT fused. numpy float32 arithmetic reproduces it bit for bit. scale and offset must be finite;
 * (1, 1, 1), (0, 0, 0) gives voxel-index coordinates. tbrm_host_surface_unit_cube fills them for the unit cube in the convention of
 * tbrm_host_hit_voxel: voxel i at i / (N - 1) — scale_a = (float) (1.0 / (N_a - 1)), 0 for N_a = 1, offset 0.
 * tbrm_host_surface_positions is the same arithmetic on the host, for records already downloaded.
 *
 * Capacities. vertex_capacity counts vertices, quad_capacity quads. The call always counts. With TBRM_SURFACE_MEASURE it writes
 * nothing and null outputs are fine. Otherwise, if either count exceeds its capacity, nothing is written to any output, the result
 * still carries both counts and the call fails with TBRM_ERR_INVALID_ARG naming the short buffer (the n_out convention of
 * tbrm_host_paint_stroke). A null vertices or indices pointer has the capacity 0.
 *
 * Errors. TBRM_ERR_UNSUPPORTED: 2^32 or more vertices; a slab-resident handle; a colour handle, as the other label calls refuse it.
 * TBRM_ERR_INVALID_ARG: a null desc or out, unknown flags, a non-zero reserved, a non-finite scale or offset, a refused box.
 * The handle errors are those of every label edit (no volume, no label volume).
 *
 * State. The call changes nothing of the handle but its scratch: the label bytes, label sets, live bits, skipping metadata and
 * every other call's counters are what they were. It is enqueued behind everything issued before on the handle's stream and complete
 * on return. The scratch only grows: a call that needs no more than an earlier one allocates nothing.
 *
 * Cost. The source set of the box's bricks as bit boards (label morphology's load), a count per block, a scan, an emit per
 * non-empty block. A block whose eight boards (its own and those at -x, -y, -z, -xy, -xz, -yz, -xyz) are all empty, or all full
 * and wholly inside the box, has no active cell and is not computed; with the tunable surface_skip = 0 (default 1) every block of
 * the range is — the test hook and the A/B switch; the result is the same. */
#ifndef TBRM_SURFACE_H
#define TBRM_SURFACE_H

#include "tbrm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TBRM_SURFACE_ABI_VERSION 1
#define TBRM_SURFACE_MAX_DIM (1 << 19)

enum { TBRM_SURFACE_TRIANGLES = 1, TBRM_SURFACE_MEASURE = 2 };

typedef struct tbrm_surface_vertex {
    int32_t cell[3];                /* the cell's low corner voxel, h - 1 */
    uint8_t sum[3];                 /* per axis: the differing edges' midpoints, in half voxels from the low corner, added up */
    uint8_t edges;                  /* edges whose corners differ, 3 .. 12 */
    int8_t  normal[3];              /* corners in S on the low side minus those on the high side, -4 .. 4 */
    uint8_t corners;                /* bit i: corner i is in S */
} tbrm_surface_vertex;

typedef struct tbrm_surface_desc {
    int32_t origin[3], extent[3];   /* the box S is cut to; extent = {0,0,0}: the whole volume */
    uint32_t flags;                 /* TBRM_SURFACE_* */
    int32_t reserved;               /* 0 */
    uint64_t vertex_capacity;       /* vertices the outputs hold */
    uint64_t quad_capacity;         /* quads the index output holds (4 or 6 indices each) */
    float scale[3], offset[3];      /* of the positions */
    uint32_t source[8];             /* the set S: voxels whose label has its bit here */
} tbrm_surface_desc;

typedef struct tbrm_surface_result {
    uint64_t set_voxels;                   /* |S| */
    uint64_t vertices, quads;              /* counted, whether written or not */
    uint64_t quads_axis[3];                /* quads across an x, y, z lattice edge */
    int32_t  cell_min[3], cell_max[3];     /* of the active cells' low corners (`cell`), inclusive; none: the volume's dims and -1 */
    int32_t  blocks_evaluated;             /* blocks of the range computed bit by bit */
    int32_t  blocks_skipped;               /* blocks the board classes decided */
    int32_t  launches;                     /* kernel launches of the call */
    int32_t  written;                      /* 1: the outputs hold the mesh; 0: nothing was written */
    int32_t  reserved;                     /* 0 */
} tbrm_surface_result;

TBRM_API int tbrm_surface_abi_version(void);
/* vertices: vertex_capacity records; indices: 4 (6 with TBRM_SURFACE_TRIANGLES) x quad_capacity; positions: 3 x vertex_capacity
 * floats, or null. Host memory: */
TBRM_API int tbrm_label_surface(tbrm_resources* res, const tbrm_surface_desc* desc, tbrm_surface_vertex* vertices, uint32_t* indices, float* positions, tbrm_surface_result* out);
/* ... and device memory of the handle's device, 4-byte aligned, written on the handle's stream: */
TBRM_API int tbrm_label_surface_device(tbrm_resources* res, const tbrm_surface_desc* desc, void* d_vertices, void* d_indices, void* d_positions, tbrm_surface_result* out);
/* Cumulative per handle: [0] calls, [1] vertices written, [2] quads written, [3] blocks evaluated; [4] bytes of scratch held now,
 * [5] times the scratch was taken or grown. */
TBRM_API int tbrm_surface_counters(const tbrm_resources* res, uint64_t out[6]);
/* host only, no handle, no device (above) */
TBRM_API int tbrm_host_surface_positions(const tbrm_surface_vertex* vertices, size_t n, const float scale[3], const float offset[3], float* out_positions);
TBRM_API int tbrm_host_surface_unit_cube(const int32_t dims[3], float scale[3], float offset[3]);

#ifdef __cplusplus
}
#endif
#endif /* TBRM_SURFACE_H */
