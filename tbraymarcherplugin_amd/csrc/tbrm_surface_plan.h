// tbrm_surface_plan.h — what the kernels of tbrm_surface_kernels.hip compute (include/tbrm_surface.h), as integer
// arithmetic that also compiles as plain host C++: tests/cpp/surface_plan_test.cpp holds it to a voxel-by-voxel extraction under the
// sanitizers. The boards, rows and boxes are tbrm_brick_boards.h's and tbrm_box.h's (§17).
//
// A BLOCK is the 8^3 cells h with h >> 3 = (bx, by, bz); its cell (x, y, z) is bit y * 8 + x of slice word z, as a board's voxel is.
// The corners of the block's cells are voxels of the eight bricks (bx, by, bz) + {-1, 0}^3. CORNER WORD i of slice z holds, for every
// cell of the slice, whether its corner i is in S: word 7 is the block's own board slice, the others are that slice (i & 4) or the
// one below it, shifted by a column (no i & 1) and a row (no i & 2) with the carries from the neighbour boards.
#pragma once
#include <stdint.h>
#include <string.h>

#include "tbrm_box.h"

namespace tbrm {

constexpr int kSurfaceMaxDim = 1 << 19;  // 24 * cell + 12 stays below 2^24: a position's numerator is exact in float32
enum : uint32_t { SURFACE_TRIANGLES = 1u, SURFACE_MEASURE = 2u, SURFACE_FLAGS = 3u };

struct SurfaceVertex {                   // tbrm_surface_vertex
    int32_t cell[3];
    uint8_t sum[3], edges;
    int8_t normal[3];
    uint8_t corners;
};
static_assert(sizeof(SurfaceVertex) == 20, "five dwords");
constexpr int kSurfaceVertexWords = 5;

TBRM_BOARDS_HD int surface_popc(uint64_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __popcll(v);
#else
    return __builtin_popcountll(v);
#endif
}

// ---- blocks and boxes ----------------------------------------------------------------------------------------------------------------
// the blocks of the cells o <= h <= e of a box [o, e): nb[c] from b0[c] on
TBRM_BOARDS_HD BrickRange surface_blocks(const VoxelBox& box)
{
    BrickRange r{};
    for (int c = 0; c < 3; ++c) {
        r.b0[c] = box.origin[c] >> kBrickShift;
        r.nb[c] = (box.end[c] >> kBrickShift) - r.b0[c] + 1;
    }
    return r;
}

// the bits of the slice z (a voxel coordinate) of the brick column (bx, by) that lie inside the box
TBRM_BOARDS_HD uint64_t slice_in_box(const VoxelBox& b, int bx, int by, int z)
{
    if (z < b.origin[2] || z >= b.end[2]) return 0ull;
    const uint64_t xs = (uint64_t) row_bits(b.origin[0] - bx * kBrick, b.end[0] - bx * kBrick);
    const uint64_t ys = (uint64_t) row_bits(b.origin[1] - by * kBrick, b.end[1] - by * kBrick); // bit j: the row y = by * 8 + j
    uint64_t rows = 0ull;
    TBRM_BOARDS_UNROLL
    for (int j = 0; j < kBrick; ++j) rows |= ((ys >> j) & 1ull) << (8 * j);
    return rows * xs; // (xs < 256: no carry between the rows)
}

// is every voxel of the brick inside the box?
TBRM_BOARDS_HD bool brick_inside_box(const VoxelBox& b, int bx, int by, int bz)
{
    const int at[3] = {bx, by, bz};
    for (int c = 0; c < 3; ++c)
        if (at[c] * kBrick < b.origin[c] || at[c] * kBrick + kBrick > b.end[c]) return false;
    return true;
}

// ---- the corner words of a slice -------------------------------------------------------------------------------------------------------
// fetch(dx, dy, dz, s): slice word s of the board of S at the brick (bx + dx, by + dy, bz + dz), dx, dy, dz in {-1, 0}, cut to the
// box; 0 where there is no such brick
template <class Fetch> TBRM_BOARDS_HD void surface_corner_words(Fetch&& fetch, int z, uint64_t c[8])
{
    TBRM_BOARDS_UNROLL
    for (int hi = 0; hi < 2; ++hi) {
        const int s = (z - 1 + hi) & 7, dz = (z - 1 + hi) < 0 ? -1 : 0;
        const uint64_t w = fetch(0, 0, dz, s), wx = fetch(-1, 0, dz, s), wy = fetch(0, -1, dz, s), wxy = fetch(-1, -1, dz, s);
        const uint64_t y = (w << 8) | (wy >> 56), yx = (wx << 8) | (wxy >> 56);     // the rows one down
        c[4 * hi + 3] = w;
        c[4 * hi + 2] = ((w << 1) & ~kSliceX0) | ((wx >> 7) & kSliceX0);            // the columns one down
        c[4 * hi + 1] = y;
        c[4 * hi + 0] = ((y << 1) & ~kSliceX0) | ((yx >> 7) & kSliceX0);
    }
}

struct SurfaceSlice { uint64_t active, edge[3]; }; // the active cells; the cells whose owned edge along x, y, z has differing ends

TBRM_BOARDS_HD SurfaceSlice surface_slice(const uint64_t c[8])
{
    uint64_t any = 0ull, all = ~0ull;
    TBRM_BOARDS_UNROLL
    for (int i = 0; i < 8; ++i) { any |= c[i]; all &= c[i]; }
    return SurfaceSlice{any & ~all, {c[6] ^ c[7], c[5] ^ c[7], c[3] ^ c[7]}};
}

// the position of the r-th set bit of w, r < popcount(w): which cell of a slice the vertex with the rank r in it belongs to
TBRM_BOARDS_HD int surface_nth_bit(uint64_t w, int r)
{
    int at = 0;
    TBRM_BOARDS_UNROLL
    for (int half = 32; half > 0; half >>= 1) {
        const int n = surface_popc((w >> at) & ((1ull << half) - 1ull));
        if (r >= n) {
            r -= n;
            at += half;
        }
    }
    return at;
}

// the corners byte of the cell at `bit` of the slice
TBRM_BOARDS_HD uint32_t surface_corners(const uint64_t c[8], int bit)
{
    uint32_t v = 0u;
    TBRM_BOARDS_UNROLL
    for (int i = 0; i < 8; ++i) v |= (uint32_t) ((c[i] >> bit) & 1ull) << i;
    return v;
}

// ---- a cell ----------------------------------------------------------------------------------------------------------------------------
// the record of the active cell with the high corner h and the corners byte
TBRM_BOARDS_HD SurfaceVertex surface_vertex(uint32_t corners, int hx, int hy, int hz)
{
    const uint32_t c = corners & 255u;
    // bit i: the edge from corner i along x / y / z (to corner i + 1 / 2 / 4) has differing ends
    const uint32_t dx = (c ^ (c >> 1)) & 0x55u, dy = (c ^ (c >> 2)) & 0x33u, dz = (c ^ (c >> 4)) & 0x0fu;
    const auto n = [](uint32_t v) { return (int) surface_popc((uint64_t) v); };
    SurfaceVertex v;
    v.cell[0] = hx - 1;
    v.cell[1] = hy - 1;
    v.cell[2] = hz - 1;
    v.edges = (uint8_t) (n(dx) + n(dy) + n(dz));
    // an edge along a has its midpoint at 1 along a; along the others it lies at 0 or 2: the corner's own bit
    v.sum[0] = (uint8_t) (n(dx) + 2 * (n(dy & 0xaau) + n(dz & 0xaau)));
    v.sum[1] = (uint8_t) (n(dy) + 2 * (n(dx & 0xccu) + n(dz & 0xccu)));
    v.sum[2] = (uint8_t) (n(dz) + 2 * (n(dx & 0xf0u) + n(dy & 0xf0u)));
    v.normal[0] = (int8_t) (n(c & 0x55u) - n(c & 0xaau));
    v.normal[1] = (int8_t) (n(c & 0x33u) - n(c & 0xccu));
    v.normal[2] = (int8_t) (n(c & 0x0fu) - n(c & 0xf0u));
    v.corners = (uint8_t) c;
    return v;
}

// the record as the five dwords it is stored as (little-endian, as the target is)
TBRM_BOARDS_HD void surface_vertex_words(const SurfaceVertex& v, uint32_t w[kSurfaceVertexWords])
{
    w[0] = (uint32_t) v.cell[0];
    w[1] = (uint32_t) v.cell[1];
    w[2] = (uint32_t) v.cell[2];
    w[3] = (uint32_t) v.sum[0] | (uint32_t) v.sum[1] << 8 | (uint32_t) v.sum[2] << 16 | (uint32_t) v.edges << 24;
    w[4] = (uint32_t) (uint8_t) v.normal[0] | (uint32_t) (uint8_t) v.normal[1] << 8 | (uint32_t) (uint8_t) v.normal[2] << 16 | (uint32_t) v.corners << 24;
}

// one coordinate of the position: (2 edges cell + sum) / (2 edges), times the scale, plus the offset: three float32 operations, each
// rounded to nearest, none fused
TBRM_BOARDS_HD float surface_position(int32_t cell, uint32_t sum, uint32_t edges, float scale, float offset)
{
    const float num = (float) (2 * (int32_t) edges * cell + (int32_t) sum), den = (float) (2 * (int32_t) edges); // both exact
#if defined(__HIP_DEVICE_COMPILE__)
    return __fadd_rn(__fmul_rn(scale, __fdiv_rn(num, den)), offset);
#else
    volatile float q = num / den;
    volatile float m = scale * q; // (volatile: no compiler contracts the two into one)
    return m + offset;
#endif
}

// ---- indices ---------------------------------------------------------------------------------------------------------------------------
// The index of the vertex of the active cell h. look(k, z): of block k (its position in `blocks`) and slice z, the vertices before
// that slice (the block's base and the slice's prefix) and the slice's active word.
struct SurfaceLook { uint64_t before, active; };

template <class Look> TBRM_BOARDS_HD uint32_t surface_index(const BrickRange& blocks, Look&& look, int hx, int hy, int hz)
{
    const uint32_t k = range_position(blocks, hx >> kBrickShift, hy >> kBrickShift, hz >> kBrickShift);
    const SurfaceLook l = look(k, hz & 7);
    const int bit = (hy & 7) * 8 + (hx & 7);
    return (uint32_t) (l.before + (uint64_t) surface_popc(l.active & ((1ull << bit) - 1ull)));
}

// The quad of the owned edge along `axis` of the cell h, whose own vertex has the index `self`; low_in_set: the edge's low end is in S.
template <class Look> TBRM_BOARDS_HD void surface_quad(const BrickRange& blocks, Look&& look, int hx, int hy, int hz, int axis, bool low_in_set, uint32_t self, uint32_t q[4])
{
    const int b = (axis + 1) % 3, c = (axis + 2) % 3;
    int k1[3] = {hx, hy, hz}, k2[3] = {hx, hy, hz}, k3[3] = {hx, hy, hz};
    ++k1[b];
    ++k2[b];
    ++k2[c];
    ++k3[c];
    const uint32_t i1 = surface_index(blocks, look, k1[0], k1[1], k1[2]), i2 = surface_index(blocks, look, k2[0], k2[1], k2[2]), i3 = surface_index(blocks, look, k3[0], k3[1], k3[2]);
    q[0] = self;
    q[1] = low_in_set ? i1 : i3;
    q[2] = i2;
    q[3] = low_in_set ? i3 : i1;
}

// a quad's indices as stored: itself, or the triangles (q0, q1, q2), (q0, q2, q3); returns how many
TBRM_BOARDS_HD int surface_quad_indices(const uint32_t q[4], bool triangles, uint32_t out[6])
{
    if (!triangles) {
        for (int i = 0; i < 4; ++i) out[i] = q[i];
        return 4;
    }
    out[0] = q[0]; out[1] = q[1]; out[2] = q[2];
    out[3] = q[0]; out[4] = q[2]; out[5] = q[3];
    return 6;
}

} // namespace tbrm
