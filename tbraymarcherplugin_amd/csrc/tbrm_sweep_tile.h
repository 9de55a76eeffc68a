// tbrm_sweep_tile.h — the index rules of a tile of the propagation sweep (k_light_sweep / k_light_sweep_chain), stated
// once: which cell of a tile a hand-off word carries and which halo cell it lands in, where a pixel lies in the LDS plane, which 16
// bytes of a light-volume brick layer a compute thread stages and where a pixel's voxel then is, and which progress word of the pass
// before a chained tile waits for. The kernel (tbrm_light_sweep.hip) and the host planner (through tbrm_light_sweep.h) take them from here.
//
// Everything here also compiles as plain host C++: tests/cpp/sweep_tile_test.cpp checks it by brute force under the sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define TBRM_SWEEP_HD __host__ __device__ __forceinline__
#else
#define TBRM_SWEEP_HD inline
#endif

namespace tbrm {

constexpr int kSweepTile = 32;                         // a tile's edge: 32 x 32 pixels
// LDS plane: 48 columns x 48 cells (tile + halo <= 14 + guard ring), COLUMN-major — a pixel's two taps of one column
// (rows iy, iy + 1) are neighbours in memory and arrive as one register pair, ready for a packed lerp along x over (top, bottom)
// — with an odd column stride of 49 floats: the 32 columns of a wave's lanes fall into 32 different banks
constexpr int kSweepCols = 48;
constexpr int kSweepColStride = kSweepTile + 17;
constexpr int kSweepPlane = kSweepCols * kSweepColStride;
constexpr int kSweepLvBrick = 528;                     // bytes per staged light-volume brick: 512 + 16, so that the four bricks
                                                       // under a tile row start 4 banks apart

TBRM_SWEEP_HD int sweep_min(int a, int b) { return a < b ? a : b; }
TBRM_SWEEP_HD int sweep_max(int a, int b) { return a > b ? a : b; }

// ---- hand-off words -------------------------------------------------------------------------------------------------------------------
// A stream's taps of the previous slice lie on side sx / sy of their pixel (+1, -1, 0: none) and reach hx columns / hy rows beyond the
// tile. A tile publishes E_x = its hx columns and E_y = its hy rows on the side AWAY from the light, words [row][column of E_x] then
// [row of E_y][column]; its halo is the same cells of the three upstream neighbours: hx columns, hy rows and an hx x hy corner.
struct SweepSides {
    int sx, sy, hx, hy;
};
// hand-off words a tile reads per slice and stream, in chunks of 64 (one per lane of the hand-off wave)
TBRM_SWEEP_HD int sweep_halo_chunks(int hx, int hy) { return (kSweepTile * (hx + hy) + hx * hy + 63) / 64; }
// words of a tile's hand-off record per slice (and per stream of a float light volume): its hx columns and hy rows away from the light
TBRM_SWEEP_HD int sweep_record_words(int hx, int hy) { return kSweepTile * (hx + hy); }

// (a) the tile cell (cx, cy) this tile publishes as word w; false: the record has no word w
TBRM_SWEEP_HD bool sweep_published_cell(int w, const SweepSides& g, int tile, int& cx, int& cy)
{
    const int e0x = g.sx > 0 ? 0 : tile - g.hx, e0y = g.sy > 0 ? 0 : tile - g.hy;
    cx = 0; cy = 0;
    if (w < tile * g.hx) { cy = w / sweep_max(g.hx, 1); cx = e0x + (w - cy * g.hx); }
    else { const int m = w - tile * g.hx; cy = e0y + m / tile; cx = m % tile; }
    return w < tile * g.hx + tile * g.hy;
}
// (b) halo word w of the tile (tile_x, tile_y): the neighbour it comes from — (ntx, nty) = (tile_x + dx, tile_y + dy), one tile towards
// the light along x, along y or both —, that neighbour's word, and the halo cell (cx, cy) in THIS tile's coordinates (negative or >= tile:
// outside the tile, on the light's side). on false: the halo has no word w
struct SweepHaloWord {
    bool on;
    int ntx, nty;
    int word;
    int cx, cy;
};
TBRM_SWEEP_HD SweepHaloWord sweep_halo_word(int w, const SweepSides& g, int tile, int tile_x, int tile_y)
{
    const int hx = g.hx, hy = g.hy;
    const int e0y = g.sy > 0 ? 0 : tile - hy;
    const int nx = tile * hx, ny = tile * hy, nc = hx * hy;
    int ntx = tile_x, nty = tile_y, word = 0, cxh = 0, cyh = 0;
    bool on = false;
    if (w < nx) { const int row = w / sweep_max(hx, 1), kx = w - row * hx; ntx += g.sx; word = row * hx + kx; cxh = (g.sx > 0 ? tile : -hx) + kx; cyh = row; on = true; } // the x-neighbour's E_x
    else if (w < nx + ny) { const int m = w - nx, ky = m / tile, col = m - ky * tile; nty += g.sy; word = nx + ky * tile + col; cxh = col; cyh = (g.sy > 0 ? tile : -hy) + ky; on = true; } // the y-neighbour's E_y
    else if (w < nx + ny + nc) { // the corner: rows e0y .. of the diagonal neighbour's E_x
        const int m = w - nx - ny, ky = m / sweep_max(hx, 1), kx = m - ky * hx;
        ntx += g.sx; nty += g.sy;
        word = (e0y + ky) * hx + kx;
        cxh = (g.sx > 0 ? tile : -hx) + kx; cyh = (g.sy > 0 ? tile : -hy) + ky;
        on = true;
    }
    return SweepHaloWord{on, ntx, nty, word, cxh, cyh};
}
// ---- the LDS plane --------------------------------------------------------------------------------------------------------------------
// Plane coordinate of tile pixel 0 along one plane axis: behind the guard ring and whatever halo lies on the low side. (s, h): the
// launch's own streams; (r_s, r_h): the stream that comes from records (a two-way Change) — 0, 0 for a one-way launch.
TBRM_SWEEP_HD int sweep_plane_origin(int s, int h, int r_s, int r_h) { return 1 + sweep_max(s < 0 ? h : 0, r_s < 0 ? r_h : 0); }
// the cell of tile coordinates (cx, cy) — halo cells included — in a plane whose tile pixel (0, 0) lies at (ox, oy)
TBRM_SWEEP_HD int sweep_plane_cell(int ox, int oy, int cx, int cy) { return (ox + cx) * kSweepColStride + oy + cy; }

// ---- light-volume staging ---------------------------------------------------------------------------------------------------------------
// A layer = the 4 x 4 bricks under the tile at one brick position along the pass's axis, staged brick by brick (kSweepLvBrick bytes
// apart) in pieces of 16 bytes, one per compute thread: piece i is piece i & 31 of brick i >> 5 of the layer, bricks [row v][column u].
// plane axes (u, v) -> volume axes
constexpr int sweep_dim_u(int axis) { return axis == 0 ? 1 : 0; }
constexpr int sweep_dim_v(int axis) { return axis == 2 ? 1 : 2; }
struct SweepPiece {
    bool exists;           // (the tile may hang over the volume's last bricks)
    uint32_t off;          // byte offset of the piece in layer 0 of the bricked volume
    uint32_t layer_stride; // bytes from a layer to the next along the pass's axis
    int brick, part;       // where it is staged: brick of the layer, 16-byte piece of the brick (byte brick * kSweepLvBrick + part * 16)
};
// lbn: bricks of the volume per axis; (base_x, base_y): the tile's first pixel. This function is the rule's statement and what
// tests/cpp/sweep_tile_test.cpp checks; the kernel spells the same arithmetic out (as a function, with a struct or with reference results,
// it moved the chained kernels' spilled scalar registers: profiles/r15_sweep_roles.txt).
template <int AXIS>
TBRM_SWEEP_HD SweepPiece sweep_piece(int piece, int base_x, int base_y, const int (&lbn)[3])
{
    constexpr int dim_u = AXIS == 0 ? 1 : 0, dim_v = AXIS == 2 ? 1 : 2, dim_s = AXIS;
    SweepPiece pc;
    const int lb = piece >> 5;
    const int bu = (base_x >> 3) + (lb & 3), bv = (base_y >> 3) + (lb >> 2);
    pc.exists = bu < lbn[dim_u] && bv < lbn[dim_v];
    int b3[3], l3[3] = {0, 0, 0};
    b3[dim_u] = bu; b3[dim_v] = bv; b3[dim_s] = 0;
    l3[dim_s] = 1;
    pc.off = pc.exists ? (uint32_t) ((b3[2] * lbn[1] + b3[1]) * lbn[0] + b3[0]) * 512u + (uint32_t) (piece & 31) * 16u : 0u;
    pc.layer_stride = (uint32_t) ((l3[2] * lbn[1] + l3[1]) * lbn[0] + l3[0]) * 512u;
    pc.brick = piece >> 5;
    pc.part = piece & 31;
    return pc;
}
// byte of the voxel of tile pixel (column c, row r) in a staged layer, at the layer's first slice; the next slice is sweep_lv_step
// bytes on, the next row sweep_lv_row_step (rows of one brick)
template <int AXIS>
TBRM_SWEEP_HD uint32_t sweep_lv_at(int c, int r)
{
    const uint32_t lb = (uint32_t) ((r >> 3) * 4 + (c >> 3)) * (uint32_t) kSweepLvBrick;
    if (AXIS == 0) return lb + (uint32_t) (r & 7) * 64u + (uint32_t) (c & 7) * 8u;
    else if (AXIS == 1) return lb + (uint32_t) (r & 7) * 64u + (uint32_t) (c & 7);
    else return lb + (uint32_t) (r & 7) * 8u + (uint32_t) (c & 7);
}
constexpr uint32_t sweep_lv_step(int axis) { return axis == 0 ? 1u : (axis == 1 ? 8u : 64u); }
constexpr uint32_t sweep_lv_row_step(int axis) { return axis == 2 ? 8u : 64u; }

// ---- chained launches -------------------------------------------------------------------------------------------------------------------
// Which tile of the pass before owns the bricks of this tile's volume layer L, and how many of ITS layers it must have written back.
// The tile's bricks along the pass before's axis a: one layer when a is this pass's axis, else the four bricks of the tile's extent
// along a; along the pass before's plane axes they lie inside one of its tiles (a range of bricks under a tile is aligned to it, a
// single layer lies inside one). Both are affine in L:
//   progress word  c0 + c1 * (L >> 2)      (L >> 2: the tile of the pass before that holds layer L, when this pass's axis is one of
//   layers needed  n0 + n1 * L              its plane axes — 4 brick layers per 32-pixel tile)
struct SweepDep {
    int c0, c1, n0, n1;
};
// axis: this pass's; in_*: the fields of SweepLink; lo: the tile's first brick per volume axis (0 along this pass's axis)
TBRM_SWEEP_HD SweepDep sweep_chain_dep(int axis, int in_axis, int in_tiles_x, int in_down, int in_layer0, const int (&lo)[3])
{
    const int a = in_axis;
    const int ua = a == 0 ? 1 : 0, va = a == 2 ? 1 : 2;
    const int lo_a = a == 0 ? lo[0] : (a == 1 ? lo[1] : lo[2]), lo_u = ua == 0 ? lo[0] : lo[1], lo_v = va == 1 ? lo[1] : lo[2];
    SweepDep d = {0, 0, 0, 0};
    if (axis == a) { // same axis: the same tile of the pass before, layer by layer
        d.c0 = (lo_v >> 2) * in_tiles_x + (lo_u >> 2);
        d.n0 = in_down ? in_layer0 + 1 : 1 - in_layer0;
        d.n1 = in_down ? -1 : 1;
    } else {
        // the tile's four bricks along a, [lo_a, lo_a + 4): the last of them in the pass before's order
        d.n0 = (in_down ? in_layer0 - lo_a : lo_a + 3 - in_layer0) + 1;
        if (axis == ua) { d.c0 = (lo_v >> 2) * in_tiles_x; d.c1 = 1; }
        else { d.c0 = lo_u >> 2; d.c1 = in_tiles_x; }
    }
    return d;
}
// layers the owner must have written back before layer L is read (bricks past the volume's end belong to no layer of the pass before)
TBRM_SWEEP_HD uint32_t sweep_dep_needed(const SweepDep& d, int L, int in_G) { return (uint32_t) sweep_min(sweep_max(d.n0 + d.n1 * L, 0), in_G); }
// ... and its progress word, [tile] of the pass before
TBRM_SWEEP_HD int sweep_dep_word(const SweepDep& d, int L) { return d.c0 + d.c1 * (L >> 2); }

} // namespace tbrm
