// tbrm_brick_boards.h — the index rules that the brick-per-wave kernels of the statistics, region growing, label morphology and label
// islands share, stated once. A board is the 512 voxels of an 8^3 brick as 8 uint64 slice words: word k is the slice
// z = k, bit y * 8 + x; on this little-endian target byte i of a board's 64 bytes is the x row (y, z) = (i & 7, i >> 3), the row
// that lane i of a brick's wave holds, and that row's 8 label bytes are one uint2.
//
// Everything above the device-only part is integer arithmetic that also compiles as plain host C++:
// tests/cpp/brick_boards_test.cpp checks it voxel by voxel under the sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define TBRM_BOARDS_HD __host__ __device__ __forceinline__
#define TBRM_BOARDS_UNROLL _Pragma("unroll")
#else
#define TBRM_BOARDS_HD inline
#define TBRM_BOARDS_UNROLL
#endif

namespace tbrm {

constexpr int kBrick = 8;      // empty-space-skipping brick edge in voxels
constexpr int kBrickShift = 3;

enum : int { FMT_U8 = 0, FMT_U16 = 1, FMT_F32 = 2 };                    // the stored values of a volume
enum : uint32_t { MORPH_EMPTY = 0, MORPH_FULL = 1, MORPH_MIXED = 2 }; // the class of a board: no bit, every in-volume bit, neither
TBRM_BOARDS_HD uint32_t board_class(bool any, bool all) { return !any ? MORPH_EMPTY : (all ? MORPH_FULL : MORPH_MIXED); }

struct BrickRange { int b0[3], nb[3]; };      // the bricks nb[c] from b0[c] on, on the volume's brick grid; position k runs x fastest
struct VoxelBox { int origin[3], end[3]; };   // the voxels [origin, end)

// ---- brick ranges and the brick grid -----------------------------------------------------------------------------------------------
TBRM_BOARDS_HD uint64_t range_bricks(const BrickRange& r) { return (uint64_t) r.nb[0] * (uint64_t) r.nb[1] * (uint64_t) r.nb[2]; }

// position k of the range -> brick coordinates
TBRM_BOARDS_HD void range_brick(const BrickRange& r, uint32_t k, int& bx, int& by, int& bz)
{
    const uint32_t ix = k % (uint32_t) r.nb[0], q = k / (uint32_t) r.nb[0];
    bx = r.b0[0] + (int) ix;
    by = r.b0[1] + (int) (q % (uint32_t) r.nb[1]);
    bz = r.b0[2] + (int) (q / (uint32_t) r.nb[1]);
}

TBRM_BOARDS_HD bool range_holds(const BrickRange& r, int bx, int by, int bz)
{
    return bx >= r.b0[0] && bx < r.b0[0] + r.nb[0] && by >= r.b0[1] && by < r.b0[1] + r.nb[1] && bz >= r.b0[2] && bz < r.b0[2] + r.nb[2];
}

// brick coordinates -> position in the range (which holds the brick)
TBRM_BOARDS_HD uint32_t range_position(const BrickRange& r, int bx, int by, int bz)
{
    return ((uint32_t) (bz - r.b0[2]) * (uint32_t) r.nb[1] + (uint32_t) (by - r.b0[1])) * (uint32_t) r.nb[0] + (uint32_t) (bx - r.b0[0]);
}

// brick coordinates -> index on the volume's brick grid (bnx bricks along x, bnxy to a z layer)
TBRM_BOARDS_HD size_t grid_index(int bnx, int bnxy, int bx, int by, int bz)
{
    return (size_t) bz * (size_t) bnxy + (size_t) by * (size_t) bnx + (size_t) bx;
}

// ---- row and slice masks -----------------------------------------------------------------------------------------------------------
// The x row of brick column bx at the voxel coordinates (y, z): bit i is the voxel x = bx * 8 + i.
TBRM_BOARDS_HD uint32_t row_bits(int lo, int hi) // the bits [lo, hi) of a row, clipped to it
{
    lo = lo < 0 ? 0 : lo;
    hi = hi > kBrick ? kBrick : hi;
    if (hi <= lo) return 0u;
    return (0xffu >> (kBrick - hi)) & (0xffu << lo) & 0xffu;
}

// the bits of the row that lie inside the box; 0 for a row the box does not touch
TBRM_BOARDS_HD uint32_t row_in_box(const VoxelBox& b, int bx, int y, int z)
{
    if (y < b.origin[1] || y >= b.end[1] || z < b.origin[2] || z >= b.end[2]) return 0u;
    return row_bits(b.origin[0] - bx * kBrick, b.end[0] - bx * kBrick);
}

// the bits of the row that lie inside the volume (bx, y, z >= 0)
TBRM_BOARDS_HD uint32_t row_in_volume(const int dims[3], int bx, int y, int z)
{
    if (y >= dims[1] || z >= dims[2]) return 0u;
    return row_bits(0, dims[0] - bx * kBrick);
}

// the bits of the slice z of the brick column (bx, by) that lie inside the volume
TBRM_BOARDS_HD uint64_t slice_in_volume(const int dims[3], int bx, int by, int z)
{
    if (z >= dims[2]) return 0ull;
    const uint64_t xs = (uint64_t) row_bits(0, dims[0] - bx * kBrick) * 0x0101010101010101ull;
    const int rows = dims[1] - by * kBrick;
    return rows >= kBrick ? xs : (rows <= 0 ? 0ull : xs & ((1ull << (8 * rows)) - 1ull));
}

// ---- windows clipped to the volume ---------------------------------------------------------------------------------------------------
// the voxels of [v - r, v + r] that lie inside an axis of `dim` voxels (r >= 0); 0 for a v outside it, whose window may hold none
TBRM_BOARDS_HD int clipped_extent(int dim, int v, int r)
{
    if (v < 0 || v >= dim) return 0;
    const int lo = v - r < 0 ? 0 : v - r;
    const int hi = v > dim - 1 - r ? dim - 1 : v + r; // (no overflow: dim - 1 - r is formed, not v + r)
    return hi - lo + 1;
}

// The x window of a row as bits: a row word holds the brick's own byte at the bits 16 .. 23 and its neighbours' bytes either side of
// it (bit p: the voxel x = bx * 8 - 16 + p, p < 40); the window of radius r <= 16 of the brick's voxel i is 2 r + 1 bits from 16 + i - r on
constexpr int kRowWordShift = 16;
TBRM_BOARDS_HD uint64_t row_window(int i, int r) { return ((1ull << (2 * r + 1)) - 1ull) << (kRowWordShift + i - r); }

// ---- the 8 bytes of a row (Row8: uint2, or anything with 32-bit x and y) -------------------------------------------------------------
template <class Row8> TBRM_BOARDS_HD uint32_t byte_of(const Row8& v, int i) { return ((i < 4 ? v.x : v.y) >> (8 * (i & 3))) & 255u; }

template <class Row8> TBRM_BOARDS_HD void set_byte(Row8& v, int i, uint32_t to)
{
    const int sh = 8 * (i & 3);
    if (i < 4) v.x = (v.x & ~(255u << sh)) | (to << sh);
    else v.y = (v.y & ~(255u << sh)) | (to << sh);
}

// bit i: label byte i of the row has its bit in the 256-bit mask
template <class Row8> TBRM_BOARDS_HD uint32_t row_in_mask(const Row8& l, const uint32_t* mask)
{
    uint32_t m = 0u;
    TBRM_BOARDS_UNROLL
    for (int i = 0; i < 8; ++i) {
        const uint32_t L = byte_of(l, i);
        m |= ((mask[L >> 5] >> (L & 31)) & 1u) << i;
    }
    return m;
}

// ---- the in-slice part of a dilation -------------------------------------------------------------------------------------------------
constexpr uint64_t kSliceX0 = 0x0101010101010101ull, kSliceX7 = 0x8080808080808080ull; // a slice's columns x = 0 and x = 7

// what a slice word reaches inside its own slice: 6: the word and its four shifts; 26: the 3 x 3 neighbourhood of every bit
template <int CONN26> TBRM_BOARDS_HD uint64_t slice_spread(uint64_t w)
{
    const uint64_t x3 = w | ((w << 1) & ~kSliceX0) | ((w >> 1) & ~kSliceX7);
    if constexpr (!CONN26) return x3 | (w << 8) | (w >> 8);
    else return x3 | (x3 << 8) | (x3 >> 8);
}

#if defined(__HIPCC__)
// ---- device only: a wave per brick ---------------------------------------------------------------------------------------------------
// The prologue of a kernel that gives every brick of a range a wave, THREADS / 64 bricks to a workgroup: the brick's position k in the
// range, its coordinates, its index b on the volume's grid and the lane's x row (y, z); false for a wave beyond the range.
struct WaveBrick { uint32_t k; int bx, by, bz; size_t b; int y, z; };
template <int THREADS> __device__ __forceinline__ bool wave_brick(const BrickRange& r, int bnx, int bnxy, WaveBrick& w)
{
    const int lane = threadIdx.x & 63;
    w.k = blockIdx.x * (THREADS / 64) + (uint32_t) (threadIdx.x >> 6);
    if (w.k >= (uint32_t) range_bricks(r)) return false;
    range_brick(r, w.k, w.bx, w.by, w.bz);
    w.b = grid_index(bnx, bnxy, w.bx, w.by, w.bz);
    w.y = w.by * kBrick + (lane & 7);
    w.z = w.bz * kBrick + (lane >> 3);
    return true;
}

// a wave's result row (this lane's byte of the brick's board, `vol` its in-volume bits) and, from the whole wave, the board's class
__device__ __forceinline__ void store_board_row(uint64_t* board, uint32_t* cls, int lane, uint32_t row, uint32_t vol)
{
    reinterpret_cast<uint8_t*>(board)[lane] = (uint8_t) row;
    const bool any = __ballot(row != 0u) != 0ull, all = __ballot(row != vol) == 0ull;
    if (lane == 0) *cls = board_class(any, all);
}

// ---- device only: the stored values of a row and the gate ----------------------------------------------------------------------------
// the 8 values from element `first` of the bricked volume on (a row of a brick): codes in c (G8, G16) or floats in f (R32F)
template <int FMT> __device__ __forceinline__ void row_values(const void* data, size_t first, uint32_t c[8], float f[8])
{
    if constexpr (FMT == FMT_U8) {
        const uint2 v = *reinterpret_cast<const uint2*>((const uint8_t*) data + first);
#pragma unroll
        for (int i = 0; i < 8; ++i) c[i] = byte_of(v, i);
    } else if constexpr (FMT == FMT_U16) {
        const uint4 v = *reinterpret_cast<const uint4*>((const uint16_t*) data + first);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 8; ++i) c[i] = (w[i >> 1] >> (16 * (i & 1))) & 65535u;
    } else {
        const float4 a = *reinterpret_cast<const float4*>((const float*) data + first);
        const float4 b = *reinterpret_cast<const float4*>((const float*) data + first + 4);
        f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
    }
}

// bit i: value i of the row lies in lo .. hi (a NaN fails both comparisons)
template <int FMT> __device__ __forceinline__ uint32_t row_gate(const uint32_t c[8], const float f[8], uint32_t lo_code, uint32_t hi_code, float lo_f, float hi_f)
{
    uint32_t gate = 0u;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        if constexpr (FMT == FMT_F32) gate |= (uint32_t) (f[i] >= lo_f && f[i] <= hi_f) << i;
        else gate |= (uint32_t) (c[i] >= lo_code && c[i] <= hi_code) << i;
    }
    return gate;
}

// ---- device only: reductions over the wave -------------------------------------------------------------------------------------------
template <typename T> __device__ __forceinline__ T wave_sum(T v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// The bounding box of the voxels a wave moved. A lane takes its bits, the wave reduces, lane 0 commits to the call's six
// consecutive control words MIN_X, MIN_Y, MIN_Z, MAX_X, MAX_Y, MAX_Z (which start as the volume's dims and -1).
struct WaveBounds {
    int mn[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, mx[3] = {-1, -1, -1};

    // the bits of the x row (y, z) of brick column bx
    __device__ __forceinline__ void take_row(uint32_t bits, int bx, int y, int z)
    {
        if (!bits) return;
        mn[0] = bx * kBrick + (__ffs((int) bits) - 1);
        mx[0] = bx * kBrick + (31 - __clz((int) bits));
        mn[1] = mx[1] = y;
        mn[2] = mx[2] = z;
    }
    // the bits of the slice z of brick column (bx, by)
    __device__ __forceinline__ void take_slice(uint64_t w, int bx, int by, int z)
    {
        if (!w) return;
        uint32_t cols = (uint32_t) (w | (w >> 32)); // the OR of the eight rows
        cols |= cols >> 16;
        take_row((cols | (cols >> 8)) & 0xffu, bx, 0, z);
        mn[1] = by * kBrick + ((__ffsll((long long) w) - 1) >> 3);
        mx[1] = by * kBrick + ((63 - __clzll((long long) w)) >> 3);
    }
    __device__ __forceinline__ void reduce()
    {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                mn[c] = min(mn[c], __shfl_xor(mn[c], o, 64));
                mx[c] = max(mx[c], __shfl_xor(mx[c], o, 64));
            }
    }
    // after reduce(): lane 0 commits, when the wave took a bit at all
    __device__ __forceinline__ void commit(int32_t* min_x, int lane) const
    {
        if (lane != 0 || mx[0] < 0) return;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            atomicMin(min_x + c, mn[c]);
            atomicMax(min_x + 3 + c, mx[c]);
        }
    }
};
#endif

} // namespace tbrm
