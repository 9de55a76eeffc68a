// tbrm_occ_footprint.h — the footprint rules of the light occlusion, stated once: the work unit's size, where a
// voxel of the light volume samples the data volume, which data texels and bricks the samples of a unit can touch, whether those
// bricks are staged in LDS and where a tap then lies in the staged block, and how large a block of factors is. k_occ_flags, the
// three forms of the occlusion kernel and the host's block-list signature and planners all take them
// from here: the block-list cache is correct because the host's integers ARE the kernel's (one body, IEEE single operations,
// -ffp-contract=off on both sides).
//
// Everything here also compiles as plain host C++: tests/cpp/occ_footprint_test.cpp checks it by brute force under the sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define TBRM_OCC_HD __host__ __device__ __forceinline__
#else
#define TBRM_OCC_HD inline
#endif

namespace tbrm {

// ---- the work unit ------------------------------------------------------------------------------------------------------------------
constexpr int kOccTile = 16;  // pixels per side
constexpr int kOccDepth = 8;  // slices per workgroup (16 was measured: fewer halo bricks per sample, but no faster)
constexpr int kOccSliceFloats = kOccTile * kOccTile;         // factors of one slice of a block
constexpr int kOccBlockFloats = kOccDepth * kOccSliceFloats; // a factor block: [slice][row][column] floats
constexpr int kOccMaxBricks = 192;                           // staged bricks per workgroup (96 KiB of UNORM8 bricks)
constexpr int kBrickVoxels = 512;

TBRM_OCC_HD int occ_min(int a, int b) { return a < b ? a : b; }
TBRM_OCC_HD int occ_max(int a, int b) { return a > b ? a : b; }

// The factor block of rank `rank` in a pass's ascending work list: kept (a factor cache entry) below `cap`, in the handle's scratch
// store beyond (cap = 0: nothing is kept). This function is the rule's statement and what tests/cpp/occ_footprint_test.cpp checks; no
// kernel calls it. The occlusion kernels' three stores (tbrm_light_kernels.hip) and the sweep's reader (tbrm_light_sweep.hip) spell the
// expression out: as a function both pointers are read before the comparison instead of in the arm that uses one, which cost
// k_light_occlusion_runs<0, 0> 20 and k_light_occlusion<0, 1, 2> 45 more spilled scalars and moved the sweep chain's spill counts
// (profiles/r14_occlusion_rules.txt).
template <class T>
TBRM_OCC_HD T* factor_block(T* keep, T* spill, uint32_t cap, uint32_t rank)
{
    return rank < cap ? keep + (size_t) rank * kOccBlockFloats : spill + (size_t) (rank - cap) * kOccBlockFloats;
}

// ---- texel split ----------------------------------------------------------------------------------------------------------------------
// The texel coordinate u * N - 0.5 of a normalised coordinate, clamped to +-2^30 so that the conversion to int is defined (NaN -> -2^30)
TBRM_OCC_HD float texel_coord(float u, float n)
{
    const float x = u * n - 0.5f;
    return __builtin_fminf(__builtin_fmaxf(x, -0x1p30f), 0x1p30f);
}
// Texel split of a normalised coordinate: floor / frac of the texel coordinate
TBRM_OCC_HD void texel_split(float u, float n, int& i0, float& f)
{
    const float x = texel_coord(u, n);
    const float fl = __builtin_floorf(x);
    i0 = (int) fl;
    f = x - fl;
}
TBRM_OCC_HD int base_tap(float u, float n) // texel_split's lower tap alone
{
    return (int) __builtin_floorf(texel_coord(u, n));
}

// ---- where a voxel of the light volume samples: GetUVW(pos, res) + UVWOffset (AddDirLightShader.usf:85), one component ------------------
TBRM_OCC_HD float sample_coord(int pos, int lv_dim, float uvw_off)
{
    return (((float) (uint32_t) pos + 0.5f) / (float) (uint32_t) lv_dim) + uvw_off;
}

// ---- units and their end positions --------------------------------------------------------------------------------------------------
// first and last pixel of block b along a plane axis of `size` pixels
TBRM_OCC_HD void block_ends(int b, int size, int& first, int& last)
{
    first = b * kOccTile;
    last = occ_min(first + kOccTile, size) - 1;
}
// first and last slice of the slice group that starts k0 slices into a pass part of n slices from `start` on (k0 < n)
TBRM_OCC_HD void group_ends(int k0, int n, int start, int dir, int& first, int& last)
{
    const int nk = occ_min(kOccDepth, n - k0);
    first = start + k0 * dir;
    last = first + (nk - 1) * dir;
}

// ---- the tap span: lowest base tap and highest +1 tap of the positions first .. last of one axis ----------------------------------------
// The coordinate is monotonic in the position, so the two end positions decide the span (in either order: dir = -1 hands them over
// swapped). tap_span_add widens [lo, hi] by one stream; start from an empty span (lo = INT32_MAX, hi = INT32_MIN).
TBRM_OCC_HD void tap_span_add(int i0, int& lo, int& hi)
{
    lo = occ_min(lo, i0);
    hi = occ_max(hi, i0 + 1);
}
TBRM_OCC_HD void tap_span_add(int first, int last, int lv_dim, float uvw_off, int data_dim, int& lo, int& hi)
{
    tap_span_add(base_tap(sample_coord(first, lv_dim, uvw_off), (float) data_dim), lo, hi);
    tap_span_add(base_tap(sample_coord(last, lv_dim, uvw_off), (float) data_dim), lo, hi);
}

// ---- brick range, border flag, staging decision ------------------------------------------------------------------------------------------
// The bricks nb from b0 on (of bn along the axis, data_dim texels) that hold the span's taps clamped into the volume; `border`: some
// tap lies outside the volume (the sampler's border colour applies, and k_occ_flags never flags the unit).
TBRM_OCC_HD void brick_span(int lo, int hi, int data_dim, int bn, int& b0, int& nb, bool& border)
{
    const int b_hi = occ_min(hi >> 3, bn - 1);
    b0 = occ_max(lo >> 3, 0);
    nb = occ_max(b_hi - b0 + 1, 0);
    border = lo < 0 || hi >= data_dim;
}
// Are `count` bricks of esz-byte voxels staged in LDS? (else the unit reads its taps from global memory)
TBRM_OCC_HD bool bricks_staged(int count, int esz, int lds_budget_bytes)
{
    return count > 0 && count <= kOccMaxBricks && count * kBrickVoxels * esz <= lds_budget_bytes;
}
// LDS bytes a launch asks for: the staged bricks of the worst unit as estimated from the ratio of data to light-volume resolution.
// `axis`: the launch's slice axis (a unit is kOccDepth positions along it, kOccTile along the others).
inline size_t occ_lds_estimate(const int data_dims[3], const int lv_dims[3], int axis, int esz)
{
    size_t n = 1;
    for (int dim = 0; dim < 3; ++dim) {
        const int pixels = dim == axis ? kOccDepth : kOccTile;
        const double ratio = (double) data_dims[dim] / (double) lv_dims[dim];
        const int texels = (int) ((pixels - 1) * ratio) + 2; // first base tap .. last +1 tap (a workgroup that needs one
        n *= (size_t) ((texels - 1 + 7) / 8 + 1);            // more brick than this reads its taps from global memory)
    }
    return n * kBrickVoxels * (size_t) esz;
}

// ---- offsets in the bricked layout: separable in x, y, z ------------------------------------------------------------------------------------
TBRM_OCC_HD uint32_t brick_off_x(int x) { return ((uint32_t) (x >> 3) << 9) | (uint32_t) (x & 7); }
TBRM_OCC_HD uint32_t brick_off_y(int y, int bnx) { return ((uint32_t) ((y >> 3) * bnx) << 9) | ((uint32_t) (y & 7) << 3); }
TBRM_OCC_HD uint32_t brick_off_z(int z, int bnxy) { return ((uint32_t) ((z >> 3) * bnxy) << 9) | ((uint32_t) (z & 7) << 6); }

// ---- the staged block ------------------------------------------------------------------------------------------------------------------------
// The staged bricks lie in LDS in the order local brick lx + nbx * (ly + nby * lz), each as its 16-byte pieces in order: piece c of
// the copy is piece c % pieces of local brick c / pieces and lands at byte 16 c.
// global index of the x / y part of local brick lxy = lx + nbx * ly, and of z layer lz
TBRM_OCC_HD uint32_t staged_brick_xy(int lxy, int b0x, int b0y, int nbx, int bnx) { return (uint32_t) ((b0y + lxy / nbx) * bnx + (b0x + lxy % nbx)); }
TBRM_OCC_HD uint32_t staged_brick_z(int lz, int b0z, int bnxy) { return (uint32_t) ((b0z + lz) * bnxy); }
// byte offset in the bricked volume of piece c of the copy, whose brick is global brick gb
TBRM_OCC_HD size_t staged_piece_src(uint32_t gb, int c, int pieces, int esz) { return (size_t) gb * kBrickVoxels * esz + (size_t) (c % pieces) * 16; }

// A tap's coordinate clamped into the volume (out-of-range taps are replaced by the border colour after the load); its offset is then
// brick_off_x / _y / _z in the bricked volume, or staged_off in the staged block.
TBRM_OCC_HD int tap_coord(int c, int data_dim) { return occ_min(occ_max(c, 0), data_dim - 1); }
// Offset (in voxels) of the coordinate c (inside the volume) along one axis inside the staged block: its brick clamped into the staged
// range, local brick index * brick stride * 512 + in-brick part. stride: 1, nbx, nbx * nby; AXIS: 0, 1, 2.
template <int AXIS>
TBRM_OCC_HD uint32_t staged_off(int c, int b0, int nb, uint32_t stride)
{
    const int lb = occ_min(occ_max(c >> 3, b0), b0 + nb - 1) - b0;
    return (uint32_t) lb * stride * 512u + ((uint32_t) (c & 7) << (3 * AXIS));
}

// ---- a pass's tap spans: what k_occ_flags reads of a one-chunk pass besides the emptiness bits --------------------------------------------
struct OccPassShape {
    int axis, W, H, dir;                     // slice axis, plane size, direction
    int start, slices;                       // first slice, slices of the pass part the groups cover
    int blocks_x, blocks_y, groups;
    int data_dims[3], lv_dims[3];
    int ns;                                  // streams
    float uvw_off[2][3];
};
// the tap span of block column bx / block row by / slice group zg over the streams; false: a group past the last slice (never computed)
TBRM_OCC_HD bool pass_tap_span(const OccPassShape& s, int part, int index, int& lo, int& hi)
{
    const int dim_u = s.axis == 0 ? 1 : 0, dim_v = s.axis == 2 ? 1 : 2;
    const int dim = part == 0 ? dim_u : (part == 1 ? dim_v : s.axis);
    int first, last;
    if (part == 0) block_ends(index, s.W, first, last);
    else if (part == 1) block_ends(index, s.H, first, last);
    else {
        if (index * kOccDepth >= s.slices) return false;
        group_ends(index * kOccDepth, s.slices, s.start, s.dir, first, last);
    }
    lo = INT32_MAX;
    hi = INT32_MIN;
    for (int si = 0; si < s.ns; ++si) tap_span_add(first, last, s.lv_dims[dim], s.uvw_off[si][dim], s.data_dims[dim], lo, hi);
    return true;
}
// f(lo, hi) for every block column, then every block row, then every slice group ((0, -1) for a group past the last slice)
template <class F>
inline void pass_tap_spans(const OccPassShape& s, F&& f)
{
    const int count[3] = {s.blocks_x, s.blocks_y, s.groups};
    for (int part = 0; part < 3; ++part)
        for (int i = 0; i < count[part]; ++i) {
            int lo = 0, hi = -1;
            (void) pass_tap_span(s, part, i, lo, hi);
            f(lo, hi);
        }
}

} // namespace tbrm
