// tbrm_box.h — the box of a call against the volume, the bricks a box touches and a call's range of stored values,
// stated once: no device, no handle, plain arithmetic. Every entry point that takes an origin and an extent resolves them here;
// tests/cpp/brick_boards_test.cpp runs it on its own under the sanitizers.
#pragma once
#include <limits.h>

#include <cmath>

#include "tbrm_brick_boards.h"

namespace tbrm {

enum BoxRefusal : int { BOX_OK = 0, BOX_EMPTY, BOX_LEAVES }; // an extent <= 0; origin < 0 or origin + extent beyond the volume
struct BoxVerdict { int what, axis; };                       // a BoxRefusal and, of a refusal, its axis

// the bricks that the voxels [lo, hi) of one axis touch: nb from b0 on
inline void axis_bricks(int lo, int hi, int& b0, int& nb)
{
    b0 = lo >> kBrickShift;
    nb = ((hi - 1) >> kBrickShift) - b0 + 1;
}

// The box [origin, origin + extent) against a volume of `dims` voxels. With zero_is_whole an all-zero (or null) extent is the whole
// volume, whatever the origin. dims may be null when the volume is not known yet: then only what no volume can hold is refused.
// On BOX_OK *box is the box in use and *range the bricks it touches (either may be null); a refusal leaves both alone.
inline BoxVerdict box_resolve(const int* dims, const int32_t* origin, const int32_t* extent, bool zero_is_whole, VoxelBox* box, BrickRange* range)
{
    const bool whole = zero_is_whole && dims && (!extent || (extent[0] == 0 && extent[1] == 0 && extent[2] == 0));
    VoxelBox b{};
    for (int c = 0; c < 3; ++c) {
        const int o = whole ? 0 : origin[c], e = whole ? dims[c] : extent[c];
        if (e <= 0) return {BOX_EMPTY, c};
        if (o < 0 || e > (dims ? dims[c] : INT_MAX) - o) return {BOX_LEAVES, c}; // (dims - o is formed, not o + e: no overflow)
        b.origin[c] = o;
        b.end[c] = o + e;
    }
    if (box) *box = b;
    if (range)
        for (int c = 0; c < 3; ++c) axis_bricks(b.origin[c], b.end[c], range->b0[c], range->nb[c]);
    return {BOX_OK, 0};
}

inline const char* box_refusal_text(int what, bool zero_is_whole)
{
    if (what == BOX_EMPTY) return zero_is_whole ? "box extent: must be > 0 along every axis (or all three 0: the whole volume)" : "box extent: must be > 0 along every axis";
    return "the box leaves the volume";
}

// the inverse for a bounding box: the voxels [mn, mx] lie in the bricks [b0, b1)
inline void bbox_bricks(const int32_t mn[3], const int32_t mx[3], int b0[3], int b1[3])
{
    for (int c = 0; c < 3; ++c) {
        b0[c] = mn[c] >> kBrickShift;
        b1[c] = (mx[c] >> kBrickShift) + 1;
    }
}

// A range lo .. hi of stored values as a call gives it: lo <= hi (a NaN fails); of float32 data both finite as float32; of UNORM data
// integral codes within least .. top (tbrm_grow_region's relative_to_seed takes offsets: least = -top).
enum RangeRefusal : int { RANGE_OK = 0, RANGE_ORDER, RANGE_FLOAT, RANGE_CODES };
inline int value_range_refusal(double lo, double hi, bool is_float, double least, double top)
{
    if (!(lo <= hi)) return RANGE_ORDER;
    if (is_float) return std::isfinite(lo) && std::isfinite(hi) && std::isfinite((float) lo) && std::isfinite((float) hi) ? RANGE_OK : RANGE_FLOAT;
    return lo >= least && hi <= top && lo == std::floor(lo) && hi == std::floor(hi) ? RANGE_OK : RANGE_CODES;
}

} // namespace tbrm
