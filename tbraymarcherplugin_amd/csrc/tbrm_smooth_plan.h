// tbrm_smooth_plan.h — the plan of tbrm_smooth_labels (include/tbrm_smooth.h) as pure host code: no device, no
// handle, nothing but integers and doubles. tests/cpp/smooth_plan_test.cpp runs it on its own under the sanitizers.
//
// A pass is a rank filter over the box [v - r, v + r]: a result voxel depends on source voxels at most r_a away along axis a. The
// passes chain, so their reaches add up as in morph_plan and margin_plan: the call works on the bricks that the box grown by
// iterations * r_a, clamped to the volume, touches.
#pragma once
#include <math.h>
#include <stdint.h>

#include "tbrm_box.h"

namespace tbrm {

constexpr int kSmoothMaxRadius = 16;
constexpr int kSmoothMaxIterations = 64;
constexpr int kSmoothMaxReach = 64;
constexpr int kSmoothMaxRankDen = 256;
constexpr int kSmoothLaunchesPerPass = 1;

// what smooth_arguments refuses, by field (SMOOTH_OK: nothing)
enum SmoothRefusal : int { SMOOTH_OK = 0, SMOOTH_RADIUS, SMOOTH_NO_RADIUS, SMOOTH_ITERATIONS, SMOOTH_REACH, SMOOTH_RANK_DEN, SMOOTH_RANK_NUM };

// the bounds of include/tbrm_smooth.h; *axis: of SMOOTH_RADIUS and SMOOTH_REACH, the axis (may be null)
inline SmoothRefusal smooth_arguments(const int32_t radius[3], int32_t rank_num, int32_t rank_den, int32_t iterations, int* axis)
{
    for (int c = 0; c < 3; ++c)
        if (radius[c] < 0 || radius[c] > kSmoothMaxRadius) { if (axis) *axis = c; return SMOOTH_RADIUS; }
    if (radius[0] == 0 && radius[1] == 0 && radius[2] == 0) return SMOOTH_NO_RADIUS;
    if (iterations < 1 || iterations > kSmoothMaxIterations) return SMOOTH_ITERATIONS;
    for (int c = 0; c < 3; ++c)
        if (iterations * radius[c] > kSmoothMaxReach) { if (axis) *axis = c; return SMOOTH_REACH; } // (<= 64 * 16: no overflow)
    if (rank_den < 1 || rank_den > kSmoothMaxRankDen) return SMOOTH_RANK_DEN;
    if (rank_num < 0 || rank_num >= rank_den) return SMOOTH_RANK_NUM;
    return SMOOTH_OK;
}

struct SmoothPlan {
    int radius[3];      // of one pass
    int reach[3];       // of the call: iterations * radius
    int b0[3], nb[3];   // the bricks of the box grown by the reach: nb[c] from b0[c] on
    int wb0[3], wnb[3]; // the bricks of the box itself
    int passes;
};

// dims: the volume in voxels; [origin, end): the box, inside the volume and not empty. False (and *out untouched) when an argument
// is out of range.
inline bool smooth_plan(const int dims[3], const int origin[3], const int end[3], const int32_t radius[3], int32_t iterations, SmoothPlan* out)
{
    if (!dims || !origin || !end || !radius || !out) return false;
    if (smooth_arguments(radius, 0, 1, iterations, nullptr) != SMOOTH_OK) return false;
    for (int c = 0; c < 3; ++c)
        if (dims[c] < 1 || origin[c] < 0 || end[c] <= origin[c] || end[c] > dims[c]) return false;
    SmoothPlan p{};
    p.passes = iterations;
    for (int c = 0; c < 3; ++c) {
        p.radius[c] = radius[c];
        const int t = p.reach[c] = iterations * radius[c];
        const int lo = origin[c] - t < 0 ? 0 : origin[c] - t;
        const int hi = end[c] > dims[c] - t ? dims[c] : end[c] + t; // (no overflow: dims[c] - t is formed, not end + t)
        axis_bricks(lo, hi, p.b0[c], p.nb[c]);
        axis_bricks(origin[c], end[c], p.wb0[c], p.wnb[c]);
    }
    *out = p;
    return true;
}

// Physical units: the voxel spacing and a radius in the same unit -> radii, r_a = floor(radius / spacing_a + 0.5). False (and radii
// untouched) for non-finite or non-positive input, a radius above kSmoothMaxRadius and radii that are all 0.
inline bool smooth_radii(const double spacing[3], double radius, int32_t radii[3])
{
    if (!spacing || !radii) return false;
    if (!isfinite(radius) || !(radius > 0.0)) return false;
    int32_t r[3];
    for (int c = 0; c < 3; ++c) {
        if (!isfinite(spacing[c]) || !(spacing[c] > 0.0)) return false;
        const double q = floor(radius / spacing[c] + 0.5);
        if (!isfinite(q) || !(q <= (double) kSmoothMaxRadius)) return false;
        r[c] = (int32_t) q;
    }
    if (r[0] == 0 && r[1] == 0 && r[2] == 0) return false;
    for (int c = 0; c < 3; ++c) radii[c] = r[c];
    return true;
}

} // namespace tbrm
