// tbrm_margin_plan.h — the plan of tbrm_margin_labels and tbrm_label_distance (include/tbrm_margin.h) as pure host
// code: no device, no handle, nothing but integers and doubles. tests/cpp/margin_plan_test.cpp runs it on its own under the sanitizers.
//
// A transform is a capped squared-distance transform with the reach n_a = isqrt(limit / w_a) along axis a: a result voxel depends on
// source voxels at most n_a away along a. Expand and shrink are one transform, open and close two, whose reaches add up as in
// morph_plan: the call works on the bricks that the box grown by the total reach, clamped to the volume, touches.
#pragma once
#include <math.h>
#include <stdint.h>

#include "tbrm_box.h"

namespace tbrm {

constexpr int kMarginMaxReach = 64;
constexpr uint32_t kMarginFar = 0xFFFFFFFFu;
constexpr uint32_t kMarginLimitEnd = 0x80000000u; // limit < 2^31
constexpr int kMarginLaunchesPerTransform = 3;    // the bricks' states, the x and y axes, the z axis
enum : int { MARGIN_EXPAND = 0, MARGIN_SHRINK = 1, MARGIN_OPEN = 2, MARGIN_CLOSE = 3 };

// the largest n with w n^2 <= limit (w >= 1): isqrt(limit / w), in integers
inline int margin_reach(uint32_t w, uint32_t limit)
{
    const uint32_t q = limit / w;
    uint32_t n = 0;
    for (uint32_t bit = 1u << 15; bit; bit >>= 1) { // q < 2^32: n < 2^16
        const uint32_t t = n | bit;
        if ((uint64_t) t * t <= q) n = t;
    }
    return (int) n;
}

// the reaches of a call, or false: a weight of 0, a limit of 0 or >= 2^31, a reach above kMarginMaxReach, every reach 0
inline bool margin_reaches(const uint32_t weights[3], uint32_t limit, int reach[3])
{
    if (!weights || !reach || limit == 0 || limit >= kMarginLimitEnd) return false;
    int n[3];
    for (int c = 0; c < 3; ++c) {
        if (weights[c] == 0) return false;
        n[c] = margin_reach(weights[c], limit);
        if (n[c] > kMarginMaxReach) return false;
    }
    if (n[0] == 0 && n[1] == 0 && n[2] == 0) return false;
    for (int c = 0; c < 3; ++c) reach[c] = n[c];
    return true;
}

struct MarginPlan {
    int reach[3];       // of one transform
    int total[3];       // of the call: reach, or twice that for open and close
    int b0[3], nb[3];   // the bricks of the box grown by the total reach: nb[c] from b0[c] on
    int wb0[3], wnb[3]; // the bricks of the box itself
    int transforms;     // 1 or 2
    uint8_t shrink[2];  // of transform i: 1 = on the complement inside the volume
};

// dims: the volume in voxels; [origin, end): the box, inside the volume and not empty. False (and *out untouched) when an argument
// is out of range.
inline bool margin_plan(const int dims[3], const int origin[3], const int end[3], int op, const uint32_t weights[3], uint32_t limit, MarginPlan* out)
{
    if (!dims || !origin || !end || !out) return false;
    if (op < MARGIN_EXPAND || op > MARGIN_CLOSE) return false;
    for (int c = 0; c < 3; ++c)
        if (dims[c] < 1 || origin[c] < 0 || end[c] <= origin[c] || end[c] > dims[c]) return false;
    MarginPlan p{};
    if (!margin_reaches(weights, limit, p.reach)) return false;
    const bool two = op == MARGIN_OPEN || op == MARGIN_CLOSE;
    p.transforms = two ? 2 : 1;
    const bool first_shrinks = op == MARGIN_SHRINK || op == MARGIN_OPEN;
    p.shrink[0] = (uint8_t) first_shrinks;
    p.shrink[1] = (uint8_t) (two ? !first_shrinks : 0);
    for (int c = 0; c < 3; ++c) {
        const int t = p.total[c] = p.transforms * p.reach[c];
        const int lo = origin[c] - t < 0 ? 0 : origin[c] - t;
        const int hi = end[c] > dims[c] - t ? dims[c] : end[c] + t; // (no overflow: dims[c] - t is formed, not end + t)
        axis_bricks(lo, hi, p.b0[c], p.nb[c]);
        axis_bricks(origin[c], end[c], p.wb0[c], p.wnb[c]);
    }
    *out = p;
    return true;
}

// Physical units: the voxel spacing and a radius in the same unit -> weights and limit. With s the smallest spacing,
// w_a = llround((spacing_a / s)^2 * 256), limit = floor((radius / s)^2 * 256). False for non-finite or non-positive input and for
// whatever margin_reaches refuses.
inline bool margin_weights(const double spacing[3], double radius, uint32_t weights[3], uint32_t* limit)
{
    if (!spacing || !weights || !limit) return false;
    if (!isfinite(radius) || !(radius > 0.0)) return false;
    double s = 0.0;
    for (int c = 0; c < 3; ++c) {
        if (!isfinite(spacing[c]) || !(spacing[c] > 0.0)) return false;
        if (c == 0 || spacing[c] < s) s = spacing[c];
    }
    uint32_t w[3];
    for (int c = 0; c < 3; ++c) {
        const double q = spacing[c] / s, v = q * q * 256.0;
        if (!isfinite(v) || !(v < 4294967295.0)) return false;
        w[c] = (uint32_t) llround(v);
        if (w[c] == 0) return false; // (q >= 1: cannot happen; kept for the bound's sake)
    }
    const double q = radius / s, l = floor(q * q * 256.0);
    if (!isfinite(l) || !(l >= 1.0) || !(l < (double) kMarginLimitEnd)) return false;
    int reach[3];
    if (!margin_reaches(w, (uint32_t) l, reach)) return false;
    for (int c = 0; c < 3; ++c) weights[c] = w[c];
    *limit = (uint32_t) l;
    return true;
}

} // namespace tbrm
