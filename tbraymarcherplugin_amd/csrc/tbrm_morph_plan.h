// tbrm_morph_plan.h — the step plan of tbrm_morph_labels (include/tbrm_morphology.h) as pure host code: no device,
// no handle, nothing but integers. tests/cpp/morph_plan_test.cpp runs it on its own under the sanitizers.
//
// An operator of radius r is r unit steps of one kind (dilate, erode) or two such sequences (open: erode then dilate; close: dilate
// then erode). A step moves a bit by at most one voxel, so a result voxel depends on source voxels at most `reach` away: r, or 2r
// for open and close. The call works on the bricks that the box grown by the reach, clamped to the volume, touches; a launch of
// k_morph_steps iterates up to `per_launch` (1 .. 8) steps of one kind, so a sequence of r steps is ceil(r / per_launch) launches.
#pragma once
#include <stdint.h>

#include "tbrm_box.h"

namespace tbrm {

constexpr int kMorphMaxRadius = 64;
constexpr int kMorphMaxSteps = 8;                       // steps of one launch: what a brick's 3 x 3 x 3 brick neighbourhood determines
constexpr int kMorphMaxLaunches = 2 * kMorphMaxRadius;  // open / close of the largest radius at one step per launch
enum : int { MORPH_DILATE = 0, MORPH_ERODE = 1, MORPH_OPEN = 2, MORPH_CLOSE = 3 };

struct MorphPlan {
    int reach;
    int b0[3], nb[3];   // the bricks of the box grown by the reach: nb[c] from b0[c] on
    int wb0[3], wnb[3]; // the bricks of the box itself
    int launches;
    uint8_t steps[kMorphMaxLaunches]; // of launch i: 1 .. per_launch
    uint8_t erode[kMorphMaxLaunches]; // of launch i: 1 = an erosion step sequence
};

// dims: the volume in voxels; [origin, end): the box, inside the volume and not empty. False (and *out untouched) when an argument
// is out of range.
inline bool morph_plan(const int dims[3], const int origin[3], const int end[3], int op, int radius, int per_launch, MorphPlan* out)
{
    if (!dims || !origin || !end || !out) return false;
    if (op < MORPH_DILATE || op > MORPH_CLOSE || radius < 1 || radius > kMorphMaxRadius) return false;
    for (int c = 0; c < 3; ++c)
        if (dims[c] < 1 || origin[c] < 0 || end[c] <= origin[c] || end[c] > dims[c]) return false;
    if (per_launch < 1) per_launch = 1;
    if (per_launch > kMorphMaxSteps) per_launch = kMorphMaxSteps;
    MorphPlan p{};
    const bool two = op == MORPH_OPEN || op == MORPH_CLOSE;
    p.reach = two ? 2 * radius : radius;
    for (int c = 0; c < 3; ++c) {
        const int lo = origin[c] - p.reach < 0 ? 0 : origin[c] - p.reach;
        const int hi = end[c] > dims[c] - p.reach ? dims[c] : end[c] + p.reach; // (no overflow: dims[c] - reach is formed, not end + reach)
        axis_bricks(lo, hi, p.b0[c], p.nb[c]);
        axis_bricks(origin[c], end[c], p.wb0[c], p.wnb[c]);
    }
    const int first_erodes = op == MORPH_ERODE || op == MORPH_OPEN;
    for (int phase = 0; phase < (two ? 2 : 1); ++phase)
        for (int left = radius; left > 0;) {
            const int k = left < per_launch ? left : per_launch;
            p.steps[p.launches] = (uint8_t) k;
            p.erode[p.launches] = (uint8_t) (phase == 0 ? first_erodes : !first_erodes);
            ++p.launches;
            left -= k;
        }
    *out = p;
    return true;
}

} // namespace tbrm
