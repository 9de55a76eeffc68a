// tbrm_compete_kernels.h — what tbrm_api_compete.cpp and tbrm_compete_kernels.hip share (include/tbrm_compete.h): the
// parameters of the three kernels and their launchers.
#pragma once
#include "tbrm_internal.h"
#include "tbrm_compete_plan.h"

namespace tbrm {

static_assert(COMPETE_MAX_Z == COMPETE_MIN_X + 5, "WaveBounds commits to six consecutive words");

struct CompeteParams {
    const void* data;      // bricked data volume
    uint8_t* labels;       // bricked label volume on the same grid
    int fmt;
    int bnx, bnxy;         // the volume's brick grid (data and labels are indexed by it)
    VoxelBox box;          // inside the volume
    BrickRange range;      // the bricks it touches; the scratch is indexed by a brick's position in it
    uint32_t lo_code, hi_code; // UNORM: the gate
    float lo_f, hi_f;          // R32_FLOAT: the gate (NaN voxels fail both)
    float float_origin, float_scale;
    uint32_t seeds[8], writable[8];
    uint32_t step[3];
    int shift;
    uint32_t limit;        // 1 .. kCompeteMaxCost
    uint32_t* keys;        // 512 words per brick of the range, a brick's voxel (x, y, z) at (z * 8 + y) * 8 + x
    uint8_t* claim;        // 64 bytes per brick of the range: byte i is the x row (y, z) = (i & 7, i >> 3), bit x: claimable
    uint32_t* act[2];      // per brick of the range: due in this pass ([0]: read and cleared) / in the next ([1]: set)
    unsigned long long* counts; // COMPETE_COUNTS
    int32_t* ctl;          // COMPETE_CTL_WORDS
    int changed_word;      // COMPETE_CHANGED + the pass's index in its batch
    int write;             // k_compete_write stores the label bytes
    uint32_t* costs;       // the costs of the box, x fastest (null: not asked for)
};

hipError_t launch_compete_init(const CompeteParams& p, hipStream_t s);
hipError_t launch_compete_pass(const CompeteParams& p, hipStream_t s);
hipError_t launch_compete_write(const CompeteParams& p, hipStream_t s);

} // namespace tbrm
