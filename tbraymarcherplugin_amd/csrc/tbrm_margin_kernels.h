// tbrm_margin_kernels.h — what tbrm_api_margin.cpp and tbrm_margin_kernels.hip share (include/tbrm_margin.h): the
// parameters of a transform and the launchers. The boards, their classes and the control words are label morphology's (MorphParams).
#pragma once
#include "tbrm_internal.h"

namespace tbrm {

// the state of a brick of the range in a transform, in working form (the set, or its complement inside the volume when shrinking):
// what its neighbourhood's classes say about its result
enum : uint8_t {
    MARGIN_FAR_BRICK = 0,   // nothing set within the reach: every distance is TBRM_MARGIN_FAR
    MARGIN_FULL_BRICK = 1,  // every in-volume voxel set: every distance is 0
    MARGIN_COMPUTE = 2
};

struct MarginParams {
    int bnx, bnxy;
    int dims[3];           // the volume in voxels
    BrickRange range;      // the bricks of the box grown by the call's reach: the only bricks whose scratch a call reads or writes
    VoxelBox box;          // k_margin_z<true>: the voxels of the distance map
    uint32_t w[3], limit;
    int reach[3];          // n_a = isqrt(limit / w_a), 0 .. 64
    int kb[3];             // ceil(n_a / 8): the bricks per axis a voxel's reach touches beyond its own
    uint64_t* bits;        // per brick (global brick index) 16 words: board 0, board 1
    uint32_t* cls[2];      // per brick: the class of board 0 / 1
    int from;              // the transform reads board `from` and writes the other
    int shrink;            // the working form is the complement inside the volume
    int skip;              // 0: every brick of the range is MARGIN_COMPUTE
    uint8_t* state;        // per position of the range
    uint16_t* field;       // per position of the range 512 pairs, voxel z * 64 + y * 8 + x: the distance after x and y as (a, b) —
                           // w_x a^2 + w_y b^2, a = 255: TBRM_MARGIN_FAR
    uint32_t* dist;        // k_margin_z<true>: the slices [z0, z1) of the box, dense, x fastest
    int z0, z1;
    int layer0;            // k_margin_z: the launch's first brick layer of the range (its grid: whole layers)
    int32_t* ctl;          // MorphCtl: MORPH_WINDOWS counts the bricks computed
};

hipError_t launch_margin_states(const MarginParams& p, hipStream_t s);
hipError_t launch_margin_xy(const MarginParams& p, hipStream_t s);
hipError_t launch_margin_z(const MarginParams& p, bool distance_map, int layers, hipStream_t s);

} // namespace tbrm
