// tbrm_smooth_kernels.h — what tbrm_api_smooth.cpp and tbrm_smooth_kernels.hip share (include/tbrm_smooth.h): the
// parameters of a pass and its launcher. The boards, their classes and the control words are label morphology's (MorphParams).
#pragma once
#include "tbrm_internal.h"

namespace tbrm {

struct SmoothParams {
    int bnx, bnxy;
    int dims[3];           // the volume in voxels
    BrickRange range;      // the bricks of the box grown by the call's reach: the only bricks whose scratch a call reads or writes
    int radius[3];         // r_a, 0 .. 16
    int kb[3];             // ceil(r_a / 8): the bricks per axis a voxel's window touches beyond its own
    uint32_t rank_num, rank_den; // set where c * rank_den > n * rank_num
    uint64_t* bits;        // per brick (global brick index) 16 words: board 0, board 1
    uint32_t* cls[2];      // per brick: the class of board 0 / 1
    int from;              // the pass reads board `from` and writes the other
    int skip;              // 0: every brick of the range is computed
    int32_t* ctl;          // MorphCtl: MORPH_WINDOWS counts the bricks computed
};

size_t smooth_lds_bytes(const SmoothParams& p); // dynamic LDS of a workgroup
hipError_t launch_smooth_count(const SmoothParams& p, hipStream_t s);

} // namespace tbrm
