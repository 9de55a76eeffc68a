// tbrm_scissors_kernels.h — what tbrm_api_scissors.cpp and tbrm_scissors_kernels.hip share (include/tbrm_scissors.h):
// the parameters of the mask summary and of k_scissors, and the launchers. The boards, their classes and the control words are label
// morphology's (MorphParams).
#pragma once
#include "tbrm_internal.h"
#include "tbrm_scissors_plan.h"

namespace tbrm {

// the control words of a call beyond label morphology's, inside the GROW_CTL_WORDS words of the scratch: two more 64-bit counts.
// MORPH_WINDOWS counts the bricks projected voxel by voxel.
enum ScissorsCtl : int {
    SCISSORS_CTL_INSIDE = (MORPH_CTL_WORDS + 1) / 2, SCISSORS_CTL_OUTSIDE, // uint64 each
    SCISSORS_CTL_WORDS = 2 * (SCISSORS_CTL_OUTSIDE + 1)
};
static_assert((int) SCISSORS_CTL_WORDS <= (int) GROW_CTL_WORDS, "the scissors' control words live in the region growing scratch");

struct ScissorsParams {
    int bnx, bnxy;
    int dims[3];            // the volume in voxels
    BrickRange range;       // the bricks of the box: the only bricks whose scratch a call reads or writes
    ScissorsRows rows;
    int op;
    int skip;               // 0: no verdicts, every brick of the range is projected
    const uint32_t* mask;   // height rows of row_words words, on the device
    int row_words;
    ScissorsCell* summary;  // (cells_y + 1) x (cells_x + 1) entries (null with skip == 0: not built, not read)
    int cells_x, cells_y;
    uint64_t* bits;         // per brick (global brick index) 16 words: board 0 (read), board 1 (written)
    uint32_t* cls[2];       // per brick: the class of board 0 / 1
    int32_t* ctl;
};

hipError_t launch_scissors_summary(const ScissorsParams& p, hipStream_t s); // kScissorsSummaryLaunches launches
hipError_t launch_scissors(const ScissorsParams& p, hipStream_t s);

} // namespace tbrm
