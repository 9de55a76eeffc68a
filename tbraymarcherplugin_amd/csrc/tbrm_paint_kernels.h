// tbrm_paint_kernels.h — what tbrm_api_paint.cpp and tbrm_paint_kernels.hip share (include/tbrm_paint.h): the
// parameters of k_paint and its launcher. The boards, their classes and the control words are label morphology's (MorphParams).
#pragma once
#include "tbrm_internal.h"
#include "tbrm_paint_plan.h"

namespace tbrm {

// the control words of a call beyond label morphology's, inside the GROW_CTL_WORDS words of the scratch: three more 64-bit counts.
// MORPH_WINDOWS counts the bricks tested voxel by voxel.
enum PaintCtl : int {
    PAINT_CTL_STAMP = (MORPH_CTL_WORDS + 1) / 2, PAINT_CTL_WHOLE, PAINT_CTL_UNTOUCHED, // uint64 each
    PAINT_CTL_WORDS = 2 * (PAINT_CTL_UNTOUCHED + 1)
};
static_assert((int) PAINT_CTL_WORDS <= (int) GROW_CTL_WORDS, "the brush's control words live in the region growing scratch");

constexpr int kPaintNoGate = -1; // PaintParams::fmt without a gate

struct PaintParams {
    int bnx, bnxy;
    int dims[3];            // the volume in voxels
    VoxelBox work;          // the work box: what stamp_voxels counts
    BrickRange range;       // the bricks of the work box: the only bricks whose scratch a call reads or writes
    int32_t w[3];
    int32_t limit;
    int op;
    int skip;               // 0: no verdicts, no culling: every brick of the range tests every voxel against every segment
    const PaintSegment* segs;
    const PaintRun* runs;
    int n_segs, n_runs;
    const void* data;       // the gate: the bricked data volume (not read without one)
    int fmt;                // FMT_U8 / FMT_U16 / FMT_F32, or kPaintNoGate
    uint32_t lo_code, hi_code;
    float lo_f, hi_f;
    uint64_t* bits;         // per brick (global brick index) 16 words: board 0 (read), board 1 (written)
    uint32_t* cls[2];       // per brick: the class of board 0 / 1
    int32_t* ctl;
};

hipError_t launch_paint(const PaintParams& p, hipStream_t s);

} // namespace tbrm
