// tbrm_surface_kernels.h — what tbrm_api_surface.cpp and tbrm_surface_kernels.hip share (include/tbrm_surface.h): the
// parameters of k_surface_count, the scan and k_surface_emit, and their launchers. The boards of S and their classes are label
// morphology's board 0 (k_morph_load, as it stands), in the scratch of region growing.
#pragma once
#include "tbrm_internal.h"
#include "tbrm_surface_plan.h"

namespace tbrm {

constexpr int kSurfaceTile = 1024; // blocks to a tile of the scan

// the control words of a call: 64-bit counts, then the 32-bit bounding box of the active cells' HIGH corners
enum SurfaceCtl : int {
    SURF_SET_VOXELS, SURF_QUADS_X, SURF_QUADS_Y, SURF_QUADS_Z, SURF_EVALUATED, SURF_SKIPPED, SURF_VERTICES, SURF_QUADS, SURF_CTL_COUNTS, // uint64 each
    SURF_MIN_X = 2 * SURF_CTL_COUNTS, SURF_MIN_Y, SURF_MIN_Z, SURF_MAX_X, SURF_MAX_Y, SURF_MAX_Z, SURF_CTL_WORDS                          // int32 each
};
static_assert(SURF_MAX_Z == SURF_MIN_X + 5, "WaveBounds commits to six consecutive words");

struct SurfaceParams {
    int bnx, bnxy;
    VoxelBox box;               // what S is cut to
    BrickRange bricks;          // the bricks of the box: where board 0 and its class are S's
    BrickRange blocks;          // the blocks of the cells; position k runs x fastest
    uint32_t n_blocks;
    int skip;                   // 0: every block of the range is computed
    int triangles;
    const uint64_t* bits;       // per brick (global brick index) 16 words: board 0 (read)
    const uint32_t* cls;        // per brick: the class of board 0
    // per block k
    uint64_t* active;           // 8 words: the active cells of its slices
    uint32_t* prefix;           // 8 words: of slice z, the block's vertices before it | its quads before it << 16
    uint32_t* count[2];         // its vertices / quads
    uint32_t* base[2];          // ... before it within its tile
    uint64_t* tile_sum[2];      // per tile
    uint64_t* tile_base[2];
    int32_t* ctl;               // SURF_CTL_WORDS words
    // the outputs (k_surface_emit)
    uint32_t* vertices;         // kSurfaceVertexWords dwords each
    uint32_t* indices;
    float* positions;           // null: none
    float scale[3], offset[3];
};

hipError_t launch_surface_count(const SurfaceParams& p, hipStream_t s);
hipError_t launch_surface_scan(const SurfaceParams& p, hipStream_t s); // two launches
hipError_t launch_surface_emit(const SurfaceParams& p, hipStream_t s);

} // namespace tbrm
