// tbrm_islands_kernels.h — what tbrm_api_islands.cpp and tbrm_islands_kernels.hip share (include/tbrm_islands.h): the
// control words, the parameter block and the launches of a tbrm_label_islands call.
#pragma once
#include "tbrm_internal.h"
#include "tbrm_islands_rule.h"

namespace tbrm {

constexpr int kIslandsTile = 1024; // bricks to a tile of the block scan

// the control words of a call (IslandsParams::ctl): 64-bit counts, then 32-bit words
enum IslandsCtl : int {
    ISL_SET_VOXELS, ISL_KEPT, ISL_DROPPED, ISL_KEPT_VOXELS, ISL_DROPPED_VOXELS, ISL_RELABELLED, ISL_BRICKS_WRITTEN, ISL_CTL_COUNTS, // uint64 each
    ISL_TOTAL = 2 * ISL_CTL_COUNTS, // local components: the slots
    ISL_ROOTS, ISL_SPARED, ISL_LARGEST,
    ISL_MIN_X, ISL_MIN_Y, ISL_MIN_Z, ISL_MAX_X, ISL_MAX_Y, ISL_MAX_Z, ISL_CTL_WORDS // int32 each
};
static_assert(ISL_MAX_Z == ISL_MIN_X + 5, "WaveBounds commits to six consecutive words");

struct IslandsEntry { // an island of the table as the device leaves it; the host turns it into a tbrm_island
    uint32_t voxels, first;
    int32_t label;        // what the rule gives: -1 .. 255
    uint32_t flags;
    uint32_t lo, hi;      // the smallest and largest label byte among its voxels before the write
};

struct IslandsParams {
    uint8_t* labels;       // bricked label volume
    int bnx, bnxy;
    int dims[3];           // the volume in voxels
    VoxelBox box;
    BrickRange range;      // the bricks of the box; a brick's scratch is indexed by its position k in this range
    uint32_t nbox;         // nb[0] * nb[1] * nb[2]
    uint32_t source[8];
    int conn26, spare, write;
    IslandsRule rule;
    int32_t* ctl;
    // per brick of the box
    uint64_t* boards;      // 8 slice words: bit y * 8 + x of word z
    uint8_t* lid;          // 512 bytes: the local component of each set voxel, laid out as the label bytes are
    uint32_t* cnt;         // local components, 0 .. 256
    uint32_t* base;        // their first slot, relative to the tile's (k_islands_scan_tiles)
    uint32_t* tile_sum;    // per tile of kIslandsTile bricks
    uint32_t* tile_base;
    // per slot
    uint32_t total;
    uint32_t* parent;      // the union-find forest: parent[s] <= s
    uint32_t* root;        // after the merge
    uint32_t* size;        // of the local component; of the island at its root after k_islands_flatten
    uint32_t* first;
    uint32_t* border;
    uint32_t* rank;        // of a root: its position in the order, 0xffffffff when spared
    int32_t* act;          // of a root: the label its voxels get, -1: none
    uint64_t* keys_in;     // the ordered roots, as k_islands_roots compacts them
    uint32_t* vals_in;
    // per island
    uint32_t n_roots;
    uint64_t* keys_out;
    uint32_t* vals_out;
    IslandsEntry* table;
    uint32_t table_cap;    // entries of it: min(capacity, islands)
};

hipError_t launch_islands_local(const IslandsParams& p, hipStream_t s);
hipError_t launch_islands_scan(const IslandsParams& p, hipStream_t s);
hipError_t launch_islands_slots(const IslandsParams& p, hipStream_t s);
hipError_t launch_islands_merge(const IslandsParams& p, hipStream_t s);
hipError_t launch_islands_flatten(const IslandsParams& p, hipStream_t s); // k_islands_flatten, k_islands_roots
hipError_t islands_sort_bytes(uint32_t n, size_t* bytes);
hipError_t launch_islands_sort(const IslandsParams& p, void* temp, size_t temp_bytes, hipStream_t s);
hipError_t launch_islands_rule(const IslandsParams& p, hipStream_t s);
hipError_t launch_islands_write(const IslandsParams& p, hipStream_t s);

} // namespace tbrm
