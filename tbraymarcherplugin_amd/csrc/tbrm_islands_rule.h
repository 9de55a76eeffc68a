// tbrm_islands_rule.h — the rule of tbrm_label_islands (include/tbrm_islands.h) and the validation of its arguments,
// stated once: no device, no handle, nothing but integers. The host validates with it, the kernels apply it per island
// (k_islands_rule), tests/cpp/islands_rule_test.cpp runs it on its own under the sanitizers.
#pragma once
#include <stdint.h>

#include "tbrm_box.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TBRM_ISLANDS_HD __host__ __device__
#else
#define TBRM_ISLANDS_HD
#endif

namespace tbrm {

constexpr uint32_t kIslandsMeasure = 1u;   // TBRM_ISLANDS_MEASURE
constexpr uint32_t kIslandKept = 1u, kIslandBorder = 2u; // TBRM_ISLAND_KEPT, TBRM_ISLAND_BORDER
constexpr int kIslandsLeave = -1;          // a label that means: the bytes stay as they are

struct IslandsRule {
    uint64_t min_voxels;
    int32_t max_islands;    // 0: no limit by position
    int32_t keep_label;     // -1 .. 255
    int32_t label_step;     // 0 / 1
    int32_t drop_label;     // -1 .. 255
};

// The island at `position` of the order (size descending, first voxel ascending; spared islands are not in it) with `size` voxels:
// is it kept, and what do its voxels get (kIslandsLeave: nothing)?
TBRM_ISLANDS_HD inline bool islands_kept(const IslandsRule& r, uint64_t position, uint64_t size)
{
    return (r.max_islands == 0 || position < (uint64_t) r.max_islands) && size >= r.min_voxels;
}
TBRM_ISLANDS_HD inline int islands_label(const IslandsRule& r, uint64_t position, uint64_t size)
{
    if (!islands_kept(r, position, size)) return r.drop_label;
    if (r.keep_label < 0) return kIslandsLeave;
    return r.keep_label + (r.label_step ? (int) position : 0); // (validated: position < max_islands, keep_label + max_islands - 1 <= 255)
}

// the order's key: smaller keys come first. Sizes and first voxels are below 2^32 (the volume has fewer voxels than that).
TBRM_ISLANDS_HD inline uint64_t islands_key(uint32_t size, uint32_t first) { return (uint64_t) (~size) << 32 | (uint64_t) first; }
TBRM_ISLANDS_HD inline uint32_t islands_key_size(uint64_t key) { return ~(uint32_t) (key >> 32); }
TBRM_ISLANDS_HD inline uint32_t islands_key_first(uint64_t key) { return (uint32_t) key; }

// What is wrong with the arguments: nullptr when nothing is. dims: the volume in voxels; on success box_origin / box_end are the box
// in use (an all-zero extent: the whole volume).
inline const char* islands_validate(const int dims[3], const int32_t origin[3], const int32_t extent[3], int connectivity, int max_islands,
                                    int keep_label, int label_step, int drop_label, int spare_border, uint32_t flags, uint32_t reserved,
                                    int box_origin[3], int box_end[3])
{
    if (!dims || !origin || !extent || !box_origin || !box_end) return "null argument";
    if (connectivity != 6 && connectivity != 26) return "connectivity: must be 6 or 26";
    if (max_islands < 0) return "max_islands: must be >= 0 (0: no limit)";
    if (keep_label < -1 || keep_label > 255) return "keep_label: must be 0 .. 255, or -1 to leave the bytes";
    if (drop_label < -1 || drop_label > 255) return "drop_label: must be 0 .. 255, or -1 to leave the bytes";
    if (label_step != 0 && label_step != 1) return "label_step: must be 0 or 1";
    if (label_step == 1) {
        if (keep_label < 0) return "label_step 1 needs a keep_label";
        if (max_islands < 1) return "label_step 1 needs max_islands >= 1";
        if (max_islands - 1 > 255 - keep_label) return "label_step 1 needs keep_label + max_islands - 1 <= 255";
    }
    if (spare_border != 0 && spare_border != 1) return "spare_border: must be 0 or 1";
    if (flags & ~kIslandsMeasure) return "flags: unknown bits";
    if (reserved != 0) return "reserved: must be 0";
    for (int c = 0; c < 3; ++c)
        if (dims[c] < 1) return "the volume is empty";
    VoxelBox box;
    const BoxVerdict v = box_resolve(dims, origin, extent, true, &box, nullptr);
    if (v.what != BOX_OK) return box_refusal_text(v.what, true);
    for (int c = 0; c < 3; ++c) { box_origin[c] = box.origin[c]; box_end[c] = box.end[c]; }
    return nullptr;
}

} // namespace tbrm
