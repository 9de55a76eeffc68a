// tbrm_compete_plan.h — the rules of competitive growing (include/tbrm_compete.h) that the host and the kernels
// share, stated once: the validation of a call's numbers, the code of a float voxel, the weight of a step, key packing and the
// scratch size. No device, no handle; integer arithmetic and one float rule that also compile as plain host C++:
// tests/cpp/compete_plan_test.cpp checks them against a voxel-by-voxel restatement under the sanitizers.
#pragma once
#include <math.h>

#include "tbrm_box.h"

namespace tbrm {

constexpr uint32_t kCompeteMaxCost = 0xFFFFFFu;   // 2^24 - 1: a key is (cost << 8) | label in one 32-bit word
constexpr uint32_t kCompeteUnreached = 0xFFFFFFFFu; // the word of a voxel nothing has reached: the largest key, so min() needs no special case
constexpr int kCompeteMaxStepCost = 65535, kCompeteMaxShift = 16;
constexpr uint32_t kCompeteMaxCode = 65535u;

// ---- validation ----------------------------------------------------------------------------------------------------------------------
enum CompeteRefusal : int {
    COMPETE_OK = 0, COMPETE_CONNECTIVITY, COMPETE_MEASURE, COMPETE_STEP_COST, COMPETE_SHIFT, COMPETE_LIMIT, COMPETE_RESERVED, COMPETE_RANGE,
    COMPETE_RANGE_CODES, COMPETE_RANGE_FLOAT, COMPETE_FLOAT_SCALE, COMPETE_FLOAT_ORIGIN
};
struct CompeteVerdict { int what, axis; };

// the numbers of a desc (everything but the box); top: 255 / 65535 for UNORM8 / UNORM16, 0: an R32_FLOAT volume
inline CompeteVerdict compete_arguments(int connectivity, int measure_only, const int32_t step_cost[3], int value_shift, uint32_t cost_limit, int reserved,
                                        double lo, double hi, double top, float float_origin, float float_scale)
{
    if (connectivity != 6) return {COMPETE_CONNECTIVITY, 0};
    if (measure_only != 0 && measure_only != 1) return {COMPETE_MEASURE, 0};
    for (int a = 0; a < 3; ++a)
        if (step_cost[a] < 0 || step_cost[a] > kCompeteMaxStepCost) return {COMPETE_STEP_COST, a};
    if (value_shift < 0 || value_shift > kCompeteMaxShift) return {COMPETE_SHIFT, 0};
    if (cost_limit > kCompeteMaxCost) return {COMPETE_LIMIT, 0};
    if (reserved != 0) return {COMPETE_RESERVED, 0};
    if (!(lo <= hi)) return {COMPETE_RANGE, 0};
    if (top > 0.0) {
        if (!(lo >= 0.0 && hi <= top) || lo != floor(lo) || hi != floor(hi)) return {COMPETE_RANGE_CODES, 0};
    } else {
        if (!isfinite(lo) || !isfinite(hi) || !isfinite((float) lo) || !isfinite((float) hi)) return {COMPETE_RANGE_FLOAT, 0};
        if (!isfinite(float_scale) || !(float_scale > 0.0f)) return {COMPETE_FLOAT_SCALE, 0};
        if (!isfinite(float_origin)) return {COMPETE_FLOAT_ORIGIN, 0};
    }
    return {COMPETE_OK, 0};
}

inline uint32_t compete_limit(uint32_t cost_limit) { return cost_limit == 0u ? kCompeteMaxCost : cost_limit; } // 0: no limit but the key's

// tbrm_host_compete_float_range: false when the range has no codes
inline bool compete_float_range(double lo, double hi, float* origin, float* scale)
{
    if (!isfinite(lo) || !isfinite(hi) || !(hi > lo)) return false;
    const float o = (float) lo, s = (float) (65535.0 / (hi - lo));
    if (!isfinite(o) || !isfinite(s) || !(s > 0.0f)) return false;
    *origin = o;
    *scale = s;
    return true;
}

// ---- codes, weights, keys -----------------------------------------------------------------------------------------------------------
// The code of a float voxel. The subtraction and the multiplication are two float32 operations: on the device the intrinsics
// __fsub_rn / __fmul_rn, which the compiler never contracts into an FMA; on the host two statements (the units that include this
// header are built with -ffp-contract=off). A NaN gives 0 (fmaxf returns its other argument); NaN voxels are walls or sourceless
// seeds, so the value is never used.
TBRM_BOARDS_HD uint32_t compete_float_code(float v, float origin, float scale)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const float d = __fsub_rn(v, origin);
    const float m = __fmul_rn(d, scale);
#else
    volatile float d = v - origin; // (volatile: the difference is rounded to float32 before the product is formed, whatever the flags)
    const float m = d * scale;
#endif
    return (uint32_t) rintf(fminf(fmaxf(m, 0.0f), 65535.0f));
}

// the weight of a step along an axis whose step cost is `step`, between voxels with the codes cu and cv (both <= 65535): < 2^17
TBRM_BOARDS_HD uint32_t compete_weight(uint32_t step, uint32_t cu, uint32_t cv, int shift)
{
    return step + ((cu > cv ? cu - cv : cv - cu) >> shift);
}

TBRM_BOARDS_HD uint32_t compete_key(uint32_t cost, uint32_t label) { return (cost << 8) | label; } // cost <= kCompeteMaxCost
TBRM_BOARDS_HD uint32_t compete_key_cost(uint32_t key) { return key >> 8; }
TBRM_BOARDS_HD uint32_t compete_key_label(uint32_t key) { return key & 255u; }

// The key a voxel is offered by a neighbour that holds `from`, over a step of weight w (< 2^17), under `limit` (<= kCompeteMaxCost):
// the sum is formed on costs (< 2^24 + 2^17: no overflow) and packed only when it passes the limit. An unreached neighbour offers
// at best the unreached word itself (w == 0 under the largest limit), which lowers nothing.
TBRM_BOARDS_HD uint32_t compete_offer(uint32_t from, uint32_t w, uint32_t limit)
{
    const uint32_t cost = compete_key_cost(from) + w;
    return cost <= limit ? compete_key(cost, compete_key_label(from)) : kCompeteUnreached;
}

// ---- the scratch ---------------------------------------------------------------------------------------------------------------------
constexpr int kCompeteMaxBatch = 64;
// the control words of a call: 64-bit counts, then 32-bit words
enum CompeteCount : int { COMPETE_SEEDS, COMPETE_CLAIMABLE, COMPETE_CLAIMED, COMPETE_RELABELLED, COMPETE_VISITS, COMPETE_BRICKS_WRITTEN, COMPETE_PER_LABEL, COMPETE_COUNTS = COMPETE_PER_LABEL + 256 };
enum CompeteCtl : int { COMPETE_MIN_X, COMPETE_MIN_Y, COMPETE_MIN_Z, COMPETE_MAX_X, COMPETE_MAX_Y, COMPETE_MAX_Z, COMPETE_MAX_COST, COMPETE_CHANGED, COMPETE_CTL_WORDS = COMPETE_CHANGED + kCompeteMaxBatch };

// Where the parts lie in one allocation for n_bricks bricks, each part 256-byte aligned:
// [keys: 512 words per brick][claimable: 64 bytes per brick][activity: 2 x 1 word per brick][counts][control words]
struct CompeteLayout { size_t keys, claim, act[2], counts, ctl, bytes; };
inline CompeteLayout compete_layout(uint64_t n_bricks)
{
    CompeteLayout l{};
    size_t off = 0;
    auto part = [&off](size_t n_bytes) { const size_t at = off; off += (n_bytes + 255) / 256 * 256; return at; };
    l.keys = part((size_t) n_bricks * 512 * sizeof(uint32_t));
    l.claim = part((size_t) n_bricks * 64);
    l.act[0] = part((size_t) n_bricks * sizeof(uint32_t));
    l.act[1] = part((size_t) n_bricks * sizeof(uint32_t));
    l.counts = part((size_t) COMPETE_COUNTS * sizeof(uint64_t));
    l.ctl = part((size_t) COMPETE_CTL_WORDS * sizeof(int32_t));
    l.bytes = off;
    return l;
}
// ... of the bricks a box touches
inline size_t compete_scratch_bytes(const VoxelBox& box)
{
    BrickRange r{};
    for (int c = 0; c < 3; ++c) axis_bricks(box.origin[c], box.end[c], r.b0[c], r.nb[c]);
    return compete_layout(range_bricks(r)).bytes;
}

} // namespace tbrm
