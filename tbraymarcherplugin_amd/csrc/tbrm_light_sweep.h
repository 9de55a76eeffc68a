// tbrm_light_sweep.h — what k_light_sweep (tbrm_light_sweep.hip, compiled as one translation unit per mode)
// and the host-side planner (tbrm_light_plan.cpp) have to agree on: tile shape, LDS budget, hand-off record layout (the index rules: tbrm_sweep_tile.h). Internal.
#pragma once
#include "tbrm_internal.h"
#include "tbrm_sweep_tile.h"

namespace tbrm {

// (the tile, the LDS plane and the staged brick: tbrm_sweep_tile.h)
constexpr int kSweepRing = 8;                          // register ring of requested hand-off words (slices)
constexpr int kSweepComputeWaves = kSweepTile / 4;     // a wave: 32 columns x 4 rows (two rows per lane)
// + the hand-off waves + one factor loader per stream (an LDS-DMA costs its wave 60 - 180 cycles of issue: the eight of a
// two-stream slice in one wave took longer than the slice)
constexpr bool sweep_two_streams(int mode) { return mode == PASS_CHANGE || mode == PASS_ADD2; }
// Hand-off waves per tile: a publisher and a consumer (each slice's chain of LDS read -> convert -> store and of
// load -> decode -> LDS write run side by side instead of one after the other)
constexpr int kSweepHandoffWaves = 2;
constexpr int sweep_threads(int mode) { return (kSweepComputeWaves + kSweepHandoffWaves + (sweep_two_streams(mode) ? 2 : 1)) * 64; }
constexpr int kSweepFlagGroups = 128;                  // slice groups of a span (1024 slices)
constexpr int kSweepFBlock = 256 + 16;                 // floats per staged 16 x 16 block slice of occlusion factors: the four
                                                       // blocks under a tile start 16 banks apart (a lane pair's columns c, c + 16)

// slots of the LDS ring of factor slices; the loader runs one less ahead. Eight for one and for two streams (round 5: with a
// ring of eight a slice's factors land a barrier earlier and the compute waves read them in front of the barrier instead of
// behind it: a fused Change's sweeps 0.63 -> 0.61 ms; rounds 3 and 4 ran two-stream passes with four slots to leave LDS to
// occlusion workgroups beside them, which never paid)
constexpr int kSweepFactorSlots = 8;

constexpr int kSweepBlocks = 2 * (kSweepTile / 16);    // 16 x 16 occlusion blocks under a tile
constexpr int kSweepBricks = 4 * (kSweepTile / 8);     // light-volume bricks under a tile

inline size_t sweep_lds_bytes(int mode, int slices, int lv_fmt)
{
    const int ns = sweep_two_streams(mode) ? 2 : 1;
    const int groups = (slices + 7) / 8; // (the rank table is as long as the pass: every KiB not taken is the occlusion workgroups')
    // planes, three brick layers (UNORM8 light volumes: a float light volume is updated in place), block ranks, the ring of factor slices
    return (size_t) 2 * ns * kSweepPlane * 4 + (lv_fmt == FMT_U8 ? 3 * kSweepBricks * kSweepLvBrick : 0) + (size_t) ns * kSweepBlocks * groups * 4 +
           (size_t) kSweepFactorSlots * ns * kSweepBlocks * kSweepFBlock * 4;
}

inline int sweep_max_slices() { return 8 * kSweepFlagGroups; }

// one translation unit per mode: tbrm_light_sweep.hip compiled with -DTBRM_SWEEP_UNIT_MODE
template <int MODE>
hipError_t launch_sweep_unit(const ChunkParams& p, const SweepParams& q, hipStream_t s);
template <int MODE>
hipError_t launch_sweep_chain_unit(const SweepChainArgs& c, hipStream_t s);

} // namespace tbrm
