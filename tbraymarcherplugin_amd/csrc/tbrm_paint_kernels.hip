// tbrm_paint_kernels.hip — the 3D paint brush (include/tbrm_paint.h): the set M of the voxels within a stroke's
// segments (and inside the gate), combined with the source set of board 0 into board 1. Everything is integer arithmetic
// (tbrm_paint_plan.h: paint_within is the rule, paint_row_within a row of it).
//
// k_paint: a wave per brick of the range (the bricks of the work box), lane l on the x row (y, z) = (l & 7, l >> 3)
// (tbrm_brick_boards.h).
//   1. culling: lane r tests run r's grown box against the brick's in-volume part (a stroke has at most 64 runs); for every run that
//      meets it, lane j tests the box of the run's segment j. The survivors of a run are the ballot word of that test, kept by lane r:
//      one word per run, so there is no list that could overflow and nothing is ever truncated. No survivor: the brick is untouched.
//   2. the whole-brick verdict, in the same step: a lane whose segment survives also tests the brick's eight corner voxels against it;
//      all eight within that one segment put the whole brick in the stamp (the set is convex) and end the culling.
//   3. otherwise every voxel: a lane tests its row against every survivor, ee and de advancing along x by additions. The survivor
//      words are made wave-uniform first, so a segment is fetched once per wave.
//   4. the gate, read only by bricks the stroke reaches: the row's 8 stored values against lo .. hi (row_values, row_gate).
// With skip == 0 there is neither culling nor verdict: every row is tested against every segment of the stroke.
// Inside its launch nothing that is read is written: board 0, the data volume, the segments and the runs in; board 1 and its class out.
//
// All stores are ordinary vector stores and vector atomics in plain HIP.
#include "tbrm_paint_kernels.h"

namespace tbrm {

namespace {

constexpr int kPaintThreads = 256; // four bricks to a workgroup, a wave each
enum : int { PAINT_EVALUATE = 0, PAINT_WHOLE = 1, PAINT_UNTOUCHED = 2 };

} // namespace

template <int FMT>
__global__ __launch_bounds__(kPaintThreads) void k_paint(const PaintParams p)
{
    const int tid = threadIdx.x, lane = tid & 63;
    WaveBrick wb;
    if (!wave_brick<kPaintThreads>(p.range, p.bnx, p.bnxy, wb)) return;
    const int bx = wb.bx, by = wb.by, bz = wb.bz, x0 = bx * kBrick, y = wb.y, z = wb.z;
    const size_t b = wb.b;
    const uint32_t vol = row_in_volume(p.dims, bx, y, z);
    const uint32_t S = reinterpret_cast<const uint8_t*>(p.bits + b * 16)[lane];
    unsigned long long* const counts = reinterpret_cast<unsigned long long*>(p.ctl);
    const int64_t limit = p.limit;

    int verdict = PAINT_EVALUATE;
    uint32_t M = 0u;
    if (!p.skip) {
        if (vol) // (a row outside the volume forms nothing)
            for (int s = 0; s < p.n_segs; ++s) M |= paint_row_within(p.segs[s], p.w, limit, x0, y, z);
    } else {
        // the brick's in-volume part
        const int32_t blo[3] = {x0, by * kBrick, bz * kBrick};
        const int32_t bhi[3] = {paint_corner(p.dims[0], bx, 1), paint_corner(p.dims[1], by, 1), paint_corner(p.dims[2], bz, 1)};
        bool run_meets = false;
        if (lane < p.n_runs) run_meets = paint_boxes_meet(p.runs[lane].lo, p.runs[lane].hi, blo, bhi);
        const unsigned long long met = __ballot(run_meets);
        unsigned long long mine = 0ull; // lane r: the survivors of run r
        bool whole = false, any = false;
        for (unsigned long long rm = met; rm != 0ull && !whole; rm &= rm - 1ull) {
            const int r = __ffsll((long long) rm) - 1;
            const int first = p.runs[r].first, count = p.runs[r].count;
            bool survives = false, holds = false;
            if (lane < count) {
                const PaintSegment& g = p.segs[first + lane];
                survives = paint_boxes_meet(g.lo, g.hi, blo, bhi);
                holds = survives && paint_corners_within(g, p.w, limit, blo, bhi);
            }
            whole = __ballot(holds) != 0ull;
            const unsigned long long m = __ballot(survives);
            if (lane == r) mine = m;
            any = any || m != 0ull;
        }
        if (whole) {
            verdict = PAINT_WHOLE;
            M = vol;
        } else if (!any) {
            verdict = PAINT_UNTOUCHED;
        } else {
            for (unsigned long long rm = met; rm != 0ull; rm &= rm - 1ull) {
                const int r = __ffsll((long long) rm) - 1;
                const unsigned long long mv = (unsigned long long) __shfl((long long) mine, r, 64);
                // the same word in every lane: say so, and the segment below is fetched once for the wave (the builtin returns an
                // int: through uint32_t, or a survivor in lane 31 would extend its sign over the upper half)
                const uint32_t m_lo = (uint32_t) __builtin_amdgcn_readfirstlane((int) (uint32_t) mv);
                const uint32_t m_hi = (uint32_t) __builtin_amdgcn_readfirstlane((int) (uint32_t) (mv >> 32));
                unsigned long long m = (unsigned long long) m_lo | ((unsigned long long) m_hi << 32);
                const int first = p.runs[r].first;
                for (; m != 0ull; m &= m - 1ull) {
                    const int j = __ffsll((long long) m) - 1;
                    if (vol) M |= paint_row_within(p.segs[first + j], p.w, limit, x0, y, z);
                }
            }
        }
    }
    M &= vol;
    if constexpr (FMT != kPaintNoGate) {
        if (verdict != PAINT_UNTOUCHED) {
            uint32_t c[8];
            float f[8];
            row_values<FMT>(p.data, b * 512 + (size_t) lane * 8, c, f);
            M &= row_gate<FMT>(c, f, p.lo_code, p.hi_code, p.lo_f, p.hi_f);
        }
    }

    const int stamp = wave_sum((int) __popc(M & row_in_box(p.work, bx, y, z)));
    if (lane == 0) {
        if (stamp) atomicAdd(counts + PAINT_CTL_STAMP, (unsigned long long) stamp);
        atomicAdd(counts + (verdict == PAINT_EVALUATE ? (int) MORPH_WINDOWS : (verdict == PAINT_WHOLE ? (int) PAINT_CTL_WHOLE : (int) PAINT_CTL_UNTOUCHED)), 1ull);
    }

    store_board_row(p.bits + b * 16 + 8, &p.cls[1][b], lane, paint_apply(p.op, S, M), vol);
}

hipError_t launch_paint(const PaintParams& p, hipStream_t s)
{
    const uint64_t total = range_bricks(p.range);
    if (total == 0) return hipSuccess;
    const dim3 grid((unsigned) ((total + 3) / 4)), block(kPaintThreads);
    switch (p.fmt) {
        case FMT_U8: hipLaunchKernelGGL(k_paint<FMT_U8>, grid, block, 0, s, p); break;
        case FMT_U16: hipLaunchKernelGGL(k_paint<FMT_U16>, grid, block, 0, s, p); break;
        case FMT_F32: hipLaunchKernelGGL(k_paint<FMT_F32>, grid, block, 0, s, p); break;
        default: hipLaunchKernelGGL(k_paint<kPaintNoGate>, grid, block, 0, s, p); break;
    }
    return hipGetLastError();
}

} // namespace tbrm
