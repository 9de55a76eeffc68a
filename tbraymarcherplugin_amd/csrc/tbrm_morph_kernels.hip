// tbrm_morph_kernels.hip — binary morphology of the label volume (include/tbrm_morphology.h): the source set from the
// label bytes (k_morph_load), the unit steps (k_morph_steps) and the comparison with the label bytes, the counts and the write
// (k_morph_write).
//
// The boards and their index rules are tbrm_brick_boards.h's. A brick has two boards in the scratch; a
// launch of k_morph_steps reads one of every brick and writes the other of its own brick, so within a launch nothing that is read
// is written: the kernel boundary is the only hand-off between bricks. Bits outside the volume — the padding of ragged edge
// bricks — are never set in a board.
//
// A unit step moves a bit by at most one voxel, so up to 8 steps of a brick depend only on its 3 x 3 x 3 bricks. A workgroup takes
// a brick, builds the 24^3 bit window of those 27 boards in LDS as 576 x rows of 24 bits (row r = z * 24 + y of the window, three
// rows to a thread), iterates the steps there — a workgroup barrier between two — and stores the centre 8^3. A row's step is
//   6:  the row dilated along x | the rows at y - 1, y + 1, z - 1, z + 1
//   26: the OR of the 3 x 3 rows round it, dilated along x
// cut to the volume after every step. What lies outside the window counts as unset: after k steps the rows and bits within k of the
// window's faces are wrong, the centre (8 away) is right for k <= 8. Bricks outside the call's brick range and outside the volume
// are unset too. Erosion is the same loop on the complement inside the volume: erode(S) = ~dilate(~S), so what lies outside the
// volume counts as set and a label on a volume face is not eaten from outside; the boards always hold the set itself.
//
// Every board has a class (empty, full: every in-volume bit set, mixed). A brick whose output the classes give — the working set
// (the set, or its complement when eroding) is full in the brick, or empty in all 27 — is written without a window; in a window an
// empty or full neighbour is not loaded.
//
// All stores are ordinary vector stores and vector atomics in plain HIP.
#include "tbrm_internal.h"

namespace tbrm {

namespace {

constexpr int kMorphWaveThreads = 256; // k_morph_load, k_morph_write: four bricks to a workgroup, a wave each
constexpr int kWin = 24;               // the window's edge in voxels
constexpr int kWinRows = kWin * kWin;  // 576
// k_morph_steps: a workgroup of kStepThreads threads per brick, thread t on the rows t, t + kStepThreads, ... of the window. Measured
// (DESIGN.md §15): 192 (three rows to a thread) and 64 (a wave per brick, nine rows to a lane) do not separate — they differ by what
// two runs of one build differ by, but for the 26-connected dilation by 8, where 192 is 2 % ahead; 576 is 17 - 60 % slower. The others
// build with -DTBRM_MORPH_STEP_THREADS=n (tools/build_variant.py).
#ifndef TBRM_MORPH_STEP_THREADS
#define TBRM_MORPH_STEP_THREADS 192
#endif
constexpr int kStepThreads = TBRM_MORPH_STEP_THREADS;
constexpr int kStepRows = kWinRows / kStepThreads; // rows to a thread
static_assert(kStepThreads % 64 == 0 && kStepRows * kStepThreads == kWinRows, "whole waves, whole rows");

} // namespace

// ---- the source set ---------------------------------------------------------------------------------------------------------------
// A wave per brick of the call's brick range, lane l on the row (y, z) = (l & 7, l >> 3): its 8 label bytes in, one byte of board 0
// out (64 contiguous bytes per wave), and the board's class.
__global__ __launch_bounds__(kMorphWaveThreads) void k_morph_load(const MorphParams p)
{
    __shared__ uint32_t s_source[8];
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < 8) s_source[tid] = p.source[tid];
    __syncthreads();
    WaveBrick w;
    if (!wave_brick<kMorphWaveThreads>(p.range, p.bnx, p.bnxy, w)) return;
    const uint32_t vol = row_in_volume(p.dims, w.bx, w.y, w.z);
    const uint2 l = *reinterpret_cast<const uint2*>(p.labels + w.b * 512 + (size_t) lane * 8);
    store_board_row(p.bits + w.b * 16, &p.cls[0][w.b], lane, row_in_mask(l, s_source) & vol, vol);
}

hipError_t launch_morph_load(const MorphParams& p, hipStream_t s)
{
    const uint64_t total = range_bricks(p.range);
    if (total == 0) return hipSuccess;
    hipLaunchKernelGGL(k_morph_load, dim3((unsigned) ((total + 3) / 4)), dim3(kMorphWaveThreads), 0, s, p);
    return hipGetLastError();
}

// ---- the steps --------------------------------------------------------------------------------------------------------------------
template <int CONN26>
__global__ __launch_bounds__(kStepThreads) void k_morph_steps(const MorphParams p)
{
    __shared__ uint64_t s_stage[27 * 8];        // the 27 boards in working form: [neighbour (dz, dy, dx)][slice]
    __shared__ uint32_t s_win[2][kWinRows];
    __shared__ uint32_t s_cls[27];              // the neighbours' classes in working form
    const int tid = threadIdx.x;
    int bx, by, bz;
    range_brick(p.range, blockIdx.x, bx, by, bz); // (the grid is the brick range)
    const size_t b = grid_index(p.bnx, p.bnxy, bx, by, bz);
    const uint64_t* const in = p.bits + 8 * p.from;
    uint8_t* const out = reinterpret_cast<uint8_t*>(p.bits + b * 16 + 8 * (1 - p.from));
    const uint32_t* const cls_in = p.cls[p.from];
    const bool erode = p.erode != 0;

    // neighbour c = (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1): inside the brick range (which lies inside the volume)?
    auto neighbour = [&](int c, int& nx, int& ny, int& nz) -> bool {
        nx = bx + c % 3 - 1;
        ny = by + (c / 3) % 3 - 1;
        nz = bz + c / 9 - 1;
        return range_holds(p.range, nx, ny, nz);
    };
    uint32_t mine = MORPH_EMPTY;
    if (tid < 27) {
        int nx, ny, nz;
        if (neighbour(tid, nx, ny, nz)) {
            mine = cls_in[grid_index(p.bnx, p.bnxy, nx, ny, nz)];
            if (erode && mine != MORPH_MIXED) mine ^= 1u; // the complement of an empty board is full, of a full one empty
        }
        s_cls[tid] = mine;
    }
    const bool some = __syncthreads_or(mine != MORPH_EMPTY) != 0; // (also: s_cls is written)
    const uint32_t centre = s_cls[13];
    if (centre == MORPH_FULL || !some) { // the working set stays full here, or nothing can reach this brick: no window
        const bool full = (centre == MORPH_FULL) != erode; // of the set itself
        if (tid < 64) out[tid] = full ? (uint8_t) row_in_volume(p.dims, bx, by * kBrick + (tid & 7), bz * kBrick + (tid >> 3)) : (uint8_t) 0;
        if (tid == 0) p.cls[1 - p.from][b] = full ? MORPH_FULL : MORPH_EMPTY;
        return;
    }

    for (int i = tid; i < 27 * 8; i += kStepThreads) {
        const int c = i >> 3, s = i & 7;
        const uint32_t cl = s_cls[c];
        uint64_t w = 0ull;
        if (cl != MORPH_EMPTY) { // (a neighbour outside the range was given the class empty)
            int nx, ny, nz;
            neighbour(c, nx, ny, nz);
            const uint64_t vol = slice_in_volume(p.dims, nx, ny, nz * kBrick + s);
            if (cl == MORPH_FULL) w = vol;
            else {
                w = in[grid_index(p.bnx, p.bnxy, nx, ny, nz) * 16 + s];
                if (erode) w = ~w & vol;
            }
        }
        s_stage[i] = w;
    }
    __syncthreads();

    // this thread's rows and the in-volume bits of each
    uint32_t inside[kStepRows];
    {
        const int x0 = (bx - 1) * kBrick;
        const int lo = max(-x0, 0), hi = min(p.dims[0] - x0, kWin); // hi > lo: the centre brick is in the volume
        const uint32_t xs = ((1u << hi) - 1u) & ~((1u << lo) - 1u);
        const uint8_t* const stage = reinterpret_cast<const uint8_t*>(s_stage);
#pragma unroll
        for (int i = 0; i < kStepRows; ++i) {
            const int r = tid + kStepThreads * i, Y = r % kWin, Z = r / kWin;
            const int gy = (by - 1) * kBrick + Y, gz = (bz - 1) * kBrick + Z;
            inside[i] = (gy >= 0 && gy < p.dims[1] && gz >= 0 && gz < p.dims[2]) ? xs : 0u;
            const int at = (((Z >> 3) * 3 + (Y >> 3)) * 3) * 64 + (Z & 7) * 8 + (Y & 7); // the row's byte in the board at x - 1
            s_win[0][r] = (uint32_t) stage[at] | (uint32_t) stage[at + 64] << 8 | (uint32_t) stage[at + 128] << 16;
        }
    }
    __syncthreads();

    const int steps = min(max(p.steps, 1), 8);
    for (int step = 0; step < steps; ++step) {
        const uint32_t* const cur = s_win[step & 1];
        uint32_t* const nxt = s_win[(step + 1) & 1];
#pragma unroll
        for (int i = 0; i < kStepRows; ++i) {
            const int r = tid + kStepThreads * i, Y = r % kWin, Z = r / kWin;
            uint32_t v;
            if constexpr (!CONN26) {
                const uint32_t c = cur[r];
                v = c | (c << 1) | (c >> 1);
                if (Y > 0) v |= cur[r - 1];
                if (Y < kWin - 1) v |= cur[r + 1];
                if (Z > 0) v |= cur[r - kWin];
                if (Z < kWin - 1) v |= cur[r + kWin];
            } else {
                uint32_t o = 0u;
#pragma unroll
                for (int dz = -1; dz <= 1; ++dz) {
                    if (Z + dz < 0 || Z + dz >= kWin) continue;
#pragma unroll
                    for (int dy = -1; dy <= 1; ++dy)
                        if (Y + dy >= 0 && Y + dy < kWin) o |= cur[r + dz * kWin + dy];
                }
                v = o | (o << 1) | (o >> 1);
            }
            nxt[r] = v & inside[i]; // (inside has no bit beyond 23)
        }
        __syncthreads();
    }

    uint32_t row = 0u, vol = 0u;
    if (tid < 64) {
        const int y = tid & 7, s = tid >> 3;
        vol = row_in_volume(p.dims, bx, by * kBrick + y, bz * kBrick + s);
        row = (s_win[steps & 1][(kBrick + s) * kWin + kBrick + y] >> kBrick) & 0xffu;
        if (erode) row = ~row & vol;
        out[tid] = (uint8_t) row;
    }
    const bool any = __syncthreads_or(row != 0u) != 0, all = __syncthreads_and(row == vol) != 0;
    if (tid == 0) {
        p.cls[1 - p.from][b] = board_class(any, all);
        atomicAdd(reinterpret_cast<unsigned long long*>(p.ctl) + MORPH_WINDOWS, 1ull);
    }
}

hipError_t launch_morph_steps(const MorphParams& p, hipStream_t s)
{
    const uint64_t total = range_bricks(p.range);
    if (total == 0) return hipSuccess;
    if (p.conn26) hipLaunchKernelGGL(k_morph_steps<1>, dim3((unsigned) total), dim3(kStepThreads), 0, s, p);
    else hipLaunchKernelGGL(k_morph_steps<0>, dim3((unsigned) total), dim3(kStepThreads), 0, s, p);
    return hipGetLastError();
}

// ---- the comparison and the write ---------------------------------------------------------------------------------------------------
// A wave per brick of the box, lane l on the row (l & 7, l >> 3) as above. S: the row's source bits, again from its label bytes;
// R: its byte of board `from`. Inside the box the bits of R \ S whose label is writable join (new_label), those of S \ R leave
// (erase_label); the row is stored where it changes. The counts and the bounding box of what joined or left are reduced over the
// wave: one atomic per wave and quantity that has something to say.
__global__ __launch_bounds__(kMorphWaveThreads) void k_morph_write(const MorphParams p)
{
    __shared__ uint32_t s_source[8], s_writable[8];
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < 8) { s_source[tid] = p.source[tid]; s_writable[tid] = p.writable[tid]; }
    __syncthreads();
    WaveBrick w;
    if (!wave_brick<kMorphWaveThreads>(p.wrange, p.bnx, p.bnxy, w)) return;
    const int bx = w.bx, y = w.y, z = w.z;
    const size_t b = w.b;
    const uint32_t box = row_in_box(p.box, bx, y, z); // (the box lies inside the volume)
    uint2* const bytes = reinterpret_cast<uint2*>(p.labels + b * 512 + (size_t) lane * 8);
    const uint2 old = *bytes;
    const uint32_t S = row_in_mask(old, s_source) & box;
    const uint32_t R = (uint32_t) reinterpret_cast<const uint8_t*>(p.bits + b * 16 + 8 * p.from)[lane] & box;
    const uint32_t joins = R & ~S & row_in_mask(old, s_writable), leaves = S & ~R, moved = joins | leaves;

    int changed = 0;
    if (p.new_label >= 0 && moved) {
        uint2 l = old;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (!((moved >> i) & 1u)) continue;
            const uint32_t to = (uint32_t) (((joins >> i) & 1u) ? p.new_label : p.erase_label);
            changed += byte_of(l, i) != to;
            set_byte(l, i, to);
        }
        if (changed) *bytes = l;
    }
    int n[5] = {(int) __popc(S), (int) __popc(R), (int) __popc(joins), (int) __popc(leaves), changed};
    WaveBounds bounds;
    bounds.take_row(moved, bx, y, z);
    const bool wrote = __ballot(changed != 0) != 0ull;
    if (__ballot((S | R) != 0u) == 0ull) return; // nothing to count (and then nothing moved)
#pragma unroll
    for (int c = 0; c < 5; ++c) n[c] = wave_sum(n[c]);
    bounds.reduce();
    if (lane == 0) {
        unsigned long long* const counts = reinterpret_cast<unsigned long long*>(p.ctl);
#pragma unroll
        for (int c = 0; c < 5; ++c)
            if (n[c]) atomicAdd(counts + MORPH_SOURCE + c, (unsigned long long) n[c]);
        if (wrote) atomicAdd(counts + MORPH_BRICKS_WRITTEN, 1ull);
    }
    bounds.commit(p.ctl + MORPH_MIN_X, lane);
}

hipError_t launch_morph_write(const MorphParams& p, hipStream_t s)
{
    const uint64_t total = range_bricks(p.wrange);
    if (total == 0) return hipSuccess;
    hipLaunchKernelGGL(k_morph_write, dim3((unsigned) ((total + 3) / 4)), dim3(kMorphWaveThreads), 0, s, p);
    return hipGetLastError();
}

} // namespace tbrm
