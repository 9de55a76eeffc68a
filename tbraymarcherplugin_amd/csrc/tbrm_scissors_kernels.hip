// tbrm_scissors_kernels.hip — view-space scissors (include/tbrm_scissors.h): the set M of the voxels under a screen
// mask, combined with the source set of board 0 into board 1. Everything is integer arithmetic but the estimate of a quotient, which an
// integer correction settles (tbrm_scissors_plan.h: scissors_quotient).
//
// The mask summary: k_scissors_cells classes every cell of 32 x 8 pixels (full, clear or neither) into a table with a zero border,
// k_scissors_scan_x and k_scissors_scan_y turn it into a summed-area table of both counts, a wave per row and per column. A rectangle
// of pixels is then all set / all clear when the cells it touches all are: four reads.
//
// k_scissors: a wave per brick of the range, lane l on the x row (y, z) = (l & 7, l >> 3) (tbrm_brick_boards.h).
//   1. the verdict from S alone: an empty board stays empty under an erase, a full one full under a fill;
//   2. the verdict from the corners: lane l projects corner l & 7 of the brick's in-volume part, the wave reduces the extremes, and
//      scissors_verdict says inside, outside or neither;
//   3. otherwise every voxel: U, V, W at the row's start are three 64-bit dot products and advance along x by additions; a voxel in
//      view and in frame costs two quotients and one word of the mask.
// Inside its launch nothing that is read is written: board 0, its class, the mask and the summary in; board 1 and its class out.
//
// All stores are ordinary vector stores and vector atomics in plain HIP.
#include "tbrm_scissors_kernels.h"

namespace tbrm {

namespace {

constexpr int kScissorsThreads = 256; // four bricks to a workgroup, a wave each

__device__ __forceinline__ ScissorsCell wave_prefix(ScissorsCell v, int lane) // inclusive, over the wave
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t f = __shfl_up(v.full, o, 64), c = __shfl_up(v.clear, o, 64);
        if (lane >= o) { v.full += f; v.clear += c; }
    }
    return v;
}

} // namespace

// ---- the mask summary -----------------------------------------------------------------------------------------------------------------
// a thread per entry of the table: the border is 0, entry (cy + 1, cx + 1) the class of cell (cy, cx)
__global__ __launch_bounds__(kScissorsThreads) void k_scissors_cells(const ScissorsParams p)
{
    const int pitch = p.cells_x + 1;
    const uint32_t e = blockIdx.x * kScissorsThreads + threadIdx.x;
    if (e >= (uint32_t) pitch * (uint32_t) (p.cells_y + 1)) return;
    const int ey = (int) (e / (uint32_t) pitch), ex = (int) (e % (uint32_t) pitch);
    ScissorsCell cell{0u, 0u};
    if (ex > 0 && ey > 0) {
        const int cx = ex - 1, y0 = (ey - 1) * kScissorsCellRows;
        const int in_frame = p.rows.width - cx * 32; // >= 1
        const uint32_t frame = in_frame >= 32 ? ~0u : (1u << in_frame) - 1u;
        uint32_t every = ~0u, any = 0u;
        for (int j = 0; j < kScissorsCellRows && y0 + j < p.rows.height; ++j) {
            const uint32_t w = p.mask[(size_t) (y0 + j) * (size_t) p.row_words + (size_t) cx];
            every &= w;
            any |= w;
        }
        cell.full = (every & frame) == frame;
        cell.clear = (any & frame) == 0u;
    }
    p.summary[e] = cell;
}

// a wave per row of cells: the inclusive prefix along x, 64 entries at a time with a carry
__global__ __launch_bounds__(kScissorsThreads) void k_scissors_scan_x(const ScissorsParams p)
{
    const int lane = threadIdx.x & 63, pitch = p.cells_x + 1;
    const int ey = 1 + (int) (blockIdx.x * (kScissorsThreads / 64) + (threadIdx.x >> 6));
    if (ey > p.cells_y) return;
    ScissorsCell* const row = p.summary + (size_t) ey * (size_t) pitch;
    ScissorsCell carry{0u, 0u};
    for (int x0 = 1; x0 <= p.cells_x; x0 += 64) {
        const int ex = x0 + lane;
        ScissorsCell v = ex <= p.cells_x ? row[ex] : ScissorsCell{0u, 0u};
        v = wave_prefix(v, lane);
        v.full += carry.full;
        v.clear += carry.clear;
        if (ex <= p.cells_x) row[ex] = v;
        carry.full = __shfl(v.full, 63, 64);
        carry.clear = __shfl(v.clear, 63, 64);
    }
}

// a wave per column of cells: the same along y
__global__ __launch_bounds__(kScissorsThreads) void k_scissors_scan_y(const ScissorsParams p)
{
    const int lane = threadIdx.x & 63, pitch = p.cells_x + 1;
    const int ex = 1 + (int) (blockIdx.x * (kScissorsThreads / 64) + (threadIdx.x >> 6));
    if (ex > p.cells_x) return;
    ScissorsCell carry{0u, 0u};
    for (int y0 = 1; y0 <= p.cells_y; y0 += 64) {
        const int ey = y0 + lane;
        ScissorsCell* const at = p.summary + (size_t) ey * (size_t) pitch + (size_t) ex; // (formed, read only where ey <= cells_y)
        ScissorsCell v = ey <= p.cells_y ? *at : ScissorsCell{0u, 0u};
        v = wave_prefix(v, lane);
        v.full += carry.full;
        v.clear += carry.clear;
        if (ey <= p.cells_y) *at = v;
        carry.full = __shfl(v.full, 63, 64);
        carry.clear = __shfl(v.clear, 63, 64);
    }
}

hipError_t launch_scissors_summary(const ScissorsParams& p, hipStream_t s)
{
    const uint32_t entries = (uint32_t) (p.cells_x + 1) * (uint32_t) (p.cells_y + 1);
    hipLaunchKernelGGL(k_scissors_cells, dim3((entries + kScissorsThreads - 1) / kScissorsThreads), dim3(kScissorsThreads), 0, s, p);
    hipLaunchKernelGGL(k_scissors_scan_x, dim3((unsigned) (p.cells_y + 3) / 4), dim3(kScissorsThreads), 0, s, p);
    hipLaunchKernelGGL(k_scissors_scan_y, dim3((unsigned) (p.cells_x + 3) / 4), dim3(kScissorsThreads), 0, s, p);
    return hipGetLastError();
}

// ---- the scissors ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kScissorsThreads) void k_scissors(const ScissorsParams p)
{
    const int tid = threadIdx.x, lane = tid & 63;
    WaveBrick wb;
    if (!wave_brick<kScissorsThreads>(p.range, p.bnx, p.bnxy, wb)) return;
    const int bx = wb.bx, by = wb.by, bz = wb.bz, y = wb.y, z = wb.z;
    const size_t b = wb.b;
    const uint32_t vol = row_in_volume(p.dims, bx, y, z);
    const uint32_t S = reinterpret_cast<const uint8_t*>(p.bits + b * 16)[lane];
    unsigned long long* const counts = reinterpret_cast<unsigned long long*>(p.ctl);

    int verdict = SCISSORS_PROJECT;
    bool from_source = false; // the result is S whatever M is
    if (p.skip) {
        const uint32_t c = p.cls[0][b];
        from_source = p.op <= SCISSORS_ERASE_OUTSIDE ? c == MORPH_EMPTY : c == MORPH_FULL;
        if (!from_source) {
            const int cx = scissors_corner(p.dims[0], bx, lane & 1), cy = scissors_corner(p.dims[1], by, (lane >> 1) & 1), cz = scissors_corner(p.dims[2], bz, (lane >> 2) & 1);
            const int64_t W = scissors_dot(p.rows.w, cx, cy, cz);
            ScissorsCorners q;
            q.positive = __popcll(__ballot(W > 0) & 0xffull);
            if (q.positive == 8) {
                const float rcp = scissors_rcp(W);
                q.w_lo = q.w_hi = W;
                q.px0 = q.px1 = scissors_pixel(scissors_dot(p.rows.u, cx, cy, cz), W, rcp, p.rows.width);
                q.py0 = q.py1 = scissors_pixel(scissors_dot(p.rows.v, cx, cy, cz), W, rcp, p.rows.height);
#pragma unroll
                for (int o = 1; o < 8; o <<= 1) { // (every group of eight lanes holds the eight corners)
                    q.w_lo = min(q.w_lo, (int64_t) __shfl_xor((long long) q.w_lo, o, 64));
                    q.w_hi = max(q.w_hi, (int64_t) __shfl_xor((long long) q.w_hi, o, 64));
                    q.px0 = min(q.px0, __shfl_xor(q.px0, o, 64));
                    q.px1 = max(q.px1, __shfl_xor(q.px1, o, 64));
                    q.py0 = min(q.py0, __shfl_xor(q.py0, o, 64));
                    q.py1 = max(q.py1, __shfl_xor(q.py1, o, 64));
                }
            }
            verdict = scissors_verdict(q, p.rows, p.summary, p.cells_x);
        }
    }

    uint32_t M = verdict == SCISSORS_INSIDE ? vol : 0u;
    if (!from_source && verdict == SCISSORS_PROJECT) {
        if (vol) { // (a row outside the volume forms nothing: its y or z is beyond what the bounds cover)
            const int x0 = bx * kBrick;
            // unsigned so that the additions past the volume's last voxel of a ragged row may wrap unseen
            uint64_t Uq = (uint64_t) scissors_dot(p.rows.u, x0, y, z), Vq = (uint64_t) scissors_dot(p.rows.v, x0, y, z), Wq = (uint64_t) scissors_dot(p.rows.w, x0, y, z);
#pragma unroll
            for (int i = 0; i < kBrick; ++i) {
                const int64_t U = (int64_t) Uq, V = (int64_t) Vq, W = (int64_t) Wq;
                if (((vol >> i) & 1u) && W > 0 && W >= p.rows.w_min && W <= p.rows.w_max && U >= 0 && V >= 0 && U < (int64_t) p.rows.width * W &&
                    V < (int64_t) p.rows.height * W) {
                    const float rcp = scissors_rcp(W);
                    const int32_t px = scissors_quotient(U, W, rcp, p.rows.width), py = scissors_quotient(V, W, rcp, p.rows.height);
                    const uint32_t word = p.mask[(size_t) py * (size_t) p.row_words + (size_t) (px >> 5)];
                    M |= ((word >> (px & 31)) & 1u) << i;
                }
                Uq += (uint64_t) p.rows.u[0];
                Vq += (uint64_t) p.rows.v[0];
                Wq += (uint64_t) p.rows.w[0];
            }
        }
    }
    if (lane == 0 && !from_source)
        atomicAdd(counts + (verdict == SCISSORS_PROJECT ? (int) MORPH_WINDOWS : (verdict == SCISSORS_INSIDE ? (int) SCISSORS_CTL_INSIDE : (int) SCISSORS_CTL_OUTSIDE)), 1ull);

    store_board_row(p.bits + b * 16 + 8, &p.cls[1][b], lane, from_source ? S : scissors_apply(p.op, S, M, vol), vol);
}

hipError_t launch_scissors(const ScissorsParams& p, hipStream_t s)
{
    const uint64_t total = range_bricks(p.range);
    if (total == 0) return hipSuccess;
    hipLaunchKernelGGL(k_scissors, dim3((unsigned) ((total + 3) / 4)), dim3(kScissorsThreads), 0, s, p);
    return hipGetLastError();
}

} // namespace tbrm
