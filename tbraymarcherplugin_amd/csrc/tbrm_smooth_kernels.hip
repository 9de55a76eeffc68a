// tbrm_smooth_kernels.hip — smoothing of labels (include/tbrm_smooth.h): a rank filter over a box, from one bit board
// to the other. Morphology and margins ask "is there a set voxel within reach"; this asks "how many": it counts.
//
// c(v), the set voxels of the window [v - r, v + r], separates per axis:
//   cx(x, y, z) = the set bits of the row (y, z) within r_x of x           one popcount of a row word under a window mask
//   cy(x, y, z) = sum over |y - j| <= r_y of cx(x, j, z)                   <= 33^2: 16 bits
//   c (x, y, z) = sum over |z - j| <= r_z of cy(x, y, j)                   <= 33^3: 16 bits
// Bits outside the volume and bricks outside the call's range are unset in every row word, so the sums never count them; n(v), the
// voxels of the window that lie inside the volume, is the product of the three clipped extents (clipped_extent) and is not stored.
// The result bit is c * rank_den > n * rank_num, in 32 bits (include/tbrm_smooth.h's bounds).
//
// One launch per pass, a workgroup per brick of the range; inside it nothing that is read is written: k_smooth_count reads board
// `from` and its classes of every brick, and writes the other board and its class of its own brick. A brick whose result the classes
// of its neighbourhood give writes that board without counting.
//
// All stores are ordinary vector stores and vector atomics in plain HIP.
#include "tbrm_smooth_kernels.h"

namespace tbrm {

namespace {

constexpr int kSmoothThreads = 256; // a workgroup per brick: two voxels to a thread

__device__ __forceinline__ bool axis_holds(const BrickRange& r, int c, int b) { return b >= r.b0[c] && b < r.b0[c] + r.nb[c]; }

} // namespace

// LDS: [K][J] the x counts of the rows y0 - r_y + J, z0 - r_z + K of the brick's 8 columns, a byte each (8 bytes a row: 12.5 KiB at
// radius 16), then [K][y][x] the y sums as uint16 (5 KiB at radius 16). The row words themselves live in registers only: the thread
// that assembles a row is the one that counts it.
__global__ __launch_bounds__(kSmoothThreads) void k_smooth_count(const SmoothParams p)
{
    extern __shared__ uint2 s_smooth[];
    const int tid = threadIdx.x, lane = tid & 63;
    int bx, by, bz;
    range_brick(p.range, blockIdx.x, bx, by, bz); // (the grid is the brick range)
    const size_t b = grid_index(p.bnx, p.bnxy, bx, by, bz);
    uint64_t* const out = p.bits + b * 16 + 8 * (1 - p.from);

    // Every brick of the volume within kb[a] bricks per axis full: c = n for each voxel, the brick stays full; all of them empty:
    // c = 0, it stays empty — for every admissible rank. A brick outside the volume has no vote (the window is clipped); one inside
    // the volume and outside the range is staged as unset below, so it counts as empty here too.
    if (p.skip) {
        const int sx = 2 * p.kb[0] + 1, sy = 2 * p.kb[1] + 1, sz = 2 * p.kb[2] + 1; // at most 5 each
        bool full = true, empty = true;
        if (tid < sx * sy * sz) {
            const int cx = bx - p.kb[0] + tid % sx, cy = by - p.kb[1] + (tid / sx) % sy, cz = bz - p.kb[2] + tid / (sx * sy);
            if (cx >= 0 && cy >= 0 && cz >= 0 && cx * kBrick < p.dims[0] && cy * kBrick < p.dims[1] && cz * kBrick < p.dims[2]) {
                const uint32_t c = range_holds(p.range, cx, cy, cz) ? p.cls[p.from][grid_index(p.bnx, p.bnxy, cx, cy, cz)] : (uint32_t) MORPH_EMPTY;
                full = c == MORPH_FULL;
                empty = c == MORPH_EMPTY;
            }
        }
        const bool all_full = __syncthreads_and(full) != 0, all_empty = __syncthreads_and(empty) != 0;
        if (all_full || all_empty) {
            if (tid < kBrick) out[tid] = all_full ? slice_in_volume(p.dims, bx, by, bz * kBrick + tid) : 0ull;
            if (tid == 0) p.cls[1 - p.from][b] = all_full ? MORPH_FULL : MORPH_EMPTY;
            return;
        }
    }
    if (tid == 0) atomicAdd(reinterpret_cast<unsigned long long*>(p.ctl) + MORPH_WINDOWS, 1ull);

    const int rx = p.radius[0], ry = p.radius[1], rz = p.radius[2];
    const int NY = kBrick + 2 * ry, NZ = kBrick + 2 * rz;
    uint2* const s_x = s_smooth;
    uint16_t* const s_y = reinterpret_cast<uint16_t*>(s_smooth + NY * NZ);
    const uint8_t* const boards = reinterpret_cast<const uint8_t*>(p.bits);

    // ---- x: a row word (row_window: the brick's byte at the bits 16 .. 23, up to two bricks either side), eight popcounts
    for (int r = tid; r < NY * NZ; r += kSmoothThreads) {
        const int K = r / NY, J = r - K * NY;
        const int gy = by * kBrick - ry + J, gz = bz * kBrick - rz + K;
        uint2 counts = make_uint2(0u, 0u);
        if (gy >= 0 && gy < p.dims[1] && gz >= 0 && gz < p.dims[2]) {
            const int nby = gy >> kBrickShift, nbz = gz >> kBrickShift;
            if (axis_holds(p.range, 1, nby) && axis_holds(p.range, 2, nbz)) {
                const size_t at = (size_t) (p.from * 64 + (gz & 7) * kBrick + (gy & 7)); // the row's byte in a board
                uint64_t w = 0ull;
                for (int j = -p.kb[0]; j <= p.kb[0]; ++j)
                    if (axis_holds(p.range, 0, bx + j))
                        w |= (uint64_t) boards[grid_index(p.bnx, p.bnxy, bx + j, nby, nbz) * 128 + at] << (kRowWordShift + kBrick * j);
                uint32_t d[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) d[i] = (uint32_t) __popcll(w & row_window(i, rx)); // <= 33
                counts.x = d[0] | d[1] << 8 | d[2] << 16 | d[3] << 24;
                counts.y = d[4] | d[5] << 8 | d[6] << 16 | d[7] << 24;
            }
        }
        s_x[r] = counts;
    }
    __syncthreads();

    // ---- y: four columns to an item, as two pairs of 16-bit sums in one register each (a sum is at most 33 * 33)
    {
        const uint32_t* const sx32 = reinterpret_cast<const uint32_t*>(s_x);
        uint32_t* const sy32 = reinterpret_cast<uint32_t*>(s_y);
        for (int e = tid; e < NZ * 16; e += kSmoothThreads) {
            const int K = e >> 4, y = (e >> 1) & 7, h = e & 1;
            const int base = (K * NY + y) * 2 + h;
            uint32_t a02 = 0u, a13 = 0u; // the columns 4 h + 0 and 4 h + 2; 4 h + 1 and 4 h + 3
            for (int dj = 0; dj <= 2 * ry; ++dj) {
                const uint32_t v = sx32[base + 2 * dj];
                a02 += v & 0x00ff00ffu;
                a13 += (v >> 8) & 0x00ff00ffu;
            }
            const int o = K * 32 + y * 4 + 2 * h;
            sy32[o] = (a02 & 0xffffu) | (a13 << 16);
            sy32[o + 1] = (a02 >> 16) | (a13 & 0xffff0000u);
        }
    }
    __syncthreads();

    // ---- z, and the comparison: a wave's ballot over its 64 voxels is a slice word
    bool any = false, all = true;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int v = tid + kSmoothThreads * h, z = v >> 6, xy = v & 63; // (z = 4 h + tid / 64: one slice to a wave)
        uint32_t c = 0u;
        for (int dk = 0; dk <= 2 * rz; ++dk) c += s_y[(z + dk) * 64 + xy];
        const int gx = bx * kBrick + (xy & 7), gy = by * kBrick + (xy >> 3), gz = bz * kBrick + z;
        const uint32_t n = (uint32_t) (clipped_extent(p.dims[0], gx, rx) * clipped_extent(p.dims[1], gy, ry) * clipped_extent(p.dims[2], gz, rz));
        const uint64_t vol = slice_in_volume(p.dims, bx, by, gz);
        const uint64_t word = __ballot(c * p.rank_den > n * p.rank_num) & vol;
        if (lane == 0) {
            out[z] = word;
            any = any || word != 0ull;
            all = all && word == vol;
        }
    }
    const bool some = __syncthreads_or(any) != 0, every = __syncthreads_and(all) != 0;
    if (tid == 0) p.cls[1 - p.from][b] = board_class(some, every);
}

size_t smooth_lds_bytes(const SmoothParams& p)
{
    const size_t NY = (size_t) (kBrick + 2 * p.radius[1]), NZ = (size_t) (kBrick + 2 * p.radius[2]);
    return NY * NZ * 8 + NZ * 128;
}

hipError_t launch_smooth_count(const SmoothParams& p, hipStream_t s)
{
    const uint64_t total = range_bricks(p.range);
    if (total == 0) return hipSuccess;
    hipLaunchKernelGGL(k_smooth_count, dim3((unsigned) total), dim3(kSmoothThreads), smooth_lds_bytes(p), s, p);
    return hipGetLastError();
}

} // namespace tbrm
