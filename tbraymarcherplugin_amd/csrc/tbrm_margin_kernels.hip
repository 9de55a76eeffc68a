// tbrm_margin_kernels.hip — Euclidean margins of labels (include/tbrm_margin.h): a capped, anisotropic, exact
// squared-distance transform from one bit board to the other.
//
// D(v) = min over set u of w_x dx^2 + w_y dy^2 + w_z dz^2 separates per axis. With d1(x, y, z) the distance in voxels along x to the
// nearest set bit of the row (y, z) within the reach n_x (255: none),
//   g(x, y, z) = min over |y - j| <= n_y of w_x d1(x, j, z)^2 + w_y (y - j)^2          (k_margin_xy)
//   D(x, y, z) = min over |z - j| <= n_z of g(x, y, j) + w_z (z - j)^2                 (k_margin_z)
// each cut to TBRM_MARGIN_FAR above `limit` (what exceeds it after two axes exceeds it after three). Under the header's bounds
// (w_a n_a^2 <= limit < 2^31) every sum is below 2^32.
//
// The boards always hold the set itself; a transform works on the working form: the set (expand) or its complement inside the
// volume (shrink). Bits outside the volume and bricks outside the call's range are unset in it. A voxel of the padding of a ragged
// brick is never a source: every axis pass takes its minimum over voxels of the same row, column or pile, and the first starts from
// set bits, which lie inside the volume.
//
// Three launches per transform; inside one, nothing that is read is written:
//   k_margin_states  reads the classes of board `from`                      writes the bricks' states
//   k_margin_xy      reads board `from` and the states                      writes the field g of its own brick
//   k_margin_z       reads the field and the states                         writes board 1 - `from` and its class (or the distance map)
// g is kept as the pair (a, b) = (d1, |y - j|) of a minimum: two bytes a voxel, expanded to w_x a^2 + w_y b^2 when staged.
//
// All stores are ordinary vector stores and vector atomics in plain HIP.
#include "tbrm_margin_kernels.h"

namespace tbrm {

namespace {

constexpr int kMarginThreads = 256;        // a workgroup per brick: two voxels to a thread
constexpr uint32_t kFar = 0xFFFFFFFFu;     // TBRM_MARGIN_FAR
constexpr uint32_t kFarByte = 255u;

__device__ __forceinline__ uint32_t working_class(uint32_t c, int shrink)
{
    return (shrink && c != MORPH_MIXED) ? c ^ 1u : c; // the complement of an empty board is full, of a full one empty
}

__device__ __forceinline__ bool axis_holds(const BrickRange& r, int c, int b) { return b >= r.b0[c] && b < r.b0[c] + r.nb[c]; }

} // namespace

// ---- the bricks' states ---------------------------------------------------------------------------------------------------------------
// A thread per brick of the range. Full in working form: full afterwards. Empty, and every brick within kb[a] bricks per axis empty
// (outside the range: unset): nothing within reach. Everything else is computed, and counted.
__global__ __launch_bounds__(kMarginThreads) void k_margin_states(const MarginParams p)
{
    const uint32_t total = (uint32_t) range_bricks(p.range);
    const uint32_t k = blockIdx.x * kMarginThreads + threadIdx.x;
    bool computed = false;
    if (k < total) {
        int bx, by, bz;
        range_brick(p.range, k, bx, by, bz);
        const uint32_t* const cls = p.cls[p.from];
        const uint32_t own = working_class(cls[grid_index(p.bnx, p.bnxy, bx, by, bz)], p.shrink);
        uint8_t st = MARGIN_FAR_BRICK;
        if (!p.skip || own == MORPH_MIXED) st = MARGIN_COMPUTE;
        else if (own == MORPH_FULL) st = MARGIN_FULL_BRICK;
        else {
            const int x0 = max(bx - p.kb[0], p.range.b0[0]), x1 = min(bx + p.kb[0], p.range.b0[0] + p.range.nb[0] - 1);
            const int y0 = max(by - p.kb[1], p.range.b0[1]), y1 = min(by + p.kb[1], p.range.b0[1] + p.range.nb[1] - 1);
            const int z0 = max(bz - p.kb[2], p.range.b0[2]), z1 = min(bz + p.kb[2], p.range.b0[2] + p.range.nb[2] - 1);
            for (int z = z0; z <= z1 && st == MARGIN_FAR_BRICK; ++z)
                for (int y = y0; y <= y1 && st == MARGIN_FAR_BRICK; ++y)
                    for (int x = x0; x <= x1; ++x)
                        if (working_class(cls[grid_index(p.bnx, p.bnxy, x, y, z)], p.shrink) != MORPH_EMPTY) { st = MARGIN_COMPUTE; break; }
        }
        p.state[k] = st;
        computed = st == MARGIN_COMPUTE;
    }
    const unsigned long long n = __ballot(computed);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(reinterpret_cast<unsigned long long*>(p.ctl) + MORPH_WINDOWS, (unsigned long long) __popcll(n));
}

hipError_t launch_margin_states(const MarginParams& p, hipStream_t s)
{
    const uint64_t total = range_bricks(p.range);
    if (total == 0) return hipSuccess;
    hipLaunchKernelGGL(k_margin_states, dim3((unsigned) ((total + kMarginThreads - 1) / kMarginThreads)), dim3(kMarginThreads), 0, s, p);
    return hipGetLastError();
}

// ---- x from the bits, then y ------------------------------------------------------------------------------------------------------------
// A workgroup per computed brick. It stages d1 of its 8 x columns for the rows y0 - n_y .. y0 + 7 + n_y of its 8 slices in LDS, 8 bytes
// a row: 64 (8 + 2 n_y) bytes, 8.5 KiB at the largest reach. A row's d1 comes from a bit string: the row's byte C of this brick, the
// 64 bits L to its left and the 64 bits R to its right (the same row of up to 8 bricks either side). For the voxel i of the row the
// bits at the distances 0 .. 63 to the left are one 64-bit word, most significant first, and count-leading-zeros is the distance; to
// the right count-trailing-zeros; the distance 64 is one bit of L or R each.
__global__ __launch_bounds__(kMarginThreads) void k_margin_xy(const MarginParams p)
{
    extern __shared__ uint2 s_rows[]; // [z][J][x] bytes, J = y - (y0 - n_y)
    const uint32_t k = blockIdx.x;    // (the grid is the brick range)
    if (p.state[k] != MARGIN_COMPUTE) return;
    const int tid = threadIdx.x;
    int bx, by, bz;
    range_brick(p.range, k, bx, by, bz);
    const int nx = p.reach[0], ny = p.reach[1], NJ = kBrick + 2 * ny;
    const uint8_t* const boards = reinterpret_cast<const uint8_t*>(p.bits);

    for (int r = tid; r < kBrick * NJ; r += kMarginThreads) {
        const int z = r / NJ, J = r - z * NJ;
        const int gy = by * kBrick - ny + J, gz = bz * kBrick + z;
        uint2 out = make_uint2(kFar, kFar); // eight times 255
        const int nby = gy >> kBrickShift;
        if (gy >= 0 && gy < p.dims[1] && gz < p.dims[2] && axis_holds(p.range, 1, nby) &&
            p.state[range_position(p.range, bx, nby, bz)] != MARGIN_FAR_BRICK) {
            const int at = p.from * 64 + z * kBrick + (gy & 7); // the row's byte in a board
            auto row = [&](int cx) -> uint64_t {                // ... of brick column cx, in working form
                if (!axis_holds(p.range, 0, cx)) return 0ull;
                uint32_t v = boards[grid_index(p.bnx, p.bnxy, cx, nby, bz) * 128 + (size_t) at];
                if (p.shrink) v = ~v & row_bits(0, p.dims[0] - cx * kBrick);
                return (uint64_t) v;
            };
            const uint64_t C = row(bx);
            uint64_t L = 0ull, R = 0ull; // bit m of L: the voxel x0 - 64 + m; of R: x0 + 8 + m
            for (int j = 1; j <= p.kb[0]; ++j) {
                L |= row(bx - j) << (8 * (8 - j));
                R |= row(bx + j) << (8 * (j - 1));
            }
            uint32_t d[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const uint64_t wl = (L >> (i + 1)) | (C << (63 - i)); // bit 63 - t: the voxel t to the left
                const uint64_t wr = (C >> i) | (R << (8 - i));        // bit t: the voxel t to the right
                uint32_t dl = wl ? (uint32_t) __clzll((long long) wl) : kFarByte;
                uint32_t dr = wr ? (uint32_t) (__ffsll((long long) wr) - 1) : kFarByte;
                if ((L >> i) & 1ull) dl = min(dl, 64u);
                if ((R >> (56 + i)) & 1ull) dr = min(dr, 64u);
                const uint32_t m = min(dl, dr);
                d[i] = m <= (uint32_t) nx ? m : kFarByte;
            }
            out.x = d[0] | d[1] << 8 | d[2] << 16 | d[3] << 24;
            out.y = d[4] | d[5] << 8 | d[6] << 16 | d[7] << 24;
        }
        s_rows[r] = out;
    }
    __syncthreads();

    const uint8_t* const d1 = reinterpret_cast<const uint8_t*>(s_rows);
    uint16_t* const field = p.field + (size_t) k * 512;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int v = tid + kMarginThreads * h, x = v & 7, y = (v >> 3) & 7, z = v >> 6;
        const int base = (z * NJ + y + ny) * kBrick + x;
        uint32_t best = kFar, ba = kFarByte, bb = 0u;
        for (int dj = 0; dj <= ny; ++dj) {
            const uint32_t wj = p.w[1] * (uint32_t) (dj * dj); // <= limit
            if (wj >= best) break;                             // nothing further away along y is nearer
            const uint32_t a0 = d1[base - dj * kBrick], a1 = d1[base + dj * kBrick];
            if (a0 != kFarByte) { const uint32_t c = p.w[0] * a0 * a0 + wj; if (c < best) { best = c; ba = a0; bb = (uint32_t) dj; } }
            if (a1 != kFarByte) { const uint32_t c = p.w[0] * a1 * a1 + wj; if (c < best) { best = c; ba = a1; bb = (uint32_t) dj; } }
        }
        if (best > p.limit) { ba = kFarByte; bb = 0u; }
        field[v] = (uint16_t) (ba | bb << 8);
    }
}

hipError_t launch_margin_xy(const MarginParams& p, hipStream_t s)
{
    const uint64_t total = range_bricks(p.range);
    if (total == 0) return hipSuccess;
    const size_t lds = (size_t) 64 * (size_t) (kBrick + 2 * p.reach[1]);
    hipLaunchKernelGGL(k_margin_xy, dim3((unsigned) total), dim3(kMarginThreads), lds, s, p);
    return hipGetLastError();
}

// ---- z, and the threshold ---------------------------------------------------------------------------------------------------------------
// A workgroup per brick of the launch's layers. A computed brick stages g of its 64 piles for the slices z0 - n_z .. z0 + 7 + n_z in
// LDS, 256 (8 + 2 n_z) bytes, 34 KiB at the largest reach (four workgroups to a CU's 160 KiB); a neighbour that was not computed gives
// 0 (full, inside the volume) or FAR. Board form: a wave's ballot of "within the limit" over its 64 voxels is a slice word; it is
// cut to the volume, complemented back for a shrink, and stored by one lane. Map form: the voxels of the box in the slices [z0, z1)
// get their distance.
template <bool MAP>
__global__ __launch_bounds__(kMarginThreads) void k_margin_z(const MarginParams p)
{
    extern __shared__ uint32_t s_g[]; // [slice][y][x]
    const int tid = threadIdx.x, lane = tid & 63;
    const uint32_t k = (uint32_t) p.layer0 * (uint32_t) (p.range.nb[0] * p.range.nb[1]) + blockIdx.x;
    int bx, by, bz;
    range_brick(p.range, k, bx, by, bz);
    const size_t b = grid_index(p.bnx, p.bnxy, bx, by, bz);
    const uint8_t st = p.state[k];
    const int nz = p.reach[2], NS = kBrick + 2 * nz;
    uint64_t* const out = p.bits + b * 16 + 8 * (1 - p.from);

    auto map_store = [&](int v, uint32_t value) { // voxel v = z * 64 + y * 8 + x of this brick
        const int gx = bx * kBrick + (v & 7), gy = by * kBrick + ((v >> 3) & 7), gz = bz * kBrick + (v >> 6);
        if (gx < p.box.origin[0] || gx >= p.box.end[0] || gy < p.box.origin[1] || gy >= p.box.end[1] || gz < p.z0 || gz >= p.z1) return;
        const size_t ex = (size_t) (p.box.end[0] - p.box.origin[0]), ey = (size_t) (p.box.end[1] - p.box.origin[1]);
        p.dist[((size_t) (gz - p.z0) * ey + (size_t) (gy - p.box.origin[1])) * ex + (size_t) (gx - p.box.origin[0])] = value;
    };

    if (st != MARGIN_COMPUTE) { // the classes gave it: full or empty in working form
        const bool full = st == MARGIN_FULL_BRICK;
        if constexpr (MAP) {
#pragma unroll
            for (int h = 0; h < 2; ++h) map_store(tid + kMarginThreads * h, full ? 0u : kFar); // (the box lies inside the volume)
        } else {
            const bool set_full = full != (p.shrink != 0); // of the set itself
            if (tid < kBrick) out[tid] = set_full ? slice_in_volume(p.dims, bx, by, bz * kBrick + tid) : 0ull;
            if (tid == 0) p.cls[1 - p.from][b] = set_full ? MORPH_FULL : MORPH_EMPTY;
        }
        return;
    }

    for (int e = tid; e < NS * 64; e += kMarginThreads) {
        const int s = e >> 6, xy = e & 63;
        const int gz = bz * kBrick - nz + s, nbz = gz >> kBrickShift;
        uint32_t val = kFar;
        if (gz >= 0 && gz < p.dims[2] && axis_holds(p.range, 2, nbz)) {
            const uint32_t kk = range_position(p.range, bx, by, nbz);
            const uint8_t sn = p.state[kk];
            if (sn == MARGIN_COMPUTE) {
                const uint32_t pair = p.field[(size_t) kk * 512 + (size_t) ((gz & 7) * 64 + xy)];
                const uint32_t a = pair & 255u, bb = pair >> 8;
                if (a != kFarByte) val = p.w[0] * a * a + p.w[1] * bb * bb; // <= limit
            } else if (sn == MARGIN_FULL_BRICK) {
                if (bx * kBrick + (xy & 7) < p.dims[0] && by * kBrick + (xy >> 3) < p.dims[1]) val = 0u;
            }
        }
        s_g[e] = val;
    }
    __syncthreads();

    bool any = false, all = true;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int v = tid + kMarginThreads * h, z = v >> 6, xy = v & 63;
        const int base = (z + nz) * 64 + xy;
        uint32_t best = kFar;
        for (int dj = 0; dj <= nz; ++dj) {
            const uint32_t wj = p.w[2] * (uint32_t) (dj * dj); // <= limit
            if (wj >= best) break;
            const uint32_t f0 = s_g[base - dj * 64], f1 = s_g[base + dj * 64];
            if (f0 != kFar) best = min(best, f0 + wj); // (f <= limit < 2^31, wj <= limit)
            if (f1 != kFar) best = min(best, f1 + wj);
        }
        if (best > p.limit) best = kFar;
        if constexpr (MAP) map_store(v, best);
        else {
            const uint64_t vol = slice_in_volume(p.dims, bx, by, bz * kBrick + z); // (z = 4 h + tid / 64: one slice to a wave)
            uint64_t word = __ballot(best != kFar) & vol;
            if (p.shrink) word = ~word & vol;
            if (lane == 0) {
                out[z] = word;
                any = any || word != 0ull;
                all = all && word == vol;
            }
        }
    }
    if constexpr (!MAP) {
        const bool some = __syncthreads_or(any) != 0, every = __syncthreads_and(all) != 0;
        if (tid == 0) p.cls[1 - p.from][b] = board_class(some, every);
    }
}

hipError_t launch_margin_z(const MarginParams& p, bool distance_map, int layers, hipStream_t s)
{
    const uint64_t total = (uint64_t) p.range.nb[0] * (uint64_t) p.range.nb[1] * (uint64_t) layers;
    if (total == 0) return hipSuccess;
    const size_t lds = (size_t) 256 * (size_t) (kBrick + 2 * p.reach[2]);
    if (distance_map) hipLaunchKernelGGL(k_margin_z<true>, dim3((unsigned) total), dim3(kMarginThreads), lds, s, p);
    else hipLaunchKernelGGL(k_margin_z<false>, dim3((unsigned) total), dim3(kMarginThreads), lds, s, p);
    return hipGetLastError();
}

} // namespace tbrm
