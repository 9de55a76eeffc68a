// tbrm_segment_kernels.hip — seeded region growing on the bricked volume (include/tbrm_segment.h): the candidate
// bits (k_grow_candidates), the seeds (k_grow_seeds), the propagation passes (k_grow_pass), the region's size and bounding box
// (k_grow_measure) and the label write (k_grow_write).
//
// The fill is bit-parallel on the boards of tbrm_brick_boards.h. Per brick the scratch holds the candidate words
// and the visited words; visited is a subset of candidate at all times and bits are only ever set.
//
// A propagation pass looks at the activity words of 64 bricks per wave and gives each due brick 8 lanes, one per slice word, 8 bricks
// at a time. A brick reads the facing bits of its neighbours' visited words ONCE (the halo: a face word, a bit column, a single
// bit), then repeats
//     visited = dilate(visited, halo) & candidate
// until none of its bits changes — the brick-filling snake needs 142 such steps — exchanging the slice words k - 1 / k + 1 by
// cross-lane moves inside the group of 8. A brick that changed stores its words and marks itself and its 6 / 26 neighbours due in
// the next pass.
//
// No workgroup waits for another inside a launch: the kernel boundary is the only hand-off between bricks. A pass may read a
// neighbour's visited words while that neighbour rewrites them and see the old bits, the new ones or a mix. That is harmless: the
// bits read are bits the neighbour holds now or will hold (a subset of the region either way), and a neighbour that changed marks
// this brick due again, so what was missed is read in the next pass. The fixed point — no brick changed — is the region whatever
// was seen on the way; only the number of passes can differ. There are no fences here and none are needed.
//
// All stores are ordinary vector stores and vector atomics in plain HIP.
#include "tbrm_internal.h"

namespace tbrm {

constexpr int kGrowThreads = 256;

// ---- candidates -------------------------------------------------------------------------------------------------------------------
// The only pass over voxel values and label bytes. A wave per brick of the box, lane l on the row (y, z) = (l & 7, l >> 3): its
// 8 voxels (and 8 label bytes) in, one byte of the brick's candidate words out — 64 contiguous bytes per wave — and the same byte
// of the visited words: zero, or the candidates when every candidate joins (no seeds). Rows and voxels outside the box (which lies
// inside the volume: the padding of ragged bricks is outside it) give zero bits. The brick's two activity words are cleared.
template <int FMT>
__global__ __launch_bounds__(kGrowThreads) void k_grow_candidates(const GrowParams p)
{
    __shared__ uint32_t s_writable[8];
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < 8) s_writable[tid] = p.writable[tid];
    __syncthreads();
    WaveBrick w;
    if (!wave_brick<kGrowThreads>(p.range, p.bnx, p.bnxy, w)) return;
    const size_t b = w.b, first = b * 512 + (size_t) lane * 8;

    const uint32_t inside = row_in_box(p.box, w.bx, w.y, w.z);
    uint32_t c[8];
    float f[8];
    row_values<FMT>(p.data, first, c, f);
    const uint32_t in_range = row_gate<FMT>(c, f, p.lo_code, p.hi_code, p.lo_f, p.hi_f);
    uint32_t may = 0u; // bit i: the voxel's label may be grown over
    if (p.labels) may = row_in_mask(*reinterpret_cast<const uint2*>(p.labels + first), s_writable);
    else may = (s_writable[0] & 1u) ? 0xffu : 0u;
    const uint8_t cand = (uint8_t) (inside & in_range & may);
    uint8_t* const bytes = reinterpret_cast<uint8_t*>(p.bits + b * 16);
    bytes[lane] = cand;
    bytes[64 + lane] = p.all_join ? cand : (uint8_t) 0;
    if (lane < 2) p.act[lane][b] = 0u;
}

hipError_t launch_grow_candidates(const GrowParams& p, hipStream_t s)
{
    const uint64_t total = range_bricks(p.range);
    if (total == 0) return hipSuccess;
    const dim3 grid((unsigned) ((total + 3) / 4)), block(kGrowThreads);
    switch (p.fmt) {
        case FMT_U8: hipLaunchKernelGGL(k_grow_candidates<FMT_U8>, grid, block, 0, s, p); break;
        case FMT_U16: hipLaunchKernelGGL(k_grow_candidates<FMT_U16>, grid, block, 0, s, p); break;
        default: hipLaunchKernelGGL(k_grow_candidates<FMT_F32>, grid, block, 0, s, p); break;
    }
    return hipGetLastError();
}

// ---- seeds ------------------------------------------------------------------------------------------------------------------------
// A thread per seed (all inside the volume: the host checked): one that lies in the box and is a candidate sets its visited bit
// and marks its brick due in the first pass.
__global__ __launch_bounds__(kGrowThreads) void k_grow_seeds(const GrowParams p)
{
    const int i = blockIdx.x * kGrowThreads + threadIdx.x;
    if (i >= p.n_seeds) return;
    const int x = p.seeds[3 * i], y = p.seeds[3 * i + 1], z = p.seeds[3 * i + 2];
    if (x < p.box.origin[0] || x >= p.box.end[0] || y < p.box.origin[1] || y >= p.box.end[1] || z < p.box.origin[2] || z >= p.box.end[2]) return;
    const size_t b = grid_index(p.bnx, p.bnxy, x >> kBrickShift, y >> kBrickShift, z >> kBrickShift);
    uint64_t* const words = p.bits + b * 16;
    const uint64_t bit = 1ull << ((y & 7) * 8 + (x & 7));
    if (!(words[z & 7] & bit)) return;
    atomicOr(reinterpret_cast<unsigned long long*>(words + 8 + (z & 7)), (unsigned long long) bit);
    p.act[0][b] = 1u;
    atomicAdd(p.ctl + GROW_SEEDS_TAKEN, 1);
}

hipError_t launch_grow_seeds(const GrowParams& p, hipStream_t s)
{
    if (p.n_seeds <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_grow_seeds, dim3((unsigned) ((p.n_seeds + kGrowThreads - 1) / kGrowThreads)), dim3(kGrowThreads), 0, s, p);
    return hipGetLastError();
}

// ---- a propagation pass -----------------------------------------------------------------------------------------------------------
namespace {

// The in-slice part of a dilation. w: a visited slice word; l / r: the same slice of the bricks at x - 1 / x + 1; t / d: at y - 1 /
// y + 1; tl, tr, dl, dr: at the four xy corners (26 only). What of them reaches this slice of this brick:
//   6:  the word, its four in-slice shifts, and the facing column / row of l, r, t, d
//   26: the 3 x 3 neighbourhood of every set bit, the word's own and the eight neighbours' alike, cut to this brick
// `fixed` is the part that does not depend on w: it is computed once per pass.
struct SliceHalo {
    uint64_t fixed;
};

template <int CONN26>
__device__ __forceinline__ SliceHalo slice_halo(uint64_t l, uint64_t r, uint64_t t, uint64_t d, uint64_t tl, uint64_t tr, uint64_t dl, uint64_t dr)
{
    const uint64_t lc = (l >> 7) & kSliceX0, rc = (r << 7) & kSliceX7; // l's column 7 at our column 0, r's column 0 at our column 7
    SliceHalo h;
    if constexpr (!CONN26) h.fixed = lc | rc | (t >> 56) | (d << 56); // t's row 7 at our row 0, d's row 0 at our row 7
    else {
        const uint64_t side = lc | rc;
        uint64_t row_t = t >> 56, row_d = d & 0xffull; // the rows y = -1 and y = 8, 8 bits each, dilated along x with their corners
        row_t = (row_t | (row_t << 1) | (row_t >> 1) | (tl >> 63) | ((tr >> 56) & 1ull) << 7) & 0xffull;
        row_d = (row_d | (row_d << 1) | (row_d >> 1) | ((dl >> 7) & 1ull) | (dr & 1ull) << 7) & 0xffull;
        h.fixed = side | (side << 8) | (side >> 8) | row_t | (row_d << 56);
    }
    return h;
}

template <int CONN26> __device__ __forceinline__ uint64_t slice_dilate(uint64_t w, const SliceHalo& h) { return slice_spread<CONN26>(w) | h.fixed; }

} // namespace

template <int CONN26>
__global__ __launch_bounds__(kGrowThreads) void k_grow_pass(const GrowParams p)
{
    const int tid = threadIdx.x, lane = tid & 63, j = tid & 7; // j: this lane's slice
    const uint32_t total = (uint32_t) range_bricks(p.range);
    // The wave's 64 bricks of the box's brick list, a lane each: which are due? Most of a pass's waves find none and end here, at the
    // cost of one coalesced 256-byte load. (No other workgroup writes this pass's activity array in this launch.)
    const uint32_t base = (blockIdx.x * (kGrowThreads / 64) + (uint32_t) (tid >> 6)) * 64u;
    bool mine_due = false;
    if (base + (uint32_t) lane < total) {
        int bx, by, bz;
        range_brick(p.range, base + (uint32_t) lane, bx, by, bz);
        const size_t b = grid_index(p.bnx, p.bnxy, bx, by, bz);
        mine_due = p.act[0][b] != 0u;
        if (mine_due) p.act[0][b] = 0u;
    }
    unsigned long long todo = __ballot(mine_due);
    if (todo == 0ull) return;
    if (lane == 0) atomicAdd(p.ctl + GROW_VISITS, (int) __popcll(todo));
    int changed_bricks = 0;
    while (todo != 0ull) { // the due bricks, eight at a time: group g of 8 lanes takes the g-th of them (wave-uniform arithmetic)
        int pick = -1;
#pragma unroll
        for (int g = 0; g < 8; ++g) {
            if (todo != 0ull) {
                const int first = __ffsll((long long) todo) - 1;
                if ((lane >> 3) == g) pick = first;
                todo &= todo - 1ull;
            }
        }
        const bool due = pick >= 0;
        int bx = 0, by = 0, bz = 0;
        size_t b = 0;
        if (due) {
            range_brick(p.range, base + (uint32_t) pick, bx, by, bz);
            b = grid_index(p.bnx, p.bnxy, bx, by, bz);
        }
        uint64_t* const words = p.bits + b * 16;
        uint64_t cand = 0ull, vis = 0ull;
        SliceHalo halo{0ull};
        uint64_t above = 0ull; // what reaches slice 0 / 7 from the bricks at z - 1 / z + 1 (lanes 0 and 7 only)
        if (due) {
            cand = words[j];
            vis = words[8 + j];
            // slice `s` of the visited words of the brick at (dx, dy, dz) from this one; zero outside the box's bricks
            auto nbr = [&](int dx, int dy, int dz, int s) -> uint64_t {
                const int nx = bx + dx, ny = by + dy, nz = bz + dz;
                if (!range_holds(p.range, nx, ny, nz)) return 0ull;
                return p.bits[grid_index(p.bnx, p.bnxy, nx, ny, nz) * 16 + 8 + s];
            };
            if constexpr (!CONN26) {
                halo = slice_halo<0>(nbr(-1, 0, 0, j), nbr(1, 0, 0, j), nbr(0, -1, 0, j), nbr(0, 1, 0, j), 0ull, 0ull, 0ull, 0ull);
                if (j == 0) above = nbr(0, 0, -1, 7);
                if (j == 7) above = nbr(0, 0, 1, 0);
            } else {
                halo = slice_halo<1>(nbr(-1, 0, 0, j), nbr(1, 0, 0, j), nbr(0, -1, 0, j), nbr(0, 1, 0, j), nbr(-1, -1, 0, j), nbr(1, -1, 0, j),
                                     nbr(-1, 1, 0, j), nbr(1, 1, 0, j));
                if (j == 0 || j == 7) { // the facing slice of the nine bricks of the next layer, dilated in its own plane
                    const int dz = j == 0 ? -1 : 1, s = j == 0 ? 7 : 0;
                    const SliceHalo hz = slice_halo<1>(nbr(-1, 0, dz, s), nbr(1, 0, dz, s), nbr(0, -1, dz, s), nbr(0, 1, dz, s), nbr(-1, -1, dz, s),
                                                       nbr(1, -1, dz, s), nbr(-1, 1, dz, s), nbr(1, 1, dz, s));
                    above = slice_dilate<1>(nbr(0, 0, dz, s), hz);
                }
            }
        }
        const uint64_t vis0 = vis;
        // Until no brick of the wave changes. vis only grows and stays inside cand: a brick ends after 512 steps at the most, the
        // wave's eight after 4096; the bound is there so that the loop ends whatever the memory holds.
        for (int step = 0; step < 8 * 512 + 1; ++step) {
            uint64_t reach;
            if constexpr (!CONN26) {
                const uint64_t lo = __shfl_up((unsigned long long) vis, 1, 8), hi = __shfl_down((unsigned long long) vis, 1, 8);
                reach = slice_dilate<0>(vis, halo) | (j > 0 ? lo : 0ull) | (j < 7 ? hi : 0ull) | above;
            } else {
                const uint64_t own = slice_dilate<1>(vis, halo);
                const uint64_t lo = __shfl_up((unsigned long long) own, 1, 8), hi = __shfl_down((unsigned long long) own, 1, 8);
                reach = own | (j > 0 ? lo : 0ull) | (j < 7 ? hi : 0ull) | above;
            }
            const uint64_t grown = vis | (reach & cand);
            const bool moved = grown != vis;
            vis = grown;
            if (__ballot(moved) == 0ull) break;
        }
        // a brick's eight lanes agree on whether it changed (in the first pass: a seeded brick has, its neighbours have not seen the seeds)
        const bool lane_changed = vis != vis0 || (p.first_pass && vis != 0ull);
        const unsigned long long changed_lanes = __ballot(lane_changed);
        const bool changed = due && ((changed_lanes >> (lane & ~7)) & 0xffull) != 0ull;
        if (due && vis != vis0) words[8 + j] = vis;
        if (changed) { // itself and its 6 / 26 neighbours are due in the next pass: the eight lanes share the 27 cells
            for (int c = j; c < 27; c += 8) {
                const int dx = c % 3 - 1, dy = (c / 3) % 3 - 1, dz = c / 9 - 1;
                if (!CONN26 && (dx != 0) + (dy != 0) + (dz != 0) > 1) continue;
                if (range_holds(p.range, bx + dx, by + dy, bz + dz)) p.act[1][grid_index(p.bnx, p.bnxy, bx + dx, by + dy, bz + dz)] = 1u;
            }
        }
        changed_bricks += (int) __popcll(__ballot(changed && j == 0));
    }
    if (lane == 0 && changed_bricks) atomicAdd(p.ctl + p.changed_word, changed_bricks);
}

hipError_t launch_grow_pass(const GrowParams& p, hipStream_t s)
{
    const uint64_t total = range_bricks(p.range);
    if (total == 0) return hipSuccess;
    const dim3 grid((unsigned) ((total + 255) / 256)), block(kGrowThreads); // 64 bricks to a wave
    if (p.conn26) hipLaunchKernelGGL(k_grow_pass<1>, grid, block, 0, s, p);
    else hipLaunchKernelGGL(k_grow_pass<0>, grid, block, 0, s, p);
    return hipGetLastError();
}

// ---- size and bounding box --------------------------------------------------------------------------------------------------------
// A thread per visited word of the box's bricks: its popcount and, where it holds bits, the extent of their x, y and its z; reduced
// over the wave, then one atomic per word and wave that has something to say.
__global__ __launch_bounds__(kGrowThreads) void k_grow_measure(const GrowParams p)
{
    const int tid = threadIdx.x, j = tid & 7;
    const uint32_t total = (uint32_t) range_bricks(p.range);
    const uint32_t k = blockIdx.x * (kGrowThreads / 8) + (uint32_t) (tid >> 3);
    uint64_t w = 0ull;
    int bx = 0, by = 0, bz = 0;
    if (k < total) {
        range_brick(p.range, k, bx, by, bz);
        w = p.bits[grid_index(p.bnx, p.bnxy, bx, by, bz) * 16 + 8 + j];
    }
    if (__ballot(w != 0ull) == 0ull) return;
    const int n = wave_sum((int) __popcll(w));
    WaveBounds bounds;
    bounds.take_slice(w, bx, by, bz * kBrick + j);
    bounds.reduce();
    if ((tid & 63) == 0) atomicAdd(p.ctl + GROW_VOXELS, n);
    bounds.commit(p.ctl + GROW_MIN_X, tid & 63);
}

hipError_t launch_grow_measure(const GrowParams& p, hipStream_t s)
{
    const uint64_t total = range_bricks(p.range);
    if (total == 0) return hipSuccess;
    hipLaunchKernelGGL(k_grow_measure, dim3((unsigned) ((total + 31) / 32)), dim3(kGrowThreads), 0, s, p);
    return hipGetLastError();
}

// ---- the label write ----------------------------------------------------------------------------------------------------------------
// A wave per brick of the region's bounding box, lane l on the row (l & 7, l >> 3) as above: new_label where the row's visited byte
// has a bit, the row stored where it has any. Counts the bytes that changed and the bricks that held region voxels.
__global__ __launch_bounds__(kGrowThreads) void k_grow_write(const GrowParams p, const BrickRange w)
{
    const int tid = threadIdx.x, lane = tid & 63;
    WaveBrick wb;
    if (!wave_brick<kGrowThreads>(w, p.bnx, p.bnxy, wb)) return;
    const size_t b = wb.b;
    const uint32_t vis = reinterpret_cast<const uint8_t*>(p.bits + b * 16)[64 + lane];
    if (__ballot(vis != 0u) == 0ull) return;
    int changed = 0;
    if (vis) {
        uint2* const row = reinterpret_cast<uint2*>(p.labels + b * 512 + (size_t) lane * 8);
        uint2 l = *row;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (!((vis >> i) & 1u)) continue;
            changed += byte_of(l, i) != (uint32_t) p.new_label;
            set_byte(l, i, (uint32_t) p.new_label);
        }
        *row = l;
    }
    changed = wave_sum(changed);
    if (lane == 0) {
        if (changed) atomicAdd(p.ctl + GROW_RELABELLED, changed);
        atomicAdd(p.ctl + GROW_BRICKS_WRITTEN, 1);
    }
}

hipError_t launch_grow_write(const GrowParams& p, const BrickRange& w, hipStream_t s)
{
    const uint64_t total = range_bricks(w);
    if (total == 0) return hipSuccess;
    hipLaunchKernelGGL(k_grow_write, dim3((unsigned) ((total + 3) / 4)), dim3(kGrowThreads), 0, s, p, w);
    return hipGetLastError();
}

} // namespace tbrm
