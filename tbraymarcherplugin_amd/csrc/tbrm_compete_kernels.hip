// tbrm_compete_kernels.hip — competitive growing from seed labels on the bricked volume (include/tbrm_compete.h): the
// keys' start values (k_compete_init), the relaxation passes (k_compete_pass) and the result (k_compete_write). The rules — codes,
// weights, keys — are those of tbrm_compete_plan.h; the index rules those of tbrm_brick_boards.h.
//
// Every voxel of the bricks the box touches has one 32-bit word: the key (cost << 8) | label of the cheapest path found so far, a
// seed's label at cost 0, or kCompeteUnreached. A brick's claimable voxels are a bit each beside the keys; seeds and walls have no
// bit and their word never changes. A key only ever falls.
//
// A pass looks at the activity words of 64 bricks per wave and gives each due brick the whole wave, one after the other: lane l
// holds the x row (y, z) = (l & 7, l >> 3), its 8 keys in registers. The brick reads the facing keys and codes of its six neighbours
// ONCE, turns the codes into step weights, then repeats
//     key = min(key, offers of the six neighbours)       (x by a forward and a backward sweep of the row, y / z from lanes +-1 / +-8)
// until a ballot says that no key of the brick fell. A brick whose keys fell stores them and marks due in the next pass the neighbours
// behind the faces on which a key fell: a neighbour reads nothing of a brick but the plane that faces it.
//
// No workgroup waits for another inside a launch: the kernel boundary is the only hand-off between bricks. A pass may read a
// neighbour's keys while that neighbour rewrites them. The reads are single aligned 32-bit loads, so each returns a word the
// neighbour held or will hold: the key of a real path either way, never a mix of two. An offer made from it is the key of a real
// path too, so no voxel's key ever falls below its answer; and a neighbour that changed marks this brick due again, so what was
// missed is read in the next pass. The fixed point — no brick changed — is the answer whatever was seen on the way; only the number
// of passes can differ. (The facing keys are read at device scope, past this compute unit's cache, and a brick's stores are complete
// before its marks are written: what one wave stores, the bricks it takes later in the same pass read.)
//
// All stores are ordinary vector stores and vector atomics in plain HIP.
#include "tbrm_compete_kernels.h"

namespace tbrm {

constexpr int kCompeteThreads = 256;
// Steps of a brick's loop. With the facing keys fixed a step makes final every voxel whose best path has one more y / z step
// inside the brick than those final before it (the x sweeps finish the rows): at most 511 steps lower a key. The bound is there
// so that the loop ends whatever the memory holds; a brick that reaches it stays due.
constexpr int kCompeteMaxSteps = 520;

namespace {

// the codes of the 8 voxels from `first` on (a row of a brick)
template <int FMT> __device__ __forceinline__ void row_codes(const CompeteParams& p, size_t first, uint32_t c[8])
{
    float f[8];
    row_values<FMT>(p.data, first, c, f);
    if constexpr (FMT == FMT_F32) {
#pragma unroll
        for (int i = 0; i < 8; ++i) c[i] = compete_float_code(f[i], p.float_origin, p.float_scale); // (__fsub_rn, __fmul_rn: no FMA)
    }
}

template <int FMT> __device__ __forceinline__ uint32_t voxel_code(const CompeteParams& p, size_t at)
{
    if constexpr (FMT == FMT_U8) return ((const uint8_t*) p.data)[at];
    else if constexpr (FMT == FMT_U16) return ((const uint16_t*) p.data)[at];
    else return compete_float_code(((const float*) p.data)[at], p.float_origin, p.float_scale);
}

// one key of another brick, as a whole word from the device's memory side
__device__ __forceinline__ uint32_t facing_key(const uint32_t* at) { return __hip_atomic_load(at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

struct BrickAt { bool there; uint32_t k; size_t g; }; // a brick of the range: its position in it, its index on the volume's grid

__device__ __forceinline__ BrickAt brick_at(const CompeteParams& p, int bx, int by, int bz)
{
    BrickAt a{range_holds(p.range, bx, by, bz), 0u, 0};
    if (a.there) {
        a.k = range_position(p.range, bx, by, bz);
        a.g = grid_index(p.bnx, p.bnxy, bx, by, bz);
    }
    return a;
}

// the six face neighbours of a brick, for lanes 0 .. 5
__device__ __forceinline__ void face_offset(int f, int& dx, int& dy, int& dz)
{
    dx = f == 0 ? -1 : (f == 1 ? 1 : 0);
    dy = f == 2 ? -1 : (f == 3 ? 1 : 0);
    dz = f == 4 ? -1 : (f == 5 ? 1 : 0);
}

__device__ __forceinline__ uint32_t min3(uint32_t a, uint32_t b, uint32_t c) { return min(a, min(b, c)); }

} // namespace

// ---- the start values ---------------------------------------------------------------------------------------------------------------
// The only pass over the gate and the label bytes. A wave per brick of the box, lane l on the row (y, z) = (l & 7, l >> 3): its 8
// voxels and 8 label bytes in; 8 key words (2 KiB contiguous per wave) and the row's claimable byte out. Voxels outside the box
// (which lies inside the volume: the padding of ragged bricks is outside it) are walls. A brick that holds a source marks itself and
// its face neighbours due in the first pass (the host cleared both activity arrays). Counts the seed and the claimable voxels.
template <int FMT>
__global__ __launch_bounds__(kCompeteThreads) void k_compete_init(const CompeteParams p)
{
    __shared__ uint32_t s_seeds[8], s_writable[8];
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < 8) { s_seeds[tid] = p.seeds[tid]; s_writable[tid] = p.writable[tid]; }
    __syncthreads();
    WaveBrick w;
    if (!wave_brick<kCompeteThreads>(p.range, p.bnx, p.bnxy, w)) return;
    const uint32_t k = w.k;
    const int bx = w.bx, by = w.by, bz = w.bz;
    const size_t first = w.b * 512 + (size_t) lane * 8;

    const uint32_t inside = row_in_box(p.box, bx, w.y, w.z);
    uint32_t c[8];
    float f[8];
    row_values<FMT>(p.data, first, c, f);
    const uint32_t gate = row_gate<FMT>(c, f, p.lo_code, p.hi_code, p.lo_f, p.hi_f);
    uint32_t nan = 0u;
    if constexpr (FMT == FMT_F32) {
#pragma unroll
        for (int i = 0; i < 8; ++i) nan |= (uint32_t) (f[i] != f[i]) << i;
    }
    const uint2 l = *reinterpret_cast<const uint2*>(p.labels + first);
    const uint32_t seed = row_in_mask(l, s_seeds) & inside;
    const uint32_t claim = row_in_mask(l, s_writable) & inside & gate & ~seed;
    const uint32_t source = seed & ~nan;
    uint32_t key[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) key[i] = ((source >> i) & 1u) ? compete_key(0u, byte_of(l, i)) : kCompeteUnreached;
    uint4* const out = reinterpret_cast<uint4*>(p.keys + (size_t) k * 512 + (size_t) lane * 8);
    out[0] = make_uint4(key[0], key[1], key[2], key[3]);
    out[1] = make_uint4(key[4], key[5], key[6], key[7]);
    p.claim[(size_t) k * 64 + lane] = (uint8_t) claim;

    const int n_seed = wave_sum((int) __popc(seed)), n_claim = wave_sum((int) __popc(claim));
    if (lane == 0) {
        if (n_seed) atomicAdd(p.counts + COMPETE_SEEDS, (unsigned long long) n_seed);
        if (n_claim) atomicAdd(p.counts + COMPETE_CLAIMABLE, (unsigned long long) n_claim);
    }
    if (__ballot(source != 0u) == 0ull) return;
    if (lane == 6) p.act[0][k] = 1u;
    if (lane < 6) {
        int dx, dy, dz;
        face_offset(lane, dx, dy, dz);
        const BrickAt n = brick_at(p, bx + dx, by + dy, bz + dz);
        if (n.there) p.act[0][n.k] = 1u;
    }
}

hipError_t launch_compete_init(const CompeteParams& p, hipStream_t s)
{
    const uint64_t total = range_bricks(p.range);
    if (total == 0) return hipSuccess;
    const dim3 grid((unsigned) ((total + 3) / 4)), block(kCompeteThreads);
    switch (p.fmt) {
        case FMT_U8: hipLaunchKernelGGL(k_compete_init<FMT_U8>, grid, block, 0, s, p); break;
        case FMT_U16: hipLaunchKernelGGL(k_compete_init<FMT_U16>, grid, block, 0, s, p); break;
        default: hipLaunchKernelGGL(k_compete_init<FMT_F32>, grid, block, 0, s, p); break;
    }
    return hipGetLastError();
}

// ---- a relaxation pass --------------------------------------------------------------------------------------------------------------
template <int FMT>
__global__ __launch_bounds__(kCompeteThreads) void k_compete_pass(const CompeteParams p)
{
    const int tid = threadIdx.x, lane = tid & 63, y = lane & 7, z = lane >> 3;
    const uint32_t total = (uint32_t) range_bricks(p.range);
    // The wave's 64 bricks of the range, a lane each: which are due? Most of a pass's waves find none and end here, at the cost of
    // one coalesced 256-byte load. (No other workgroup writes this pass's activity array in this launch.)
    const uint32_t base = (blockIdx.x * (kCompeteThreads / 64) + (uint32_t) (tid >> 6)) * 64u;
    bool mine_due = false;
    if (base + (uint32_t) lane < total) {
        mine_due = p.act[0][base + (uint32_t) lane] != 0u;
        if (mine_due) p.act[0][base + (uint32_t) lane] = 0u;
    }
    unsigned long long todo = __ballot(mine_due);
    if (todo == 0ull) return;
    if (lane == 0) atomicAdd(p.counts + COMPETE_VISITS, (unsigned long long) __popcll(todo));
    const uint32_t limit = p.limit;
    int changed_bricks = 0;
    while (todo != 0ull) { // the due bricks, one after the other (wave-uniform)
        const uint32_t k = base + (uint32_t) (__ffsll((long long) todo) - 1);
        todo &= todo - 1ull;
        int bx, by, bz;
        range_brick(p.range, k, bx, by, bz);
        const size_t g = grid_index(p.bnx, p.bnxy, bx, by, bz);

        uint32_t key[8], code[8];
        uint32_t* const mine = p.keys + (size_t) k * 512 + (size_t) lane * 8;
        {
            const uint4 a = reinterpret_cast<const uint4*>(mine)[0], b = reinterpret_cast<const uint4*>(mine)[1];
            key[0] = a.x; key[1] = a.y; key[2] = a.z; key[3] = a.w; key[4] = b.x; key[5] = b.y; key[6] = b.z; key[7] = b.w;
        }
        row_codes<FMT>(p, g * 512 + (size_t) lane * 8, code);
        const uint32_t claim = p.claim[(size_t) k * 64 + lane];

        // the facing keys, once; the codes behind them only as the weights of the steps across the faces. A face without a brick of
        // the range behind it offers nothing.
        uint32_t xm = kCompeteUnreached, xp = kCompeteUnreached, hy[8], hz[8];
        uint32_t wx[9], wym[8], wyp[8], wzm[8], wzp[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) hy[i] = hz[i] = kCompeteUnreached;
        wx[0] = wx[8] = 0u;
        {
            const BrickAt n = brick_at(p, bx - 1, by, bz);
            if (n.there) {
                xm = facing_key(p.keys + (size_t) n.k * 512 + (size_t) lane * 8 + 7);
                wx[0] = compete_weight(p.step[0], voxel_code<FMT>(p, n.g * 512 + (size_t) lane * 8 + 7), code[0], p.shift);
            }
        }
        {
            const BrickAt n = brick_at(p, bx + 1, by, bz);
            if (n.there) {
                xp = facing_key(p.keys + (size_t) n.k * 512 + (size_t) lane * 8);
                wx[8] = compete_weight(p.step[0], voxel_code<FMT>(p, n.g * 512 + (size_t) lane * 8), code[7], p.shift);
            }
        }
#pragma unroll
        for (int i = 1; i < 8; ++i) wx[i] = compete_weight(p.step[0], code[i - 1], code[i], p.shift);
        uint32_t cy[8], cz[8]; // the codes of the rows behind the y / z faces (the lanes at a face only)
#pragma unroll
        for (int i = 0; i < 8; ++i) cy[i] = cz[i] = 0u;
        if (y == 0 || y == 7) {
            const BrickAt n = brick_at(p, bx, by + (y == 0 ? -1 : 1), bz);
            if (n.there) {
                const size_t row = (size_t) ((z << 3) | (y == 0 ? 7 : 0)) * 8;
#pragma unroll
                for (int i = 0; i < 8; ++i) hy[i] = facing_key(p.keys + (size_t) n.k * 512 + row + i);
                row_codes<FMT>(p, n.g * 512 + row, cy);
            }
        }
        if (z == 0 || z == 7) {
            const BrickAt n = brick_at(p, bx, by, bz + (z == 0 ? -1 : 1));
            if (n.there) {
                const size_t row = (size_t) (((z == 0 ? 7 : 0) << 3) | y) * 8;
#pragma unroll
                for (int i = 0; i < 8; ++i) hz[i] = facing_key(p.keys + (size_t) n.k * 512 + row + i);
                row_codes<FMT>(p, n.g * 512 + row, cz);
            }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const uint32_t up = __shfl_up(code[i], 1, 64), dn = __shfl_down(code[i], 1, 64), zu = __shfl_up(code[i], 8, 64), zd = __shfl_down(code[i], 8, 64);
            wym[i] = compete_weight(p.step[1], y == 0 ? cy[i] : up, code[i], p.shift);
            wyp[i] = compete_weight(p.step[1], y == 7 ? cy[i] : dn, code[i], p.shift);
            wzm[i] = compete_weight(p.step[2], z == 0 ? cz[i] : zu, code[i], p.shift);
            wzp[i] = compete_weight(p.step[2], z == 7 ? cz[i] : zd, code[i], p.shift);
        }

        uint32_t fell = 0u; // bit i: the key of the row's voxel i fell in this visit
        bool moving = true;
        for (int step = 0; step < kCompeteMaxSteps && moving; ++step) {
            uint32_t nk[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) { // what the rows y +- 1 and z +- 1 offer
                const uint32_t up = __shfl_up(key[i], 1, 64), dn = __shfl_down(key[i], 1, 64), zu = __shfl_up(key[i], 8, 64), zd = __shfl_down(key[i], 8, 64);
                const uint32_t a = min(compete_offer(y == 0 ? hy[i] : up, wym[i], limit), compete_offer(y == 7 ? hy[i] : dn, wyp[i], limit));
                const uint32_t b = min(compete_offer(z == 0 ? hz[i] : zu, wzm[i], limit), compete_offer(z == 7 ? hz[i] : zd, wzp[i], limit));
                nk[i] = ((claim >> i) & 1u) ? min3(key[i], a, b) : key[i];
            }
            // the row itself: forward from x - 1, backward from x + 1
            if (claim & 1u) nk[0] = min(nk[0], compete_offer(xm, wx[0], limit));
#pragma unroll
            for (int i = 1; i < 8; ++i)
                if ((claim >> i) & 1u) nk[i] = min(nk[i], compete_offer(nk[i - 1], wx[i], limit));
            if (claim & 128u) nk[7] = min(nk[7], compete_offer(xp, wx[8], limit));
#pragma unroll
            for (int i = 6; i >= 0; --i)
                if ((claim >> i) & 1u) nk[i] = min(nk[i], compete_offer(nk[i + 1], wx[i + 1], limit));
            uint32_t moved = 0u;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                moved |= (uint32_t) (nk[i] != key[i]) << i;
                key[i] = nk[i];
            }
            fell |= moved;
            moving = __ballot(moved != 0u) != 0ull;
        }
        if (__ballot(fell != 0u) == 0ull) continue;
        // which of the six faces hold a key that fell: a neighbour reads nothing of this brick but the plane facing it
        const unsigned long long face_fell[6] = {__ballot((fell & 1u) != 0u), __ballot((fell & 128u) != 0u), __ballot(fell != 0u && y == 0), __ballot(fell != 0u && y == 7),
                                                 __ballot(fell != 0u && z == 0), __ballot(fell != 0u && z == 7)};
        if (fell) {
            reinterpret_cast<uint4*>(mine)[0] = make_uint4(key[0], key[1], key[2], key[3]);
            reinterpret_cast<uint4*>(mine)[1] = make_uint4(key[4], key[5], key[6], key[7]);
        }
        __threadfence(); // the keys are in memory before the marks: a brick that finds itself due finds the keys that made it so
        if (lane < 6) { // the neighbours behind those faces are due in the next pass (the brick itself is at its fixed point until one of them changes)
            bool mark = false;
#pragma unroll
            for (int f = 0; f < 6; ++f) mark |= lane == f && face_fell[f] != 0ull;
            int dx, dy, dz;
            face_offset(lane, dx, dy, dz);
            const BrickAt n = brick_at(p, bx + dx, by + dy, bz + dz);
            if (mark && n.there) p.act[1][n.k] = 1u;
        }
        if (lane == 6 && moving) p.act[1][k] = 1u; // the loop's bound was reached: the brick goes on in the next pass
        ++changed_bricks;
    }
    if (lane == 0 && changed_bricks) atomicAdd(p.ctl + p.changed_word, changed_bricks);
}

hipError_t launch_compete_pass(const CompeteParams& p, hipStream_t s)
{
    const uint64_t total = range_bricks(p.range);
    if (total == 0) return hipSuccess;
    const dim3 grid((unsigned) ((total + 255) / 256)), block(kCompeteThreads); // 64 bricks to a wave
    switch (p.fmt) {
        case FMT_U8: hipLaunchKernelGGL(k_compete_pass<FMT_U8>, grid, block, 0, s, p); break;
        case FMT_U16: hipLaunchKernelGGL(k_compete_pass<FMT_U16>, grid, block, 0, s, p); break;
        default: hipLaunchKernelGGL(k_compete_pass<FMT_F32>, grid, block, 0, s, p); break;
    }
    return hipGetLastError();
}

// ---- the result ---------------------------------------------------------------------------------------------------------------------
// A wave per brick of the box, lane l on the row (l & 7, l >> 3) as above. A claimable voxel whose word is a key is claimed: its
// label byte becomes the key's label (a writing call), it joins the bounding box, the count of its label (one atomic per wave and
// label present) and the largest cost. The costs of the box, when asked for: the cost of a claimed voxel, 0 for a seed voxel,
// 0xFFFFFFFF everywhere else.
__global__ __launch_bounds__(kCompeteThreads) void k_compete_write(const CompeteParams p)
{
    __shared__ uint32_t s_seeds[8];
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < 8) s_seeds[tid] = p.seeds[tid];
    __syncthreads();
    WaveBrick w;
    if (!wave_brick<kCompeteThreads>(p.range, p.bnx, p.bnxy, w)) return;
    const uint32_t k = w.k;
    const int bx = w.bx, y = w.y, z = w.z;
    const size_t first = w.b * 512 + (size_t) lane * 8;

    uint32_t key[8];
    {
        const uint4* const mine = reinterpret_cast<const uint4*>(p.keys + (size_t) k * 512 + (size_t) lane * 8);
        const uint4 a = mine[0], b = mine[1];
        key[0] = a.x; key[1] = a.y; key[2] = a.z; key[3] = a.w; key[4] = b.x; key[5] = b.y; key[6] = b.z; key[7] = b.w;
    }
    const uint32_t claim = p.claim[(size_t) k * 64 + lane];
    uint32_t claimed = 0u;
#pragma unroll
    for (int i = 0; i < 8; ++i) claimed |= (uint32_t) (((claim >> i) & 1u) && key[i] != kCompeteUnreached) << i;
    uint2* const row = reinterpret_cast<uint2*>(p.labels + first);
    uint2 l = *row;
    if (p.costs) {
        const uint32_t inside = row_in_box(p.box, bx, y, z);
        if (inside) {
            const uint32_t seed = row_in_mask(l, s_seeds);
            const size_t ex = (size_t) (p.box.end[0] - p.box.origin[0]), ey = (size_t) (p.box.end[1] - p.box.origin[1]);
            uint32_t* const out = p.costs + ((size_t) (z - p.box.origin[2]) * ey + (size_t) (y - p.box.origin[1])) * ex;
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if ((inside >> i) & 1u)
                    out[bx * kBrick + i - p.box.origin[0]] = ((claimed >> i) & 1u) ? compete_key_cost(key[i]) : (((seed >> i) & 1u) ? 0u : kCompeteUnreached);
        }
    }
    if (__ballot(claimed != 0u) == 0ull) return;

    int changed = 0;
    uint32_t top = 0u;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        if (!((claimed >> i) & 1u)) continue;
        changed += byte_of(l, i) != compete_key_label(key[i]);
        set_byte(l, i, compete_key_label(key[i]));
        top = max(top, compete_key_cost(key[i]));
    }
    if (p.write && changed) *row = l;
    changed = wave_sum(changed);
    const int n = wave_sum((int) __popc(claimed));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) top = max(top, (uint32_t) __shfl_xor((int) top, o, 64));
    WaveBounds bounds;
    bounds.take_row(claimed, bx, y, z);
    bounds.reduce();
    bounds.commit(p.ctl + COMPETE_MIN_X, lane);
    if (lane == 0) {
        atomicAdd(p.counts + COMPETE_CLAIMED, (unsigned long long) n);
        atomicMax(p.ctl + COMPETE_MAX_COST, (int) top);
        if (p.write) {
            if (changed) atomicAdd(p.counts + COMPETE_RELABELLED, (unsigned long long) changed);
            atomicAdd(p.counts + COMPETE_BRICKS_WRITTEN, 1ull);
        }
    }
    // the counts per label: the label of the first voxel left, every lane's voxels of it, one atomic; until none is left
    uint32_t rest = claimed;
    for (;;) {
        const unsigned long long holders = __ballot(rest != 0u);
        if (holders == 0ull) break;
        uint32_t first_label = 0u;
#pragma unroll
        for (int i = 7; i >= 0; --i)
            if ((rest >> i) & 1u) first_label = compete_key_label(key[i]);
        const uint32_t L = (uint32_t) __shfl((int) first_label, __ffsll((long long) holders) - 1, 64);
        int mine = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (((rest >> i) & 1u) && compete_key_label(key[i]) == L) {
                ++mine;
                rest &= ~(1u << i);
            }
        mine = wave_sum(mine);
        if (lane == 0) atomicAdd(p.counts + COMPETE_PER_LABEL + L, (unsigned long long) mine);
    }
}

hipError_t launch_compete_write(const CompeteParams& p, hipStream_t s)
{
    const uint64_t total = range_bricks(p.range);
    if (total == 0) return hipSuccess;
    hipLaunchKernelGGL(k_compete_write, dim3((unsigned) ((total + 3) / 4)), dim3(kCompeteThreads), 0, s, p);
    return hipGetLastError();
}

} // namespace tbrm
