// tbrm_islands_kernels.hip — the islands of a label (include/tbrm_islands.h): connected-component labelling of a set
// of labels over the 8^3 bricks of the box, the order of the components and the rule over them.
//
//   k_islands_local       a wave per brick: the set's bit board from the label bytes, cut to box and volume; the brick's own components
//                         by bit-parallel flooding from the lowest unclaimed bit, on chip; a local id per set voxel, the local count
//   k_islands_scan_*      the exclusive scan of the local counts: every local component gets a slot
//   k_islands_slots       a wave per set brick: size, first voxel and border bit of its local components into their slots
//   k_islands_merge       a wave per set brick: union-find over the slots across the brick faces (edges and corners for 26)
//   k_islands_flatten     a thread per slot: its root; size, first voxel and border go to the root
//   k_islands_roots       a thread per slot: the roots compacted into sort keys (or counted as spared)
//   (the sort)            rocprim's radix sort of the 64-bit keys: size descending, first voxel ascending
//   k_islands_rule        a thread per island: the rule (tbrm_islands_rule.h), the counts, the table
//   k_islands_write       a wave per set brick: voxel -> local id -> slot -> root -> label; rows stored where a byte changes
//
// The boards and their index rules are tbrm_brick_boards.h's. The union-find forest keeps parent[s] <= s; during the merge its words are shared between workgroups of one launch
// and are read and written with relaxed agent-scope atomics only, no workgroup waits for another, and every loop over it carries a
// hard bound. Which slot becomes a root depends on timing; nothing that leaves these kernels does: the order, the labels and the
// table come from sizes and first voxels alone.
//
// All stores are ordinary vector stores and vector atomics in plain HIP.
#include "tbrm_islands_kernels.h"

#include <cstring>

#include <rocprim/rocprim.hpp>

namespace tbrm {

namespace {

constexpr int kWaveThreads = 256; // four bricks to a workgroup, a wave each
constexpr int kWaves = kWaveThreads / 64;
constexpr int kSlotThreads = 256; // the per-slot kernels

__device__ __forceinline__ uint64_t uniform64(uint64_t v)
{
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t) v), hi = __builtin_amdgcn_readfirstlane((uint32_t) (v >> 32));
    return (uint64_t) hi << 32 | lo;
}

// bit i of b -> byte i all ones
__device__ __forceinline__ uint64_t spread_bits(uint32_t b)
{
    uint64_t x = b;
    x = (x | x << 28) & 0x0000000f0000000full;
    x = (x | x << 14) & 0x0003000300030003ull;
    x = (x | x << 7) & 0x0101010101010101ull;
    return x * 0xffull;
}

__device__ __forceinline__ uint32_t slot_base(const IslandsParams& p, uint32_t k) { return p.base[k] + p.tile_base[k / kIslandsTile]; }

// ---- the union-find forest -----------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t parent_of(const uint32_t* parent, uint32_t s)
{
    return __hip_atomic_load(parent + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root of s, halving the path on the way. parent[] only ever decreases along a path, so the walk ends within `bound` (the slot
// count) steps whatever else happens; the bound ends it whatever memory holds.
__device__ __forceinline__ uint32_t find_root(uint32_t* parent, uint32_t s, uint32_t bound)
{
    for (uint32_t i = 0; i < bound; ++i) {
        const uint32_t q = parent_of(parent, s);
        if (q == s || q >= bound) return s;
        const uint32_t g = parent_of(parent, q);
        if (g == q || g >= bound) return q;
        __hip_atomic_fetch_min(parent + s, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); // g is an ancestor of s and stays one
        s = g;
    }
    return s;
}

// Unite the sets of a and b: the larger root is linked under the smaller by a compare-and-swap that succeeds only while it is still a
// root. A lost race means another link was made; there are fewer links than slots.
__device__ __forceinline__ void unite(uint32_t* parent, uint32_t a, uint32_t b, uint32_t bound)
{
    for (uint32_t i = 0; i < bound; ++i) {
        a = find_root(parent, a, bound);
        b = find_root(parent, b, bound);
        if (a == b) return;
        if (a < b) { const uint32_t t = a; a = b; b = t; }
        uint32_t expected = a;
        if (__hip_atomic_compare_exchange_strong(parent + a, &expected, b, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
    }
}

} // namespace

// ---- the board and the local components ----------------------------------------------------------------------------------------
// Lane l of a brick's wave is on the row (y, z) = (l & 7, l >> 3): its 8 label bytes in, its byte of the board out. The 8 slice words
// are then the same in every lane (scalar registers); a component is flooded from the lowest unclaimed bit by in-place sweeps over
// the slices until a sweep changes nothing, and every lane takes its row's bits of it as the component's id.
template <int CONN26>
__global__ __launch_bounds__(kWaveThreads) void k_islands_local(const IslandsParams p)
{
    __shared__ uint32_t s_source[8];
    __shared__ uint64_t s_board[kWaves][8];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < 8) s_source[tid] = p.source[tid];
    __syncthreads();
    const uint32_t k = blockIdx.x * kWaves + (uint32_t) wave;
    const bool valid = k < p.nbox;
    uint32_t set = 0u;
    if (valid) {
        int bx, by, bz;
        range_brick(p.range, k, bx, by, bz);
        const uint32_t box = row_in_box(p.box, bx, by * kBrick + (lane & 7), bz * kBrick + (lane >> 3)); // (the box lies inside the volume)
        if (box) {
            const uint2 l = *reinterpret_cast<const uint2*>(p.labels + grid_index(p.bnx, p.bnxy, bx, by, bz) * 512 + (size_t) lane * 8);
            set = row_in_mask(l, s_source) & box;
        }
    }
    reinterpret_cast<uint8_t*>(s_board[wave])[lane] = (uint8_t) set;
    __syncthreads();
    if (!valid) return;
    uint64_t S[8], rem[8];
    uint32_t voxels = 0u;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        S[s] = rem[s] = uniform64(s_board[wave][s]);
        voxels += (uint32_t) __popcll(S[s]);
    }
    reinterpret_cast<uint8_t*>(p.boards + (size_t) k * 8)[lane] = (uint8_t) set;
    uint32_t count = 0u;
    uint64_t ids = 0ull; // this lane's 8 local ids
    if (voxels == 512u) count = 1u; // a full brick is one component, id 0 everywhere
    else if (voxels) {
        for (int guard = 0; guard < 512; ++guard) { // (a component takes at least one bit of the 512)
            uint64_t m[8];
            bool seeded = false;
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                m[s] = (!seeded && rem[s]) ? (rem[s] & (0ull - rem[s])) : 0ull;
                seeded = seeded || rem[s] != 0ull;
            }
            if (!seeded) break;
            for (int sweep = 0; sweep < 512; ++sweep) { // (a sweep that changes something adds at least one bit)
                bool changed = false;
#pragma unroll
                for (int s = 0; s < 8; ++s) {
                    const uint64_t below = s > 0 ? m[s - 1] : 0ull, above = s < 7 ? m[s + 1] : 0ull;
                    uint64_t n;
                    if constexpr (CONN26) n = slice_spread<1>(m[s] | below | above);
                    else n = slice_spread<0>(m[s]) | below | above;
                    n &= S[s];
                    changed = changed || n != m[s];
                    m[s] = n;
                }
                if (!changed) break;
            }
            uint64_t mine = 0ull;
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                rem[s] &= ~m[s];
                mine = (lane >> 3) == s ? m[s] : mine;
            }
            const uint64_t bytes = spread_bits((uint32_t) (mine >> (8 * (lane & 7))) & 0xffu);
            ids = (ids & ~bytes) | (bytes & ((uint64_t) count * 0x0101010101010101ull));
            ++count;
        }
    }
    if (voxels) {
        uint2 out;
        out.x = (uint32_t) ids;
        out.y = (uint32_t) (ids >> 32);
        *reinterpret_cast<uint2*>(p.lid + (size_t) k * 512 + (size_t) lane * 8) = out;
    }
    if (lane == 0) {
        p.cnt[k] = count;
        if (voxels) atomicAdd(reinterpret_cast<unsigned long long*>(p.ctl) + ISL_SET_VOXELS, (unsigned long long) voxels);
    }
}

hipError_t launch_islands_local(const IslandsParams& p, hipStream_t s)
{
    if (p.nbox == 0) return hipSuccess;
    const dim3 grid((p.nbox + kWaves - 1) / kWaves), block(kWaveThreads);
    if (p.conn26) hipLaunchKernelGGL(k_islands_local<1>, grid, block, 0, s, p);
    else hipLaunchKernelGGL(k_islands_local<0>, grid, block, 0, s, p);
    return hipGetLastError();
}

// ---- the slots -------------------------------------------------------------------------------------------------------------------
// the exclusive scan of 1024 values held one to a thread; `total` in every thread
__device__ __forceinline__ uint32_t block_scan_1024(uint32_t v, uint32_t* s_waves, uint32_t& total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    __syncthreads(); // (s_waves may still be read from the call before)
    if (lane == 63) s_waves[wave] = inc;
    __syncthreads();
    uint32_t before = 0u;
    total = 0u;
#pragma unroll
    for (int w = 0; w < kIslandsTile / 64; ++w) {
        const uint32_t t = s_waves[w];
        before += w < wave ? t : 0u;
        total += t;
    }
    return before + inc - v;
}

// a workgroup per tile of 1024 bricks: base[k] within the tile, the tile's sum
__global__ __launch_bounds__(kIslandsTile) void k_islands_scan_tiles(const IslandsParams p)
{
    __shared__ uint32_t s_waves[kIslandsTile / 64];
    const uint32_t k = blockIdx.x * kIslandsTile + threadIdx.x;
    const uint32_t v = k < p.nbox ? p.cnt[k] : 0u;
    uint32_t total;
    const uint32_t ex = block_scan_1024(v, s_waves, total);
    if (k < p.nbox) p.base[k] = ex;
    if (threadIdx.x == 0) p.tile_sum[blockIdx.x] = total;
}

// one workgroup: the tiles' bases and the total
__global__ __launch_bounds__(kIslandsTile) void k_islands_scan_top(const IslandsParams p)
{
    __shared__ uint32_t s_waves[kIslandsTile / 64];
    const uint32_t tiles = (p.nbox + kIslandsTile - 1) / kIslandsTile;
    uint32_t carry = 0u;
    for (uint32_t t0 = 0; t0 < tiles; t0 += kIslandsTile) {
        const uint32_t t = t0 + threadIdx.x;
        const uint32_t v = t < tiles ? p.tile_sum[t] : 0u;
        uint32_t total;
        const uint32_t ex = block_scan_1024(v, s_waves, total);
        if (t < tiles) p.tile_base[t] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) p.ctl[ISL_TOTAL] = (int32_t) carry;
}

hipError_t launch_islands_scan(const IslandsParams& p, hipStream_t s)
{
    if (p.nbox == 0) return hipSuccess;
    hipLaunchKernelGGL(k_islands_scan_tiles, dim3((p.nbox + kIslandsTile - 1) / kIslandsTile), dim3(kIslandsTile), 0, s, p);
    hipLaunchKernelGGL(k_islands_scan_top, dim3(1), dim3(kIslandsTile), 0, s, p);
    return hipGetLastError();
}

// A wave per brick: the size, first voxel and border bit of each local component, collected in LDS (an LDS atomic per voxel and
// quantity) and written to the component's slot; the slot is its own parent.
__global__ __launch_bounds__(kWaveThreads) void k_islands_slots(const IslandsParams p)
{
    __shared__ uint32_t s_size[kWaves][256], s_first[kWaves][256], s_border[kWaves][256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t k = blockIdx.x * kWaves + (uint32_t) wave;
    const uint32_t count = k < p.nbox ? min(p.cnt[k], 256u) : 0u;
    for (uint32_t c = lane; c < count; c += 64) {
        s_size[wave][c] = 0u;
        s_first[wave][c] = 0xffffffffu;
        s_border[wave][c] = 0u;
    }
    __syncthreads();
    if (count) {
        int bx, by, bz;
        range_brick(p.range, k, bx, by, bz);
        const uint32_t set = reinterpret_cast<const uint8_t*>(p.boards + (size_t) k * 8)[lane];
        if (set) {
            const uint2 ids = *reinterpret_cast<const uint2*>(p.lid + (size_t) k * 512 + (size_t) lane * 8);
            const int y = by * kBrick + (lane & 7), z = bz * kBrick + (lane >> 3);
            const bool face_yz = y == p.box.origin[1] || y == p.box.end[1] - 1 || z == p.box.origin[2] || z == p.box.end[2] - 1;
            const uint32_t row = (uint32_t) (((uint64_t) z * (uint64_t) p.dims[1] + (uint64_t) y) * (uint64_t) p.dims[0]); // (the volume has fewer than 2^32 voxels)
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                if (!((set >> i) & 1u)) continue;
                const uint32_t c = byte_of(ids, i);
                const int x = bx * kBrick + i;
                atomicAdd(&s_size[wave][c], 1u);
                atomicMin(&s_first[wave][c], row + (uint32_t) x);
                if (face_yz || x == p.box.origin[0] || x == p.box.end[0] - 1) atomicOr(&s_border[wave][c], 1u);
            }
        }
    }
    __syncthreads();
    if (count) {
        const uint32_t base = slot_base(p, k);
        for (uint32_t c = lane; c < count; c += 64) {
            const uint32_t s = base + c;
            if (s >= p.total) continue;
            p.size[s] = s_size[wave][c];
            p.first[s] = s_first[wave][c];
            p.border[s] = s_border[wave][c];
            p.parent[s] = s;
        }
    }
}

hipError_t launch_islands_slots(const IslandsParams& p, hipStream_t s)
{
    if (p.nbox == 0 || p.total == 0) return hipSuccess;
    hipLaunchKernelGGL(k_islands_slots, dim3((p.nbox + kWaves - 1) / kWaves), dim3(kWaveThreads), 0, s, p);
    return hipGetLastError();
}

// ---- the merge -------------------------------------------------------------------------------------------------------------------
// A wave per brick. Every pair of touching set voxels that lie in different bricks is met once, from the voxel for which the step to
// the other is one of the "half" directions (dz > 0, or dz == 0 and dy > 0, or dz == dy == 0 and dx > 0): three of them for 6, thirteen
// for 26. The boards of the bricks such a step can lead into (3 for 6; for 26 the 17 others of this and the next brick layer: a step
// up in z that stays in the layer may leave through any side) are staged in LDS, index (cz, cy + 1, cx + 1); a lane takes its
// row against the row it steps to, shifted by dx over the three bricks that row crosses, and unites the slots of every touching pair.
template <int CONN26>
__global__ __launch_bounds__(kWaveThreads) void k_islands_merge(const IslandsParams p)
{
    __shared__ uint64_t s_nb[kWaves][18][8];
    __shared__ int32_t s_k[kWaves][18];       // the neighbour's position in the box's brick range; -1: none, or nothing set in it
    __shared__ uint32_t s_base[kWaves][18];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t k = blockIdx.x * kWaves + (uint32_t) wave;
    const uint32_t count = k < p.nbox ? p.cnt[k] : 0u;
    int bx = 0, by = 0, bz = 0;
    if (count) range_brick(p.range, k, bx, by, bz);
    if (lane < 18) {
        int32_t at = -1;
        uint32_t base = 0u;
        const int cx = lane % 3 - 1, cy = (lane / 3) % 3 - 1, cz = lane / 9;
        // 26: a half step can lead into every brick of this and the next brick layer but the brick itself; 6: into +x, +y, +z
        const bool needed = CONN26 ? lane != 4 : ((cx == 1 && cy == 0 && cz == 0) || (cx == 0 && cy == 1 && cz == 0) || (cx == 0 && cy == 0 && cz == 1));
        if (count && needed) {
            if (range_holds(p.range, bx + cx, by + cy, bz + cz)) {
                const uint32_t kn = range_position(p.range, bx + cx, by + cy, bz + cz);
                if (p.cnt[kn]) {
                    at = (int32_t) kn;
                    base = slot_base(p, kn);
                }
            }
        }
        s_k[wave][lane] = at;
        s_base[wave][lane] = base;
    }
    __syncthreads();
    bool any = false;
    for (int n = 0; n < 18; ++n) {
        const int32_t at = s_k[wave][n];
        reinterpret_cast<uint8_t*>(s_nb[wave][n])[lane] = at >= 0 ? reinterpret_cast<const uint8_t*>(p.boards + (size_t) at * 8)[lane] : (uint8_t) 0;
        any = any || at >= 0;
    }
    __syncthreads();
    if (!count || !any) return; // (the whole wave)
    const uint32_t mine = reinterpret_cast<const uint8_t*>(p.boards + (size_t) k * 8)[lane];
    uint2 ids = make_uint2(0u, 0u);
    if (mine) ids = *reinterpret_cast<const uint2*>(p.lid + (size_t) k * 512 + (size_t) lane * 8);
    const uint32_t my_base = slot_base(p, k);
    const int y = lane & 7, z = lane >> 3;
    constexpr int kSteps = CONN26 ? 5 : 3;
    const int step_dz[5] = {0, 0, 1, 1, 1}, step_dy26[5] = {0, 1, -1, 0, 1};
    const int step_dy6[3] = {0, 1, 0}, step_dz6[3] = {0, 0, 1};
    constexpr uint64_t kNone = ~0ull;
    uint64_t last = kNone; // the pair this lane met last: a face of two solid bricks is the same pair 64 times
#pragma unroll
    for (int d = 0; d < kSteps; ++d) {
        const int dy = CONN26 ? step_dy26[d] : step_dy6[d], dz = CONN26 ? step_dz[d] : step_dz6[d];
        const int yy = y + dy, zz = z + dz;
        const int cy = yy < 0 ? -1 : (yy > 7 ? 1 : 0), cz = zz > 7 ? 1 : 0;
        const int ry = yy & 7, rz = zz & 7;
        const int n0 = cz * 9 + (cy + 1) * 3; // the brick at cx = -1 of the row stepped to
        const bool own = cy == 0 && cz == 0;
        const uint32_t L = (uint32_t) (s_nb[wave][n0][rz] >> (8 * ry)) & 0xffu;
        const uint32_t C = own ? 0u : (uint32_t) (s_nb[wave][n0 + 1][rz] >> (8 * ry)) & 0xffu; // (pairs inside the brick are its own components)
        const uint32_t R = (uint32_t) (s_nb[wave][n0 + 2][rz] >> (8 * ry)) & 0xffu;
        const uint32_t ext = ((L >> 7) & 1u) | (C << 1) | ((R & 1u) << 9); // bit x + 1: the voxel x of that row, x = -1 .. 8
        const int dx_lo = (d == 0) ? 1 : (CONN26 ? -1 : 0), dx_hi = (d == 0) ? 1 : (CONN26 ? 1 : 0);
        for (int dx = dx_lo; dx <= dx_hi; ++dx) {
            const uint32_t touch = mine & (ext >> (1 + dx)) & 0xffu;
            if (__ballot(touch != 0u) == 0ull) continue;
            // The wave walks the row's voxels together. A pair equal to the lane's last, or to the pair of the first lane that has one
            // at this voxel, is that pair again and is left to the lane that had it first.
            for (int i = 0; i < 8; ++i) {
                uint64_t key = kNone;
                if ((touch >> i) & 1u) {
                    const int xx = i + dx;
                    const int n = n0 + (xx < 0 ? 0 : (xx > 7 ? 2 : 1));
                    const int32_t at = s_k[wave][n];
                    if (at >= 0) { // (else its board was staged as empty: not reached)
                        const uint32_t other = p.lid[(size_t) at * 512 + (size_t) ((rz * 8 + ry) * 8 + (xx & 7))];
                        const uint32_t a = my_base + byte_of(ids, i), b = s_base[wave][n] + other;
                        if (a < p.total && b < p.total) key = (uint64_t) a << 32 | (uint64_t) b;
                    }
                }
                const uint64_t lanes = __ballot(key != kNone);
                if (!lanes) continue;
                const int leader = __ffsll((unsigned long long) lanes) - 1;
                const uint32_t lead_a = __shfl((uint32_t) (key >> 32), leader, 64), lead_b = __shfl((uint32_t) key, leader, 64);
                const uint64_t lead_key = (uint64_t) lead_a << 32 | (uint64_t) lead_b;
                const bool go = key != kNone && key != last && (key != lead_key || lane == leader);
                if (key != kNone) last = key;
                if (go) unite(p.parent, (uint32_t) (key >> 32), (uint32_t) key, p.total);
            }
        }
    }
}

hipError_t launch_islands_merge(const IslandsParams& p, hipStream_t s)
{
    if (p.nbox == 0 || p.total == 0) return hipSuccess;
    const dim3 grid((p.nbox + kWaves - 1) / kWaves), block(kWaveThreads);
    if (p.conn26) hipLaunchKernelGGL(k_islands_merge<1>, grid, block, 0, s, p);
    else hipLaunchKernelGGL(k_islands_merge<0>, grid, block, 0, s, p);
    return hipGetLastError();
}

// ---- roots, order, rule ----------------------------------------------------------------------------------------------------------
// A thread per slot: its root (the forest no longer changes; the walk only reads); what the slot's local component has goes to the
// root's slot — an atomic per slot and quantity, not per voxel. Only roots are added to, only other slots are read.
__global__ __launch_bounds__(kSlotThreads) void k_islands_flatten(const IslandsParams p)
{
    const uint32_t s = blockIdx.x * kSlotThreads + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool valid = s < p.total;
    uint32_t r = s;
    if (valid) {
        for (uint32_t i = 0; i < p.total; ++i) {
            const uint32_t q = parent_of(p.parent, r);
            if (q == r || q >= p.total) break;
            r = q;
        }
        p.root[s] = r;
    }
    bool pending = valid && r != s;
    uint32_t size = pending ? p.size[s] : 0u, first = pending ? p.first[s] : 0xffffffffu, border = pending ? p.border[s] : 0u;
    // Neighbouring slots mostly share a root (a large island is most of the slots): up to four times the lanes that share the first
    // pending lane's root are reduced over the wave and sent by that lane alone; what is left goes lane by lane.
    for (int group = 0; group < 4; ++group) {
        const uint64_t lanes = __ballot(pending);
        if (!lanes) break;
        const int leader = __ffsll((unsigned long long) lanes) - 1;
        const bool in = pending && r == __shfl(r, leader, 64);
        uint32_t n = in ? size : 0u, f = in ? first : 0xffffffffu, b = in ? border : 0u;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            n += __shfl_xor(n, o, 64);
            f = min(f, __shfl_xor(f, o, 64));
            b |= __shfl_xor(b, o, 64);
        }
        if (lane == leader) {
            atomicAdd(p.size + r, n);
            atomicMin(p.first + r, f);
            if (b) atomicOr(p.border + r, 1u);
        }
        pending = pending && !in;
    }
    if (pending) {
        atomicAdd(p.size + r, size);
        atomicMin(p.first + r, first);
        if (border) atomicOr(p.border + r, 1u);
    }
}

// A thread per slot: a root becomes a sort key (one atomic per wave for the places), or — a border island that is spared — is counted.
__global__ __launch_bounds__(kSlotThreads) void k_islands_roots(const IslandsParams p)
{
    const uint32_t s = blockIdx.x * kSlotThreads + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool is_root = s < p.total && p.root[s] == s;
    const bool spared = is_root && p.spare && p.border[s] != 0u;
    const bool ordered = is_root && !spared;
    const uint64_t ordered_lanes = __ballot(ordered), spared_lanes = __ballot(spared);
    uint32_t place = 0u;
    if (lane == 0) {
        if (ordered_lanes) place = atomicAdd(reinterpret_cast<uint32_t*>(p.ctl + ISL_ROOTS), (uint32_t) __popcll(ordered_lanes));
        if (spared_lanes) atomicAdd(reinterpret_cast<uint32_t*>(p.ctl + ISL_SPARED), (uint32_t) __popcll(spared_lanes));
    }
    place = __shfl(place, 0, 64) + (uint32_t) __popcll(ordered_lanes & ((1ull << lane) - 1ull));
    if (ordered && place < p.total) {
        p.keys_in[place] = islands_key(p.size[s], p.first[s]);
        p.vals_in[place] = s;
    }
    if (spared) {
        p.rank[s] = 0xffffffffu;
        p.act[s] = kIslandsLeave;
    }
}

hipError_t launch_islands_flatten(const IslandsParams& p, hipStream_t s)
{
    if (p.total == 0) return hipSuccess;
    const dim3 grid((p.total + kSlotThreads - 1) / kSlotThreads), block(kSlotThreads);
    hipLaunchKernelGGL(k_islands_flatten, grid, block, 0, s, p);
    hipLaunchKernelGGL(k_islands_roots, grid, block, 0, s, p);
    return hipGetLastError();
}

hipError_t islands_sort_bytes(uint32_t n, size_t* bytes)
{
    *bytes = 0;
    return rocprim::radix_sort_pairs(nullptr, *bytes, (uint64_t*) nullptr, (uint64_t*) nullptr, (uint32_t*) nullptr, (uint32_t*) nullptr, (size_t) n, 0u, 64u, (hipStream_t) 0);
}

hipError_t launch_islands_sort(const IslandsParams& p, void* temp, size_t temp_bytes, hipStream_t s)
{
    if (p.n_roots == 0) return hipSuccess;
    return rocprim::radix_sort_pairs(temp, temp_bytes, p.keys_in, p.keys_out, p.vals_in, p.vals_out, (size_t) p.n_roots, 0u, 64u, s);
}

// A thread per island, in order: the rule, the root's label and rank, the counts (reduced over the wave: one atomic per wave and
// quantity), the table's entry.
__global__ __launch_bounds__(kSlotThreads) void k_islands_rule(const IslandsParams p)
{
    const uint32_t i = blockIdx.x * kSlotThreads + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool valid = i < p.n_roots;
    bool kept = false;
    uint32_t size = 0u;
    if (valid) {
        const uint64_t key = p.keys_out[i];
        const uint32_t s = p.vals_out[i];
        size = islands_key_size(key);
        kept = islands_kept(p.rule, i, size);
        const int label = islands_label(p.rule, i, size);
        if (s < p.total) {
            p.act[s] = label;
            p.rank[s] = i;
        }
        if (i == 0) p.ctl[ISL_LARGEST] = (int32_t) size;
        if (i < p.table_cap) {
            IslandsEntry e;
            e.voxels = size;
            e.first = islands_key_first(key);
            e.label = label;
            e.flags = (kept ? kIslandKept : 0u) | ((s < p.total && p.border[s]) ? kIslandBorder : 0u);
            e.lo = 255u;
            e.hi = 0u;
            p.table[i] = e;
        }
    }
    const uint64_t kept_lanes = __ballot(valid && kept), dropped_lanes = __ballot(valid && !kept);
    unsigned long long kv = kept ? size : 0u, dv = (valid && !kept) ? size : 0u;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        kv += __shfl_xor(kv, o, 64);
        dv += __shfl_xor(dv, o, 64);
    }
    if (lane == 0) {
        unsigned long long* const counts = reinterpret_cast<unsigned long long*>(p.ctl);
        if (kept_lanes) atomicAdd(counts + ISL_KEPT, (unsigned long long) __popcll(kept_lanes));
        if (dropped_lanes) atomicAdd(counts + ISL_DROPPED, (unsigned long long) __popcll(dropped_lanes));
        if (kv) atomicAdd(counts + ISL_KEPT_VOXELS, kv);
        if (dv) atomicAdd(counts + ISL_DROPPED_VOXELS, dv);
    }
}

hipError_t launch_islands_rule(const IslandsParams& p, hipStream_t s)
{
    if (p.n_roots == 0) return hipSuccess;
    hipLaunchKernelGGL(k_islands_rule, dim3((p.n_roots + kSlotThreads - 1) / kSlotThreads), dim3(kSlotThreads), 0, s, p);
    return hipGetLastError();
}

// ---- the write -------------------------------------------------------------------------------------------------------------------
// A wave per brick, lane l on the row (l & 7, l >> 3). The label and the rank of each local component's island are fetched once per
// component into LDS; a voxel of the set goes local id -> label there. A row is stored only where a byte changes. The changed bytes
// and their bounding box are reduced over the wave: one atomic per wave and quantity that has something to say. For the table the
// range of the label bytes of each local component is collected in LDS and sent to the island's entry once per component.
__global__ __launch_bounds__(kWaveThreads) void k_islands_write(const IslandsParams p)
{
    __shared__ int32_t s_act[kWaves][256];
    __shared__ uint32_t s_rank[kWaves][256], s_lo[kWaves][256], s_hi[kWaves][256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t k = blockIdx.x * kWaves + (uint32_t) wave;
    const uint32_t count = k < p.nbox ? min(p.cnt[k], 256u) : 0u;
    const uint32_t base = count ? slot_base(p, k) : 0u;
    for (uint32_t c = lane; c < count; c += 64) {
        const uint32_t s = base + c;
        const uint32_t r = s < p.total ? p.root[s] : 0xffffffffu;
        s_act[wave][c] = r < p.total ? p.act[r] : kIslandsLeave;
        s_rank[wave][c] = r < p.total ? p.rank[r] : 0xffffffffu;
        s_lo[wave][c] = 255u;
        s_hi[wave][c] = 0u;
    }
    __syncthreads();
    int changed = 0;
    WaveBounds bounds;
    if (count) {
        int bx, by, bz;
        range_brick(p.range, k, bx, by, bz);
        const uint32_t set = reinterpret_cast<const uint8_t*>(p.boards + (size_t) k * 8)[lane];
        if (set) {
            const uint2 ids = *reinterpret_cast<const uint2*>(p.lid + (size_t) k * 512 + (size_t) lane * 8);
            uint2* const bytes = reinterpret_cast<uint2*>(p.labels + grid_index(p.bnx, p.bnxy, bx, by, bz) * 512 + (size_t) lane * 8);
            const uint2 old = *bytes;
            uint2 l = old;
            uint32_t moved = 0u;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                if (!((set >> i) & 1u)) continue;
                const uint32_t c = byte_of(ids, i), was = byte_of(old, i);
                if (p.table_cap && s_rank[wave][c] < p.table_cap) {
                    atomicMin(&s_lo[wave][c], was);
                    atomicMax(&s_hi[wave][c], was);
                }
                const int to = s_act[wave][c];
                if (p.write && to >= 0 && (uint32_t) to != was) {
                    set_byte(l, i, (uint32_t) to);
                    moved |= 1u << i;
                    ++changed;
                }
            }
            if (moved) *bytes = l;
            bounds.take_row(moved, bx, by * kBrick + (lane & 7), bz * kBrick + (lane >> 3));
        }
    }
    __syncthreads();
    if (p.table_cap)
        for (uint32_t c = lane; c < count; c += 64) {
            const uint32_t rk = s_rank[wave][c];
            if (rk < p.table_cap && s_lo[wave][c] <= s_hi[wave][c]) {
                atomicMin(&p.table[rk].lo, s_lo[wave][c]);
                atomicMax(&p.table[rk].hi, s_hi[wave][c]);
            }
        }
    if (__ballot(changed != 0) == 0ull) return;
    changed = wave_sum(changed);
    bounds.reduce();
    if (lane == 0) {
        unsigned long long* const counts = reinterpret_cast<unsigned long long*>(p.ctl);
        atomicAdd(counts + ISL_RELABELLED, (unsigned long long) changed);
        atomicAdd(counts + ISL_BRICKS_WRITTEN, 1ull);
    }
    bounds.commit(p.ctl + ISL_MIN_X, lane);
}

hipError_t launch_islands_write(const IslandsParams& p, hipStream_t s)
{
    if (p.nbox == 0 || p.total == 0) return hipSuccess;
    hipLaunchKernelGGL(k_islands_write, dim3((p.nbox + kWaves - 1) / kWaves), dim3(kWaveThreads), 0, s, p);
    return hipGetLastError();
}

} // namespace tbrm
