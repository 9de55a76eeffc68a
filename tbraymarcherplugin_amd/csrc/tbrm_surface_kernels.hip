// tbrm_surface_kernels.hip — the surface of a set of labels as an indexed mesh (include/tbrm_surface.h): surface nets
// on the boards of S. What a slice, a cell and an index are is tbrm_surface_plan.h's, which the host runs too; this file deals the
// work to lanes and stores.
//
//   k_surface_count   eight lanes per block of the cell range, a lane per slice (eight blocks to a wave, a wave over as many octets as
//                     the capped grid leaves it): the slice's eight corner words from the block's own board and the seven at -x, -y,
//                     -z, -xy, -xz, -yz, -xyz, its active word, its owned-edge words; the block's active board, per-slice prefixes and
//                     counts. A block whose eight boards are all empty, or all full and wholly inside the box, is decided by the
//                     classes (skip = 0: computed like the others). The call's counts go out once per workgroup.
//   k_surface_scan_*  the exclusive scan of the two counts: tiles of 1024 blocks, then the tiles (the pattern of k_islands_scan_*).
//   k_surface_emit    a wave per non-empty block, lane l on the block's vertices l, l + 64, ..: the slice of a vertex from the per-slice
//                     prefixes, its cell as the bit of that rank in the slice's active word; the vertex record, the position and the
//                     quads of the cell's owned edges at base + rank; the other three vertices of a quad by the active boards and
//                     bases of the blocks at +x, +y, +z, +xy, +xz, +yz. Neighbouring lanes write neighbouring records.
// Inside a launch nothing that is read is written. Every record and every index goes out as whole dwords.
//
// All stores are ordinary vector stores and vector atomics in plain HIP.
#include "tbrm_surface_kernels.h"

namespace tbrm {

namespace {

constexpr int kSurfaceThreads = 256;
constexpr int kSurfaceCountGroups = 2048; // k_surface_count: at most this many workgroups, each over as many blocks as it takes (8 per CU of 256)

// the boards of S, cut to the box: tbrm_surface_plan.h's fetch for the block (bx, by, bz)
struct BoardFetch {
    const SurfaceParams& p;
    int bx, by, bz;
    __device__ __forceinline__ uint64_t operator()(int dx, int dy, int dz, int s) const
    {
        const int nx = bx + dx, ny = by + dy, nz = bz + dz;
        if (!range_holds(p.bricks, nx, ny, nz)) return 0ull; // (the range lies inside the brick grid)
        return p.bits[grid_index(p.bnx, p.bnxy, nx, ny, nz) * 16 + s] & slice_in_box(p.box, nx, ny, nz * kBrick + s);
    }
};

// tbrm_surface_plan.h's look: the vertices before a slice of a block, and the slice's active cells
struct BlockLook {
    const SurfaceParams& p;
    __device__ __forceinline__ SurfaceLook operator()(uint32_t k, int z) const
    {
        const size_t at = (size_t) k * 8 + (size_t) z;
        return SurfaceLook{p.tile_base[0][k / kSurfaceTile] + (uint64_t) p.base[0][k] + (uint64_t) (p.prefix[at] & 0xffffu), p.active[at]};
    }
};

template <typename T> __device__ __forceinline__ T octet_scan(T v, int z, T& total) // exclusive, over the eight lanes of a block
{
    T inc = v;
#pragma unroll
    for (int o = 1; o < 8; o <<= 1) {
        const T t = __shfl_up(inc, o, 8);
        if (z >= o) inc += t;
    }
    total = __shfl(inc, 7, 8);
    return inc - v;
}

__device__ __forceinline__ bool octet_all(bool v)
{
    int a = v ? 1 : 0;
#pragma unroll
    for (int o = 1; o < 8; o <<= 1) a &= __shfl_xor(a, o, 8);
    return a != 0;
}

} // namespace

__global__ __launch_bounds__(kSurfaceThreads) void k_surface_count(const SurfaceParams p)
{
    __shared__ int s_n[kSurfaceThreads / 64][6], s_box[kSurfaceThreads / 64][6];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, z = lane & 7;
    const uint32_t stride = gridDim.x * (kSurfaceThreads / 8);
    // what the lane has seen of its blocks: the counts and the bounding box are reduced once, after the last of them, and committed
    // once per workgroup — a launch of one wave per eight blocks spent its time on atomics to the same few words
    int n[6] = {0, 0, 0, 0, 0, 0};
    WaveBounds bounds;
    for (uint32_t k = (blockIdx.x * kSurfaceThreads + (uint32_t) tid) >> 3; k < p.n_blocks; k += stride) { // (the eight lanes of a block stay together)
        int bx, by, bz;
        range_brick(p.blocks, k, bx, by, bz);

        // the verdict of the classes: lane j of the block looks at the board at -(j & 1, j >> 1 & 1, j >> 2 & 1)
        bool empty = true, full = false;
        {
            const int nx = bx - (z & 1), ny = by - ((z >> 1) & 1), nz = bz - ((z >> 2) & 1);
            if (range_holds(p.bricks, nx, ny, nz)) {
                const uint32_t cl = p.cls[grid_index(p.bnx, p.bnxy, nx, ny, nz)];
                empty = cl == MORPH_EMPTY;
                full = cl == MORPH_FULL && brick_inside_box(p.box, nx, ny, nz);
            }
        }
        const bool all_empty = octet_all(empty), all_full = octet_all(full);
        const bool computed = !(p.skip && (all_empty || all_full));

        SurfaceSlice sl{0ull, {0ull, 0ull, 0ull}};
        if (computed) {
            uint64_t c[8];
            surface_corner_words(BoardFetch{p, bx, by, bz}, z, c);
            sl = surface_slice(c);
            n[0] += surface_popc(c[7]);
        } else if (all_full) {
            n[0] += 64; // the block's own brick is full and inside the box
        }
        const int qa[3] = {surface_popc(sl.edge[0]), surface_popc(sl.edge[1]), surface_popc(sl.edge[2])};
        const uint32_t v = (uint32_t) surface_popc(sl.active), q = (uint32_t) (qa[0] + qa[1] + qa[2]);
        uint32_t v_total, q_total;
        const uint32_t v_before = octet_scan(v, z, v_total), q_before = octet_scan(q, z, q_total);
        p.active[(size_t) k * 8 + z] = sl.active;
        p.prefix[(size_t) k * 8 + z] = v_before | (q_before << 16); // (at most 512 and 1536)
        if (z == 0) {
            p.count[0][k] = v_total;
            p.count[1][k] = q_total;
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) n[1 + a] += qa[a];
        n[4] += (computed && z == 0) ? 1 : 0;
        n[5] += (!computed && z == 0) ? 1 : 0;
        WaveBounds here;
        here.take_slice(sl.active, bx, by, bz * kBrick + z);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            bounds.mn[a] = min(bounds.mn[a], here.mn[a]);
            bounds.mx[a] = max(bounds.mx[a], here.mx[a]);
        }
    }
#pragma unroll
    for (int c = 0; c < 6; ++c) n[c] = wave_sum(n[c]);
    bounds.reduce();
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 6; ++c) s_n[wave][c] = n[c];
#pragma unroll
        for (int a = 0; a < 3; ++a) { s_box[wave][a] = bounds.mn[a]; s_box[wave][3 + a] = bounds.mx[a]; }
    }
    __syncthreads();
    if (tid < 6) {
        int sum = 0;
#pragma unroll
        for (int w = 0; w < kSurfaceThreads / 64; ++w) sum += s_n[w][tid];
        if (sum) atomicAdd(reinterpret_cast<unsigned long long*>(p.ctl) + SURF_SET_VOXELS + tid, (unsigned long long) sum);
    } else if (tid < 12) {
        const int c = tid - 6;
        int v = s_box[0][c];
#pragma unroll
        for (int w = 1; w < kSurfaceThreads / 64; ++w) v = c < 3 ? min(v, s_box[w][c]) : max(v, s_box[w][c]);
        if (c < 3 ? v != 0x7fffffff : v >= 0) {
            if (c < 3) atomicMin(p.ctl + SURF_MIN_X + c, v);
            else atomicMax(p.ctl + SURF_MIN_X + c, v);
        }
    }
}

hipError_t launch_surface_count(const SurfaceParams& p, hipStream_t s)
{
    if (p.n_blocks == 0) return hipSuccess;
    const uint64_t groups = ((uint64_t) p.n_blocks * 8 + kSurfaceThreads - 1) / kSurfaceThreads;
    hipLaunchKernelGGL(k_surface_count, dim3((unsigned) (groups < (uint64_t) kSurfaceCountGroups ? groups : (uint64_t) kSurfaceCountGroups)), dim3(kSurfaceThreads), 0, s, p);
    return hipGetLastError();
}

// ---- the scan --------------------------------------------------------------------------------------------------------------------------
namespace {

// the exclusive scan of 1024 values held one to a thread; `total` in every thread
__device__ __forceinline__ uint64_t tile_scan(uint64_t v, uint64_t* s_waves, uint64_t& total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint64_t t = (uint64_t) __shfl_up((unsigned long long) inc, o, 64);
        if (lane >= o) inc += t;
    }
    __syncthreads(); // (s_waves may still be read from the call before)
    if (lane == 63) s_waves[wave] = inc;
    __syncthreads();
    uint64_t before = 0ull;
    total = 0ull;
#pragma unroll
    for (int w = 0; w < kSurfaceTile / 64; ++w) {
        const uint64_t t = s_waves[w];
        before += w < wave ? t : 0ull;
        total += t;
    }
    return before + inc - v;
}

} // namespace

// a workgroup per tile of 1024 blocks and count (blockIdx.y): base[k] within the tile, the tile's sum
__global__ __launch_bounds__(kSurfaceTile) void k_surface_scan_tiles(const SurfaceParams p)
{
    __shared__ uint64_t s_waves[kSurfaceTile / 64];
    const int w = blockIdx.y;
    const uint32_t k = blockIdx.x * kSurfaceTile + threadIdx.x;
    const uint64_t v = k < p.n_blocks ? (uint64_t) p.count[w][k] : 0ull;
    uint64_t total;
    const uint64_t ex = tile_scan(v, s_waves, total);
    if (k < p.n_blocks) p.base[w][k] = (uint32_t) ex; // (below 1024 * 1536)
    if (threadIdx.x == 0) p.tile_sum[w][blockIdx.x] = total;
}

// a workgroup per count: the tiles' bases and the total
__global__ __launch_bounds__(kSurfaceTile) void k_surface_scan_top(const SurfaceParams p)
{
    __shared__ uint64_t s_waves[kSurfaceTile / 64];
    const int w = blockIdx.x;
    const uint32_t tiles = (p.n_blocks + kSurfaceTile - 1) / kSurfaceTile;
    uint64_t carry = 0ull;
    for (uint32_t t0 = 0; t0 < tiles; t0 += kSurfaceTile) {
        const uint32_t t = t0 + threadIdx.x;
        const uint64_t v = t < tiles ? p.tile_sum[w][t] : 0ull;
        uint64_t total;
        const uint64_t ex = tile_scan(v, s_waves, total);
        if (t < tiles) p.tile_base[w][t] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) reinterpret_cast<unsigned long long*>(p.ctl)[SURF_VERTICES + w] = carry;
}

hipError_t launch_surface_scan(const SurfaceParams& p, hipStream_t s)
{
    if (p.n_blocks == 0) return hipSuccess;
    hipLaunchKernelGGL(k_surface_scan_tiles, dim3((p.n_blocks + kSurfaceTile - 1) / kSurfaceTile, 2), dim3(kSurfaceTile), 0, s, p);
    hipLaunchKernelGGL(k_surface_scan_top, dim3(2), dim3(kSurfaceTile), 0, s, p);
    return hipGetLastError();
}

// ---- the emit --------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kSurfaceThreads) void k_surface_emit(const SurfaceParams p)
{
    const int tid = threadIdx.x, lane = tid & 63;
    const uint32_t k = blockIdx.x * (kSurfaceThreads / 64) + (uint32_t) (tid >> 6);
    if (k >= p.n_blocks) return; // (the whole wave)
    const uint32_t vertices = p.count[0][k];
    if (vertices == 0u) return;
    int bx, by, bz;
    range_brick(p.blocks, k, bx, by, bz);
    uint32_t pre[8]; // the same for every lane
#pragma unroll
    for (int s = 0; s < 8; ++s) pre[s] = p.prefix[(size_t) k * 8 + s];
    const size_t tile = k / kSurfaceTile;
    const uint64_t v_base = p.tile_base[0][tile] + (uint64_t) p.base[0][k], q_base = p.tile_base[1][tile] + (uint64_t) p.base[1][k];
    const BlockLook look{p};
    const int per_quad = p.triangles ? 6 : 4;

    // lane l takes the block's vertices l, l + 64, ..: neighbouring lanes write neighbouring records
    for (uint32_t j = (uint32_t) lane; j < vertices; j += 64u) {
        int z = 0;
        uint32_t mine = pre[0];
#pragma unroll
        for (int s = 1; s < 8; ++s)
            if ((pre[s] & 0xffffu) <= j) { // the last slice that begins at or before j holds it: the prefixes never fall
                z = s;
                mine = pre[s];
            }
        uint64_t c[8];
        surface_corner_words(BoardFetch{p, bx, by, bz}, z, c);
        const SurfaceSlice sl = surface_slice(c);
        const int bit = surface_nth_bit(sl.active, (int) (j - (mine & 0xffffu)));
        const uint64_t below = (1ull << bit) - 1ull;
        const uint64_t vi = v_base + (uint64_t) j;
        uint64_t qi = q_base + (uint64_t) (mine >> 16) + (uint64_t) (surface_popc(sl.edge[0] & below) + surface_popc(sl.edge[1] & below) + surface_popc(sl.edge[2] & below));
        const int hx = bx * kBrick + (bit & 7), hy = by * kBrick + (bit >> 3), hz = bz * kBrick + z;
        const SurfaceVertex v = surface_vertex(surface_corners(c, bit), hx, hy, hz);
        uint32_t w[kSurfaceVertexWords];
        surface_vertex_words(v, w);
        uint32_t* const rec = p.vertices + vi * kSurfaceVertexWords;
#pragma unroll
        for (int i = 0; i < kSurfaceVertexWords; ++i) rec[i] = w[i];
        if (p.positions) {
#pragma unroll
            for (int a = 0; a < 3; ++a) p.positions[vi * 3 + a] = surface_position(v.cell[a], v.sum[a], v.edges, p.scale[a], p.offset[a]);
        }
        const uint64_t low_end[3] = {c[6], c[5], c[3]};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (!((sl.edge[a] >> bit) & 1ull)) continue;
            uint32_t q[4], out[6];
            surface_quad(p.blocks, look, hx, hy, hz, a, ((low_end[a] >> bit) & 1ull) != 0ull, (uint32_t) vi, q);
            surface_quad_indices(q, p.triangles != 0, out);
            uint32_t* const to = p.indices + qi * (uint64_t) per_quad;
            for (int i = 0; i < per_quad; ++i) to[i] = out[i];
            ++qi;
        }
    }
}

hipError_t launch_surface_emit(const SurfaceParams& p, hipStream_t s)
{
    if (p.n_blocks == 0) return hipSuccess;
    hipLaunchKernelGGL(k_surface_emit, dim3((p.n_blocks + 3) / 4), dim3(kSurfaceThreads), 0, s, p);
    return hipGetLastError();
}

} // namespace tbrm
