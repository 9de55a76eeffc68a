// tbrm_stats_kernels.hip — statistics of the bricked data volume (include/tbrm_volume_stats.h): the value histogram
// (k_volume_histogram) and the per-label count / sum / min / max (k_label_statistics). Both read the volume as it lies, and the
// bricked label volume on the same grid.
//
// Common shape. The work is the list of the bricks the box touches (the range and row rules are tbrm_brick_boards.h's, DESIGN.md
// §17). A wave takes one brick at a time: lane l holds the x row (y, z) = (l & 7, l >> 3) of the brick, 8 voxels — one 16-byte load for UNORM16 (the whole 1 KiB brick in one wave instruction),
// 8 bytes for UNORM8 and for the labels, two 16-byte loads for float32 — and the next brick's row is requested before this one
// is counted. The grid is sized to the device (a few workgroups per compute unit, the waves striding over the bricks), so what
// the workgroups flush to global memory at the end is bounded by the grid, not by the volume.
//   A brick inside the box on all three axes (the box lies inside the volume, so such a brick holds no padding either) is "whole":
// no per-voxel tests. Any other brick the box touches is "cut": a lane tests its row's y and z once and each voxel's x.
// Every brick of the bricked allocation exists in full (ragged edge bricks are zero-padded), so the loads need no guard.
//
// All stores are ordinary vector stores and vector atomics in plain HIP. Compiled with -ffp-contract=off: the float binning
// rule is two separate float32 operations.
#include "tbrm_internal.h"

#include <type_traits>

namespace tbrm {

namespace {

constexpr int kStatsThreads = 256;
constexpr int kStatsWaves = kStatsThreads / 64;

// a lane's 8 voxels, as loaded
template <int FMT> struct Row;
template <> struct Row<FMT_U8> {
    uint2 v;
    __device__ __forceinline__ void load(const void* data, size_t first) { v = *reinterpret_cast<const uint2*>((const uint8_t*) data + first); }
    __device__ __forceinline__ uint32_t code(int i) const { return byte_of(v, i); }
};
template <> struct Row<FMT_U16> {
    uint4 v;
    __device__ __forceinline__ void load(const void* data, size_t first) { v = *reinterpret_cast<const uint4*>((const uint16_t*) data + first); }
    __device__ __forceinline__ uint32_t code(int i) const
    {
        const uint32_t w = (i >> 1) == 0 ? v.x : ((i >> 1) == 1 ? v.y : ((i >> 1) == 2 ? v.z : v.w));
        return (w >> (16 * (i & 1))) & 65535u;
    }
};
template <> struct Row<FMT_F32> {
    uint4 a, b;
    __device__ __forceinline__ void load(const void* data, size_t first)
    {
        a = *reinterpret_cast<const uint4*>((const float*) data + first);
        b = *reinterpret_cast<const uint4*>((const float*) data + first + 4);
    }
    __device__ __forceinline__ uint32_t code(int i) const // the float's bits
    {
        const uint4& q = i < 4 ? a : b;
        return (i & 3) == 0 ? q.x : ((i & 3) == 1 ? q.y : ((i & 3) == 2 ? q.z : q.w));
    }
};

struct BrickAt {
    size_t first;  // element index of the brick's first voxel
    int bx, by, bz;
    bool whole;
};

// brick k of the box's brick list (k is uniform over the wave)
__device__ __forceinline__ BrickAt brick_at(const StatsParams& p, uint32_t k)
{
    BrickAt b;
    range_brick(p.range, k, b.bx, b.by, b.bz);
    b.first = grid_index(p.bnx, p.bnxy, b.bx, b.by, b.bz) * 512;
    const int x0 = b.bx * kBrick, y0 = b.by * kBrick, z0 = b.bz * kBrick;
    b.whole = x0 >= p.box.origin[0] && x0 + kBrick <= p.box.end[0] && y0 >= p.box.origin[1] && y0 + kBrick <= p.box.end[1] &&
              z0 >= p.box.origin[2] && z0 + kBrick <= p.box.end[2];
    return b;
}

// One count into a lane's LDS histogram, aggregated inside the wave first. Real scans are spikes — most of a CT is one air value —
// and 64 lanes adding 1 to one LDS word serialise. Two rounds of: take the first lane that still has something to add, ballot the
// lanes that hold the same bin, let that lane add the popcount once. A wave that holds one value throughout costs one LDS atomic;
// a wave that is 90 % one value leaves about six lanes for the plain atomics that follow, whatever bin its first lane holds
// (the second round takes the majority when the first took a stray). Called in wave-uniform control flow.
__device__ __forceinline__ void hist_add(uint32_t* hist, bool on, uint32_t bin, int lane)
{
    unsigned long long todo = __ballot(on);
#pragma unroll
    for (int round = 0; round < 2; ++round) {
        if (todo == 0ull) return;
        const int leader = __builtin_amdgcn_readfirstlane(__ffsll((long long) todo) - 1);
        const uint32_t b = (uint32_t) __builtin_amdgcn_readlane((int) bin, leader);
        const unsigned long long same = __ballot(on && bin == b);
        if (lane == leader) atomicAdd(&hist[b], (uint32_t) __popcll(same));
        on = on && bin != b;
        todo &= ~same;
    }
    if (on) atomicAdd(&hist[bin], 1u);
}

// the order-preserving map of the non-NaN floats onto uint32 (-inf lowest)
__device__ __forceinline__ uint32_t float_key(uint32_t bits) { return bits ^ ((bits >> 31) ? 0xffffffffu : 0x80000000u); }

} // namespace

// ---- the histogram ----------------------------------------------------------------------------------------------------------------
// Privatised: each workgroup keeps `copies` LDS histograms (copies * n_bins <= 4096 words, 16 KiB), a lane counting into copy
// (4 * wave + (lane & 3)) mod copies — with few bins the waves, and the lanes of a wave, would otherwise meet on the same words —,
// updates them with LDS integer atomics, and at the end adds the non-zero bins (the copies summed) to the uint32 global counters:
// consecutive lanes on consecutive bins, 256 contiguous bytes per wave instruction. The four tallies are kept per lane in
// registers and reduced once per wave.
template <int FMT, int MASKED>
__global__ __launch_bounds__(kStatsThreads) void k_volume_histogram(const StatsParams p)
{
    __shared__ uint32_t s_hist[kStatsMaxBins];
    __shared__ uint32_t s_tally[4];
    __shared__ uint32_t s_mask[8];
    const int tid = threadIdx.x, lane = tid & 63;
    const uint32_t wave = (uint32_t) __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t n_bins = p.n_bins;
    for (uint32_t i = tid; i < p.copies * n_bins; i += kStatsThreads) s_hist[i] = 0u;
    if (tid < 4) s_tally[tid] = 0u;
    if (tid < 8) s_mask[tid] = p.mask[tid];
    __syncthreads();
    uint32_t* const hist = s_hist + ((4u * wave + (uint32_t) (lane & 3)) & (p.copies - 1u)) * n_bins;

    const uint32_t total = (uint32_t) range_bricks(p.range);
    const uint32_t stride = gridDim.x * kStatsWaves;
    uint32_t below = 0u, above = 0u, nans = 0u, visited = 0u;
    const float n_bins_f = (float) n_bins;

    auto count_row = [&](const Row<FMT>& row, const uint2 lab, const uint32_t inside) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            bool on = (inside >> i) & 1u;
            if constexpr (MASKED) {
                const uint32_t l = byte_of(lab, i);
                on = on && ((s_mask[l >> 5] >> (l & 31)) & 1u);
            }
            uint32_t bin = 0u;
            bool binned = false;
            if constexpr (FMT == FMT_F32) {
                const float v = __uint_as_float(row.code(i));
                if (v != v) nans += on;
                else if (v < p.lo_f) below += on;
                else {
                    const float d = v - p.lo_f;
                    const float t = d * p.scale;
                    if (t < n_bins_f) { bin = (uint32_t) (int) t; binned = true; }
                    else if (v <= p.hi_f) { bin = n_bins - 1u; binned = true; }
                    else above += on;
                }
            } else {
                const uint32_t c = row.code(i);
                if (c < p.lo_code) below += on;
                else if (c > p.hi_code) above += on;
                else { bin = __umulhi((c - p.lo_code) * n_bins, p.div_mul) >> p.div_shift; binned = true; }
            }
            visited += on;
            hist_add(hist, on && binned, min(bin, n_bins - 1u), lane);
        }
    };

    uint32_t k = blockIdx.x * kStatsWaves + wave;
    Row<FMT> row, next_row;
    uint2 lab = make_uint2(0u, 0u), next_lab = make_uint2(0u, 0u);
    if (k < total) {
        const BrickAt b = brick_at(p, k);
        row.load(p.data, b.first + (size_t) lane * 8);
        if constexpr (MASKED) lab = *reinterpret_cast<const uint2*>(p.labels + b.first + (size_t) lane * 8);
    }
    while (k < total) {
        const uint32_t kn = k + stride;
        if (kn < total) { // the next brick's row is on its way while this one is counted
            const BrickAt bn = brick_at(p, kn);
            next_row.load(p.data, bn.first + (size_t) lane * 8);
            if constexpr (MASKED) next_lab = *reinterpret_cast<const uint2*>(p.labels + bn.first + (size_t) lane * 8);
        }
        const BrickAt b = brick_at(p, k);
        if (b.whole) count_row(row, lab, 0xffu);
        else count_row(row, lab, row_in_box(p.box, b.bx, b.by * kBrick + (lane & 7), b.bz * kBrick + (lane >> 3)));
        row = next_row;
        lab = next_lab;
        k = kn;
    }

    below = wave_sum(below); above = wave_sum(above); nans = wave_sum(nans); visited = wave_sum(visited);
    if (lane == 0) {
        if (below) atomicAdd(&s_tally[0], below);
        if (above) atomicAdd(&s_tally[1], above);
        if (nans) atomicAdd(&s_tally[2], nans);
        if (visited) atomicAdd(&s_tally[3], visited);
    }
    __syncthreads();
    for (uint32_t b = tid; b < n_bins; b += kStatsThreads) {
        uint32_t n = 0u;
        for (uint32_t c = 0; c < p.copies; ++c) n += s_hist[c * n_bins + b];
        if (n) atomicAdd(&p.out[b], n);
    }
    if (tid < 4 && s_tally[tid]) atomicAdd(&p.out[n_bins + tid], s_tally[tid]);
}

hipError_t launch_volume_histogram(const StatsParams& p, bool masked, int grid, hipStream_t s)
{
    if (grid <= 0) return hipSuccess;
#define TBRM_HIST(F)                                                                                              \
    do {                                                                                                          \
        if (masked) hipLaunchKernelGGL((k_volume_histogram<F, 1>), dim3(grid), dim3(kStatsThreads), 0, s, p);     \
        else hipLaunchKernelGGL((k_volume_histogram<F, 0>), dim3(grid), dim3(kStatsThreads), 0, s, p);            \
    } while (0)
    switch (p.fmt) {
        case FMT_U8: TBRM_HIST(FMT_U8); break;
        case FMT_U16: TBRM_HIST(FMT_U16); break;
        default: TBRM_HIST(FMT_F32); break;
    }
#undef TBRM_HIST
    return hipGetLastError();
}

// ---- per-label statistics -----------------------------------------------------------------------------------------------------------
// 256 LDS records per workgroup: count, nan count, sum (uint64 of codes / float64), ~min key and max key (uint32: the code, or the
// order-preserving key of the float — both kept as maxima, so that all-zero words are the empty record).
//   Segments are coherent: most bricks hold ONE label (always, without a label volume). A wave keeps registers for the label of the
// last such brick it saw — per lane count / nan / sum / min / max — and counts a one-label brick into them with no atomics at all;
// a one-label brick of another label reduces the registers over the wave into the LDS record (a few shuffles) and starts over.
// Only bricks that mix labels, and cut bricks of a labelled volume, go voxel by voxel through LDS atomics.
//   The integer results are deterministic; the float64 sum depends on the order the partial sums meet.
template <int FMT, int LABELS>
__global__ __launch_bounds__(kStatsThreads) void k_label_statistics(const StatsParams p)
{
    using Sum = typename std::conditional<FMT == FMT_F32, double, unsigned long long>::type;
    __shared__ uint32_t s_count[256], s_nan[256], s_min_inv[256], s_max[256];
    __shared__ Sum s_sum[256];
    const int tid = threadIdx.x, lane = tid & 63;
    const uint32_t wave = (uint32_t) __builtin_amdgcn_readfirstlane(tid >> 6);
    s_count[tid] = 0u; s_nan[tid] = 0u; s_min_inv[tid] = 0u; s_max[tid] = 0u; s_sum[tid] = Sum(0);
    __syncthreads();

    const uint32_t total = (uint32_t) range_bricks(p.range);
    const uint32_t stride = gridDim.x * kStatsWaves;
    // the registers of label `cur` (uniform over the wave; -1: none yet)
    int cur = -1;
    uint32_t r_count = 0u, r_nan = 0u, r_min = 0xffffffffu, r_max = 0u;
    Sum r_sum = Sum(0);
    bool r_any = false; // (this lane has seen a non-NaN voxel)

    auto flush_registers = [&]() {
        if (cur < 0) return;
        const uint32_t n = wave_sum(r_count), nn = wave_sum(r_nan);
        uint32_t mn = r_any ? ~r_min : 0u, mx = r_any ? r_max : 0u;
        Sum sum = r_sum;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            mn = max(mn, (uint32_t) __shfl_xor(mn, o, 64));
            mx = max(mx, (uint32_t) __shfl_xor(mx, o, 64));
            sum += __shfl_xor(sum, o, 64);
        }
        const bool any = __ballot(r_any) != 0ull;
        if (lane == 0 && n) {
            atomicAdd(&s_count[cur], n);
            if (nn) atomicAdd(&s_nan[cur], nn);
            if (any) {
                atomicAdd(&s_sum[cur], sum);
                atomicMax(&s_min_inv[cur], mn);
                atomicMax(&s_max[cur], mx);
            }
        }
        r_count = 0u; r_nan = 0u; r_min = 0xffffffffu; r_max = 0u; r_sum = Sum(0); r_any = false;
    };

    uint32_t k = blockIdx.x * kStatsWaves + wave;
    Row<FMT> row, next_row;
    uint2 lab = make_uint2(0u, 0u), next_lab = make_uint2(0u, 0u);
    if (k < total) {
        const BrickAt b = brick_at(p, k);
        row.load(p.data, b.first + (size_t) lane * 8);
        if constexpr (LABELS) lab = *reinterpret_cast<const uint2*>(p.labels + b.first + (size_t) lane * 8);
    }
    while (k < total) {
        const uint32_t kn = k + stride;
        if (kn < total) {
            const BrickAt bn = brick_at(p, kn);
            next_row.load(p.data, bn.first + (size_t) lane * 8);
            if constexpr (LABELS) next_lab = *reinterpret_cast<const uint2*>(p.labels + bn.first + (size_t) lane * 8);
        }
        const BrickAt b = brick_at(p, k);
        const uint32_t inside = b.whole ? 0xffu : row_in_box(p.box, b.bx, b.by * kBrick + (lane & 7), b.bz * kBrick + (lane >> 3));
        int one_label = 0; // the brick's label when it holds one label only, else -1
        if constexpr (LABELS) {
            const uint32_t first = (uint32_t) __builtin_amdgcn_readfirstlane((int) (lab.x & 255u));
            const bool same = lab.x == first * 0x01010101u && lab.y == first * 0x01010101u;
            one_label = (b.whole && __ballot(same) == ~0ull) ? (int) first : -1;
        }
        if (one_label >= 0) {
            if (one_label != cur) { flush_registers(); cur = one_label; }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const bool on = (inside >> i) & 1u;
                const uint32_t c = row.code(i);
                if constexpr (FMT == FMT_F32) {
                    const float v = __uint_as_float(c);
                    if (v != v) r_nan += on;
                    else if (on) { r_sum += (double) v; r_min = min(r_min, float_key(c)); r_max = max(r_max, float_key(c)); r_any = true; }
                } else if (on) { r_sum += c; r_min = min(r_min, c); r_max = max(r_max, c); r_any = true; }
                r_count += on;
            }
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                if (!((inside >> i) & 1u)) continue;
                const uint32_t l = byte_of(lab, i);
                const uint32_t c = row.code(i);
                atomicAdd(&s_count[l], 1u);
                if constexpr (FMT == FMT_F32) {
                    const float v = __uint_as_float(c);
                    if (v != v) atomicAdd(&s_nan[l], 1u);
                    else { atomicAdd(&s_sum[l], (double) v); atomicMax(&s_min_inv[l], ~float_key(c)); atomicMax(&s_max[l], float_key(c)); }
                } else { atomicAdd(&s_sum[l], (unsigned long long) c); atomicMax(&s_min_inv[l], ~c); atomicMax(&s_max[l], c); }
            }
        }
        row = next_row;
        lab = next_lab;
        k = kn;
    }
    flush_registers();
    __syncthreads();
    if (s_count[tid]) { // one record per thread; what is added is bounded by the grid
        atomicAdd(&p.out[tid], s_count[tid]);
        if (s_nan[tid]) atomicAdd(&p.out[256 + tid], s_nan[tid]);
        if (s_count[tid] > s_nan[tid]) {
            atomicMax(&p.out[512 + tid], s_min_inv[tid]);
            atomicMax(&p.out[768 + tid], s_max[tid]);
            atomicAdd(reinterpret_cast<Sum*>(p.out + 1024) + tid, s_sum[tid]);
        }
    }
}

hipError_t launch_label_statistics(const StatsParams& p, int grid, hipStream_t s)
{
    if (grid <= 0) return hipSuccess;
#define TBRM_LSTAT(F)                                                                                             \
    do {                                                                                                          \
        if (p.labels) hipLaunchKernelGGL((k_label_statistics<F, 1>), dim3(grid), dim3(kStatsThreads), 0, s, p);   \
        else hipLaunchKernelGGL((k_label_statistics<F, 0>), dim3(grid), dim3(kStatsThreads), 0, s, p);            \
    } while (0)
    switch (p.fmt) {
        case FMT_U8: TBRM_LSTAT(FMT_U8); break;
        case FMT_U16: TBRM_LSTAT(FMT_U16); break;
        default: TBRM_LSTAT(FMT_F32); break;
    }
#undef TBRM_LSTAT
    return hipGetLastError();
}

} // namespace tbrm
