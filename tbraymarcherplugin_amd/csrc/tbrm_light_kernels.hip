// tbrm_light_kernels.hip — gfx950 kernels of the illumination pass (Sunden/Ropinski selective light updates).
//
//   k_occ_flags, k_occ_compact        : once per axis pass — which 16x16x8 occlusion blocks can only see empty bricks,
//                                       and per span the ascending list of the blocks that cannot.
//   k_light_occlusion                 : once per span of up to 128 slices — the factor 1 - CurrentSample
//                                       (AddDirLightShader.usf:85-117) of every voxel of the span, no halo, fully
//                                       parallel, live blocks dealt evenly over the CUs from the list.
//   k_light_sweep (tbrm_light_sweep.hip): once per axis pass — every 32x32 tile of the slice plane walks ALL slices of the
//                                       pass, the tiles a pipeline with dword hand-offs through memory (UNORM8 light
//                                       volumes, passes of whole brick layers: what a loaded scan produces).
//   k_light_chain (tbrm_light_chain.hip): once per chunk of 16 / 8 / 4 / 2 slices — advances EVERY 32x32 tile of the
//                                       slice plane through the chunk, recomputing a halo instead of waiting for its
//                                       neighbours: the passes the sweep declines, and slab-partitioned passes.
//   k_propagate_slice                 : the reference's structure, one slice per launch (AddDirLightShader.usf:68-128,
//                                       ChangeDirLightShader.usf:74-156). Fallback for passes the chunk kernels
//                                       decline (degenerate offsets) and the A/B baseline (tunable force_slice_kernel).
//
// Why chunks work: slice k only needs the previous slice's propagated light inside a small bilinear footprint,
// offset by the constant PrevPixelOffset. A workgroup that owns a 32x32 tile at the END of a chunk therefore only
// needs a (32 + steps*g)^2 window of the plane at the START of the chunk (g = width of the footprint in texels,
// normally 1) and recomputes that shrinking window privately in LDS — no inter-workgroup traffic inside a chunk,
// one kernel boundary between chunks. The expensive part of a voxel — the windowed, opacity-corrected data sample
// "CurrentSample" (AddDirLightShader.usf:85-114) — does not depend on the propagated light, so it is computed once per
// voxel, without halo, by k_light_occlusion and handed over through a scratch plane stack that k_light_chain stages
// into LDS with asynchronous global->LDS copies two slices ahead of their use; the chain itself is then a handful of
// LDS reads and one multiply per voxel, with no memory latency between slices. Arithmetic per voxel is exactly the
// reference's, including the per-slice UNORM8 re-quantisation of the propagated light (RaymarchVolume.cpp:857-866).
#include "tbrm_device_sampling.h"
#include "tbrm_light_chain.h"

#include <type_traits>

namespace tbrm {

// ------------------------------------------------------------------------------------------------------------
// one slice per launch

template <int LFMT>
__device__ __forceinline__ float sample_buffer_bilinear(const void* buf, int w, int h, float u, float v, float border)
{
    int ix, iy;
    float fx, fy;
    texel_split(u, (float) w, ix, fx);
    texel_split(v, (float) h, iy, fy);
    float t[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int x = ix + (k & 1), y = iy + (k >> 1);
        const bool in = (unsigned) x < (unsigned) w && (unsigned) y < (unsigned) h;
        t[k] = in ? load_voxel<LFMT>(buf, (size_t) y * w + x) : border;
    }
    return lerp_(lerp_(t[0], t[1], fx), lerp_(t[2], t[3], fx), fy);
}

template <int DFMT, int LFMT, bool GUARD>
__device__ __forceinline__ float propagate_stream(const PropParams& p, const PropStream& s, const float* tf_alpha,
                                                  int px, int py, const int* pos)
{
    const float pu = (((float) (uint32_t) px + 0.5f) / (float) p.td[0]) + s.off_u;
    const float pv = (((float) (uint32_t) py + 0.5f) / (float) p.td[1]) + s.off_v;
    const float prev = sample_buffer_bilinear<LFMT>(s.read, p.td[0], p.td[1], pu, pv, s.border_light);

    const float u = sample_coord(pos[0], p.lv_dims[0], s.uvw_off[0]), v = sample_coord(pos[1], p.lv_dims[1], s.uvw_off[1]), w = sample_coord(pos[2], p.lv_dims[2], s.uvw_off[2]);

    const float aw = p.clip_mode ? clip_alpha_weight(u, v, w, p.cc, p.cd, p.lv_dims) : 1.0f;
    float cur = 0.0f;
    bool inside = true;
    if constexpr (GUARD) inside = (u == saturate_(u)) && (v == saturate_(v)) && (w == saturate_(w));
    if (aw > 0.0f && inside) {
        const float val = sample_trilinear_border_uvw<DFMT>(p.data, u, v, w, p.data_border);
        cur = windowed_alpha<DFMT != FMT_F32>(val, s.step100, tf_alpha, p.win) * aw;
    }
    return prev * (1 - cur);
}

template <int DFMT, int LFMT, bool CHANGE>
__global__ __launch_bounds__(256) void k_propagate_slice(const PropParams p)
{
    __shared__ float s_alpha[256];
    s_alpha[threadIdx.x] = p.tf[threadIdx.x].w;
    __syncthreads();
    const int px = blockIdx.x * 16 + (threadIdx.x & 15);
    const int py = (blockIdx.y + p.row_block0) * 16 + (threadIdx.x >> 4);
    if (px >= p.td[0] || py >= p.td[1]) return; // D3D drops the overhanging threads' writes
    int pos[3];
    if (p.axis == 0) { pos[0] = p.loop; pos[1] = px; pos[2] = py; }
    else if (p.axis == 1) { pos[0] = px; pos[1] = p.loop; pos[2] = py; }
    else { pos[0] = px; pos[1] = py; pos[2] = p.loop; }
    const size_t bi = (size_t) py * p.td[0] + px;
    const size_t li = brick_off(pos[0], pos[1], pos[2], p.lv_bnx, p.lv_bnxy);
    if constexpr (!CHANGE) {
        const float l = propagate_stream<DFMT, LFMT, true>(p, p.a, s_alpha, px, py, pos);
        store_voxel<LFMT>(p.a.write, bi, l);
        if (fabsf(l) > 1e-3f) store_voxel<LFMT>(p.light, li, load_voxel<LFMT>(p.light, li) + (l * p.b_added));
    } else {
        const float lr = propagate_stream<DFMT, LFMT, false>(p, p.r, s_alpha, px, py, pos);
        const float la = propagate_stream<DFMT, LFMT, false>(p, p.a, s_alpha, px, py, pos);
        store_voxel<LFMT>(p.r.write, bi, lr);
        store_voxel<LFMT>(p.a.write, bi, la);
        if (fabsf(la - lr) > 1e-3f) store_voxel<LFMT>(p.light, li, load_voxel<LFMT>(p.light, li) + la - lr);
    }
}

template <int DFMT, int LFMT>
static hipError_t launch_prop2(const PropParams& p, bool change, hipStream_t s)
{
    const dim3 grid((p.td[0] + 15) / 16, p.row_blocks > 0 ? p.row_blocks : (p.td[1] + 15) / 16), block(256);
    if (change) hipLaunchKernelGGL((k_propagate_slice<DFMT, LFMT, true>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((k_propagate_slice<DFMT, LFMT, false>), grid, block, 0, s, p);
    return hipGetLastError();
}
template <int DFMT>
static hipError_t launch_prop1(const PropParams& p, bool change, hipStream_t s)
{
    return p.lv_fmt == FMT_U8 ? launch_prop2<DFMT, FMT_U8>(p, change, s) : launch_prop2<DFMT, FMT_F32>(p, change, s);
}
hipError_t launch_propagate_slice(const PropParams& p, bool change, hipStream_t s)
{
    switch (p.data.fmt) {
        case FMT_U8: return launch_prop1<FMT_U8>(p, change, s);
        case FMT_U16: return launch_prop1<FMT_U16>(p, change, s);
        default: return launch_prop1<FMT_F32>(p, change, s);
    }
}

// ------------------------------------------------------------------------------------------------------------
// a chunk of slices per launch pair

// LDS bytes of a chain workgroup; 1 GiB when no instantiated kernel shape holds the chunk's hull
// (tbrm_light_chain.hip launch_chain3 lists the shapes: square planes of RS 40 / 56 for everything, 72 for a plain Add —
// ten 72 x 72 planes exceed the LDS — and the rectangular 72 x 48 / 56 x 64 for an Add, UNORM8)
size_t chunk_lds_bytes(const ChunkParams& p, int mode, int lv_fmt)
{
    const ChunkGeom g = chunk_geometry(p);
    const int ns = mode == PASS_ADD ? 1 : 2; // streams propagated = planes staged per slice
    const bool rect = g.RR != g.RS; // 72 x 48 / 56 x 64: instantiated for an Add over a UNORM8 light volume
    if (rect && !(mode == PASS_ADD && lv_fmt == FMT_U8)) return (size_t) 1 << 30;
    if (rect && g.HX * g.HY - kChunkTile * kChunkTile > 2 * kChunkThreads) return (size_t) 1 << 30; // (two halo slots per thread)
    if (g.RS == 0 || (mode != PASS_ADD && !rect && g.RS > 56)) return (size_t) 1 << 30;
    size_t total = (size_t) (2 * ns + kOccRing * ns) * chain_plane_elems(g.RS, g.RR) * 4; // windows + staged ring
    if (lv_fmt == FMT_U8) total += (size_t) 16 * g.lv_layers * 512;                        // light-volume tile
    return total;
}

// ---- k_light_occlusion: CurrentSample (AddDirLightShader.usf:85-114) for every voxel of a chunk ------------------
// One workgroup = 16x16 plane pixels x 8 slices. It first copies every data brick its samples can touch into LDS
// with coalesced 16-byte global->LDS copies (a few dozen wide vector-memory instructions), then each thread filters
// its 8 samples out of LDS: the 8 narrow gather loads per sample that bounded the first version (the texture-address
// path handles ~one 64-lane gather per 20 cycles) become LDS reads. Addressing is separable in the bricked layout:
// the two in-plane axes contribute per-thread constants, the slice axis a per-step value from a small LDS table
// (which also carries the reference's per-thread (Loop+0.5)/res division out of the loop).
// The unit's size, the sample coordinate, tap spans, brick ranges, the staging decision and the staged block's layout are
// tbrm_occ_footprint.h's; the pieces of the sample loop that the kernel's forms share follow here.

struct AxisTaps {        // one axis of a trilinear footprint with border addressing
    int i0;              // base tap index (unclamped)
    bool ok0, ok1;       // tap inside the volume (else the sampler's border colour applies)
    float f;             // interpolation weight
};

__device__ __forceinline__ AxisTaps axis_taps(float coord, int n)
{
    AxisTaps t;
    texel_split(coord, (float) n, t.i0, t.f);
    t.ok0 = (unsigned) t.i0 < (unsigned) n;
    t.ok1 = (unsigned) (t.i0 + 1) < (unsigned) n;
    return t;
}

template <int FMT>
__device__ __forceinline__ float lds_voxel(const void* p, uint32_t i)
{
    if constexpr (FMT == FMT_U8) return decode_u8(((const uint8_t*) p)[i]);
    else if constexpr (FMT == FMT_U16) return decode_u16(((const uint16_t*) p)[i]);
    else return ((const float*) p)[i];
}

constexpr int fmt_bytes(int fmt) { return fmt == FMT_U8 ? 1 : (fmt == FMT_U16 ? 2 : 4); }

// LDS bytes for the staged bricks: worst case over workgroups, from the ratio of data to light-volume resolution
size_t occlusion_lds_bytes(const ChunkParams& p)
{
    const int dd[3] = {p.data.nx, p.data.ny, p.data.nz};
    return occ_lds_estimate(dd, p.lv_dims, p.axis, fmt_bytes(p.data.fmt));
}

// ---- the pieces of the sample loop that k_light_occlusion and k_light_occlusion_runs share ---------------------------------------
// the transfer function's alpha as pairs (alpha[clamp(i)], alpha[clamp(i + 1)]) at i + 1 (sample_tf_alpha), one texel per thread
__device__ __forceinline__ void fill_alpha_pairs(float2 (&s_alpha)[257], const float4* tf)
{
    const float a_t = tf[threadIdx.x].w, a_n = tf[min((int) threadIdx.x + 1, 255)].w;
    s_alpha[threadIdx.x + 1] = make_float2(a_t, a_n);
    if (threadIdx.x == 0) s_alpha[0] = make_float2(a_t, a_t);
}

// What a slice contributes to each of its samples (wave-uniform): the slice-axis coordinate, its texel split and
// flags: bit0 tap0 in range, bit1 tap1 in range, bit2 w == saturate(w)
struct OccSliceEntry {
    float w, f;
    int i0, flags;
};
__device__ __forceinline__ OccSliceEntry occ_slice_entry(int j, int lv_dim, float uvw_off, int data_dim)
{
    OccSliceEntry e;
    e.w = sample_coord(j, lv_dim, uvw_off);
    const AxisTaps t = axis_taps(e.w, data_dim);
    e.f = t.f;
    e.i0 = t.i0;
    e.flags = (t.ok0 ? 1 : 0) | (t.ok1 ? 2 : 0) | ((e.w == saturate_(e.w)) ? 4 : 0);
    return e;
}

// one tap: from the staged block in LDS or the bricked volume; outside the volume (never, in an INTERIOR unit) the border colour
template <int DFMT, bool STAGED, bool INTERIOR>
__device__ __forceinline__ float occ_tap(const char* smem, const void* data, uint32_t off, bool ok, float border)
{
    if constexpr (INTERIOR) return STAGED ? lds_voxel<DFMT>(smem, off) : load_voxel<DFMT>(data, off);
    else return ok ? (STAGED ? lds_voxel<DFMT>(smem, off) : load_voxel<DFMT>(data, off)) : border;
}

// The sample loop is specialised on workgroup-uniform facts so that the common case carries no dead branches:
//   STAGED   taps come from LDS (else from global memory: a workgroup whose bricks did not fit)
//   INTERIOR every tap of every sample lies inside the volume (no border-colour selects)
//   CLIP     the clip plane can change a sample's weight (else AlphaWeight is exactly 1)
//   NONNEG   the opacity correction's step sizes are >= 0 (they are unless the host was handed garbage)
// f(STAGED, INTERIOR, CLIP, NONNEG) is called with the form's constants. NONNEG is decided once per unit over all its streams' step
// sizes (the NONNEG = false forms compute the same bits for steps >= 0, so a stream that alone would qualify loses nothing but time).
template <class NN, class F>
__device__ __forceinline__ void occ_forms_of(bool staged, bool interior, bool clip, NN nonneg_c, F& f)
{
    using T_ = std::true_type; using F_ = std::false_type;
    if (staged && interior && !clip) f(T_{}, T_{}, F_{}, nonneg_c); // the common case
    else if (staged && !clip) f(T_{}, F_{}, F_{}, nonneg_c);         // shell of the volume
    else if (staged) f(T_{}, F_{}, T_{}, nonneg_c);                  // clip plane active
    else f(F_{}, F_{}, T_{}, nonneg_c);                              // bricks did not fit in LDS
}
template <class F>
__device__ __forceinline__ void occ_forms(bool staged, bool interior, bool clip, bool nonneg, F& f)
{
    if (nonneg) occ_forms_of(staged, interior, clip, std::true_type{}, f);
    else occ_forms_of(staged, interior, clip, std::false_type{}, f);
}

// The held-plane window. A texel plane of the footprint is the taps at one slice-axis coordinate, reduced as far as the filter
// order (x, then y, then z) allows before the slice-axis weight is applied (P: 1, 2 or 4 values). Consecutive slices of a pass
// usually sample consecutive texel planes, so the +1 plane of one step is the base plane of the next: `lo` (texel index `held`)
// and `hi` (the plane after it) are kept in registers and only one new plane is fetched per step instead of two. i is wave-uniform:
// scalar branches. fetch(upper) fetches the plane at i (false) or i + 1 (true).
template <class P, class Fetch>
__device__ __forceinline__ void held_planes_step(P& lo, P& hi, int& held, int i, Fetch&& fetch)
{
    if (i == held + 1) { lo = hi; hi = fetch(true); }
    else if (i == held - 1) { hi = lo; lo = fetch(false); }
    else if (i != held) { lo = fetch(false); hi = fetch(true); }
    held = i;
}
constexpr int kNoPlaneHeld = INT32_MIN / 2;

// One sample: clip weight (c0 .. c2: its coordinate in the volume's axis order), the Add shader's guard, the windowed and
// opacity-corrected alpha of value() for one step size (occ0) or two (DUAL: occ0, occ1), times the weight.
template <int DFMT, bool CLIP, bool NONNEG, bool DUAL, class V>
__device__ __forceinline__ void occ_sample(const ChunkParams& p, float c0, float c1, float c2, bool inside, V&& value, float step0, float step1, const float2* s_alpha, float& occ0, float& occ1)
{
    float aw = 1.0f;
    if constexpr (CLIP) aw = clip_alpha_weight(c0, c1, c2, p.cc, p.cd, p.lv_dims);
    occ0 = 0.0f;
    occ1 = 0.0f;
    if (aw > 0.0f && inside) {
        if constexpr (DUAL) {
            windowed_alpha2<DFMT != FMT_F32, NONNEG>(value(), step0, step1, s_alpha, p.win, occ0, occ1);
            occ0 = occ0 * aw;
            occ1 = occ1 * aw;
        } else occ0 = windowed_alpha<DFMT != FMT_F32, NONNEG>(value(), step0, s_alpha, p.win) * aw;
    }
}

// slice q's factors of a dual launch into the two passes' blocks (null: block flagged empty)
__device__ __forceinline__ void dual_store(float* const* out2, const int* step, int q, float occ0, float occ1)
{
    if (out2[0]) out2[0][q * step[0]] = 1 - occ0;
    if (out2[1]) out2[1][q * step[1]] = 1 - occ1;
}

// ---- k_occ_flags: once per pass, which occlusion workgroups are empty ---------------------------------------------
// One thread per occlusion workgroup (16x16 pixels x 8 slices of one chunk). The workgroup is empty when the brick of
// every sample's base tap has its k_brick_empty bit set: the bit vouches for every value the 8 taps of a sample based
// in that brick can take (the brick plus its +1 apron), so every CurrentSample is exactly 0. Workgroups with taps
// outside the volume are never flagged (a blend with the sampler's border colour can leave both value ranges).
template <int NS, int AXIS>
__global__ __launch_bounds__(256) void k_occ_flags(const ChunkParams p, int n_chunks)
{
    const int per_chunk = p.occ_groups * p.occ_blocks_y * p.occ_blocks_x;
    const int id = blockIdx.x * 256 + threadIdx.x;
    if (id >= n_chunks * per_chunk) return;
    const int c = id / per_chunk, rem = id % per_chunk;
    const int bx = rem % p.occ_blocks_x, by = (rem / p.occ_blocks_x) % p.occ_blocks_y, zg = rem / (p.occ_blocks_x * p.occ_blocks_y);
    uint8_t flag = 0;
    if (by < p.roi_by0 || by >= p.roi_by1) flag = 1; // outside the slab's reach: never computed, never read
    else {
        OccPassShape s = occ_pass_shape(p, NS, c);
        s.axis = AXIS;
        const int bn[3] = {p.data.bnx, p.data.bnxy / p.data.bnx, (p.data.nz + 7) >> 3};
        constexpr int dims[3] = {AXIS == 0 ? 1 : 0, AXIS == 2 ? 1 : 2, AXIS}; // plane axes, slice axis -> volume axes
        const int index[3] = {bx, by, zg};
        bool ok = true; // every tap inside the volume (and the group not past the chunk's last slice)
        int b0[3], nb[3];
#pragma unroll
        for (int part = 0; part < 3; ++part) {
            int lo, hi;
            bool border = true;
            if (pass_tap_span(s, part, index[part], lo, hi)) brick_span(lo, hi, s.data_dims[dims[part]], bn[dims[part]], b0[dims[part]], nb[dims[part]], border);
            ok = ok && !border;
        }
        if (ok) {
            for (int z = b0[2]; z < b0[2] + nb[2] && ok; ++z)
                for (int y = b0[1]; y < b0[1] + nb[1] && ok; ++y)
                    for (int x = b0[0]; x < b0[0] + nb[0]; ++x) {
                        const int b = z * p.data.bnxy + y * p.data.bnx + x;
                        if (!((p.empty_bits[b >> 5] >> (b & 31)) & 1u)) { ok = false; break; }
                    }
            flag = ok ? 1 : 0;
        }
    }
    p.occ_flags_out[id] = flag;
}

// ---- k_occ_compact: per chunk, the ascending list of workgroups that are NOT flagged -----------------------------
// A workgroup takes a segment of 4096 of the chunk's flags (16 per thread, one 16-byte load). It first counts the live
// flags of every segment before its own — up to 64 KiB of coalesced reads out of the L2, instead of a second kernel or a
// chain of workgroups waiting for each other — then scans its own: every live workgroup gets its list position
// (deterministic, ascending) and, if wanted, every block its rank (-1: flagged). Flags are bytes of 0 / 1.
constexpr int kCompactSeg = 4096;
__global__ __launch_bounds__(256) void k_occ_compact(const ChunkParams p, int segs)
{
    constexpr int NT = 256;
    __shared__ int s_scan[NT];
    __shared__ int s_base;
    const int per_chunk = p.occ_groups * p.occ_blocks_y * p.occ_blocks_x;
    const int c = (int) blockIdx.x / segs, seg = (int) blockIdx.x % segs;
    const uint8_t* flags = p.occ_flags_out + (size_t) c * per_chunk;
    uint32_t* list = p.occ_list_out + (size_t) c * per_chunk;
    int32_t* const slot = p.occ_slot_out ? p.occ_slot_out + (size_t) c * per_chunk : nullptr;
    const int n = min(p.chunk_slices, p.pass_slices - c * p.chunk_slices);
    const int live_groups = (n + kOccDepth - 1) / kOccDepth;       // slice groups past the chunk's last slice have no work
    const int live = live_groups * p.occ_blocks_y * p.occ_blocks_x;
    const bool wide = (((size_t) flags) & 15) == 0;
    // 16 flags from position i on as four words (bytes past the live part read as flagged)
    auto load16 = [&](int i, uint32_t (&w)[4]) {
        if (wide && i + 16 <= live) {
            const uint4 v = *(const uint4*) (flags + i);
            w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                w[k] = 0;
#pragma unroll
                for (int b = 0; b < 4; ++b) w[k] |= (uint32_t) ((i + 4 * k + b < live) ? (flags[i + 4 * k + b] ? 1u : 0u) : 1u) << (8 * b);
            }
        }
    };
    auto live_of = [](const uint32_t (&w)[4]) { return 16 - (__builtin_popcount(w[0] & 0x01010101u) + __builtin_popcount(w[1] & 0x01010101u) + __builtin_popcount(w[2] & 0x01010101u) + __builtin_popcount(w[3] & 0x01010101u)); };
    // live flags before this segment
    int before = 0;
    for (int i = (int) threadIdx.x * 16; i < seg * kCompactSeg; i += NT * 16) {
        uint32_t w[4];
        load16(i, w);
        before += live_of(w);
    }
    s_scan[threadIdx.x] = before;
    __syncthreads();
    for (int d = NT / 2; d > 0; d >>= 1) {
        if ((int) threadIdx.x < d) s_scan[threadIdx.x] += s_scan[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0) s_base = s_scan[0];
    __syncthreads();
    const int base = s_base;
    __syncthreads();
    // this segment
    const int i0 = seg * kCompactSeg + (int) threadIdx.x * 16;
    uint32_t w[4] = {0x01010101u, 0x01010101u, 0x01010101u, 0x01010101u};
    if (i0 < per_chunk) load16(i0, w);
    const int mine = i0 < per_chunk ? live_of(w) : 0;
    s_scan[threadIdx.x] = mine;
    __syncthreads();
    for (int d = 1; d < NT; d <<= 1) { // inclusive Hillis-Steele scan
        const int v = (int) threadIdx.x >= d ? s_scan[threadIdx.x - d] : 0;
        __syncthreads();
        s_scan[threadIdx.x] += v;
        __syncthreads();
    }
    int pos = base + s_scan[threadIdx.x] - mine;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int i = i0 + k;
        if (i >= per_chunk) break;
        const bool flagged = ((w[k >> 2] >> (8 * (k & 3))) & 1u) != 0;
        if (slot) slot[i] = flagged ? -1 : pos;
        if (!flagged) list[pos++] = (uint32_t) i;
    }
    if (seg == segs - 1 && threadIdx.x == NT - 1) {
        p.occ_count_out[c] = base + s_scan[NT - 1];
        if (p.occ_count_host && c == 0) *p.occ_count_host = base + s_scan[NT - 1]; // (visible to the host once an event behind the launch has completed)
    }
}

template <int NS> // (flags only depend on the stream count)
static hipError_t launch_flags2(const ChunkParams& p, int n_chunks, hipStream_t s)
{
    const int total = n_chunks * p.occ_groups * p.occ_blocks_y * p.occ_blocks_x;
    const dim3 grid((total + 255) / 256), block(256);
    if (p.axis == 0) hipLaunchKernelGGL((k_occ_flags<NS, 0>), grid, block, 0, s, p, n_chunks);
    else if (p.axis == 1) hipLaunchKernelGGL((k_occ_flags<NS, 1>), grid, block, 0, s, p, n_chunks);
    else hipLaunchKernelGGL((k_occ_flags<NS, 2>), grid, block, 0, s, p, n_chunks);
    if (p.occ_list_out) {
        const int per_chunk = p.occ_groups * p.occ_blocks_y * p.occ_blocks_x, segs = (per_chunk + kCompactSeg - 1) / kCompactSeg;
        hipLaunchKernelGGL(k_occ_compact, dim3(n_chunks * segs), dim3(256), 0, s, p, segs);
    }
    return hipGetLastError();
}
hipError_t launch_occ_flags(const ChunkParams& p, int mode, int n_chunks, hipStream_t s)
{
    return occ_mode_streams(mode) == 1 ? launch_flags2<1>(p, n_chunks, s) : launch_flags2<2>(p, n_chunks, s);
}

// DUAL (tbrm_internal.h DualOcc): the launch walks the light volume as a virtual pass along AXIS (z: see DualOcc) and every
// voxel's sample serves both real passes — one filter, one transfer-function look-up, one logarithm, two exponents.
template <int DFMT, int MODE, int AXIS, bool DUAL = false>
#ifndef TBRM_OCC_WAVES_PER_EU
#define TBRM_OCC_WAVES_PER_EU 5
#endif
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(TBRM_OCC_WAVES_PER_EU, 8))) void k_light_occlusion(const ChunkParams p, int lds_budget_bytes, const DualOcc d)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NS = occ_mode_streams(MODE);
    constexpr bool GUARD = MODE == PASS_ADD || MODE == PASS_ADD2; // all(uvw == saturate(uvw)): the Add shader only (AddDirLightShader.usf:98)
    constexpr int ESZ = fmt_bytes(DFMT);
    __shared__ float2 s_alpha[257];
    __shared__ float s_w[2][kOccDepth], s_f[2][kOccDepth]; // the slice-table entries (OccSliceEntry), [stream][slice]
    __shared__ int s_i[2][kOccDepth], s_flags[2][kOccDepth];
    __shared__ int s_b0[3], s_nb[3], s_staged, s_interior;
    __shared__ uint32_t s_o0[2][kOccDepth], s_o1[2][kOccDepth];
    __shared__ int s_ends[12], s_end_dim[12];
    __shared__ uint32_t s_brick[kOccMaxBricks];

    constexpr int dim_u = AXIS == 0 ? 1 : 0, dim_v = AXIS == 2 ? 1 : 2, dim_s = AXIS; // plane axes -> volume axes
    const int data_dims[3] = {p.data.nx, p.data.ny, p.data.nz};
    // The launch is a 1-D grid rounded up to a multiple of 8 workgroups. Workgroups are dealt to the 8 XCDs round-robin by
    // id (an affinity used for speed only): XCD x takes the x-th eighth of the work, so blocks that are neighbours in the
    // volume — and stage the same halo bricks — run behind the same L2.
    //
    // The grid may be smaller than the work (a launch that runs beside the chain of the previous span on the occlusion
    // stream, tbrm_light_enqueue.cpp, holds only as many workgroups as fit next to the chain's on every CU, all resident from
    // the start, so none is ever waiting to take a slot the next chain launch needs): a workgroup then walks its XCD's
    // eighth with the stride of the grid.
    const int groups = (p.n_steps + kOccDepth - 1) / kOccDepth;
    const int total = p.occ_list ? *p.occ_count : groups * p.occ_blocks_y * p.occ_blocks_x;
    const int per_xcd = (total + 7) >> 3;
    const int xcd_stride = (int) gridDim.x >> 3;
  for (int slot = (int) blockIdx.x >> 3; slot < per_xcd; slot += xcd_stride) {
    const int entry = ((int) blockIdx.x & 7) * per_xcd + slot;
    if (entry >= total) break;
    if (slot != ((int) blockIdx.x >> 3)) __syncthreads(); // the previous block's tables and staged bricks are done with
    // which block of the span: the entry itself, or (sparse spans) that entry of the span's work list — workgroups flagged
    // empty by k_occ_flags (every CurrentSample exactly 0, and the chain knows it) are not on the list
    const int id = p.occ_list ? (int) p.occ_list[entry] : entry;
    const int gx = id % p.occ_blocks_x, gy = (id / p.occ_blocks_x) % p.occ_blocks_y, gz = id / (p.occ_blocks_x * p.occ_blocks_y);
    if (!p.occ_list && p.occ_flags && p.occ_flags[id]) continue; // list off (A/B runs)
    if (gy < p.roi_by0 || gy >= p.roi_by1) continue;             // dense span of a slab-partitioned pass
    const int px0 = gx * kOccTile, py0 = gy * kOccTile, k0 = gz * kOccDepth;
    const int nk = min(kOccDepth, p.n_steps - k0);

    fill_alpha_pairs(s_alpha, p.tf);
    if (threadIdx.x < NS * kOccDepth) { // slice-axis taps of each step of this workgroup (wave-uniform values)
        const int si = threadIdx.x / kOccDepth, q = threadIdx.x % kOccDepth;
        const ChunkStream& s = si == 0 ? p.a : p.r;
        const OccSliceEntry e = occ_slice_entry(p.j0 + min(k0 + q, p.n_steps - 1) * p.dir, p.lv_dims[dim_s], s.uvw_off[dim_s], data_dims[dim_s]);
        s_w[si][q] = e.w; s_f[si][q] = e.f; s_i[si][q] = e.i0; s_flags[si][q] = e.flags;
    }
    if (threadIdx.x >= 64 && threadIdx.x < 64 + NS * 6) { // base tap of the first / last pixel and slice, one lane each
        const int t = threadIdx.x - 64, si = t / 6, a = (t % 6) >> 1, e = t & 1;
        const ChunkStream& s = si == 0 ? p.a : p.r;
        int first, last;
        if (a == 0) block_ends(gx, p.W, first, last);
        else if (a == 1) block_ends(gy, p.H, first, last);
        else group_ends(k0, p.n_steps, p.j0, p.dir, first, last);
        const int dim = a == 0 ? dim_u : (a == 1 ? dim_v : dim_s);
        const int lvd = dim == 0 ? p.lv_dims[0] : (dim == 1 ? p.lv_dims[1] : p.lv_dims[2]);
        const float off = dim == 0 ? s.uvw_off[0] : (dim == 1 ? s.uvw_off[1] : s.uvw_off[2]);
        const int dd = dim == 0 ? p.data.nx : (dim == 1 ? p.data.ny : p.data.nz);
        s_ends[t] = base_tap(sample_coord(e ? last : first, lvd, off), (float) dd);
        s_end_dim[t] = dim;
    }
    __syncthreads();
    if (threadIdx.x == 0) { // brick range the workgroup's samples can touch (union over the streams)
        int lo[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, hi[3] = {INT32_MIN, INT32_MIN, INT32_MIN};
        for (int t = 0; t < NS * 6; ++t) {
            const int dm = s_end_dim[t], i0 = s_ends[t];
            if (dm == 0) tap_span_add(i0, lo[0], hi[0]);
            else if (dm == 1) tap_span_add(i0, lo[1], hi[1]);
            else tap_span_add(i0, lo[2], hi[2]);
        }
        const int bn[3] = {p.data.bnx, p.data.bnxy / p.data.bnx, (p.data.nz + 7) >> 3};
        int count = 1;
        bool touches_border = false;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            int b0a, nba;
            bool border;
            brick_span(lo[a], hi[a], data_dims[a], bn[a], b0a, nba, border);
            s_b0[a] = b0a;
            s_nb[a] = nba;
            count *= nba;
            touches_border = touches_border || border;
        }
        s_staged = bricks_staged(count, ESZ, lds_budget_bytes) ? 1 : 0;
        s_interior = touches_border ? 0 : 1;
    }
    __syncthreads();

    const bool staged = s_staged != 0;
    const int b0[3] = {s_b0[0], s_b0[1], s_b0[2]}, nb[3] = {s_nb[0], s_nb[1], s_nb[2]};
    if (staged) { // copy the bricks: 512*ESZ bytes each, 16 bytes per lane
        constexpr int PIECES = kBrickVoxels * ESZ / 16; // a power of two
        const int bricks = nb[0] * nb[1] * nb[2];
        // global index of every staged brick, once (the integer divisions stay out of the copy loop)
        if ((int) threadIdx.x < bricks) {
            const int lb = threadIdx.x, nxy = nb[0] * nb[1];
            s_brick[lb] = staged_brick_xy(lb % nxy, b0[0], b0[1], nb[0], p.data.bnx) + staged_brick_z(lb / nxy, b0[2], p.data.bnxy);
        }
        __syncthreads();
        const int total = bricks * PIECES;
        const int wave_base = (threadIdx.x >> 6) * 64, lane = threadIdx.x & 63;
        for (int cb = wave_base; cb < total; cb += 256) {
            const int c = cb + lane;
            if (c < total) dma_16((const char*) p.data.data + staged_piece_src(s_brick[c / PIECES], c, PIECES, ESZ), smem + (size_t) cb * 16);
        }
    }

    // offset of voxel coordinate c along an axis: in the staged block, or in the bricked global volume
    auto voff = [&](int c, auto axis_c) -> uint32_t {
        constexpr int axis = decltype(axis_c)::value;
        c = tap_coord(c, data_dims[axis]);
        if (staged) return staged_off<axis>(c, b0[axis], nb[axis], axis == 0 ? 1u : (axis == 1 ? (uint32_t) nb[0] : (uint32_t) (nb[0] * nb[1])));
        return axis == 0 ? brick_off_x(c) : (axis == 1 ? brick_off_y(c, p.data.bnx) : brick_off_z(c, p.data.bnxy));
    };
    using AU = std::integral_constant<int, dim_u>; using AV = std::integral_constant<int, dim_v>; using AS = std::integral_constant<int, dim_s>;
    if (threadIdx.x < NS * kOccDepth) { // slice-axis tap offsets of each step (wave-uniform), in the layout just chosen
        const int si = threadIdx.x / kOccDepth, q = threadIdx.x % kOccDepth;
        s_o0[si][q] = voff(s_i[si][q], AS{});
        s_o1[si][q] = voff(s_i[si][q] + 1, AS{});
    }

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int px = px0 + (wave & 1) * 8 + (lane & 7);
    const int py = py0 + (wave >> 1) * 8 + (lane >> 3);
    const bool pixel_ok = px < p.W && py < p.H;
    const int plane_elems = p.H * p.W;

    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    auto run = [&](auto staged_c, auto interior_c, auto clip_c, auto nonneg_c) {
        constexpr bool STAGED = decltype(staged_c)::value, INTERIOR = decltype(interior_c)::value, CLIP = decltype(clip_c)::value, NONNEG = decltype(nonneg_c)::value;
        const float border = p.data_border;
        auto tap = [&](uint32_t off, bool ok) -> float { return occ_tap<DFMT, STAGED, INTERIOR>(smem, p.data.data, off, ok, border); };
#pragma unroll
        for (int si = 0; si < NS; ++si) {
            const ChunkStream& s = si == 0 ? p.a : p.r;
            const float u = sample_coord(px, p.lv_dims[dim_u], s.uvw_off[dim_u]), v = sample_coord(py, p.lv_dims[dim_v], s.uvw_off[dim_v]);
            const AxisTaps tu = axis_taps(u, data_dims[dim_u]), tv = axis_taps(v, data_dims[dim_v]);
            const bool guard_uv = (u == saturate_(u)) && (v == saturate_(v));
            const uint32_t u0 = voff(tu.i0, AU{}), u1 = voff(tu.i0 + 1, AU{}), v0 = voff(tv.i0, AV{}), v1 = voff(tv.i0 + 1, AV{});
            const uint32_t o00 = u0 + v0, o10 = u1 + v0, o01 = u0 + v1, o11 = u1 + v1;
            const bool k00 = tu.ok0 && tv.ok0, k10 = tu.ok1 && tv.ok0, k01 = tu.ok0 && tv.ok1, k11 = tu.ok1 && tv.ok1;
            // where the factors go: the span's plane stack, or (block-compact hand-over) the block's own 8 x 16 x 16 floats —
            // `entry` is the block's rank in the pass's work list
            float* out = nullptr;
            int out_step = 0;
            float* out2[2] = {nullptr, nullptr}; // DUAL: where this thread's voxels go in the two passes' stores (null: block flagged empty)
            int out2_step[2] = {0, 0};
            if constexpr (DUAL) {
                int pos[3];
                pos[dim_u] = px; pos[dim_v] = py; pos[dim_s] = p.j0 + k0 * p.dir;
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const DualPass& P = d.pass[k];
                    const int pa = P.axis == 0 ? pos[0] : (P.axis == 1 ? pos[1] : pos[2]);
                    const int pu = P.axis == 0 ? pos[1] : pos[0], pv = P.axis == 2 ? pos[1] : pos[2]; // the pass's plane coordinates
                    const int ks = (pa - P.start) * P.dir;                                              // its slice
                    const int32_t rank = P.fs_slot[((ks >> 3) * P.blocks_y + (pv >> 4)) * P.blocks_x + (pu >> 4)];
                    if (rank >= 0) { // (factor_block, spelled out: tbrm_occ_footprint.h says why)
                        float* const blk_base = (uint32_t) rank < P.fs_cap[si] ? P.fs_keep[si] + (size_t) (uint32_t) rank * kOccBlockFloats : P.fs_spill[si] + (size_t) ((uint32_t) rank - P.fs_cap[si]) * kOccBlockFloats;
                        out2[k] = blk_base + (ks & 7) * kOccSliceFloats + (pv & 15) * kOccTile + (pu & 15);
                    }
                    // one step along the launch's loop axis, in pass k's block: its own slice axis, its columns, or its rows
                    out2_step[k] = (dim_s == P.axis ? kOccSliceFloats * P.dir : (dim_s == (P.axis == 0 ? 1 : 0) ? 1 : kOccTile)) * p.dir;
                }
            } else {
                out = s.occ_next + k0 * plane_elems + py * p.W + px;
                out_step = plane_elems;
                if (p.compact) { // (factor_block, spelled out)
                    float* const blk_base = (uint32_t) entry < s.fs_cap ? s.fs_keep + (size_t) entry * kOccBlockFloats : s.fs_spill + (size_t) ((uint32_t) entry - s.fs_cap) * kOccBlockFloats;
                    out = blk_base + (py - py0) * kOccTile + (px - px0);
                    out_step = kOccSliceFloats;
                }
            }
            // a texel plane of the footprint (held_planes_step): 1, 2 or 4 values, by the place of the slice axis in the filter order
            constexpr int PV = AXIS == 2 ? 1 : (AXIS == 1 ? 2 : 4);
            struct PlaneVal { float v[PV]; };
            auto fetch_plane = [&](int q, bool upper) -> PlaneVal {
                const uint32_t w = upper ? s_o1[si][q] : s_o0[si][q];
                const bool a = (s_flags[si][q] & (upper ? 2 : 1)) != 0;
                // tap (u, v): bit0 = u tap, bit1 = v tap
                const float t00 = tap(o00 + w, k00 && a), t10 = tap(o10 + w, k10 && a);
                const float t01 = tap(o01 + w, k01 && a), t11 = tap(o11 + w, k11 && a);
                PlaneVal r;
                if constexpr (AXIS == 2) r.v[0] = lerp_(lerp_(t00, t10, tu.f), lerp_(t01, t11, tu.f), tv.f); // (u,v,s) = (x,y,z)
                else if constexpr (AXIS == 1) { r.v[0] = lerp_(t00, t10, tu.f); r.v[1] = lerp_(t01, t11, tu.f); } // x = u, y = slice, z = v
                else { r.v[0] = t00; r.v[1] = t10; r.v[2] = t01; r.v[3] = t11; }                               // x = slice, y = u, z = v
                return r;
            };
            auto combine = [&](const PlaneVal& lo, const PlaneVal& hi, float fs) -> float {
                if constexpr (AXIS == 2) return lerp_(lo.v[0], hi.v[0], fs);
                else if constexpr (AXIS == 1) return lerp_(lerp_(lo.v[0], hi.v[0], fs), lerp_(lo.v[1], hi.v[1], fs), tv.f);
                else return lerp_(lerp_(lerp_(lo.v[0], hi.v[0], fs), lerp_(lo.v[1], hi.v[1], fs), tu.f),
                                  lerp_(lerp_(lo.v[2], hi.v[2], fs), lerp_(lo.v[3], hi.v[3], fs), tu.f), tv.f);
            };
            PlaneVal lo{}, hi{};
            int held = kNoPlaneHeld;
            // the step sizes in vector registers (as scalars they are spilled around this loop and fetched back every trip)
            float step_v0 = DUAL ? d.pass[0].step100[si] : s.step100, step_v1 = DUAL ? d.pass[1].step100[si] : 0.0f;
            asm volatile("" : "+v"(step_v0), "+v"(step_v1));
            for (int q = 0; q < nk; ++q) {
                const float fs = s_f[si][q];
                const int fl = s_flags[si][q];
                held_planes_step(lo, hi, held, __builtin_amdgcn_readfirstlane(s_i[si][q]), [&](bool upper) { return fetch_plane(q, upper); });
                const float w = CLIP ? s_w[si][q] : 0.0f;
                float occ0, occ1;
                occ_sample<DFMT, CLIP, NONNEG, DUAL>(p, AXIS == 0 ? w : u, AXIS == 0 ? u : (AXIS == 1 ? w : v), AXIS == 2 ? w : v, !GUARD || (guard_uv && (fl & 4)),
                                                     [&] { return combine(lo, hi, fs); }, step_v0, step_v1, s_alpha, occ0, occ1);
                if constexpr (DUAL) dual_store(out2, out2_step, q, occ0, occ1);
                else out[q * out_step] = 1 - occ0; // handed over as the factor of AddDirLightShader.usf:117
            }
        }
    };
    bool steps_nonneg = true;
#pragma unroll
    for (int si = 0; si < NS; ++si) steps_nonneg = steps_nonneg && (DUAL ? (d.pass[0].step100[si] >= 0.0f && d.pass[1].step100[si] >= 0.0f) : (si == 0 ? p.a : p.r).step100 >= 0.0f);
    if (!pixel_ok) continue;
    occ_forms(staged, s_interior != 0, p.clip_mode != 0, steps_nonneg, run);
  }
}

// ---- k_light_occlusion_runs: a dual launch whose workgroups take RUNS of z-adjacent live units ----------------------------------
// The same units, staging, block lists, ranks, factor layout and per-voxel arithmetic as the dual per-unit form: both kernels take
// the footprint rules from tbrm_occ_footprint.h and the sample loop's pieces from above. A workgroup takes one word of the run list (tbrm_internal.h OccRuns): up to occ_run live units of one column, bottom to top.
// What is a function of the column is set up once per run — the alpha pair table, every thread's u / v taps, weights, validity
// bits and in-plane tap offsets, the x / y brick range with the x / y part of the staged bricks' indices, the invariant part of
// the factor-store addresses — and what changes from a unit to the one above it per unit: the eight slice-table entries (two
// sets, taken in turn, so that a unit's tables are written while the one before is still being read), the z brick range with the
// staged / interior decision, the staging copy (one z layer of bricks at a time: no index list per unit) and the block ranks.
// Two barriers per unit instead of four. The texel plane a unit's last slice leaves in registers serves the first slice of
// the next unit where the texel index continues.
struct OccThreadTaps {
    uint32_t o00, o10, o01, o11; // in-plane offsets of the four taps (u, v): bit0 = u tap, bit1 = v tap
    float fu, fv, u, v;
    int ok;                      // bits 0..3: tap (u, v) inside the volume; bit 4: u and v equal their saturate (the Add shader's guard)
};

template <int DFMT, int MODE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(TBRM_OCC_WAVES_PER_EU, 8))) void k_light_occlusion_runs(const ChunkParams p, int lds_budget_bytes, const DualOcc d, const uint32_t* __restrict__ runs,
                                                                                                                                   const int* __restrict__ run_count)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NS = occ_mode_streams(MODE);
    constexpr bool GUARD = MODE == PASS_ADD || MODE == PASS_ADD2;
    constexpr int ESZ = fmt_bytes(DFMT);
    constexpr int PIECES = kBrickVoxels * ESZ / 16; // 16-byte pieces of a brick
    __shared__ float2 s_alpha[257];
    __shared__ float s_w[2][NS][kOccDepth], s_f[2][NS][kOccDepth]; // [unit parity][stream][slice]
    __shared__ int s_i[2][NS][kOccDepth], s_flags[2][NS][kOccDepth];
    __shared__ uint32_t s_o0[2][NS][kOccDepth], s_o1[2][NS][kOccDepth];
    __shared__ int s_zend[2][NS * 2], s_xyend[NS * 4];
    __shared__ uint32_t s_brick_xy[kOccMaxBricks];

    if ((int) blockIdx.x >= run_count[1]) return;
    const uint32_t word = runs[blockIdx.x];
    if (word == kRunNone) return;
    const int id = (int) (word & ((1u << kRunLenShift) - 1u)), len = (int) (word >> kRunLenShift) + 1;
    const int gx = id % p.occ_blocks_x, gy = (id / p.occ_blocks_x) % p.occ_blocks_y, gz0 = id / (p.occ_blocks_x * p.occ_blocks_y);
    const int px0 = gx * kOccTile, py0 = gy * kOccTile;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int px = px0 + (wave & 1) * 8 + (lane & 7);
    const int py = py0 + (wave >> 1) * 8 + (lane >> 3);
    const bool pixel_ok = px < p.W && py < p.H;

    // ---- once per run ----
    fill_alpha_pairs(s_alpha, p.tf);
    if (threadIdx.x >= 64 && threadIdx.x < 64 + NS * 4) { // base tap of the first / last pixel along x and y, one lane each
        const int t = threadIdx.x - 64, si = t >> 2, a = (t >> 1) & 1, e = t & 1;
        const ChunkStream& s = si == 0 ? p.a : p.r;
        int first, last;
        if (a == 0) block_ends(gx, p.W, first, last);
        else block_ends(gy, p.H, first, last);
        s_xyend[t] = base_tap(sample_coord(e ? last : first, a == 0 ? p.lv_dims[0] : p.lv_dims[1], a == 0 ? s.uvw_off[0] : s.uvw_off[1]), (float) (a == 0 ? p.data.nx : p.data.ny));
    }
    __syncthreads();
    // the x / y part of the brick range the column's samples can touch (union over the streams), the same for every thread
    int b0x, b0y, nbx, nby;
    bool border_xy;
    {
        int lo[2] = {INT32_MAX, INT32_MAX}, hi[2] = {INT32_MIN, INT32_MIN};
#pragma unroll
        for (int t = 0; t < NS * 4; ++t) tap_span_add(__builtin_amdgcn_readfirstlane(s_xyend[t]), lo[(t >> 1) & 1], hi[(t >> 1) & 1]);
        bool border_x, border_y;
        brick_span(lo[0], hi[0], p.data.nx, p.data.bnx, b0x, nbx, border_x);
        brick_span(lo[1], hi[1], p.data.ny, p.data.bnxy / p.data.bnx, b0y, nby, border_y);
        border_xy = border_x || border_y;
    }
    const int nxy = nbx * nby;
    if ((int) threadIdx.x < min(nxy, kOccMaxBricks)) // x / y part of every staged brick's index (read behind the first unit's barrier)
        s_brick_xy[threadIdx.x] = staged_brick_xy((int) threadIdx.x, b0x, b0y, nbx, p.data.bnx);

    // a thread's taps in the plane: offsets inside the staged block (STAGED_FORM) or in the bricked volume
    auto thread_taps = [&](int si, bool staged_form) -> OccThreadTaps {
        const ChunkStream& s = si == 0 ? p.a : p.r;
        OccThreadTaps t;
        t.u = sample_coord(px, p.lv_dims[0], s.uvw_off[0]);
        t.v = sample_coord(py, p.lv_dims[1], s.uvw_off[1]);
        const AxisTaps tu = axis_taps(t.u, p.data.nx), tv = axis_taps(t.v, p.data.ny);
        t.fu = tu.f;
        t.fv = tv.f;
        auto off_x = [&](int c) -> uint32_t {
            c = tap_coord(c, p.data.nx);
            return staged_form ? staged_off<0>(c, b0x, nbx, 1u) : brick_off_x(c);
        };
        auto off_y = [&](int c) -> uint32_t {
            c = tap_coord(c, p.data.ny);
            return staged_form ? staged_off<1>(c, b0y, nby, (uint32_t) nbx) : brick_off_y(c, p.data.bnx);
        };
        const uint32_t u0 = off_x(tu.i0), u1 = off_x(tu.i0 + 1), v0 = off_y(tv.i0), v1 = off_y(tv.i0 + 1);
        t.o00 = u0 + v0; t.o10 = u1 + v0; t.o01 = u0 + v1; t.o11 = u1 + v1;
        const bool guard_uv = (t.u == saturate_(t.u)) && (t.v == saturate_(t.v));
        t.ok = ((tu.ok0 && tv.ok0) ? 1 : 0) | ((tu.ok1 && tv.ok0) ? 2 : 0) | ((tu.ok0 && tv.ok1) ? 4 : 0) | ((tu.ok1 && tv.ok1) ? 8 : 0) | (guard_uv ? 16 : 0);
        return t;
    };
    // what a thread carries through the run per stream (two named sets, not arrays: they stay in registers)
    struct StreamRegs {
        uint32_t o00, o10, o01, o11;
        float fu, fv;
        int ok;
        float lo, hi; // the held planes (held_planes_step): 4 taps at one z, filtered along x and y
        int held;
    };
    auto stream_regs = [&](int si) __attribute__((always_inline)) -> StreamRegs {
        const OccThreadTaps t = thread_taps(si, true);
        return StreamRegs{t.o00, t.o10, t.o01, t.o11, t.fu, t.fv, t.ok, 0.0f, 0.0f, kNoPlaneHeld};
    };
    StreamRegs regs_a = stream_regs(0), regs_r = NS == 2 ? stream_regs(1) : StreamRegs{};
    // where a thread's factors go in the two passes' stores, as far as the column decides it: the pass's block is
    // fs_slot[inv_idx + what the unit adds], the voxel's place in it inv_off + what the unit adds (the per-unit form's out2)
    int inv_idx[2], inv_off[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const DualPass& P = d.pass[k];
        if (P.axis == 2) {
            inv_idx[k] = (py >> 4) * P.blocks_x + (px >> 4);
            inv_off[k] = (py & 15) * kOccTile + (px & 15);
        } else {
            const int pa = P.axis == 0 ? px : py, pu = P.axis == 0 ? py : px; // (the pass's rows are z)
            const int ks = (pa - P.start) * P.dir;
            inv_idx[k] = (ks >> 3) * P.blocks_y * P.blocks_x + (pu >> 4);
            inv_off[k] = (ks & 7) * kOccSliceFloats + (pu & 15);
        }
    }
    bool steps_nonneg = true;
#pragma unroll
    for (int si = 0; si < NS; ++si) steps_nonneg = steps_nonneg && d.pass[0].step100[si] >= 0.0f && d.pass[1].step100[si] >= 0.0f;

    // ---- per unit ----
    for (int ui = 0; ui < len; ++ui) {
        const int par = ui & 1;
        const int k0 = (gz0 + ui) * kOccDepth;
        const int nk = min(kOccDepth, p.n_steps - k0);
        if (threadIdx.x < NS * kOccDepth) { // z taps of each slice of the unit (wave-uniform values)
            const int si = threadIdx.x / kOccDepth, q = threadIdx.x % kOccDepth;
            const ChunkStream& s = si == 0 ? p.a : p.r;
            const OccSliceEntry e = occ_slice_entry(min(k0 + q, p.n_steps - 1), p.lv_dims[2], s.uvw_off[2], p.data.nz);
            s_w[par][si][q] = e.w; s_f[par][si][q] = e.f; s_i[par][si][q] = e.i0; s_flags[par][si][q] = e.flags;
        }
        if (threadIdx.x >= 64 && threadIdx.x < 64 + NS * 2) { // base tap of the unit's first / last slice
            const int t = threadIdx.x - 64, si = t >> 1, e = t & 1;
            const ChunkStream& s = si == 0 ? p.a : p.r;
            int first, last;
            group_ends(k0, p.n_steps, 0, 1, first, last); // (a dual launch loops up z from 0: launch_occ3)
            s_zend[par][t] = base_tap(sample_coord(e ? last : first, p.lv_dims[2], s.uvw_off[2]), (float) p.data.nz);
        }
        __syncthreads(); // (also: every thread is done with the bricks of the unit before)
        bool staged, interior;
        int b0z, nbz;
        {
            int zlo = INT32_MAX, zhi = INT32_MIN;
#pragma unroll
            for (int t = 0; t < NS * 2; ++t) tap_span_add(__builtin_amdgcn_readfirstlane(s_zend[par][t]), zlo, zhi);
            bool border_z;
            brick_span(zlo, zhi, p.data.nz, (p.data.nz + 7) >> 3, b0z, nbz, border_z);
            staged = bricks_staged(nxy * nbz, ESZ, lds_budget_bytes);
            interior = !(border_xy || border_z);
        }
        if (staged) { // copy the bricks, a z layer at a time: 512*ESZ bytes each, 16 bytes per lane
            const int layer = nxy * PIECES;
            const int wave_base = wave * 64;
            for (int lz = 0; lz < nbz; ++lz) {
                const uint32_t gz_part = staged_brick_z(lz, b0z, p.data.bnxy);
                for (int cb = wave_base; cb < layer; cb += 256) {
                    const int c = cb + lane;
                    if (c < layer) // (8-bit bricks are 32 pieces: an odd number of them ends in the middle of a wave)
                        dma_16((const char*) p.data.data + staged_piece_src(s_brick_xy[c / PIECES] + gz_part, c, PIECES, ESZ), smem + (size_t) (lz * layer + cb) * 16);
                }
            }
        }
        if (threadIdx.x < NS * kOccDepth) { // z tap offsets of each slice, in the layout just chosen
            const int si = threadIdx.x / kOccDepth, q = threadIdx.x % kOccDepth;
            auto zoff = [&](int c) -> uint32_t {
                c = tap_coord(c, p.data.nz);
                return staged ? staged_off<2>(c, b0z, nbz, (uint32_t) nxy) : brick_off_z(c, p.data.bnxy);
            };
            s_o0[par][si][q] = zoff(s_i[par][si][q]);
            s_o1[par][si][q] = zoff(s_i[par][si][q] + 1);
        }
        // the unit's blocks in the two passes (ranks are loaded while the copies are in flight)
        int32_t rank[2];
        int unit_off[2], out2_step[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const DualPass& P = d.pass[k];
            int unit_idx;
            if (P.axis == 2) {
                const int ks = (k0 - P.start) * P.dir;
                unit_idx = (ks >> 3) * P.blocks_y * P.blocks_x;
                unit_off[k] = (ks & 7) * kOccSliceFloats;
                out2_step[k] = kOccSliceFloats * P.dir;
            } else {
                unit_idx = (k0 >> 4) * P.blocks_x;
                unit_off[k] = (k0 & 15) * kOccTile;
                out2_step[k] = kOccTile;
            }
            rank[k] = pixel_ok ? P.fs_slot[inv_idx[k] + unit_idx] : -1;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (!pixel_ok) continue;

        // the sample loop in one of occ_forms' forms
        auto run = [&](auto staged_c, auto interior_c, auto clip_c, auto nonneg_c) __attribute__((always_inline)) { // (inlined early: lo / hi / held stay in registers)
            constexpr bool STAGED = decltype(staged_c)::value, INTERIOR = decltype(interior_c)::value, CLIP = decltype(clip_c)::value, NONNEG = decltype(nonneg_c)::value;
            const float border = p.data_border;
            auto tap = [&](uint32_t off, bool ok) -> float { return occ_tap<DFMT, STAGED, INTERIOR>(smem, p.data.data, off, ok, border); };
            auto stream = [&](auto si_c, StreamRegs& sr) __attribute__((always_inline)) {
                constexpr int si = decltype(si_c)::value;
                uint32_t o00 = sr.o00, o10 = sr.o10, o01 = sr.o01, o11 = sr.o11;
                float u = 0.0f, v = 0.0f;
                if constexpr (!STAGED || CLIP) { // the uncommon forms recompute what the run does not carry for them
                    const OccThreadTaps t = thread_taps(si, STAGED);
                    o00 = t.o00; o10 = t.o10; o01 = t.o01; o11 = t.o11;
                    u = t.u; v = t.v;
                }
                const float fu = sr.fu, fv = sr.fv;
                const int ok = sr.ok;
                float* out2[2]; // where this thread's voxels go in the two passes' stores (null: block flagged empty)
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    out2[k] = nullptr;
                    const DualPass& P = d.pass[k];
                    if (rank[k] >= 0) { // (factor_block, spelled out: tbrm_occ_footprint.h says why)
                        float* const blk_base = (uint32_t) rank[k] < P.fs_cap[si] ? P.fs_keep[si] + (size_t) (uint32_t) rank[k] * kOccBlockFloats : P.fs_spill[si] + (size_t) ((uint32_t) rank[k] - P.fs_cap[si]) * kOccBlockFloats;
                        out2[k] = blk_base + (inv_off[k] + unit_off[k]);
                    }
                }
                auto fetch_plane = [&](int q, bool upper) -> float {
                    const uint32_t w = upper ? s_o1[par][si][q] : s_o0[par][si][q];
                    const bool a = (s_flags[par][si][q] & (upper ? 2 : 1)) != 0;
                    const float t00 = tap(o00 + w, (ok & 1) && a), t10 = tap(o10 + w, (ok & 2) && a);
                    const float t01 = tap(o01 + w, (ok & 4) && a), t11 = tap(o11 + w, (ok & 8) && a);
                    return lerp_(lerp_(t00, t10, fu), lerp_(t01, t11, fu), fv);
                };
                // the step sizes in vector registers (as scalars they are spilled around this loop and fetched back every trip)
                float step_v0 = d.pass[0].step100[si], step_v1 = d.pass[1].step100[si];
                asm volatile("" : "+v"(step_v0), "+v"(step_v1));
                for (int q = 0; q < nk; ++q) {
                    const float fs = s_f[par][si][q];
                    const int fl = s_flags[par][si][q];
                    const int i = __builtin_amdgcn_readfirstlane(s_i[par][si][q]); // wave-uniform: scalar branches below
                    held_planes_step(sr.lo, sr.hi, sr.held, i, [&](bool upper) { return fetch_plane(q, upper); });
                    float occ0, occ1;
                    occ_sample<DFMT, CLIP, NONNEG, true>(p, u, v, CLIP ? s_w[par][si][q] : 0.0f, !GUARD || ((ok & 16) && (fl & 4)), [&] { return lerp_(sr.lo, sr.hi, fs); }, step_v0, step_v1, s_alpha,
                                                         occ0, occ1);
                    dual_store(out2, out2_step, q, occ0, occ1);
                }
            };
            stream(std::integral_constant<int, 0>{}, regs_a);
            if constexpr (NS == 2) stream(std::integral_constant<int, 1>{}, regs_r);
        };
        // (occ_forms' ladder, written out: through the function the two-stream forms spill up to 14 more vector registers —
        // profiles/r14_occlusion_rules.txt)
        using T_ = std::true_type; using F_ = std::false_type;
        auto forms = [&](auto nonneg_c) __attribute__((always_inline)) {
            if (staged && interior && !p.clip_mode) run(T_{}, T_{}, F_{}, nonneg_c);
            else if (staged && !p.clip_mode) run(T_{}, F_{}, F_{}, nonneg_c);
            else if (staged) run(T_{}, F_{}, T_{}, nonneg_c);
            else run(F_{}, F_{}, T_{}, nonneg_c);
        };
        if (steps_nonneg) forms(T_{});
        else forms(F_{});
    }
}

template <int DFMT, int MODE, int AXIS>
static hipError_t launch_occ3(const ChunkParams& p, hipStream_t s, const DualOcc* dual, const OccRuns* runs)
{
    const int blocks = ((p.W + kOccTile - 1) / kOccTile) * ((p.H + kOccTile - 1) / kOccTile) * ((p.n_steps + kOccDepth - 1) / kOccDepth);
    int wgs = 8 * ((blocks + 7) / 8);
    if (p.occ_grid_cap > 0) wgs = std::min(wgs, 8 * ((p.occ_grid_cap + 7) / 8));
    const dim3 grid(wgs), block(256);
    size_t lds = occlusion_lds_bytes(p);
    if (lds > 96 * 1024) lds = 96 * 1024; // workgroups whose bricks do not fit read their taps from global memory
    if (dual) {
        if constexpr (MODE == PASS_ADD2 || AXIS != 2) return hipErrorInvalidConfiguration; // (dual launches loop along z: DualOcc)
        else {
            if (!p.occ_list || !p.occ_count || p.dir != 1 || p.j0 != 0) return hipErrorInvalidConfiguration; // (the units come from their work list)
            if (runs) { // one workgroup per word of the run list; how many there are is known on the device only
                static std::atomic<uint64_t> attr_done3{0};
                if (const hipError_t e = allow_big_lds(k_light_occlusion_runs<DFMT, MODE>, attr_done3, 128 * 1024); e != hipSuccess) return e;
                hipLaunchKernelGGL((k_light_occlusion_runs<DFMT, MODE>), dim3(wgs + 8 * runs->len), block, lds, s, p, (int) lds, *dual, runs->list, runs->count);
                return hipGetLastError();
            }
            static std::atomic<uint64_t> attr_done2{0};
            if (const hipError_t e = allow_big_lds(k_light_occlusion<DFMT, MODE, AXIS, true>, attr_done2, 128 * 1024); e != hipSuccess) return e;
            hipLaunchKernelGGL((k_light_occlusion<DFMT, MODE, AXIS, true>), grid, block, lds, s, p, (int) lds, *dual);
            return hipGetLastError();
        }
    }
    static std::atomic<uint64_t> attr_done{0};
    if (const hipError_t e = allow_big_lds(k_light_occlusion<DFMT, MODE, AXIS>, attr_done, 128 * 1024); e != hipSuccess) return e;
    hipLaunchKernelGGL((k_light_occlusion<DFMT, MODE, AXIS>), grid, block, lds, s, p, (int) lds, DualOcc{});
    return hipGetLastError();
}
template <int DFMT, int MODE>
static hipError_t launch_occ2(const ChunkParams& p, hipStream_t s, const DualOcc* dual, const OccRuns* runs)
{
    return p.axis == 0 ? launch_occ3<DFMT, MODE, 0>(p, s, dual, runs) : (p.axis == 1 ? launch_occ3<DFMT, MODE, 1>(p, s, dual, runs) : launch_occ3<DFMT, MODE, 2>(p, s, dual, runs));
}
template <int DFMT>
static hipError_t launch_occ1(const ChunkParams& p, int mode, hipStream_t s, const DualOcc* dual, const OccRuns* runs)
{
    return mode == PASS_ADD ? launch_occ2<DFMT, PASS_ADD>(p, s, dual, runs)
           : (mode == PASS_CHANGE ? launch_occ2<DFMT, PASS_CHANGE>(p, s, dual, runs) : (mode == PASS_ADD2 ? launch_occ2<DFMT, PASS_ADD2>(p, s, dual, runs) : launch_occ2<DFMT, PASS_CHANGE_ONE>(p, s, dual, runs)));
}
// computes the occlusion of the chunk described by (j0, n_steps) into {a,r}.occ_next; dual: of BOTH passes of a light, p
// describing the virtual pass along z (tbrm_internal.h DualOcc); runs: that launch in run form (k_light_occlusion_runs)
hipError_t launch_light_occlusion(const ChunkParams& p, int mode, hipStream_t s, const DualOcc* dual, const OccRuns* runs)
{
    if (p.n_steps <= 0) return hipSuccess;
    switch (p.data.fmt) {
        case FMT_U8: return launch_occ1<FMT_U8>(p, mode, s, dual, runs);
        case FMT_U16: return launch_occ1<FMT_U16>(p, mode, s, dual, runs);
        default: return launch_occ1<FMT_F32>(p, mode, s, dual, runs);
    }
}

// ---- k_unit_flags: a dual launch's work units that have nothing to do ---------------------------------------------------------
// A unit (16 x 16 voxels in x and y, 8 in z) is part of up to two 16 x 16 x 8 blocks of each pass (one, when the pass runs along
// z: then the unit IS the block); it is flagged when all of them are (then none has a rank, and nothing would be stored). One
// thread per unit.
__global__ __launch_bounds__(256) void k_unit_flags(const ChunkParams pc, const DualOcc d, int n_units)
{
    const int id = blockIdx.x * 256 + threadIdx.x;
    if (id >= n_units) return;
    const int gx = id % pc.occ_blocks_x, gy = (id / pc.occ_blocks_x) % pc.occ_blocks_y, gz = id / (pc.occ_blocks_x * pc.occ_blocks_y);
    const int dim_u = pc.axis == 0 ? 1 : 0, dim_v = pc.axis == 2 ? 1 : 2;
    int pos0[3];
    pos0[dim_u] = gx * kOccTile; pos0[dim_v] = gy * kOccTile; pos0[pc.axis] = gz * kOccDepth;
    bool all_flagged = true;
    for (int k = 0; k < 2; ++k) {
        const DualPass& P = d.pass[k];
        for (int half = 0; half < (P.axis == pc.axis ? 1 : 2); ++half) { // (16 voxels of the pass's axis unless it is the loop axis: two slice groups)
            int pos[3] = {pos0[0], pos0[1], pos0[2]};
            pos[P.axis] += 8 * half;
            if (pos[P.axis] >= pc.lv_dims[P.axis]) continue;
            const int pu = P.axis == 0 ? pos[1] : pos[0], pv = P.axis == 2 ? pos[1] : pos[2];
            const int ks = (pos[P.axis] - P.start) * P.dir;
            all_flagged = all_flagged && P.flags[((ks >> 3) * P.blocks_y + (pv >> 4)) * P.blocks_x + (pu >> 4)] != 0;
        }
    }
    pc.occ_flags_out[id] = all_flagged ? 1 : 0;
}

hipError_t launch_unit_flags(const ChunkParams& pc, const DualOcc& d, hipStream_t s)
{
    const int per_chunk = pc.occ_groups * pc.occ_blocks_y * pc.occ_blocks_x;
    hipLaunchKernelGGL(k_unit_flags, dim3((per_chunk + 255) / 256), dim3(256), 0, s, pc, d, per_chunk);
    const int segs = (per_chunk + kCompactSeg - 1) / kCompactSeg;
    hipLaunchKernelGGL(k_occ_compact, dim3(segs), dim3(256), 0, s, pc, segs);
    return hipGetLastError();
}

// ---- k_occ_runs: the run list of a dual launch (tbrm_internal.h OccRuns) ------------------------------------------------------------
// One workgroup, its threads dealt over the columns of units: a thread packs the column's flags into 64-bit liveness words (kept in LDS), cuts every
// stretch of live units into runs of R and a shorter last one, and counts its runs per length. Then, per length from R down to 1,
// a scan over the columns gives every run its ascending position j in its class, and the run goes where the workgroup of XCD
// j / ceil(class / 8) finds it: workgroups are dealt to the 8 XCDs round-robin by id, so word 8 * slot + x of a class is XCD x's
// slot-th run, and each XCD takes a contiguous eighth of the class (columns that are neighbours in the volume behind one L2).
constexpr int kRunThreads = 256; // (four waves find a place beside a sweep's resident tiles at once; sixteen were measured waiting for one for 0.3 ms)
__global__ __launch_bounds__(kRunThreads) void k_occ_runs(const uint8_t* __restrict__ flags, int columns, int groups, int R, uint32_t* __restrict__ runs, int* __restrict__ count,
                                                           int* __restrict__ count_host)
{
    __shared__ unsigned long long s_mask[kRunMaskWords];
    __shared__ int s_hist[kOccRunMax + 1], s_start[kOccRunMax + 1], s_wave[kRunThreads / 64 + 1], s_live, s_total;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int words = (groups + 63) >> 6;
    if (tid <= kOccRunMax) s_hist[tid] = 0;
    if (tid == 0) s_live = 0;
    __syncthreads();
    // f(first unit's z, length) for every run of liveness word m (64 units of z from z0 on)
    auto for_runs = [&](unsigned long long m, int z0, auto&& f) {
        while (m) {
            const int s = __builtin_ctzll(m);
            const unsigned long long t = ~(m >> s);
            const int n = t ? min(__builtin_ctzll(t), 64 - s) : 64 - s;
            m = n == 64 ? 0ull : m & ~(((1ull << n) - 1ull) << s);
            for (int o = 0; o < n; o += R) f(z0 + s + o, min(R, n - o));
        }
    };
    for (int col = tid; col < columns; col += kRunThreads)
        for (int w = 0; w < words; ++w) {
            unsigned long long m = 0;
            const int n = min(64, groups - 64 * w);
            for (int g = 0; g < n; ++g) m |= (unsigned long long) (flags[(size_t) (64 * w + g) * columns + col] ? 0 : 1) << g;
            s_mask[(size_t) col * words + w] = m;
            atomicAdd(&s_live, __builtin_popcountll(m));
            for_runs(m, 64 * w, [&](int, int l) { atomicAdd(&s_hist[l], 1); });
        }
    __syncthreads();
    if (tid == 0) {
        int start = 0, n_runs = 0;
        for (int l = R; l >= 1; --l) {
            s_start[l] = start;
            start += 8 * ((s_hist[l] + 7) >> 3);
            n_runs += s_hist[l];
        }
        s_total = start;
        count[1] = start;
        count_host[1] = s_live - n_runs; // (visible to the host once an event behind the launch has completed)
    }
    __syncthreads();
    for (int i = tid; i < s_total; i += kRunThreads) runs[i] = kRunNone;
    __syncthreads();
    for (int l = R; l >= 1; --l) {
        const int in_class = s_hist[l];
        if (in_class == 0) continue;
        const int per_xcd = (in_class + 7) >> 3;
        int before = 0; // runs of this length in the columns already taken
        for (int col0 = 0; col0 < columns; col0 += kRunThreads) {
            const int col = col0 + tid;
            int mine = 0;
            if (col < columns)
                for (int w = 0; w < words; ++w) for_runs(s_mask[(size_t) col * words + w], 64 * w, [&](int, int n) { mine += n == l ? 1 : 0; });
            int incl = mine; // inclusive scan over the workgroup
            for (int dd = 1; dd < 64; dd <<= 1) {
                const int t = __shfl_up(incl, dd);
                if (lane >= dd) incl += t;
            }
            if (lane == 63) s_wave[wave] = incl;
            __syncthreads();
            if (tid == 0) {
                int acc = 0;
                for (int k = 0; k < kRunThreads / 64; ++k) { const int t = s_wave[k]; s_wave[k] = acc; acc += t; }
                s_wave[kRunThreads / 64] = acc;
            }
            __syncthreads();
            int j = before + s_wave[wave] + incl - mine;
            before += s_wave[kRunThreads / 64];
            if (col < columns)
                for (int w = 0; w < words; ++w)
                    for_runs(s_mask[(size_t) col * words + w], 64 * w, [&](int z, int n) {
                        if (n != l) return;
                        runs[s_start[l] + 8 * (j % per_xcd) + j / per_xcd] = ((uint32_t) (n - 1) << kRunLenShift) | (uint32_t) (z * columns + col);
                        ++j;
                    });
            __syncthreads(); // (s_wave is written again)
        }
    }
}

bool occ_runs_apply(const ChunkParams& pc)
{
    const size_t columns = (size_t) pc.occ_blocks_x * pc.occ_blocks_y;
    return columns * (size_t) ((pc.occ_groups + 63) / 64) <= kRunMaskWords && columns * (size_t) pc.occ_groups <= ((size_t) 1 << kRunLenShift);
}

hipError_t launch_occ_runs(const ChunkParams& pc, const OccRuns& runs, hipStream_t s)
{
    hipLaunchKernelGGL(k_occ_runs, dim3(1), dim3(kRunThreads), 0, s, pc.occ_flags_out, pc.occ_blocks_x * pc.occ_blocks_y, pc.occ_groups, runs.len, runs.list, runs.count, runs.count_host);
    return hipGetLastError();
}

hipError_t launch_light_chain(const ChunkParams& p, int mode, int lv_fmt, hipStream_t s)
{
    if (p.n_steps <= 0 || p.tiles_x <= 0 || p.tiles_y <= 0) return hipSuccess;
    return lv_fmt == FMT_U8 ? launch_light_chain_u8(p, mode, s) : launch_light_chain_f32(p, mode, s);
}

} // namespace tbrm
