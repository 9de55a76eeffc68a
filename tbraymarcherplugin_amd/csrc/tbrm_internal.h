// tbrm_internal.h — parameter blocks passed by value from the host C-ABI layer (tbrm_api.cpp) to the gfx950
// kernels (tbrm_kernels.hip). Plain PODs; field meanings follow the reference shader uniforms they replace
// (AddDirLightShader.usf:15-66, ChangeDirLightShader.usf:15-72, M_Raymarch material parameters).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tbrm_brick_boards.h"
#include "tbrm_occ_footprint.h"

namespace tbrm {

enum : int { ADDR_WRAP = 0, ADDR_CLAMP = 1, ADDR_BORDER = 2 };

// what a propagation pass does with its light stream(s): Add (one light, stream a), Change (a added, r removed,
// ChangeDirLightShader.usf), or two lights added in one pass (a then r: AddDirLightShader.usf twice, sharing the slice loop).
// PASS_CHANGE_ONE is an occlusion mode only: ONE stream with the Change shader's rules (no uvw == saturate(uvw) guard) — the
// added light of a Change whose removed light's factors come from the factor cache (tbrm_resources.h).
// PASS_PLANES is a sweep mode only: one stream propagated, the light volume untouched — what the launch leaves behind is its
// hand-off records (SweepParams::r_from_records of the launch after it).
enum : int { PASS_ADD = 0, PASS_CHANGE = 1, PASS_ADD2 = 2, PASS_CHANGE_ONE = 3, PASS_PLANES = 5 };

struct VolumeDev {
    const void* data; // bricked layout (tbrm_device_sampling.h)
    int nx, ny, nz;
    int fmt;
    int bnx;          // bricks along x
    int bnxy;         // bricks per z-layer of bricks (bnx * bny)
    int wrap_layer;   // slab-resident volumes: the z brick layer that is not at its own place but at `wrap_shift` voxels
    int wrap_shift;   // further along z (the copy that wrap addressing reaches from the other end); wrap_layer < 0: none
};

struct WindowDev { // WindowingParameters float4 (VolumeInfo.h:49-52)
    float center, width, low_cutoff, high_cutoff;
    // the host's licence to divide by `width` without the IEEE division sequence (tbrm_device_math.h tf_position_fast): RN(1 / width),
    // and whether the window qualifies (else 0: the division). Not part of any cache key: the results are the same bits either way.
    float inv_width;
    int fast_div;
};

// One light stream of one axis pass (what LightingShaders.cpp:100-124 computes per axis).
struct PropStream {
    float border_light;  // ReadBufferSampler border colour
    float off_u, off_v;  // PrevPixelOffset
    float uvw_off[3];    // UVWOffset
    float step100;       // StepSize * VOLUME_DENSITY
    const void* read;    // ReadBuffer
    void* write;         // WriteBuffer
};

struct PropParams {
    VolumeDev data;
    float data_border; // VolumeSampler border colour
    const float4* tf;  // 256 texels, fp16-rounded values held as fp32
    WindowDev win;
    void* light;       // ALightVolume (bricked)
    int lv_dims[3];
    int lv_bnx, lv_bnxy;
    int lv_fmt;        // FMT_U8 or FMT_F32 (buffers share it)
    float cc[3], cd[3];// LocalClippingCenter / LocalClippingDirection
    int clip_mode;     // 0: plane provably leaves every sample weight at exactly 1; 1: general
    int axis;          // 0,1,2: permutation (LightingShaderUtils.cpp:227-249)
    int td[3];         // TransposedDimensions
    int loop;          // Loop (slice index along the axis)
    int row_block0, row_blocks; // 16-row blocks of the slice plane this launch covers (slab-partitioned passes; else all)
    float b_added;     // +1 / -1 (Add only)
    PropStream a;      // the added light (Add: the only stream)
    PropStream r;      // the removed light (Change only)
};

// One light stream of a chunked propagation pass (Add: the added light; Change: a = added, r = removed).
struct ChunkStream {
    float border_light;
    float off_u, off_v;
    float uvw_off[3];
    float step100;
    float init_value;       // what the cleared read/write buffers decode to (first chunk)
    const float* plane_in;  // propagated light after the previous chunk (W x H floats); unused in the first chunk
    float* plane_out;       // propagated light after this chunk
    const float* occ_base;  // chain: the allocation holding this stream's occlusion planes. Its first 4 KiB are a page of ones: the copy
                            // source for flagged-empty blocks, which keeps the copies per wave uniform
    uint32_t occ_off;       // chain: float index, relative to occ_base, of the occlusion plane of the chunk's first slice
    const uint8_t* occ_flags; // chain: this stream's empty-block flags from the slice group holding the chunk's first slice on:
                            // [slice group][block y][block x]; null: none (the two streams of a jointly computed pass share one array)
    float* occ_next;        // occlusion launch: where the span's factors 1 - CurrentSample go, [span slices][H][W]
    // Block-compact hand-over of the occlusion factors (k_light_occlusion writes, k_light_sweep reads; ChunkParams::compact):
    // the live 16 x 16 x 8 block of rank k in the pass's ascending work list holds its factors as [slice 8][row 16][column 16]
    // floats where factor_block (tbrm_occ_footprint.h) says: at fs_keep + kOccBlockFloats k while k < fs_cap (a cache entry:
    // tbrm_resources.h FactorEntry) and at fs_spill + kOccBlockFloats (k - fs_cap) beyond (the handle's scratch store; fs_cap = 0: nothing is kept).
    float* fs_keep;
    float* fs_spill;
    uint32_t fs_cap;
    const int32_t* fs_slot; // sweep: rank of every block of the pass, [slice group][block y][block x]; -1: flagged empty (factor 1)
};

// Parameters of the chunked propagation kernels (tbrm_light_kernels.hip). One struct serves the per-pass
// launches (k_occ_flags, k_occ_compact), the occlusion launch of a span (j0 / n_steps = the span) and the chain launch
// of a chunk (j0 / n_steps = the chunk).
struct ChunkParams {
    VolumeDev data;
    float data_border;
    const float4* tf;
    WindowDev win;
    void* light;            // bricked
    int lv_dims[3];
    int lv_bnx, lv_bnxy;
    float cc[3], cd[3];
    int clip_mode;
    int axis;
    int W, H;               // TD.X, TD.Y
    int dir;                // +-1
    int j0, n_steps;        // first slice and number of slices of this launch (a span for the occlusion, a chunk for the chain)
    int first_chunk;        // chain: the pass starts here (windows start from the cleared buffers' value)
    int tiles_x, tiles_y;   // chain: 32x32 tiles of the slice plane this launch advances (tiles_y rows from tile_row0 on)
    int tile_row0;          // chain: first tile row (slab-partitioned passes run only the rows of their slab; else 0)
    int roi_by0, roi_by1;   // occlusion: block rows [roi_by0, roi_by1) can be read by those tiles; the rest is never computed
    int dx_lo, dx_hi, dy_lo, dy_hi; // range of (tap index - pixel index) of the previous-slice bilinear fetch, widened to contain 0
    int rect_planes;        // chain: hulls wider than 56 and at most 48 rows high get 72 x 48 LDS planes (chunk_geometry)
    float b_added;          // Add / two adds: +1 / -1 for stream a
    float b_added2;         // two adds: the same for stream r
    // empty-block hand-off: k_occ_flags marks, once per pass, every occlusion workgroup (16x16 pixels x 8 slices) whose
    // samples can only touch data bricks that map every value to opacity 0. Such a workgroup exits at once and the chain
    // stages the factor 1 - 0 for its pixels from a page of ones instead of the plane stack.
    const uint32_t* empty_bits;   // per data brick (k_brick_empty); used by k_occ_flags only
    const uint8_t* occ_flags;     // occlusion launch without a work list: the span's flags (null: every block is computed)
    int occ_phase;                // chain: index of the chunk's first slice within its slice group (ChunkStream::occ_flags)
    uint8_t* occ_flags_out;       // k_occ_flags: the whole pass, [chunk][slice group][block y][block x]
    int occ_blocks_x, occ_blocks_y, occ_groups; // blocks per plane row / column, slice groups per chunk
    int pass_start, pass_slices, chunk_slices;  // k_occ_flags: first slice, slices in the pass, slices per chunk
    // work list: the non-empty workgroups of each chunk in ascending order (k_occ_compact). The occlusion launch keeps its
    // full grid; workgroup i takes entry i of the list or exits, so the live ones are dealt evenly over the CUs instead
    // of landing wherever the dense part of the volume happens to map.
    const uint32_t* occ_list;     // this chunk's list; null: every workgroup takes its own grid position
    const int* occ_count;         // this chunk's number of list entries
    int occ_grid_cap;             // occlusion launch: at most this many workgroups, each walking several blocks (0: one per block)
    uint32_t* occ_list_out;       // k_occ_compact: the whole pass, [chunk][per-chunk capacity]
    int* occ_count_out;           // k_occ_compact: [chunk]
    int* occ_count_host;          // (one-chunk launches) the same count into pinned host memory as well: no copy behind the kernel
    int32_t* occ_slot_out;        // k_occ_compact: rank of every block in its chunk's list, -1 for the flagged ones (null: not wanted)
    int compact;                  // occlusion launch / sweep: the factors are handed over block-compact (ChunkStream::fs_*)
    const float* ones;            // sweep: 1024 floats of 1.0 (the factor of flagged-empty blocks and of pixels beyond the buffer)
    ChunkStream a, r;
};

// streams an occlusion launch of `mode` computes (PASS_CHANGE_ONE: one stream with the Change shader's rules)
constexpr int occ_mode_streams(int mode) { return (mode == PASS_ADD || mode == PASS_CHANGE_ONE) ? 1 : 2; }
// what the footprint rules (tbrm_occ_footprint.h) read of chunk c of a pass: k_occ_flags and the host's block-list signature (c = 0)
__host__ __device__ __forceinline__ OccPassShape occ_pass_shape(const ChunkParams& p, int ns, int c)
{
    OccPassShape s;
    s.axis = p.axis; s.W = p.W; s.H = p.H; s.dir = p.dir;
    s.start = p.pass_start + c * p.chunk_slices * p.dir;
    s.slices = p.chunk_slices < p.pass_slices - c * p.chunk_slices ? p.chunk_slices : p.pass_slices - c * p.chunk_slices;
    s.blocks_x = p.occ_blocks_x; s.blocks_y = p.occ_blocks_y; s.groups = p.occ_groups;
    s.data_dims[0] = p.data.nx; s.data_dims[1] = p.data.ny; s.data_dims[2] = p.data.nz;
    s.ns = ns;
    for (int a = 0; a < 3; ++a) { s.lv_dims[a] = p.lv_dims[a]; s.uvw_off[0][a] = p.a.uvw_off[a]; s.uvw_off[1][a] = p.r.uvw_off[a]; }
    return s;
}

// The two axis passes of ONE light sample the data volume at the same positions: UVWOffset = normalize(lightPos) / min(TD)
// whichever axis the pass runs along (LightingShaders.cpp:114-124) — only StepSize differs. A "dual" occlusion launch
// (k_light_occlusion<..., DUAL>) therefore filters, windows and looks the transfer function up ONCE per voxel and emits the
// factor 1 - CurrentSample of BOTH passes (AddDirLightShader.usf:85-117 with the two StepSize * 100 exponents, the logarithm
// of the opacity correction shared). Its work unit is 16 x 16 voxels in x and y times 8 in z, a thread walking z — whatever
// the two pass axes are (ChunkParams describes that virtual pass along z): a block of any pass holds its factors as
// [slice][row][column] with x the column axis unless the pass runs along x (then y), so lanes that span x and y write every
// pass's block-compact store in the same 32-byte segments as the pass's own launch would (measured: looping along x or y
// instead scatters one or both stores over 64 lines per instruction and costs 1.3 - 1.9x the launch).
struct DualPass {
    int axis, start, dir;       // the pass: axis, first slice, direction (tbrm_light_pass)
    int blocks_x, blocks_y;     // its 16 x 16 blocks per plane row / column
    float step100[2];           // StepSize * VOLUME_DENSITY per stream (0: a, 1: r)
    float* fs_keep[2];          // per stream: ChunkStream::fs_keep / fs_spill / fs_cap of THIS pass
    float* fs_spill[2];
    uint32_t fs_cap[2];
    const int32_t* fs_slot;     // rank of every block of this pass (k_occ_compact), shared by the streams; -1: flagged empty
    const uint8_t* flags;       // k_unit_flags: the pass's empty-block flags, [slice group][block y][block x]
};
struct DualOcc {
    int on;
    DualPass pass[2];
};
// The run list of a dual launch (k_occ_runs, tbrm_light_kernels.hip): the live units of the launch's work list as runs of up to
// `len` z-adjacent units of one column, one word each — (length - 1) << kRunLenShift | first unit — in the order the workgroups
// take them: all runs of `len` units first, then the shorter ones by descending length (the last workgroups to start are the
// shortest), each length class dealt to the 8 XCDs in eighths (spatial neighbours behind one L2) and padded with kRunNone to whole
// rounds of 8. count[1] is the number of words.
constexpr int kOccRunMax = 64;             // longest run (a run never crosses a multiple of 64 units in z)
constexpr int kRunLenShift = 26;           // a launch of more than 2^26 units takes the per-unit form
constexpr uint32_t kRunNone = 0xffffffffu; // padding: the workgroup has nothing to do
constexpr size_t kRunMaskWords = 4096;     // k_occ_runs holds a 64-bit liveness word per column and 64 units of z in LDS: larger launches take the per-unit form
struct OccRuns {
    int len;                 // TUNE_OCC_RUN, clamped to kOccRunMax
    uint32_t* list;          // k_occ_runs writes, k_light_occlusion_runs reads: room for units + 8 * kOccRunMax words
    int* count;              // BlockLists::count (16 ints)
    int* count_host;         // pinned: [1] units that are not the first of their run (tbrm_path_counters out[15])
};
// k_light_sweep (tbrm_light_sweep.hip): one launch advances every 32x32 tile of the slice plane through a whole span of
// slices. The previous-slice taps of a pass lie on ONE side of the pixel per plane axis (the constant PrevPixelOffset,
// AddDirLightShader.usf:81-82), so a tile depends on at most three neighbours — the ones towards the light — and the tiles
// form a pipeline: tile t runs a few slices behind its upstream neighbours and reads the hx columns / hy rows it needs of
// their slice from a hand-off record in global memory (dwords {16-bit launch tag, UNORM8 code of stream r, of stream a},
// written and polled with relaxed agent-scope atomics: no fences, no kernel boundary, no recomputed halo).
struct SweepParams {
    int sx, sy;             // side of the previous-slice taps along the plane's x / y: +1, -1, 0 (none: the tap is the pixel itself)
    int hx, hy;             // how many columns / rows beyond the tile they reach (both streams)
    // A fused Change whose lights pull opposite ways along a plane axis has no tile order that serves both streams. Its
    // removed light is then propagated FIRST, alone, in its own order (a PASS_PLANES launch into rec[1]); the fused launch
    // runs in the added light's order and takes the removed light's halo from those finished records.
    int r_from_records;     // PASS_CHANGE: stream r's halo comes from rec[1] (tag r_epoch), geometry r_sx .. r_hy
    int r_sx, r_sy, r_hx, r_hy;
    uint32_t r_epoch;
    uint32_t* rec[2];       // [0]: the hand-off records, [slice of the launch][tile][32*hx + 32*hy words]; [1]: r_from_records
    uint32_t epoch;         // this launch's tag, 1 .. 2^16 - 1 (records are not cleared between launches)
    int unused0;            // (0; read by nothing. It and unused1 keep every other field where it is in the kernel-argument segment: without
                            // them the compiler pairs the scalar loads of the arguments differently, and the scalar register allocation
                            // and SGPR spill counts of the sweep kernels move — a layout change wants a measurement of its own)
    int stagger_ns;         // a tile d tiles away from the upstream corner starts d * stagger_ns late: the distance it would
                            // otherwise fall behind by polling (a tile can never make up lag, and every poll that finds nothing
                            // costs a memory round trip: arriving late on purpose is cheaper than arriving early)
    int* ticket;            // [0]: next tile to start (tiles are dealt in upstream-first order: a tile only ever waits for tiles
                            // that started before it), [1]: tiles finished (the last one re-arms both)
    int debug;              // diagnostics (sweep_debug tunable): bit 0 = tiles do not wait for each other (WRONG results: slice time alone);
                            // bit 1 = every tile leaves four time stamps (10 ns units) in `stamps`
    unsigned long long* stamps; // [tile][4]: start of slice 0, end of slice 63, end of the last slice, after the write-back
    int unused1;            // (0; see unused0)
    int lv_f32;             // the light volume (and the planes) are floats: k_light_sweep<..., FMT_F32>, record words are 8-byte {float, launch tag} granules
    int reinit_slice;       // > 0: the launch's first reinit_slice slices lie in front of the volume (a pass that runs downwards from a
                            // depth that is no multiple of 8, padded to whole brick layers): slice reinit_slice - 1 hands on the pass's
                            // initial plane instead of what it computed
    int n_real;             // slices of the launch that lie inside the volume when the padding comes last (an upward pass whose depth is
                            // no multiple of 8): the slices from n_real on leave the light volume alone. n_steps: none are padding
    int* error;             // set when a tile gave up waiting (bit 0) or found its taps outside the halo (bit 1)
    unsigned long long give_up_ticks; // how long a poll waits for a neighbour's word, in 10 ns ticks of wall_clock64 (tunable sweep_timeout_ms)
};

// Several axis passes in ONE sweep launch (k_light_sweep_chain): the tiles of pass i + 1 take their tickets behind every tile of
// pass i, so they start as pass i's tiles retire — the fill of a pass runs under the drain of the one before instead of behind a
// kernel boundary (30 hops x ~2.9 us of every pass are fill / drain at 512^3). What orders the two passes' read-modify-writes of
// the light volume is data, not a boundary: a tile writes its brick layers back with write-through (sc1) stores and then
// publishes "k layers written back" in its progress word {16-bit launch tag, count} (relaxed agent-scope store behind a drained
// vmcnt); a tile of the next pass reads a brick layer (sc1 loads) only after the progress word of the ONE tile of the pass before
// that owns those bricks has reached the layer it needs. Forward progress: a tile only ever waits for tiles with smaller tickets.
struct SweepLink {
    uint32_t* prog_out;        // this pass's progress words, [tile]
    const uint32_t* prog_in;   // the pass before's (the launch's first pass: any valid words — in_G = 0, it needs nothing of them)
    uint32_t in_epoch;         // ... and its launch tag
    int in_axis, in_tiles_x;   // ... its axis and tiles per row
    int in_down, in_layer0, in_G; // ... its direction, first brick layer and number of layers
    int coherent_loads;        // this pass reads its brick layers with sc1 loads: every pass but the launch's first
    int ticket0;               // first ticket of this pass
    int total_tiles;           // tiles of the whole launch (the last one to finish re-arms the tickets)
};
constexpr int kSweepChainMax = 4; // passes per launch (the kernel's arguments hold their parameter blocks: 4 x ~0.6 KB)
struct SweepChainPass {
    ChunkParams p;
    SweepParams q;
    SweepLink link;
};
struct SweepChainArgs {
    int n;
    SweepChainPass pass[kSweepChainMax];
};

// The view cache's records of one frame (DESIGN.md 4.1 "Relit frames"): what k_raymarch_lit's recording forms write and k_relight
// reads. A wave is numbered by its workgroup's linear launch id (before the XCD band mapping) and its number in the workgroup; its
// trips that had something to accumulate are stored in order from trip offsets[wave] on. Per trip one wave-uniform word (the trip's
// first sample index) and a 64-lane block in struct-of-arrays order: a float4 row (colour.rgb, corrected opacity; w = -1: nothing to
// accumulate) and three float rows (the saturated position the light volume is sampled at).
constexpr size_t kRayRecordRowBytes = 64 * (sizeof(float4) + 3 * sizeof(float)); // 1792
constexpr size_t kRayRecordTripBytes = kRayRecordRowBytes + sizeof(int32_t);
struct RayRecord {
    uint32_t* counts;   // [wave] recorded trips (written by the count form)
    uint32_t* offsets;  // [wave] first trip of the wave (k_view_scan)
    uint32_t* meta;     // {total trips, fits the arena} (k_view_scan)
    int32_t* base;      // [trip] the wave-uniform word: the trip's first sample index
    char* rows;         // [trip] kRayRecordRowBytes each
};

struct RayParams {
    VolumeDev data;
    int data_addr_mode; // ADDR_WRAP / ADDR_CLAMP
    const float4* tf;
    WindowDev win;
    const void* light;  // bricked
    int lv_dims[3];
    int lv_bnx, lv_bnxy;
    int lv_fmt;
    float cam_pos[3], fwd[3], right[3], up[3];
    float thx, thy;
    int width, height;  // full framebuffer
    float m[12];        // WorldToLocal rows (3x3 + translation)
    float cc[3], cd[3];
    int clip_mode;      // 0: clip plane provably never clips a sample position; 1: general
    int share_grid;     // light volume has the data volume's size and wrap addressing: taps share their offsets
    int wave_skip;      // k_raymarch_lit takes the empty trips a whole wave shares in one go (pays in large volumes)
    int tile_x0, tile_y0, tile_w, tile_h, row_group_step;
    float steps;
    int jitter_frame;
    const float* depth; // may be null
    float* out;         // tile_w*tile_h*4
    const uint32_t* empty_bits; // one bit per brick; null when skipping is off
    int xcd_rows;               // k_raymarch_lit: rows of pixel blocks per band dealt to one XCD (tunable ray_xcd_rows; 0: launch order)
    const uint2* tab;           // k_raymarch_lit TAB: per axis and texel index the {voxel offset, brick-index part} of the addressed
                                // texel, laid out by ray_tab_* below; null: none (slab-resident handles)
    const uint8_t* skip_dist;   // per brick: Chebyshev distance (bricks, capped) to the nearest non-empty brick; null when skipping is off
    int bnx, bny, bnz;  // brick grid
    unsigned long long* sample_counter; // count kernel only
    int lv_wrap_layer, lv_wrap_shift; // VolumeDev::wrap_layer / wrap_shift of the light volume
    int slab_on, slab_z0, slab_z1, slab_dir; // slab stage of the lit march: owned light-volume slices, sweep direction (+1 / -1 / 0: all rays)
    const uint16_t* octree;     // octree march only: the level marched (dense, x fastest)
    int oct_dims[3];            // its dimensions
    float oct_depth0;           // depth of octree level 0 (the z coordinate is rescaled by data depth / this)
    const uint8_t* labels;      // k_raymarch_lit LABELS: the label volume, bricked on the data volume's grid (null: no label step)
    const float4* lab_colors;   // ... its colour table (256 x RGBA float)
    const void* light_g;        // k_raymarch_lit RGB (colour handles, tbrm_color_lights.h): the G and B channels of the light volume,
    const void* light_b;        // laid out like `light` (then the R channel); null: a mono light volume
    RayRecord rec;              // the recording forms of k_raymarch_lit and k_relight only (else null)
};

// What launch_ray2 / launch_ray3 decide for a frame (the view cache keys on both: tbrm_api_render.cpp)
int ray_lanes_for(const RayParams& p);   // lanes per ray: 4 or 8
bool ray_tables_for(const RayParams& p); // the LDS offset tables (k_raymarch_lit TAB) apply

// k_raymarch_hit's own arguments beside the view's RayParams (include/tbrm_hit.h; tbrm_kernels.hip compiled as the hit unit). RayParams
// itself stays as it is: the view cache compares it as a block, and k_raymarch_lit's kernel-argument segment keeps its layout.
struct HitParams {
    uint4* hits;     // tile_w x tile_h records of two 16-byte words (tbrm_hit), row-major
    float* depth;    // tile_w x tile_h floats, or null
    float threshold; // a ray's hit: the first sample after whose steps LightEnergy.a > threshold
    float dg[3], d0; // distance along camera.forward of a position u of the unit cube: dg . (u - 0.5) + d0, in world units
};

// Layout of RayParams::tab (built in tbrm_resources_create, copied into LDS and read by k_raymarch_lit TAB): the x, then the y, then
// the z axis, one entry for every texel index -kRayTabApron .. n + kRayTabApron - 1 (a base tap two texels outside the volume and its
// +1 tap still have entries), the total padded to an even count (the copy moves 16 bytes at a time).
constexpr int kRayTabApron = 2;
constexpr int ray_tab_axis_entries(int n) { return n + 2 * kRayTabApron; }
constexpr int ray_tab_index(int texel) { return texel + kRayTabApron; }
constexpr int ray_tab_last_base(int n) { return ray_tab_axis_entries(n) - 2; } // the last index of an axis whose +1 entry exists
constexpr int ray_tab_entries(int nx, int ny, int nz) { return (ray_tab_axis_entries(nx) + ray_tab_axis_entries(ny) + ray_tab_axis_entries(nz) + 1) & ~1; }

struct BrickParams {
    VolumeDev data;
    int addr_mode;
    int bnx, bny, bnz;
    float2* minmax;
    int bz0, bz1;     // brick layers whose voxels (and +1 apron) may be read; the others get the range [-inf, +inf] (never empty)
};

struct EmptyParams {
    const float2* minmax;
    int n_bricks;
    WindowDev win;
    const int* alpha_prefix; // 257 entries: # of TF texels j < i with alpha > 0 (or NaN)
    uint32_t* bits;
};

hipError_t launch_shell_transparent(const EmptyParams& p, int bnx, int bny, int bnz, float border, int* flag, hipStream_t s);

constexpr int kSkipDistCap = 32;
struct DistParams {
    const uint32_t* bits; // pass 0: the k_brick_empty bits
    const uint8_t* in;    // later passes: the previous pass (null in pass 0)
    uint8_t* out;
    int bn[3];
    int axis;
};

struct OctreeParams {
    VolumeDev data;        // level 0: the bricked data volume
    const uint16_t* lower; // levels 1..3: the level below
    int lower_dims[3];
    uint16_t* out;
    int dims[3];
};

struct RelayoutParams {
    const void* src;
    void* dst;
    int nx, ny, nz;
    int bnx, bnxy, bnz;
    int elem_bytes;
    int to_bricks; // 1: linear -> bricked (padding voxels are zeroed); 0: bricked -> linear
};

constexpr int kChunkTile = 32;      // core tile edge of the chunked propagation kernel (pixels)
constexpr int kChunkThreads = 1024;
constexpr int kChunkMaxHull = 64;   // T + steps * growth must stay within this

// Process-wide tunables (A/B switches of the measurements in DESIGN.md and of the parity tests). Each starts from the
// environment variable TBRM_<NAME> read ONCE when the library is loaded; afterwards tbrm_set_tunable changes it. No launch
// path reads the environment.
enum Tunable : int {
    TUNE_FORCE_SLICE_KERNEL, // 1: every axis pass takes the reference's one-slice-per-launch structure (k_propagate_slice)
    TUNE_CHUNK_STEPS,        // > 0: only this chunk length is tried (16 / 8 / 4 / 2)
    TUNE_OCC_SLICES,         // slices per occlusion span (0: default)
    TUNE_SPARSE_OCC,         // 0: occlusion blocks that can only see empty bricks are computed like the others
    TUNE_OCC_LIST,           // 0: live occlusion blocks keep their grid position instead of being dealt from a work list
    TUNE_LIGHT_CACHE_MB,     // HBM budget of the factor cache in MiB (0: off, < 0: an eighth of the device's memory): a light's occlusion factors, kept per axis pass
    TUNE_LIGHT_BATCHING,     // tbrm_add_dir_lights: 0 never pair passes, 1 pair when it pays, 2 pair whatever fits
    TUNE_SHARE_GRID,         // 0: the raymarch computes the light volume's tap offsets separately even on a shared grid
    TUNE_RAY_WAVE_SKIP,      // RayParams::wave_skip: 1 on, 0 off, -1 = where the data volume is at least 384 voxels a side
    TUNE_RAY_LANES,          // lanes per ray of k_raymarch_lit: 4, 8, or 0 = by load
    TUNE_CHAIN_FAST_LOOP,    // 0: full, aligned chunks run the generic slice loop too (A/B of the unrolled, branch-free loop)
    TUNE_CHAIN_RECT_PLANES,  // 0: no 72 x 48 LDS planes (a pass with taps two texels wide along x runs 8-slice chunks in square planes)
    TUNE_OCC_OVERLAP,        // workgroups per CU of an occlusion launch that runs beside the previous span's chain (0: never beside it)
    TUNE_LIGHT_SWEEP,        // 0: axis passes never take the pipelined sweep kernel (k_light_sweep); 1: where it applies
    TUNE_SWEEP_PREFETCH,     // accepted, no effect (the name is part of the C-ABI's documented surface): the distance a sweep tile requests its
                             // neighbours' hand-off words ahead is fixed per kernel instantiation — 2 slices, 3 for six-chunk records
    TUNE_STREAM_PRIORITY,    // priority of a handle's own stream, read when the handle is created: 0 = default, 1 = the highest the
                             // device offers, -1 = the lowest
    TUNE_SWEEP_DEBUG,        // diagnostics. 1: sweep tiles do not wait for each other (WRONG results), 2: per-tile time stamps, 4: host
                             // time per operator phase on stderr, 8 / 16: the occlusion stream skips its waits for the scratch
                             // store / the cache entry to be idle (WRONG results: what gates its start?), 32: no timing events
    TUNE_SWEEP_TIMEOUT_MS,   // how long a sweep tile waits for a neighbour's hand-off word before it gives up and raises the handle's error
                             // word (0: 2 s; < 0: not at all — a test hook: every word that is not there yet fails the launch)
    TUNE_FAST_WINDOW_DIV,    // 0: the kernels always divide by the window's width (IEEE sequence); 1: three fmas where the host vouches
                             // for the window (WindowDev::fast_div) — the same bits
    TUNE_SLAB_SWEEP,         // 1: a slab's share of a pass along z runs as one pipelined sweep instead of the chunked chain (measured at
                             // 1024^3: a tie at 2 and 4 slabs, 6 % slower at 8 — a 128-slice sweep over 1024 tiles is mostly pipeline fill; off)
    TUNE_GPU_TIMING,         // 0: operators do not record the HIP events behind tbrm_last_gpu_time_ms (four markers per step between
                             // dependent kernels: a host that never asks for GPU times need not pay them)
    TUNE_RAY_TABLES,         // 0: k_raymarch_lit computes the data taps' offsets per sample even where its LDS offset tables apply
    TUNE_SWEEP_EPOCH_PRESET, // > 0: a handle's first sweep launch continues from this launch tag (a test hook: the 16-bit tags of the
                             // hand-off records start over after 65535 launches)
    TUNE_OCC_DUAL,           // 1: the two axis passes of a light share ONE occlusion launch where their sampling positions are bit-equal
                             // (DualOcc); 0: one launch per pass
    TUNE_SWEEP_CHAIN,        // consecutive sweep passes of an operator per launch (k_light_sweep_chain): 1 = one launch per pass, up to 4
    TUNE_RAY_XCD_ROWS,       // k_raymarch_lit: rows of pixel blocks per band dealt to one XCD (0: blocks in launch order, i.e. round-robin)
    TUNE_RAY_LABELS,         // 1: the lit march takes the label step whenever a label volume is attached, even when no label present in
                             // it has a colour alpha > 0 (a test hook: the same frame by the other kernel); 0: only when one does
    TUNE_STATS_GROUPS,       // > 0: the statistics kernels (tbrm_stats_kernels.hip) launch at most this many workgroups, so that a wave
                             // takes many bricks of even a small volume (a test hook and an A/B switch); 0: sized to the device
    TUNE_OCC_RUN,            // dual occlusion launches: a workgroup takes up to this many z-adjacent live units of one column in a row and
                             // keeps what they share (k_light_occlusion_runs; at most kOccRunMax); 1: one unit per workgroup (the A/B switch)
    TUNE_VIEW_CACHE_MB,      // HBM budget in MiB of the view cache's records (a still view under a moving light is relit from them: k_relight);
                             // 0: off, every frame marches
    TUNE_GROW_BATCH,         // tbrm_grow_region: propagation passes enqueued between two read-backs of their changed-bricks words (1 .. 64;
                             // 1: a read-back per pass — the test hook). The result does not depend on it
    TUNE_MORPH_STEPS,        // tbrm_morph_labels: unit steps one launch of k_morph_steps iterates in a brick's 24^3 window (1 .. 8; 1: a launch
                             // per step — the test hook and the A/B switch). The result does not depend on it
    TUNE_MARGIN_SKIP,        // tbrm_margin_labels, tbrm_label_distance: 1: bricks whose result the board classes give are not computed; 0: every
                             // brick of the range is (the test hook and the A/B switch). The result does not depend on it
    TUNE_SMOOTH_SKIP,        // tbrm_smooth_labels: 1: bricks whose result the board classes give are not computed; 0: every brick of the range
                             // is (the test hook and the A/B switch). The result does not depend on it
    TUNE_SCISSORS_SKIP,      // tbrm_scissors_labels: 1: bricks whose result the source set or their corners give are not projected; 0: every brick of
                             // the range is, voxel by voxel (the test hook and the A/B switch). The result does not depend on it
    TUNE_PAINT_SKIP,         // tbrm_paint_labels: 1: a brick tests only the segments whose grown box it meets, and one whose corners lie within
                             // one segment is taken whole; 0: every brick of the range tests every voxel against every segment (the test
                             // hook and the A/B switch). The result does not depend on it
    TUNE_SURFACE_SKIP,       // tbrm_label_surface: 1: blocks of cells whose eight boards are all empty, or all full inside the box, are not
                             // computed; 0: every block of the range is (the test hook and the A/B switch). The result does not depend on it
    TUNE_COUNT
};
int tune(Tunable t);

// launchers (tbrm_kernels.hip, tbrm_light_kernels.hip)
hipError_t launch_selftest_decode(float* d_u8, float* d_u16, hipStream_t s);
hipError_t launch_selftest_roundtrip(const float* d_in, float* d_out, size_t n, hipStream_t s);
hipError_t launch_selftest_window_division(const WindowDev& w, unsigned long long* d_mismatches, hipStream_t s);
hipError_t launch_selftest_opacity_correction(float step0, float step1, unsigned long long* d_mismatches, hipStream_t s);
hipError_t launch_relayout(const RelayoutParams& p, hipStream_t s);
size_t chunk_lds_bytes(const ChunkParams& p, int mode, int lv_fmt);
size_t occlusion_lds_bytes(const ChunkParams& p); // dynamic LDS of an occlusion workgroup (the bricks it stages)
constexpr int kPlaneGuard = 4096; // floats of slack on both sides of every plane/occlusion buffer (16-byte row copies overrun rows)
hipError_t launch_occ_flags(const ChunkParams& p, int mode, int n_chunks, hipStream_t s); // + the work lists
hipError_t launch_light_occlusion(const ChunkParams& p, int mode, hipStream_t s, const DualOcc* dual = nullptr, const OccRuns* runs = nullptr); // runs: a dual launch in run form
hipError_t launch_unit_flags(const ChunkParams& pc, const DualOcc& d, hipStream_t s); // + the units' work list (pc: the virtual pass along the third axis)
bool occ_runs_apply(const ChunkParams& pc);                                          // may a dual launch over pc's units take the run form?
hipError_t launch_occ_runs(const ChunkParams& pc, const OccRuns& runs, hipStream_t s); // the run list of the units' flags (pc.occ_flags_out)
hipError_t launch_light_chain(const ChunkParams& p, int mode, int lv_fmt, hipStream_t s);
hipError_t launch_light_sweep(const ChunkParams& p, const SweepParams& q, int mode, hipStream_t s);
hipError_t launch_light_sweep_chain(const SweepChainArgs& c, int mode, hipStream_t s); // PASS_ADD / PASS_CHANGE, UNORM8 light volumes
hipError_t launch_fill(void* dst, int fmt, size_t n, float value, hipStream_t s);
hipError_t launch_propagate_slice(const PropParams& p, bool change, hipStream_t s);
hipError_t launch_raymarch(const RayParams& p, hipStream_t s);
hipError_t launch_raymarch_rgb(const RayParams& p, hipStream_t s); // (colour handles: tbrm_kernels.hip compiled as the RGB unit)
// the view cache (tbrm_kernels.hip compiled as the recording unit): the march that also counts (fill = false) or writes (true) p.rec,
// the scan between the two, and the frame from the records
hipError_t launch_raymarch_recording(const RayParams& p, bool fill, hipStream_t s);
hipError_t launch_view_scan(const RayRecord& rec, uint32_t n_waves, uint32_t cap_trips, hipStream_t s);
hipError_t launch_relight(const RayParams& p, hipStream_t s);
hipError_t launch_raymarch_hit(const RayParams& p, const HitParams& h, hipStream_t s); // (tbrm_kernels.hip compiled as the hit unit)
hipError_t launch_raymarch_intensity(const RayParams& p, hipStream_t s);
hipError_t launch_raymarch_octree(const RayParams& p, hipStream_t s);
hipError_t launch_octree_level(const OctreeParams& p, bool base, hipStream_t s);
hipError_t launch_count_samples(const RayParams& p, hipStream_t s);
hipError_t launch_brick_minmax(const BrickParams& p, hipStream_t s);
hipError_t launch_brick_empty(const EmptyParams& p, hipStream_t s);
hipError_t launch_brick_dist(const DistParams& p, int addr_mode, hipStream_t s);

// label overlay (tbrm_api_labels.cpp, tbrm_volume_kernels.hip)
struct LabelBrickParams {
    const uint8_t* labels; // bricked label volume
    uint32_t* masks;       // per brick: 8 words, the set of labels among its voxels
    int bnx, bny;          // brick grid (x, y)
    int b0[3], b1[3];      // bricks [b0, b1) per axis to (re)compute
};
struct LabelLiveParams {
    const uint32_t* masks;
    int n_bricks;
    uint32_t alive[8];     // labels whose colour alpha is > 0
    uint32_t* live;        // per brick bit: holds an alive label
    uint32_t* present;     // 8 words, OR of every brick's set (pre-cleared)
};
struct LabelMergeParams {
    const uint32_t* empty; // k_brick_empty bits of the data volume
    const uint32_t* live;  // LabelLiveParams::live
    uint32_t* out;         // empty and no live label brick within Chebyshev distance 1 (the sampler's brick addressing)
    int bn[3];
};
struct LabelRegionParams {
    const uint8_t* src;    // the sub-box, dense, x fastest
    uint8_t* dst;          // bricked label volume
    int origin[3], extent[3];
    int bnx, bnxy;
};
hipError_t launch_label_brick_masks(const LabelBrickParams& p, hipStream_t s);
hipError_t launch_label_live(const LabelLiveParams& p, hipStream_t s);
hipError_t launch_label_merge(const LabelMergeParams& p, int addr_mode, hipStream_t s);
hipError_t launch_label_region(const LabelRegionParams& p, hipStream_t s);

// data-volume region updates (tbrm_api_volume_region.cpp, tbrm_volume_kernels.hip)
struct VolumeRegionParams {
    const void* box;       // the sub-box [origin, origin + extent), dense, x fastest (written when to_bricks is 0)
    void* bricked;         // the bricked volume (read when to_bricks is 0)
    int origin[3], extent[3];
    int bnx, bnxy;
    int elem_bytes;
    int to_bricks;         // 1: box -> bricked (voxels outside the box are left alone); 0: bricked -> box
};
// the bricks whose k_brick_minmax range a box can have changed: per axis [lo, hi] and, for i beyond that range, `last`
struct BrickReach {
    int lo[3], hi[3], last[3];
    int n[3];              // bricks per axis: hi - lo + 1, + 1 when `last` is reached as well and lies outside [lo, hi]
};
hipError_t launch_volume_region(const VolumeRegionParams& p, hipStream_t s);
hipError_t launch_brick_minmax_region(const BrickParams& p, const BrickReach& q, hipStream_t s);

// volume statistics (tbrm_api_volume_stats.cpp, tbrm_stats_kernels.hip; include/tbrm_volume_stats.h)
constexpr int kStatsMaxBins = 4096;
constexpr int kStatsLabelWords = 256 * 6; // the label records: count, nan, ~min key, max key (256 uint32 each), then 256 8-byte sums
struct StatsParams {
    const void* data;      // bricked data volume
    const uint8_t* labels; // bricked label volume on the same grid (null: none)
    int fmt;
    int bnx, bnxy;
    VoxelBox box;          // inside the volume
    BrickRange range;      // the bricks it touches
    // histogram: the binning rule of tbrm_volume_stats.h
    uint32_t n_bins;
    uint32_t lo_code, hi_code;
    uint32_t div_mul, div_shift; // floor(n / (hi_code - lo_code + 1)) = mulhi(n, div_mul) >> div_shift for n < 2^28 (stats_divisor)
    float lo_f, hi_f, scale;
    uint32_t copies;       // LDS copies of the histogram per workgroup (a power of two, copies * n_bins <= kStatsMaxBins)
    uint32_t mask[8];      // MASKED: the labels that count
    uint32_t* out;         // histogram: n_bins + 4 words, added to; label statistics: kStatsLabelWords words, zeroed, added to
};
hipError_t launch_volume_histogram(const StatsParams& p, bool masked, int grid, hipStream_t s);
hipError_t launch_label_statistics(const StatsParams& p, int grid, hipStream_t s);

// seeded region growing (tbrm_api_segment.cpp, tbrm_segment_kernels.hip; include/tbrm_segment.h)
constexpr int kGrowMaxSeeds = 4096;
constexpr int kGrowMaxBatch = 64;
// the control words of a call (GrowParams::ctl; the host writes their start values and reads them back)
enum GrowCtl : int {
    GROW_VOXELS, GROW_RELABELLED, GROW_MIN_X, GROW_MIN_Y, GROW_MIN_Z, GROW_MAX_X, GROW_MAX_Y, GROW_MAX_Z, GROW_SEEDS_TAKEN,
    GROW_BRICKS_WRITTEN, GROW_VISITS,
    GROW_CHANGED = 16,        // kGrowMaxBatch words: bricks that changed in pass i of the batch
    GROW_CTL_WORDS = GROW_CHANGED + kGrowMaxBatch
};
static_assert(GROW_MAX_Z == GROW_MIN_X + 5, "WaveBounds commits to six consecutive words");
struct GrowParams {
    const void* data;      // bricked data volume
    uint8_t* labels;       // bricked label volume on the same grid (null: none, every voxel has label 0)
    int fmt;
    int bnx, bnxy;
    VoxelBox box;          // inside the volume
    BrickRange range;      // the bricks it touches — the only bricks whose scratch a call reads or writes
    uint32_t lo_code, hi_code; // UNORM: lo_code <= code <= hi_code (lo_code > hi_code: no candidate)
    float lo_f, hi_f;          // R32_FLOAT: lo_f <= v <= hi_f (NaN voxels fail both)
    uint32_t writable[8];
    int all_join;          // n_seeds == 0: visited starts as the candidates
    int conn26;
    uint64_t* bits;        // per brick (global brick index) 16 words: candidate slices z = 0 .. 7, then visited slices; bit y * 8 + x
    uint32_t* act[2];      // per brick: due in this pass ([0]: read and cleared) / in the next ([1]: set)
    const int32_t* seeds;
    int n_seeds;
    int first_pass;        // the seeds' bricks count as changed
    int changed_word;      // GROW_CHANGED + the pass's index in its batch
    int new_label;
    int32_t* ctl;          // GROW_CTL_WORDS words
};
hipError_t launch_grow_candidates(const GrowParams& p, hipStream_t s);
hipError_t launch_grow_seeds(const GrowParams& p, hipStream_t s);
hipError_t launch_grow_pass(const GrowParams& p, hipStream_t s);
hipError_t launch_grow_measure(const GrowParams& p, hipStream_t s);
hipError_t launch_grow_write(const GrowParams& p, const BrickRange& w, hipStream_t s); // into the bricks w

// label morphology (tbrm_api_morph.cpp, tbrm_morph_kernels.hip; include/tbrm_morphology.h). It works in the scratch of region growing:
// the 16 words of a brick are two boards of 8 slice words (bit y * 8 + x of word z), the two activity words are the boards' classes.
// the control words of a call (MorphParams::ctl), inside the GROW_CTL_WORDS words of the scratch: 64-bit counts, then the 32-bit box
enum MorphCtl : int {
    MORPH_SOURCE, MORPH_RESULT, MORPH_ADDED, MORPH_REMOVED, MORPH_RELABELLED, MORPH_WINDOWS, MORPH_BRICKS_WRITTEN, MORPH_CTL_COUNTS, // uint64 each
    MORPH_MIN_X = 2 * MORPH_CTL_COUNTS, MORPH_MIN_Y, MORPH_MIN_Z, MORPH_MAX_X, MORPH_MAX_Y, MORPH_MAX_Z, MORPH_CTL_WORDS             // int32 each
};
static_assert(MORPH_MAX_Z == MORPH_MIN_X + 5, "WaveBounds commits to six consecutive words");
static_assert((int) MORPH_CTL_WORDS <= (int) GROW_CTL_WORDS, "the morphology control words live in the region growing scratch");
struct MorphParams {
    uint8_t* labels;       // bricked label volume
    int bnx, bnxy;
    int dims[3];           // the volume in voxels: bits outside it are never set
    VoxelBox box;          // what may change
    BrickRange range;      // the bricks of the box grown by the operator's reach: the only bricks whose scratch a call reads or writes
    BrickRange wrange;     // the bricks of the box
    uint32_t source[8], writable[8];
    uint64_t* bits;        // per brick (global brick index) 16 words: board 0, board 1
    uint32_t* cls[2];      // per brick: the class of board 0 / 1
    int from;              // k_morph_steps reads board `from` and writes the other; k_morph_write reads board `from`
    int steps;             // unit steps of this launch, 1 .. 8
    int erode;             // the steps erode: the same loop on the complement inside the volume
    int conn26;
    int new_label;         // -1: count only
    int erase_label;
    int32_t* ctl;
};
hipError_t launch_morph_load(const MorphParams& p, hipStream_t s);
hipError_t launch_morph_steps(const MorphParams& p, hipStream_t s);
hipError_t launch_morph_write(const MorphParams& p, hipStream_t s);

} // namespace tbrm
