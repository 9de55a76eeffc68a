// tbrm_api_surface.cpp — the surface of a set of labels as an indexed mesh (include/tbrm_surface.h): validation, the
// scratch and the counters around the kernels of tbrm_surface_kernels.hip, and the two host functions (tbrm_surface_plan.h).
//
// A call is: the source set of the box's bricks from the label bytes into board 0 (k_morph_load, as it stands, in the scratch of
// region growing), k_surface_count over the blocks of the cell box, the scan of the two counts, the read-back of the control words —
// the counts the caller's capacities are held to — and, when something is to be written and fits, k_surface_emit. The host form
// emits into a staging buffer of the handle and copies from there. Nothing of the handle is written but scratch.
#include "tbrm_resources.h"
#include "tbrm_surface_kernels.h"
#include "../../include/tbrm_surface.h"

#include <cmath>
#include <cstddef>
#include <cstring>

using namespace tbrm;
using namespace tbrm_host;

static_assert(TBRM_SURFACE_MAX_DIM == kSurfaceMaxDim && TBRM_SURFACE_TRIANGLES == SURFACE_TRIANGLES && TBRM_SURFACE_MEASURE == SURFACE_MEASURE, "tbrm_surface_plan.h restates the header's constants");
static_assert(sizeof(tbrm_surface_vertex) == sizeof(SurfaceVertex) && offsetof(tbrm_surface_vertex, sum) == offsetof(SurfaceVertex, sum) && offsetof(tbrm_surface_vertex, edges) == offsetof(SurfaceVertex, edges) &&
              offsetof(tbrm_surface_vertex, normal) == offsetof(SurfaceVertex, normal) && offsetof(tbrm_surface_vertex, corners) == offsetof(SurfaceVertex, corners), "tbrm_surface_plan.h restates the header's record");

namespace {

constexpr int kSurfaceLaunchesCount = 4; // k_morph_load, k_surface_count, the scan's two

// d_surface: what the kernels keep per block and per tile, and the control words; each part 256-byte aligned
struct SurfaceScratch {
    uint64_t* active;
    uint32_t* prefix;
    uint32_t *count[2], *base[2];
    uint64_t *tile_sum[2], *tile_base[2];
    int32_t* ctl;
    size_t bytes;
};
SurfaceScratch surface_scratch(char* base, size_t n_blocks)
{
    const size_t tiles = (n_blocks + kSurfaceTile - 1) / kSurfaceTile;
    Carver c{base};
    SurfaceScratch s{};
    s.ctl = c.take<int32_t>(SURF_CTL_WORDS);
    s.active = c.take<uint64_t>(n_blocks * 8);
    s.prefix = c.take<uint32_t>(n_blocks * 8);
    for (int w = 0; w < 2; ++w) {
        s.count[w] = c.take<uint32_t>(n_blocks);
        s.base[w] = c.take<uint32_t>(n_blocks);
        s.tile_sum[w] = c.take<uint64_t>(tiles);
        s.tile_base[w] = c.take<uint64_t>(tiles);
    }
    s.bytes = c.off;
    return s;
}

// one of the handle's two surface buffers (0: the scratch, 1: the host form's staging), only ever grown: a call that needs no more
// than one before it allocates nothing
int ensure_surface_buffer(tbrm_resources* r, int which, size_t bytes)
{
    if (r->surface_bytes[which] >= bytes) return TBRM_OK;
    if (int e = ensure_bytes(r, r->d_surface[which], r->surface_bytes[which], bytes, which ? "surface staging" : "surface scratch")) return e;
    ++r->surface_counters[5];
    return TBRM_OK;
}

// the staging of the host form: [the records][the indices][the positions]
struct SurfaceStaging {
    uint32_t *vertices, *indices;
    float* positions;
    size_t bytes;
};
SurfaceStaging surface_staging(char* base, uint64_t vertices, uint64_t quads, bool triangles, bool positions)
{
    Carver c{base};
    SurfaceStaging s{};
    s.vertices = c.take<uint32_t>((size_t) vertices * kSurfaceVertexWords);
    s.indices = c.take<uint32_t>((size_t) quads * (triangles ? 6 : 4));
    s.positions = positions ? c.take<float>((size_t) vertices * 3) : nullptr;
    s.bytes = c.off;
    return s;
}

// what the call checks of a desc before the handle's state; the box
int surface_arguments(const tbrm_resources* r, const tbrm_surface_desc* d, VoxelBox& box, BrickRange& bricks)
{
    if (d->flags & ~(uint32_t) SURFACE_FLAGS) return fail(TBRM_ERR_INVALID_ARG, "flags 0x%x: unknown bits (TBRM_SURFACE_TRIANGLES | TBRM_SURFACE_MEASURE)", (unsigned) d->flags);
    if (d->reserved != 0) return fail(TBRM_ERR_INVALID_ARG, "reserved %d: must be 0", (int) d->reserved);
    for (int c = 0; c < 3; ++c)
        if (!std::isfinite(d->scale[c]) || !std::isfinite(d->offset[c])) return fail(TBRM_ERR_INVALID_ARG, "scale[%d] = %g, offset[%d] = %g: both must be finite", c, d->scale[c], c, d->offset[c]);
    const tbrm_resources::Dims dims = r->data_dims();
    const int dd[3] = {dims[0], dims[1], dims[2]};
    if (int e = begin_label_edit(r, "no label volume")) return e;
    for (int c = 0; c < 3; ++c)
        if (dd[c] > TBRM_SURFACE_MAX_DIM) return fail(TBRM_ERR_UNSUPPORTED, "a volume of %d x %d x %d: the surface takes at most %d voxels along an axis", dd[0], dd[1], dd[2], TBRM_SURFACE_MAX_DIM);
    const BoxVerdict b = box_resolve(dims, d->origin, d->extent, true, &box, &bricks);
    if (b.what != BOX_OK) return fail_box(b, true, dims, d->origin, d->extent);
    return TBRM_OK;
}

// the call, with device outputs; staged: the outputs are the handle's staging, taken once the counts are known
int surface_call(tbrm_resources* r, const tbrm_surface_desc* d, void* d_vertices, void* d_indices, void* d_positions, bool staged, bool want_positions, tbrm_surface_result* out)
{
    VoxelBox box{};
    BrickRange bricks{};
    if (int e = surface_arguments(r, d, box, bricks)) return e;
    const tbrm_resources::Dims dims = r->data_dims();
    const int dd[3] = {dims[0], dims[1], dims[2]};
    const BrickRange blocks = surface_blocks(box);
    const uint64_t n_blocks = range_bricks(blocks);
    if (n_blocks >= (1ull << 29)) return fail(TBRM_ERR_UNSUPPORTED, "a box of %llu blocks of cells: at most 2^29", (unsigned long long) n_blocks);
    const bool measure = (d->flags & SURFACE_MEASURE) != 0, triangles = (d->flags & SURFACE_TRIANGLES) != 0;

    if (int e = ensure_grow_scratch(r)) return e;
    if (int e = ensure_surface_buffer(r, 0, surface_scratch(nullptr, (size_t) n_blocks).bytes)) return e;
    const GrowScratch g = grow_scratch(r);
    const SurfaceScratch m = surface_scratch(r->d_surface[0], (size_t) n_blocks);

    MorphParams lp{}; // k_morph_load: the label bytes of the box's bricks -> board 0 and its class
    lp.labels = r->d_labels;
    lp.bnx = r->dbn[0];
    lp.bnxy = r->dbn[0] * r->dbn[1];
    for (int c = 0; c < 3; ++c) lp.dims[c] = dd[c];
    lp.box = box;
    lp.range = bricks;
    lp.wrange = bricks;
    for (int w = 0; w < 8; ++w) lp.source[w] = d->source[w];
    lp.bits = g.bits;
    lp.cls[0] = g.act[0];
    lp.cls[1] = g.act[1];
    lp.ctl = g.ctl;

    SurfaceParams p{};
    p.bnx = lp.bnx;
    p.bnxy = lp.bnxy;
    p.box = box;
    p.bricks = bricks;
    p.blocks = blocks;
    p.n_blocks = (uint32_t) n_blocks;
    p.skip = tune(TUNE_SURFACE_SKIP) != 0;
    p.triangles = triangles;
    p.bits = g.bits;
    p.cls = g.act[0];
    p.active = m.active;
    p.prefix = m.prefix;
    for (int w = 0; w < 2; ++w) { p.count[w] = m.count[w]; p.base[w] = m.base[w]; p.tile_sum[w] = m.tile_sum[w]; p.tile_base[w] = m.tile_base[w]; }
    p.ctl = m.ctl;
    for (int c = 0; c < 3; ++c) { p.scale[c] = d->scale[c]; p.offset[c] = d->offset[c]; }

    int32_t ctl[SURF_CTL_WORDS];
    ctl_start(ctl, SURF_CTL_WORDS, SURF_MIN_X, dd);
    for (int c = 0; c < 3; ++c) ctl[SURF_MIN_X + c] = dd[c] + 1; // (of HIGH corners, which reach dims)
    HIP_TRY(hipMemcpyAsync(p.ctl, ctl, sizeof(ctl), hipMemcpyHostToDevice, r->stream));
    HIP_TRY(launch_morph_load(lp, r->stream));
    HIP_TRY(launch_surface_count(p, r->stream));
    HIP_TRY(launch_surface_scan(p, r->stream));
    HIP_TRY(hipMemcpyAsync(ctl, p.ctl, sizeof(ctl), hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));

    uint64_t counts[SURF_CTL_COUNTS];
    memcpy(counts, ctl, sizeof(counts));
    memset(out, 0, sizeof(*out));
    out->set_voxels = counts[SURF_SET_VOXELS];
    out->vertices = counts[SURF_VERTICES];
    out->quads = counts[SURF_QUADS];
    for (int c = 0; c < 3; ++c) {
        out->quads_axis[c] = counts[SURF_QUADS_X + c];
        const bool none = ctl[SURF_MAX_X + c] < 0;
        out->cell_min[c] = none ? dd[c] : ctl[SURF_MIN_X + c] - 1; // the low corner of the cell with the high corner h is h - 1
        out->cell_max[c] = none ? -1 : ctl[SURF_MAX_X + c] - 1;
    }
    out->blocks_evaluated = (int32_t) counts[SURF_EVALUATED];
    out->blocks_skipped = (int32_t) counts[SURF_SKIPPED];
    out->launches = kSurfaceLaunchesCount;
    ++r->surface_counters[0];
    r->surface_counters[3] += counts[SURF_EVALUATED];

    if (out->vertices >= (1ull << 32)) return fail(TBRM_ERR_UNSUPPORTED, "%llu vertices: an index has 32 bits", (unsigned long long) out->vertices);
    if (measure) return TBRM_OK;
    const uint64_t v_room = d_vertices ? d->vertex_capacity : 0ull, q_room = d_indices ? d->quad_capacity : 0ull; // (a null output holds nothing)
    if (out->vertices > v_room) return fail(TBRM_ERR_INVALID_ARG, "vertex_capacity %llu: the surface has %llu vertices (and %llu quads)", (unsigned long long) v_room, (unsigned long long) out->vertices, (unsigned long long) out->quads);
    if (out->quads > q_room) return fail(TBRM_ERR_INVALID_ARG, "quad_capacity %llu: the surface has %llu quads (and %llu vertices)", (unsigned long long) q_room, (unsigned long long) out->quads, (unsigned long long) out->vertices);
    if (out->vertices == 0) return TBRM_OK; // nothing to write

    p.vertices = (uint32_t*) d_vertices;
    p.indices = (uint32_t*) d_indices;
    p.positions = (float*) d_positions;
    SurfaceStaging st{};
    if (staged) {
        if (int e = ensure_surface_buffer(r, 1, surface_staging(nullptr, out->vertices, out->quads, triangles, want_positions).bytes)) return e;
        st = surface_staging(r->d_surface[1], out->vertices, out->quads, triangles, want_positions);
        p.vertices = st.vertices;
        p.indices = st.indices;
        p.positions = st.positions;
    }
    HIP_TRY(launch_surface_emit(p, r->stream));
    if (staged) {
        HIP_TRY(hipMemcpyAsync(d_vertices, st.vertices, (size_t) out->vertices * sizeof(SurfaceVertex), hipMemcpyDeviceToHost, r->stream));
        HIP_TRY(hipMemcpyAsync(d_indices, st.indices, (size_t) out->quads * (triangles ? 6 : 4) * sizeof(uint32_t), hipMemcpyDeviceToHost, r->stream));
        if (want_positions) HIP_TRY(hipMemcpyAsync(d_positions, st.positions, (size_t) out->vertices * 3 * sizeof(float), hipMemcpyDeviceToHost, r->stream));
    }
    HIP_TRY(hipStreamSynchronize(r->stream));
    out->launches = kSurfaceLaunchesCount + 1;
    out->written = 1;
    r->surface_counters[1] += out->vertices;
    r->surface_counters[2] += out->quads;
    return TBRM_OK;
}

} // namespace

extern "C" {

int tbrm_surface_abi_version(void) { return TBRM_SURFACE_ABI_VERSION; }

int tbrm_host_surface_unit_cube(const int32_t dims[3], float scale[3], float offset[3])
{
    if (!dims || !scale || !offset) return fail(TBRM_ERR_INVALID_ARG, "null argument");
    for (int c = 0; c < 3; ++c)
        if (dims[c] < 1) return fail(TBRM_ERR_INVALID_ARG, "dims[%d] = %d: must be at least 1", c, (int) dims[c]);
    for (int c = 0; c < 3; ++c) {
        scale[c] = dims[c] > 1 ? (float) (1.0 / (double) (dims[c] - 1)) : 0.0f;
        offset[c] = 0.0f;
    }
    return TBRM_OK;
}

int tbrm_host_surface_positions(const tbrm_surface_vertex* vertices, size_t n, const float scale[3], const float offset[3], float* out_positions)
{
    if ((!vertices && n) || !scale || !offset || (!out_positions && n)) return fail(TBRM_ERR_INVALID_ARG, "null argument");
    for (int c = 0; c < 3; ++c)
        if (!std::isfinite(scale[c]) || !std::isfinite(offset[c])) return fail(TBRM_ERR_INVALID_ARG, "scale[%d] = %g, offset[%d] = %g: both must be finite", c, scale[c], c, offset[c]);
    for (size_t i = 0; i < n; ++i) {
        const tbrm_surface_vertex& v = vertices[i];
        if (v.edges < 1 || v.edges > 12) return fail(TBRM_ERR_INVALID_ARG, "vertex %zu: edges %d, must be 1 .. 12", i, (int) v.edges);
        for (int c = 0; c < 3; ++c)
            if (v.cell[c] < -1 || v.cell[c] >= TBRM_SURFACE_MAX_DIM) return fail(TBRM_ERR_INVALID_ARG, "vertex %zu: cell[%d] = %d, must be -1 .. %d", i, c, (int) v.cell[c], TBRM_SURFACE_MAX_DIM - 1);
    }
    for (size_t i = 0; i < n; ++i)
        for (int c = 0; c < 3; ++c) out_positions[3 * i + c] = surface_position(vertices[i].cell[c], vertices[i].sum[c], vertices[i].edges, scale[c], offset[c]);
    return TBRM_OK;
}

int tbrm_surface_counters(const tbrm_resources* r, uint64_t out[6])
{
    if (!r || !out) return fail(TBRM_ERR_INVALID_ARG, "null argument");
    for (int k = 0; k < 6; ++k) out[k] = r->surface_counters[k];
    out[4] = (uint64_t) (r->surface_bytes[0] + r->surface_bytes[1]);
    return TBRM_OK;
}

int tbrm_label_surface_device(tbrm_resources* r, const tbrm_surface_desc* d, void* d_vertices, void* d_indices, void* d_positions, tbrm_surface_result* out)
{
    if (!r || !d || !out) return fail(TBRM_ERR_INVALID_ARG, "null argument");
    if (int e = refuse_resident(r)) return e;
    return surface_call(r, d, d_vertices, d_indices, d_positions, false, d_positions != nullptr, out);
}

int tbrm_label_surface(tbrm_resources* r, const tbrm_surface_desc* d, tbrm_surface_vertex* vertices, uint32_t* indices, float* positions, tbrm_surface_result* out)
{
    if (!r || !d || !out) return fail(TBRM_ERR_INVALID_ARG, "null argument");
    if (int e = refuse_resident(r)) return e;
    return surface_call(r, d, vertices, indices, positions, true, positions != nullptr, out);
}

} // extern "C"
