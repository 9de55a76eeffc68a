// tbrm_api_scissors.cpp — view-space scissors (include/tbrm_scissors.h): validation, the mask's staging and the
// counters around the kernels of tbrm_scissors_kernels.hip, and the two host functions (tbrm_scissors_plan.h).
//
// A call is: the mask into the handle's staging and its summary beside it, the source set of the box's bricks from the label bytes
// into board 0 (k_morph_load, as it stands), k_scissors board 0 -> board 1, the comparison of board 1 with the label bytes inside the
// box (k_morph_write, as it stands) and behind a write what every label write ends with (labels_changed). The boards,
// their classes and the control words are the scratch of region growing.
#include "tbrm_resources.h"
#include "tbrm_scissors_kernels.h"
#include "../../include/tbrm_scissors.h"

#include <cstring>

using namespace tbrm;
using namespace tbrm_host;

static_assert(TBRM_SCISSORS_MAX_IMAGE == kScissorsMaxImage && TBRM_SCISSORS_COORD_BITS == kScissorsCoordBits, "tbrm_scissors_plan.h restates the header's constants");
static_assert(TBRM_SCISSORS_ERASE_INSIDE == SCISSORS_ERASE_INSIDE && TBRM_SCISSORS_ERASE_OUTSIDE == SCISSORS_ERASE_OUTSIDE && TBRM_SCISSORS_FILL_INSIDE == SCISSORS_FILL_INSIDE &&
              TBRM_SCISSORS_FILL_OUTSIDE == SCISSORS_FILL_OUTSIDE, "tbrm_scissors_plan.h restates the header's operators");

namespace {

// d_scissors: [the mask's words][the summary's entries], each part 256-byte aligned
struct ScissorsScratch {
    uint32_t* mask;
    ScissorsCell* summary;
    size_t bytes;
};
ScissorsScratch scissors_scratch(char* base, int width, int height)
{
    Carver c{base};
    ScissorsScratch s{};
    s.mask = c.take<uint32_t>(scissors_mask_words(width, height));
    s.summary = c.take<ScissorsCell>(scissors_summary_entries(width, height));
    s.bytes = c.off;
    return s;
}

// only ever grown: a call with a mask no larger than one before it allocates nothing
int ensure_scissors_scratch(tbrm_resources* r, int width, int height)
{
    const size_t bytes = scissors_scratch(nullptr, width, height).bytes;
    if (r->scissors_bytes >= bytes) return TBRM_OK;
    HIP_TRY(hipStreamSynchronize(r->stream));
    (void) hipFree(r->d_scissors);
    r->d_scissors = nullptr;
    r->scissors_bytes = 0;
    count_alloc(r, 1, "scissors mask staging");
    HIP_TRY(hipMalloc((void**) &r->d_scissors, bytes));
    r->scissors_bytes = bytes;
    return TBRM_OK;
}

// what the call checks of a desc and a mask before the handle's state; the box
int scissors_arguments_of(const tbrm_resources* r, const tbrm_scissors_desc* d, const uint32_t* mask, size_t n_words, MorphParams& p)
{
    const tbrm_resources::Dims dims = r->data_dims();
    const int dd[3] = {dims[0], dims[1], dims[2]};
    const tbrm_scissors_projection& j = d->projection;
    const long long limit = 1ll << TBRM_SCISSORS_COORD_BITS;
    const char* row = nullptr;
    switch (scissors_arguments(j, d->op, dd)) {
    case SCISSORS_OK: break;
    case SCISSORS_WIDTH: return fail(TBRM_ERR_INVALID_ARG, "width %d: must be 1 .. %d", (int) j.width, TBRM_SCISSORS_MAX_IMAGE);
    case SCISSORS_HEIGHT: return fail(TBRM_ERR_INVALID_ARG, "height %d: must be 1 .. %d", (int) j.height, TBRM_SCISSORS_MAX_IMAGE);
    case SCISSORS_U: row = "u"; break;
    case SCISSORS_V: row = "v"; break;
    case SCISSORS_W: row = "w"; break;
    case SCISSORS_W_MIN: return fail(TBRM_ERR_INVALID_ARG, "w_min %lld: must be at least 1", (long long) j.w_min);
    case SCISSORS_W_MAX: return fail(TBRM_ERR_INVALID_ARG, "w_max %lld: must be at least w_min = %lld", (long long) j.w_max, (long long) j.w_min);
    case SCISSORS_OP: return fail(TBRM_ERR_INVALID_ARG, "op %d: must be 0 .. %d", (int) d->op, kScissorsOps - 1);
    }
    if (row)
        return fail(TBRM_ERR_INVALID_ARG, "row %s: |r0| (dim_x - 1) + |r1| (dim_y - 1) + |r2| (dim_z - 1) + |r3| must be below 2^%d = %lld in a volume of %d x %d x %d",
                    row, TBRM_SCISSORS_COORD_BITS, limit, dd[0], dd[1], dd[2]);
    if (n_words != scissors_mask_words(j.width, j.height))
        return fail(TBRM_ERR_INVALID_ARG, "n_words %zu: a mask of width %d and height %d has %zu words", n_words, (int) j.width, (int) j.height, scissors_mask_words(j.width, j.height));
    const int stray = scissors_mask_stray_row(mask, j.width, j.height);
    if (stray >= 0) return fail(TBRM_ERR_INVALID_ARG, "mask_words: row %d has a bit at or beyond width %d", stray, (int) j.width);
    if (d->new_label < -1 || d->new_label > 255) return fail(TBRM_ERR_INVALID_ARG, "new_label %d: must be 0 .. 255, or -1 to measure only", (int) d->new_label);
    if (d->erase_label < 0 || d->erase_label > 255) return fail(TBRM_ERR_INVALID_ARG, "erase_label %d: must be 0 .. 255", (int) d->erase_label);
    if (d->reserved != 0) return fail(TBRM_ERR_INVALID_ARG, "reserved = %d: must be 0", (int) d->reserved);
    const BoxVerdict v = box_resolve(dims, d->origin, d->extent, true, &p.box, &p.range);
    if (v.what != BOX_OK) return fail_box(v, true, dims, d->origin, d->extent);
    for (int c = 0; c < 3; ++c) p.dims[c] = dims[c];
    return begin_label_edit(r, "no label volume");
}

// the parameters of the morphology kernels this call borrows (k_morph_load, k_morph_write) and of its own
void scissors_params(const tbrm_resources* r, const tbrm_scissors_desc* d, const GrowScratch& g, const ScissorsScratch& m, MorphParams& p, ScissorsParams& q)
{
    p.labels = r->d_labels;
    p.bnx = r->dbn[0];
    p.bnxy = r->dbn[0] * r->dbn[1];
    p.wrange = p.range; // no reach: the bricks of the box
    for (int w = 0; w < 8; ++w) { p.source[w] = d->source[w]; p.writable[w] = d->writable[w]; }
    p.bits = g.bits;
    p.cls[0] = g.act[0];
    p.cls[1] = g.act[1];
    p.new_label = d->new_label;
    p.erase_label = d->erase_label;
    p.ctl = g.ctl;

    const tbrm_scissors_projection& j = d->projection;
    q.bnx = p.bnx;
    q.bnxy = p.bnxy;
    q.range = p.range;
    for (int c = 0; c < 3; ++c) q.dims[c] = p.dims[c];
    for (int c = 0; c < 4; ++c) { q.rows.u[c] = j.u[c]; q.rows.v[c] = j.v[c]; q.rows.w[c] = j.w[c]; }
    q.rows.w_min = j.w_min;
    q.rows.w_max = j.w_max;
    q.rows.width = j.width;
    q.rows.height = j.height;
    q.op = d->op;
    q.skip = tune(TUNE_SCISSORS_SKIP) != 0;
    q.mask = m.mask;
    q.row_words = (int) scissors_row_words(j.width);
    q.summary = q.skip ? m.summary : nullptr;
    q.cells_x = scissors_cells_x(j.width);
    q.cells_y = scissors_cells_y(j.height);
    q.bits = g.bits;
    q.cls[0] = g.act[0];
    q.cls[1] = g.act[1];
    q.ctl = g.ctl;
}

} // namespace

extern "C" {

int tbrm_scissors_abi_version(void) { return TBRM_SCISSORS_ABI_VERSION; }

int tbrm_host_scissors_projection(const int32_t dims[3], const tbrm_world_params* world, const tbrm_camera* camera, double depth_min, double depth_max,
                                  tbrm_scissors_projection* out)
{
    if (!dims || !world || !camera || !out) return fail(TBRM_ERR_INVALID_ARG, "null argument");
    switch (scissors_projection(dims, world->volume_transform, *camera, depth_min, depth_max, out)) {
    case SCISSORS_PROJ_OK: return TBRM_OK;
    case SCISSORS_PROJ_DIMS: return fail(TBRM_ERR_INVALID_ARG, "dims (%d, %d, %d): must be at least 1", (int) dims[0], (int) dims[1], (int) dims[2]);
    case SCISSORS_PROJ_IMAGE: return fail(TBRM_ERR_INVALID_ARG, "camera width %d, height %d: must be 1 .. %d", (int) camera->width, (int) camera->height, TBRM_SCISSORS_MAX_IMAGE);
    case SCISSORS_PROJ_NOT_FINITE: return fail(TBRM_ERR_INVALID_ARG, "camera or volume_transform: every value must be finite");
    case SCISSORS_PROJ_TANGENT: return fail(TBRM_ERR_INVALID_ARG, "tan_half_fov (%g, %g): must be > 0", camera->tan_half_fov_x, camera->tan_half_fov_y);
    case SCISSORS_PROJ_DEPTH: return fail(TBRM_ERR_INVALID_ARG, "depth_min %g, depth_max %g: depth_max must be at least depth_min, and the range must hold a W of at least 1 at the rows' scale", depth_min, depth_max);
    default: return fail(TBRM_ERR_INVALID_ARG, "degenerate scale: the rows are all zero or no power of two brings them under 2^%d", TBRM_SCISSORS_COORD_BITS);
    }
}

int tbrm_host_scissors_polygon(const double* xy, size_t n_points, int32_t width, int32_t height, uint32_t* mask_words, size_t n_words)
{
    if (!xy || !mask_words) return fail(TBRM_ERR_INVALID_ARG, "null argument");
    if (n_points < 3) return fail(TBRM_ERR_INVALID_ARG, "n_points %zu: a polygon has at least 3", n_points);
    if (width < 1 || width > TBRM_SCISSORS_MAX_IMAGE) return fail(TBRM_ERR_INVALID_ARG, "width %d: must be 1 .. %d", (int) width, TBRM_SCISSORS_MAX_IMAGE);
    if (height < 1 || height > TBRM_SCISSORS_MAX_IMAGE) return fail(TBRM_ERR_INVALID_ARG, "height %d: must be 1 .. %d", (int) height, TBRM_SCISSORS_MAX_IMAGE);
    if (n_words != scissors_mask_words(width, height))
        return fail(TBRM_ERR_INVALID_ARG, "n_words %zu: a mask of width %d and height %d has %zu words", n_words, (int) width, (int) height, scissors_mask_words(width, height));
    if (!scissors_polygon(xy, n_points, width, height, mask_words)) return fail(TBRM_ERR_INVALID_ARG, "xy: every coordinate must be finite");
    return TBRM_OK;
}

int tbrm_scissors_counters(const tbrm_resources* r, uint64_t out[4])
{
    if (!r || !out) return fail(TBRM_ERR_INVALID_ARG, "null argument");
    for (int k = 0; k < 4; ++k) out[k] = r->scissors_counters[k];
    return TBRM_OK;
}

int tbrm_scissors_labels(tbrm_resources* r, const tbrm_scissors_desc* d, const uint32_t* mask_words, size_t n_words, tbrm_scissors_result* out)
{
    if (!r || !d || !mask_words || !out) return fail(TBRM_ERR_INVALID_ARG, "null argument");
    if (int e = refuse_resident(r)) return e;
    MorphParams p{};
    ScissorsParams q{};
    if (int e = scissors_arguments_of(r, d, mask_words, n_words, p)) return e;
    if (int e = ensure_grow_scratch(r)) return e;
    const tbrm_scissors_projection& j = d->projection;
    if (int e = ensure_scissors_scratch(r, j.width, j.height)) return e;
    const ScissorsScratch m = scissors_scratch(r->d_scissors, j.width, j.height);
    scissors_params(r, d, grow_scratch(r), m, p, q);

    int32_t ctl[SCISSORS_CTL_WORDS];
    ctl_start(ctl, SCISSORS_CTL_WORDS, MORPH_MIN_X, p.dims);
    HIP_TRY(hipMemcpyAsync(p.ctl, ctl, sizeof(ctl), hipMemcpyHostToDevice, r->stream));
    HIP_TRY(hipMemcpyAsync(m.mask, mask_words, n_words * sizeof(uint32_t), hipMemcpyHostToDevice, r->stream));
    int launches = 1;
    if (q.skip) {
        HIP_TRY(launch_scissors_summary(q, r->stream));
        launches += kScissorsSummaryLaunches;
    }
    HIP_TRY(launch_morph_load(p, r->stream));
    HIP_TRY(launch_scissors(q, r->stream));
    p.from = 1; // the board k_scissors wrote
    HIP_TRY(launch_morph_write(p, r->stream));
    HIP_TRY(hipMemcpyAsync(ctl, p.ctl, sizeof(ctl), hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream)); // (also: the caller's mask has been read)

    uint64_t counts[SCISSORS_CTL_WORDS / 2];
    memcpy(counts, ctl, sizeof(counts));
    memset(out, 0, sizeof(*out));
    out->source_voxels = counts[MORPH_SOURCE];
    out->result_voxels = counts[MORPH_RESULT];
    out->added = counts[MORPH_ADDED];
    out->removed = counts[MORPH_REMOVED];
    out->relabelled = counts[MORPH_RELABELLED];
    for (int c = 0; c < 3; ++c) { out->bbox_min[c] = ctl[MORPH_MIN_X + c]; out->bbox_max[c] = ctl[MORPH_MAX_X + c]; }
    out->bricks_inside = (int32_t) counts[SCISSORS_CTL_INSIDE];
    out->bricks_outside = (int32_t) counts[SCISSORS_CTL_OUTSIDE];
    out->bricks_projected = (int32_t) counts[MORPH_WINDOWS];
    out->launches = launches;
    ++r->scissors_counters[0];
    r->scissors_counters[1] += (uint64_t) launches;
    r->scissors_counters[2] += counts[MORPH_WINDOWS];
    r->scissors_counters[3] += counts[MORPH_BRICKS_WRITTEN];

    if (d->new_label >= 0) return labels_changed(r, out->bbox_min, out->bbox_max); // (nothing joined or left: nothing to do)
    return TBRM_OK;
}

} // extern "C"
