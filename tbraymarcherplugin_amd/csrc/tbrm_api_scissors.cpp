// tbrm_api_scissors.cpp — view-space scissors (include/tbrm_scissors.h): validation, the mask's staging and the
// counters around the kernels of tbrm_scissors_kernels.hip, and the two host functions (tbrm_scissors_plan.h).
//
// Ahead of the frame's load (tbrm_board_edit.h): the mask into the handle's staging and its summary beside it.
// Between load and write: k_scissors board 0 -> board 1.
#include "tbrm_board_edit.h"
#include "tbrm_scissors_kernels.h"
#include "../../include/tbrm_scissors.h"

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

// what the call checks of a desc and a mask before the handle's state; the box
int scissors_arguments_of(const tbrm_resources* r, const tbrm_scissors_desc* d, const uint32_t* mask, size_t n_words, BoardEdit& edit)
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
    if (int e = label_codes(d->new_label, d->erase_label, d->reserved)) return e;
    return edit.begin(r, d->origin, d->extent, &edit.p.range);
}

// the staging, the frame's bind and the parameters of the call's own kernels
int scissors_params(tbrm_resources* r, const tbrm_scissors_desc* d, BoardEdit& edit, ScissorsScratch& m, ScissorsParams& q)
{
    MorphParams& p = edit.p;
    const tbrm_scissors_projection& j = d->projection;
    if (int e = edit.bind(r, d)) return e;
    p.wrange = p.range; // no reach: the bricks of the box
    if (int e = ensure_bytes(r, r->d_scissors, r->scissors_bytes, scissors_scratch(nullptr, j.width, j.height).bytes, "scissors mask staging")) return e;
    m = scissors_scratch(r->d_scissors, j.width, j.height);

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
    q.bits = p.bits;
    q.cls[0] = p.cls[0];
    q.cls[1] = p.cls[1];
    q.ctl = p.ctl;
    return TBRM_OK;
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

int tbrm_scissors_counters(const tbrm_resources* r, uint64_t out[4]) { return copy_counters(r, &tbrm_resources::scissors_counters, out); }

int tbrm_scissors_labels(tbrm_resources* r, const tbrm_scissors_desc* d, const uint32_t* mask_words, size_t n_words, tbrm_scissors_result* out)
{
    if (!r || !d || !mask_words || !out) return fail(TBRM_ERR_INVALID_ARG, "null argument");
    if (int e = refuse_resident(r)) return e;
    BoardEdit edit(SCISSORS_CTL_WORDS);
    ScissorsParams q{};
    ScissorsScratch m;
    if (int e = scissors_arguments_of(r, d, mask_words, n_words, edit)) return e;
    if (int e = scissors_params(r, d, edit, m, q)) return e;

    HIP_TRY(hipMemcpyAsync(m.mask, mask_words, n_words * sizeof(uint32_t), hipMemcpyHostToDevice, r->stream));
    int launches = 1;
    if (q.skip) {
        HIP_TRY(launch_scissors_summary(q, r->stream));
        launches += kScissorsSummaryLaunches;
    }
    if (int e = edit.load(r)) return e;
    HIP_TRY(launch_scissors(q, r->stream));
    if (int e = edit.write(r, 1)) return e; // the board k_scissors wrote (the wait also: the caller's mask has been read)

    memset(out, 0, sizeof(*out));
    edit.result(out);
    out->bricks_inside = (int32_t) edit.count(SCISSORS_CTL_INSIDE);
    out->bricks_outside = (int32_t) edit.count(SCISSORS_CTL_OUTSIDE);
    out->bricks_projected = (int32_t) edit.count(MORPH_WINDOWS);
    out->launches = launches;
    return edit.end(r, r->scissors_counters, launches);
}

} // extern "C"
