// tbrm_api_smooth.cpp — smoothing of labels (include/tbrm_smooth.h): validation, the plan (tbrm_smooth_plan.h) and
// the counters around the kernel of tbrm_smooth_kernels.hip.
//
// Between the frame's load and write (tbrm_board_edit.h): `iterations` passes board -> board (k_smooth_count). A call
// takes no scratch beyond region growing's.
#include "tbrm_board_edit.h"
#include "tbrm_smooth_kernels.h"
#include "tbrm_smooth_plan.h"
#include "../../include/tbrm_smooth.h"

using namespace tbrm;
using namespace tbrm_host;

static_assert(TBRM_SMOOTH_MAX_RADIUS == kSmoothMaxRadius && TBRM_SMOOTH_MAX_ITERATIONS == kSmoothMaxIterations && TBRM_SMOOTH_MAX_REACH == kSmoothMaxReach &&
              TBRM_SMOOTH_MAX_RANK_DEN == kSmoothMaxRankDen, "tbrm_smooth_plan.h restates the header's constants");
static_assert(kSmoothMaxRadius <= kRowWordShift, "a row word holds 16 bits either side of the brick's byte");

namespace {

// what the call checks of a desc before the handle's state; the box and the plan
int smooth_arguments_of(const tbrm_resources* r, const tbrm_smooth_desc* d, BoardEdit& edit, SmoothPlan& plan)
{
    int axis = 0;
    switch (smooth_arguments(d->radius, d->rank_num, d->rank_den, d->iterations, &axis)) {
    case SMOOTH_OK: break;
    case SMOOTH_RADIUS: return fail(TBRM_ERR_INVALID_ARG, "radius[%d] = %d: must be 0 .. %d", axis, (int) d->radius[axis], TBRM_SMOOTH_MAX_RADIUS);
    case SMOOTH_NO_RADIUS: return fail(TBRM_ERR_INVALID_ARG, "radius (0, 0, 0): one radius must be at least 1");
    case SMOOTH_ITERATIONS: return fail(TBRM_ERR_INVALID_ARG, "iterations %d: must be 1 .. %d", (int) d->iterations, TBRM_SMOOTH_MAX_ITERATIONS);
    case SMOOTH_REACH: return fail(TBRM_ERR_INVALID_ARG, "iterations %d with radius[%d] = %d: iterations * radius must be at most %d", (int) d->iterations, axis, (int) d->radius[axis], TBRM_SMOOTH_MAX_REACH);
    case SMOOTH_RANK_DEN: return fail(TBRM_ERR_INVALID_ARG, "rank_den %d: must be 1 .. %d", (int) d->rank_den, TBRM_SMOOTH_MAX_RANK_DEN);
    case SMOOTH_RANK_NUM: return fail(TBRM_ERR_INVALID_ARG, "rank_num %d: must be 0 .. rank_den - 1 = %d", (int) d->rank_num, (int) d->rank_den - 1);
    }
    if (int e = label_codes(d->new_label, d->erase_label, d->reserved)) return e;
    if (int e = edit.begin(r, d->origin, d->extent)) return e;
    const MorphParams& p = edit.p;
    if (!smooth_plan(p.dims, p.box.origin, p.box.end, d->radius, d->iterations, &plan)) return fail(TBRM_ERR_INVALID_ARG, "no plan for these arguments");
    return TBRM_OK;
}

// the frame's bind, the plan's ranges and the parameters of the call's own kernel
int smooth_params(tbrm_resources* r, const tbrm_smooth_desc* d, const SmoothPlan& plan, BoardEdit& edit, SmoothParams& q)
{
    MorphParams& p = edit.p;
    if (int e = edit.bind(r, d)) return e;
    edit.ranges(plan);

    q.bnx = p.bnx;
    q.bnxy = p.bnxy;
    q.range = p.range;
    for (int c = 0; c < 3; ++c) {
        q.dims[c] = p.dims[c];
        q.radius[c] = plan.radius[c];
        q.kb[c] = (plan.radius[c] + kBrick - 1) / kBrick;
    }
    q.rank_num = (uint32_t) d->rank_num;
    q.rank_den = (uint32_t) d->rank_den;
    q.bits = p.bits;
    q.cls[0] = p.cls[0];
    q.cls[1] = p.cls[1];
    q.skip = tune(TUNE_SMOOTH_SKIP) != 0;
    q.ctl = p.ctl;
    return TBRM_OK;
}

} // namespace

extern "C" {

int tbrm_smooth_abi_version(void) { return TBRM_SMOOTH_ABI_VERSION; }

int tbrm_host_smooth_radii(const double spacing[3], double radius, int32_t radii[3])
{
    if (!spacing || !radii) return fail(TBRM_ERR_INVALID_ARG, "null argument");
    if (!smooth_radii(spacing, radius, radii))
        return fail(TBRM_ERR_INVALID_ARG, "spacing (%g, %g, %g), radius %g: must be finite and > 0, and give radii of at most %d voxels, one of them at least 1",
                    spacing[0], spacing[1], spacing[2], radius, TBRM_SMOOTH_MAX_RADIUS);
    return TBRM_OK;
}

int tbrm_smooth_counters(const tbrm_resources* r, uint64_t out[4]) { return copy_counters(r, &tbrm_resources::smooth_counters, out); }

int tbrm_smooth_labels(tbrm_resources* r, const tbrm_smooth_desc* d, tbrm_smooth_result* out)
{
    if (!r || !d || !out) return fail(TBRM_ERR_INVALID_ARG, "null argument");
    if (int e = refuse_resident(r)) return e;
    BoardEdit edit(MORPH_CTL_WORDS);
    SmoothParams q{};
    SmoothPlan plan;
    if (int e = smooth_arguments_of(r, d, edit, plan)) return e;
    if (int e = smooth_params(r, d, plan, edit, q)) return e;

    if (int e = edit.load(r)) return e;
    for (int i = 0; i < plan.passes; ++i) {
        q.from = i & 1;
        HIP_TRY(launch_smooth_count(q, r->stream));
    }
    if (int e = edit.write(r, plan.passes & 1)) return e; // the board the last pass wrote

    memset(out, 0, sizeof(*out));
    edit.result(out);
    for (int c = 0; c < 3; ++c) out->reach[c] = plan.reach[c];
    out->launches = plan.passes * kSmoothLaunchesPerPass;
    return edit.end(r, r->smooth_counters, out->launches);
}

} // extern "C"
