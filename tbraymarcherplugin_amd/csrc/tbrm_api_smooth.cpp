// tbrm_api_smooth.cpp — smoothing of labels (include/tbrm_smooth.h): validation, the plan (tbrm_smooth_plan.h) and
// the counters around the kernel of tbrm_smooth_kernels.hip.
//
// A call is: the source set of the planned bricks from the label bytes into board 0 (k_morph_load, as it stands), `iterations` passes
// board -> board (k_smooth_count), the comparison of the final board with the label bytes inside the box (k_morph_write, as it
// stands) and behind a write what every label write ends with (labels_changed). The boards, their classes and the
// control words are the scratch of region growing; a call takes no other.
#include "tbrm_resources.h"
#include "tbrm_smooth_kernels.h"
#include "tbrm_smooth_plan.h"
#include "../../include/tbrm_smooth.h"

#include <cstring>

using namespace tbrm;
using namespace tbrm_host;

static_assert(TBRM_SMOOTH_MAX_RADIUS == kSmoothMaxRadius && TBRM_SMOOTH_MAX_ITERATIONS == kSmoothMaxIterations && TBRM_SMOOTH_MAX_REACH == kSmoothMaxReach &&
              TBRM_SMOOTH_MAX_RANK_DEN == kSmoothMaxRankDen, "tbrm_smooth_plan.h restates the header's constants");
static_assert(kSmoothMaxRadius <= kRowWordShift, "a row word holds 16 bits either side of the brick's byte");

namespace {

// what the call checks of a desc before the handle's state; the box and the plan
int smooth_arguments_of(const tbrm_resources* r, const tbrm_smooth_desc* d, MorphParams& p, SmoothPlan& plan)
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
    if (d->new_label < -1 || d->new_label > 255) return fail(TBRM_ERR_INVALID_ARG, "new_label %d: must be 0 .. 255, or -1 to measure only", (int) d->new_label);
    if (d->erase_label < 0 || d->erase_label > 255) return fail(TBRM_ERR_INVALID_ARG, "erase_label %d: must be 0 .. 255", (int) d->erase_label);
    if (d->reserved != 0) return fail(TBRM_ERR_INVALID_ARG, "reserved = %d: must be 0", (int) d->reserved);
    const tbrm_resources::Dims dims = r->data_dims();
    const BoxVerdict v = box_resolve(dims, d->origin, d->extent, true, &p.box, nullptr);
    if (v.what != BOX_OK) return fail_box(v, true, dims, d->origin, d->extent);
    for (int c = 0; c < 3; ++c) p.dims[c] = dims[c];
    if (int e = begin_label_edit(r, "no label volume")) return e;
    if (!smooth_plan(p.dims, p.box.origin, p.box.end, d->radius, d->iterations, &plan)) return fail(TBRM_ERR_INVALID_ARG, "no plan for these arguments");
    return TBRM_OK;
}

// the parameters of the morphology kernels this call borrows (k_morph_load, k_morph_write) and of its own
void smooth_params(const tbrm_resources* r, const tbrm_smooth_desc* d, const SmoothPlan& plan, const GrowScratch& g, MorphParams& p, SmoothParams& q)
{
    p.labels = r->d_labels;
    p.bnx = r->dbn[0];
    p.bnxy = r->dbn[0] * r->dbn[1];
    for (int c = 0; c < 3; ++c) { p.range.b0[c] = plan.b0[c]; p.range.nb[c] = plan.nb[c]; p.wrange.b0[c] = plan.wb0[c]; p.wrange.nb[c] = plan.wnb[c]; }
    for (int w = 0; w < 8; ++w) { p.source[w] = d->source[w]; p.writable[w] = d->writable[w]; }
    p.bits = g.bits;
    p.cls[0] = g.act[0];
    p.cls[1] = g.act[1];
    p.new_label = d->new_label;
    p.erase_label = d->erase_label;
    p.ctl = g.ctl;

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
    q.bits = g.bits;
    q.cls[0] = g.act[0];
    q.cls[1] = g.act[1];
    q.skip = tune(TUNE_SMOOTH_SKIP) != 0;
    q.ctl = g.ctl;
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

int tbrm_smooth_counters(const tbrm_resources* r, uint64_t out[4])
{
    if (!r || !out) return fail(TBRM_ERR_INVALID_ARG, "null argument");
    for (int k = 0; k < 4; ++k) out[k] = r->smooth_counters[k];
    return TBRM_OK;
}

int tbrm_smooth_labels(tbrm_resources* r, const tbrm_smooth_desc* d, tbrm_smooth_result* out)
{
    if (!r || !d || !out) return fail(TBRM_ERR_INVALID_ARG, "null argument");
    if (int e = refuse_resident(r)) return e;
    MorphParams p{};
    SmoothParams q{};
    SmoothPlan plan;
    if (int e = smooth_arguments_of(r, d, p, plan)) return e;
    if (int e = ensure_grow_scratch(r)) return e;
    smooth_params(r, d, plan, grow_scratch(r), p, q);

    int32_t ctl[MORPH_CTL_WORDS];
    ctl_start(ctl, MORPH_CTL_WORDS, MORPH_MIN_X, p.dims);
    HIP_TRY(hipMemcpyAsync(p.ctl, ctl, sizeof(ctl), hipMemcpyHostToDevice, r->stream));
    HIP_TRY(launch_morph_load(p, r->stream));
    for (int i = 0; i < plan.passes; ++i) {
        q.from = i & 1;
        HIP_TRY(launch_smooth_count(q, r->stream));
    }
    p.from = plan.passes & 1; // the board the last pass wrote
    HIP_TRY(launch_morph_write(p, r->stream));
    HIP_TRY(hipMemcpyAsync(ctl, p.ctl, sizeof(ctl), hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));

    uint64_t counts[MORPH_CTL_COUNTS];
    memcpy(counts, ctl, sizeof(counts));
    memset(out, 0, sizeof(*out));
    out->source_voxels = counts[MORPH_SOURCE];
    out->result_voxels = counts[MORPH_RESULT];
    out->added = counts[MORPH_ADDED];
    out->removed = counts[MORPH_REMOVED];
    out->relabelled = counts[MORPH_RELABELLED];
    for (int c = 0; c < 3; ++c) { out->bbox_min[c] = ctl[MORPH_MIN_X + c]; out->bbox_max[c] = ctl[MORPH_MAX_X + c]; out->reach[c] = plan.reach[c]; }
    out->launches = plan.passes * kSmoothLaunchesPerPass;
    ++r->smooth_counters[0];
    r->smooth_counters[1] += (uint64_t) out->launches;
    r->smooth_counters[2] += counts[MORPH_WINDOWS];
    r->smooth_counters[3] += counts[MORPH_BRICKS_WRITTEN];

    if (d->new_label >= 0) return labels_changed(r, out->bbox_min, out->bbox_max); // (nothing joined or left: nothing to do)
    return TBRM_OK;
}

} // extern "C"
