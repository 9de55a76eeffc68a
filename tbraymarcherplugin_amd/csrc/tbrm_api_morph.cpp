// tbrm_api_morph.cpp — binary morphology of the label volume (include/tbrm_morphology.h): validation, the step plan
// (tbrm_morph_plan.h) and the counters around the kernels of tbrm_morph_kernels.hip.
//
// A call is: the source set of the planned bricks from the label bytes into board 0 (k_morph_load), the plan's step launches
// ping-ponging between the two boards (k_morph_steps, up to morph_steps unit steps each), the comparison of the final board with the
// label bytes inside the box (k_morph_write: counts, bounding box and — a writing call — the bytes), and behind a write what every
// label write ends with (labels_changed). It works in the
// scratch of region growing; nothing on the data side is touched, nothing waits for the occlusion stream.
#include "tbrm_resources.h"
#include "tbrm_morph_plan.h"
#include "../../include/tbrm_morphology.h"

#include <cstring>

using namespace tbrm;
using namespace tbrm_host;

static_assert(TBRM_MORPH_MAX_RADIUS == kMorphMaxRadius && TBRM_MORPH_DILATE == MORPH_DILATE && TBRM_MORPH_ERODE == MORPH_ERODE &&
              TBRM_MORPH_OPEN == MORPH_OPEN && TBRM_MORPH_CLOSE == MORPH_CLOSE, "tbrm_morph_plan.h restates the header's constants");

extern "C" {

int tbrm_morph_abi_version(void) { return TBRM_MORPH_ABI_VERSION; }

int tbrm_morph_counters(const tbrm_resources* r, uint64_t out[4])
{
    if (!r || !out) return fail(TBRM_ERR_INVALID_ARG, "null argument");
    for (int k = 0; k < 4; ++k) out[k] = r->morph_counters[k];
    return TBRM_OK;
}

int tbrm_morph_labels(tbrm_resources* r, const tbrm_morph_desc* d, tbrm_morph_result* out)
{
    if (!r || !d || !out) return fail(TBRM_ERR_INVALID_ARG, "null argument");
    if (int e = refuse_resident(r)) return e;
    if (d->op < TBRM_MORPH_DILATE || d->op > TBRM_MORPH_CLOSE) return fail(TBRM_ERR_INVALID_ARG, "op %d: must be TBRM_MORPH_DILATE .. TBRM_MORPH_CLOSE", (int) d->op);
    if (d->radius < 1 || d->radius > TBRM_MORPH_MAX_RADIUS) return fail(TBRM_ERR_INVALID_ARG, "radius %d: must be 1 .. %d", (int) d->radius, TBRM_MORPH_MAX_RADIUS);
    if (d->connectivity != 6 && d->connectivity != 26) return fail(TBRM_ERR_INVALID_ARG, "connectivity %d: must be 6 or 26", (int) d->connectivity);
    if (d->new_label < -1 || d->new_label > 255) return fail(TBRM_ERR_INVALID_ARG, "new_label %d: must be 0 .. 255, or -1 to measure only", (int) d->new_label);
    if (d->erase_label < 0 || d->erase_label > 255) return fail(TBRM_ERR_INVALID_ARG, "erase_label %d: must be 0 .. 255", (int) d->erase_label);
    if (d->reserved != 0) return fail(TBRM_ERR_INVALID_ARG, "reserved = %d: must be 0", (int) d->reserved);
    const tbrm_resources::Dims dims = r->data_dims();
    MorphParams p{};
    const BoxVerdict v = box_resolve(dims, d->origin, d->extent, true, &p.box, nullptr);
    if (v.what != BOX_OK) return fail_box(v, true, dims, d->origin, d->extent);
    for (int c = 0; c < 3; ++c) p.dims[c] = dims[c];
    if (int e = begin_label_edit(r, "no label volume")) return e;
    MorphPlan plan;
    if (!morph_plan(p.dims, p.box.origin, p.box.end, d->op, d->radius, tune(TUNE_MORPH_STEPS), &plan)) return fail(TBRM_ERR_INVALID_ARG, "no step plan for these arguments");
    if (int e = ensure_grow_scratch(r)) return e;

    const GrowScratch g = grow_scratch(r);
    p.labels = r->d_labels;
    p.bnx = r->dbn[0];
    p.bnxy = r->dbn[0] * r->dbn[1];
    for (int c = 0; c < 3; ++c) { p.range.b0[c] = plan.b0[c]; p.range.nb[c] = plan.nb[c]; p.wrange.b0[c] = plan.wb0[c]; p.wrange.nb[c] = plan.wnb[c]; }
    for (int w = 0; w < 8; ++w) { p.source[w] = d->source[w]; p.writable[w] = d->writable[w]; }
    p.bits = g.bits;
    p.cls[0] = g.act[0];
    p.cls[1] = g.act[1];
    p.conn26 = d->connectivity == 26;
    p.new_label = d->new_label;
    p.erase_label = d->erase_label;
    p.ctl = g.ctl;

    int32_t ctl[MORPH_CTL_WORDS];
    ctl_start(ctl, MORPH_CTL_WORDS, MORPH_MIN_X, dims);
    HIP_TRY(hipMemcpyAsync(g.ctl, ctl, sizeof(ctl), hipMemcpyHostToDevice, r->stream));
    HIP_TRY(launch_morph_load(p, r->stream));
    for (int i = 0; i < plan.launches; ++i) {
        p.from = i & 1;
        p.steps = plan.steps[i];
        p.erode = plan.erode[i];
        HIP_TRY(launch_morph_steps(p, r->stream));
    }
    p.from = plan.launches & 1; // the board the last launch wrote
    HIP_TRY(launch_morph_write(p, r->stream));
    HIP_TRY(hipMemcpyAsync(ctl, g.ctl, sizeof(ctl), hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));

    uint64_t counts[MORPH_CTL_COUNTS];
    memcpy(counts, ctl, sizeof(counts));
    memset(out, 0, sizeof(*out));
    out->source_voxels = counts[MORPH_SOURCE];
    out->result_voxels = counts[MORPH_RESULT];
    out->added = counts[MORPH_ADDED];
    out->removed = counts[MORPH_REMOVED];
    out->relabelled = counts[MORPH_RELABELLED];
    for (int c = 0; c < 3; ++c) { out->bbox_min[c] = ctl[MORPH_MIN_X + c]; out->bbox_max[c] = ctl[MORPH_MAX_X + c]; }
    out->launches = plan.launches;
    ++r->morph_counters[0];
    r->morph_counters[1] += (uint64_t) plan.launches;
    r->morph_counters[2] += counts[MORPH_WINDOWS];
    r->morph_counters[3] += counts[MORPH_BRICKS_WRITTEN];

    if (d->new_label >= 0) return labels_changed(r, out->bbox_min, out->bbox_max); // (nothing joined or left: nothing to do)
    return TBRM_OK;
}

} // extern "C"
