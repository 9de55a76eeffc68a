// tbrm_api_morph.cpp — binary morphology of the label volume (include/tbrm_morphology.h): validation, the step plan
// (tbrm_morph_plan.h) and the counters around the kernels of tbrm_morph_kernels.hip.
//
// Between the frame's load and write (tbrm_board_edit.h): the plan's step launches ping-ponging between the two boards
// (k_morph_steps, up to morph_steps unit steps each). Nothing on the data side is touched, nothing waits for the occlusion stream.
#include "tbrm_board_edit.h"
#include "tbrm_morph_plan.h"
#include "../../include/tbrm_morphology.h"

using namespace tbrm;
using namespace tbrm_host;

static_assert(TBRM_MORPH_MAX_RADIUS == kMorphMaxRadius && TBRM_MORPH_DILATE == MORPH_DILATE && TBRM_MORPH_ERODE == MORPH_ERODE &&
              TBRM_MORPH_OPEN == MORPH_OPEN && TBRM_MORPH_CLOSE == MORPH_CLOSE, "tbrm_morph_plan.h restates the header's constants");

extern "C" {

int tbrm_morph_abi_version(void) { return TBRM_MORPH_ABI_VERSION; }

int tbrm_morph_counters(const tbrm_resources* r, uint64_t out[4]) { return copy_counters(r, &tbrm_resources::morph_counters, out); }

int tbrm_morph_labels(tbrm_resources* r, const tbrm_morph_desc* d, tbrm_morph_result* out)
{
    if (!r || !d || !out) return fail(TBRM_ERR_INVALID_ARG, "null argument");
    if (int e = refuse_resident(r)) return e;
    if (d->op < TBRM_MORPH_DILATE || d->op > TBRM_MORPH_CLOSE) return fail(TBRM_ERR_INVALID_ARG, "op %d: must be TBRM_MORPH_DILATE .. TBRM_MORPH_CLOSE", (int) d->op);
    if (d->radius < 1 || d->radius > TBRM_MORPH_MAX_RADIUS) return fail(TBRM_ERR_INVALID_ARG, "radius %d: must be 1 .. %d", (int) d->radius, TBRM_MORPH_MAX_RADIUS);
    if (d->connectivity != 6 && d->connectivity != 26) return fail(TBRM_ERR_INVALID_ARG, "connectivity %d: must be 6 or 26", (int) d->connectivity);
    if (int e = label_codes(d->new_label, d->erase_label, d->reserved)) return e;
    BoardEdit edit(MORPH_CTL_WORDS);
    MorphParams& p = edit.p;
    if (int e = edit.begin(r, d->origin, d->extent)) return e;
    MorphPlan plan;
    if (!morph_plan(p.dims, p.box.origin, p.box.end, d->op, d->radius, tune(TUNE_MORPH_STEPS), &plan)) return fail(TBRM_ERR_INVALID_ARG, "no step plan for these arguments");
    if (int e = edit.bind(r, d)) return e;
    edit.ranges(plan);
    p.conn26 = d->connectivity == 26;

    if (int e = edit.load(r)) return e;
    for (int i = 0; i < plan.launches; ++i) {
        p.from = i & 1;
        p.steps = plan.steps[i];
        p.erode = plan.erode[i];
        HIP_TRY(launch_morph_steps(p, r->stream));
    }
    if (int e = edit.write(r, plan.launches & 1)) return e; // the board the last launch wrote

    memset(out, 0, sizeof(*out));
    edit.result(out);
    out->launches = plan.launches;
    return edit.end(r, r->morph_counters, plan.launches);
}

} // extern "C"
