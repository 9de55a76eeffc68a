// tbrm_api_compete.cpp — competitive growing from seed labels (include/tbrm_compete.h): validation, the scratch, the
// pass loop and the counters around the kernels of tbrm_compete_kernels.hip.
//
// A call is: the keys' start values and the claimable bits of the box's bricks (the only pass over the gate and the labels),
// relaxation passes until a pass changes no brick, then the result — counts, bounding box, the costs when asked for and, in a
// writing call, the label bytes — followed by what every label write ends with (labels_changed).
// The passes are enqueued grow_batch at a time and their changed-bricks words read back together, as region growing's are (§14);
// passes behind the fixed point find no brick due and do nothing, so the result does not depend on the batch. Nothing on the data
// side is touched, nothing waits for the occlusion stream (it reads neither the label volume nor the scratch).
#include "tbrm_resources.h"
#include "tbrm_compete_kernels.h"
#include "../../include/tbrm_compete.h"

#include <cmath>
#include <cstring>

using namespace tbrm;
using namespace tbrm_host;

static_assert(TBRM_COMPETE_MAX_COST == kCompeteMaxCost && TBRM_COMPETE_MAX_STEP_COST == kCompeteMaxStepCost && TBRM_COMPETE_MAX_SHIFT == kCompeteMaxShift &&
              TBRM_COMPETE_NO_COST == kCompeteUnreached, "tbrm_compete_plan.h restates the header's constants");
static_assert(kCompeteMaxBatch == kGrowMaxBatch, "the passes are batched by region growing's tunable");

namespace {

int refuse(const CompeteVerdict& v, const tbrm_compete_desc* d)
{
    switch (v.what) {
    case COMPETE_CONNECTIVITY: return fail(TBRM_ERR_INVALID_ARG, "connectivity %d: must be 6 (26-connectivity is not offered)", (int) d->connectivity);
    case COMPETE_MEASURE: return fail(TBRM_ERR_INVALID_ARG, "measure_only %d: must be 0 or 1", (int) d->measure_only);
    case COMPETE_STEP_COST: return fail(TBRM_ERR_INVALID_ARG, "step_cost[%d] = %d: must be 0 .. %d", v.axis, (int) d->step_cost[v.axis], TBRM_COMPETE_MAX_STEP_COST);
    case COMPETE_SHIFT: return fail(TBRM_ERR_INVALID_ARG, "value_shift %d: must be 0 .. %d", (int) d->value_shift, TBRM_COMPETE_MAX_SHIFT);
    case COMPETE_LIMIT: return fail(TBRM_ERR_INVALID_ARG, "cost_limit %u: must be 1 .. %u, or 0 for %u", (unsigned) d->cost_limit, TBRM_COMPETE_MAX_COST, TBRM_COMPETE_MAX_COST);
    case COMPETE_RESERVED: return fail(TBRM_ERR_INVALID_ARG, "reserved = %d: must be 0", (int) d->reserved);
    case COMPETE_RANGE: return fail(TBRM_ERR_INVALID_ARG, "range [%g, %g]: needs lo <= hi", d->lo, d->hi);
    case COMPETE_RANGE_CODES: return fail(TBRM_ERR_INVALID_ARG, "range [%g, %g]: needs integral codes inside the format's range", d->lo, d->hi);
    case COMPETE_RANGE_FLOAT: return fail(TBRM_ERR_INVALID_ARG, "range [%g, %g]: both must be finite as float32", d->lo, d->hi);
    case COMPETE_FLOAT_SCALE: return fail(TBRM_ERR_INVALID_ARG, "float_scale %g: must be finite and > 0 (tbrm_host_compete_float_range)", (double) d->float_scale);
    case COMPETE_FLOAT_ORIGIN: return fail(TBRM_ERR_INVALID_ARG, "float_origin %g: must be finite", (double) d->float_origin);
    default: return TBRM_OK;
    }
}

} // namespace

extern "C" {

int tbrm_compete_abi_version(void) { return TBRM_COMPETE_ABI_VERSION; }

int tbrm_host_compete_float_range(double lo, double hi, float* float_origin, float* float_scale)
{
    if (!float_origin || !float_scale) return fail(TBRM_ERR_INVALID_ARG, "null argument");
    if (!compete_float_range(lo, hi, float_origin, float_scale))
        return fail(TBRM_ERR_INVALID_ARG, "range [%g, %g]: needs finite lo < hi whose origin and scale 65535 / (hi - lo) are finite as float32", lo, hi);
    return TBRM_OK;
}

int tbrm_compete_counters(const tbrm_resources* r, uint64_t out[4]) { return copy_counters(r, &tbrm_resources::compete_counters, out); }

int tbrm_compete_labels(tbrm_resources* r, const tbrm_compete_desc* d, uint32_t* costs_out, tbrm_compete_result* out)
{
    if (!r || !d || !out) return fail(TBRM_ERR_INVALID_ARG, "null argument");
    if (int e = refuse_resident(r)) return e;
    const bool is_float = r->desc.data_format == TBRM_FMT_R32_FLOAT;
    const double top = is_float ? 0.0 : (r->desc.data_format == TBRM_FMT_G8 ? 255.0 : 65535.0);
    if (int e = refuse(compete_arguments(d->connectivity, d->measure_only, d->step_cost, d->value_shift, d->cost_limit, d->reserved, d->lo, d->hi, top,
                                         d->float_origin, d->float_scale), d)) return e;
    const tbrm_resources::Dims dims = r->data_dims();
    CompeteParams p{};
    const BoxVerdict v = box_resolve(dims, d->origin, d->extent, true, &p.box, &p.range);
    if (v.what != BOX_OK) return fail_box(v, true, dims, d->origin, d->extent);
    uint64_t box_voxels = 1;
    for (int c = 0; c < 3; ++c) box_voxels *= (uint64_t) (p.box.end[c] - p.box.origin[c]);
    if (int e = begin_label_edit(r, "no label volume")) return e;

    const uint64_t n_bricks = range_bricks(p.range);
    const CompeteLayout lay = compete_layout(n_bricks);
    if (int e = ensure_bytes(r, r->d_compete, r->compete_bytes, lay.bytes, "competitive growing scratch")) return e;
    if (costs_out)
        if (int e = ensure_bytes(r, r->d_compete_costs, r->compete_costs_bytes, (size_t) box_voxels * sizeof(uint32_t), "competitive growing costs")) return e;

    p.data = r->d_data;
    p.labels = r->d_labels;
    p.fmt = data_fmt(r);
    p.bnx = r->dbn[0];
    p.bnxy = r->dbn[0] * r->dbn[1];
    if (is_float) { p.lo_f = (float) d->lo; p.hi_f = (float) d->hi; p.float_origin = d->float_origin; p.float_scale = d->float_scale; }
    else { p.lo_code = (uint32_t) d->lo; p.hi_code = (uint32_t) d->hi; }
    for (int w = 0; w < 8; ++w) { p.seeds[w] = d->seeds[w]; p.writable[w] = d->writable[w]; }
    for (int a = 0; a < 3; ++a) p.step[a] = (uint32_t) d->step_cost[a];
    p.shift = d->value_shift;
    p.limit = compete_limit(d->cost_limit);
    p.keys = (uint32_t*) (r->d_compete + lay.keys);
    p.claim = (uint8_t*) (r->d_compete + lay.claim);
    uint32_t* const act[2] = {(uint32_t*) (r->d_compete + lay.act[0]), (uint32_t*) (r->d_compete + lay.act[1])};
    p.act[0] = act[0];
    p.act[1] = act[1];
    p.counts = (unsigned long long*) (r->d_compete + lay.counts);
    p.ctl = (int32_t*) (r->d_compete + lay.ctl);
    p.write = d->measure_only == 0;
    p.costs = costs_out ? (uint32_t*) r->d_compete_costs : nullptr;

    // both activity arrays, the counts and the control words start as zeros (they lie behind one another), the bounding box as (dims, -1)
    int32_t ctl[COMPETE_CTL_WORDS];
    ctl_start(ctl, COMPETE_CTL_WORDS, COMPETE_MIN_X, dims);
    HIP_TRY(hipMemsetAsync(r->d_compete + lay.act[0], 0, lay.ctl - lay.act[0], r->stream));
    HIP_TRY(hipMemcpyAsync(p.ctl, ctl, sizeof(ctl), hipMemcpyHostToDevice, r->stream));
    HIP_TRY(launch_compete_init(p, r->stream));

    // The passes. A pass that changes a brick lowers a key; with every brick's reads a pass old at the worst, pass k has made final
    // every voxel whose best path crosses fewer than k brick faces, and a path has fewer steps than the box has voxels: box_voxels + 1
    // passes always hold a pass without a change. None among that many is a defect, reported instead of looped on.
    uint64_t passes = 0;
    {
        const int batch = std::min(std::max(tune(TUNE_GROW_BATCH), 1), kCompeteMaxBatch);
        int32_t changed[kCompeteMaxBatch];
        uint64_t enqueued = 0;
        for (bool done = false; !done;) {
            if (enqueued >= box_voxels + 1) return fail(TBRM_ERR_NO_DEVICE, "competitive growing did not reach its fixed point within %llu passes", (unsigned long long) enqueued);
            if (enqueued) HIP_TRY(hipMemsetAsync(p.ctl + COMPETE_CHANGED, 0, (size_t) kCompeteMaxBatch * sizeof(int32_t), r->stream));
            for (int i = 0; i < batch; ++i, ++enqueued) {
                p.changed_word = COMPETE_CHANGED + i;
                p.act[0] = act[enqueued & 1];
                p.act[1] = act[(enqueued + 1) & 1];
                HIP_TRY(launch_compete_pass(p, r->stream));
            }
            HIP_TRY(hipMemcpyAsync(changed, p.ctl + COMPETE_CHANGED, (size_t) batch * sizeof(int32_t), hipMemcpyDeviceToHost, r->stream));
            HIP_TRY(hipStreamSynchronize(r->stream));
            for (int i = 0; i < batch && !done; ++i) {
                if (changed[i] == 0) done = true;
                else ++passes;
            }
        }
    }
    HIP_TRY(launch_compete_write(p, r->stream));
    uint64_t counts[COMPETE_COUNTS];
    HIP_TRY(hipMemcpyAsync(counts, p.counts, sizeof(counts), hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipMemcpyAsync(ctl, p.ctl, COMPETE_CHANGED * sizeof(int32_t), hipMemcpyDeviceToHost, r->stream));
    if (costs_out) HIP_TRY(hipMemcpyAsync(costs_out, p.costs, (size_t) box_voxels * sizeof(uint32_t), hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));

    memset(out, 0, sizeof(*out));
    out->seed_voxels = counts[COMPETE_SEEDS];
    out->claimable = counts[COMPETE_CLAIMABLE];
    out->claimed = counts[COMPETE_CLAIMED];
    out->relabelled = counts[COMPETE_RELABELLED];
    for (int l = 0; l < 256; ++l) out->claimed_per_label[l] = counts[COMPETE_PER_LABEL + l];
    out->max_cost = (uint32_t) ctl[COMPETE_MAX_COST];
    out->passes = (int32_t) passes;
    for (int c = 0; c < 3; ++c) { out->bbox_min[c] = ctl[COMPETE_MIN_X + c]; out->bbox_max[c] = ctl[COMPETE_MAX_X + c]; }
    ++r->compete_counters[0];
    r->compete_counters[1] += passes;
    r->compete_counters[2] += counts[COMPETE_VISITS];
    r->compete_counters[3] += counts[COMPETE_BRICKS_WRITTEN];

    if (p.write) return labels_changed(r, out->bbox_min, out->bbox_max); // (nothing claimed: nothing to do)
    return TBRM_OK;
}

} // extern "C"
