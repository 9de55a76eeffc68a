// tbrm_api_margin.cpp — Euclidean margins of labels (include/tbrm_margin.h): validation, the plan (tbrm_margin_plan.h),
// the scratch and the counters around the kernels of tbrm_margin_kernels.hip.
//
// A call is: the source set of the planned bricks from the label bytes into board 0 (k_morph_load, as it stands), one or two
// transforms board -> board (k_margin_states, k_margin_xy, k_margin_z), the comparison of the final board with the label bytes inside
// the box (k_morph_write, as it stands) and behind a write what every label write ends with (labels_changed). The
// boards, their classes and the control words are the scratch of region growing; the states, the field and a distance map's staging
// are the handle's d_margin.
#include "tbrm_resources.h"
#include "tbrm_margin_kernels.h"
#include "tbrm_margin_plan.h"
#include "../../include/tbrm_margin.h"

#include <algorithm>
#include <cstring>

using namespace tbrm;
using namespace tbrm_host;

static_assert(TBRM_MARGIN_MAX_REACH == kMarginMaxReach && TBRM_MARGIN_FAR == kMarginFar && TBRM_MARGIN_EXPAND == MARGIN_EXPAND &&
              TBRM_MARGIN_SHRINK == MARGIN_SHRINK && TBRM_MARGIN_OPEN == MARGIN_OPEN && TBRM_MARGIN_CLOSE == MARGIN_CLOSE,
              "tbrm_margin_plan.h restates the header's constants");

namespace {

// d_margin for a range of `bricks` bricks: [states: a byte per brick][field: 512 pairs per brick][map staging: 256 words per brick],
// each part 256-byte aligned — 4 bytes per voxel of the range and a byte per brick
struct MarginScratch {
    uint8_t* state;
    uint16_t* field;
    uint32_t* dist;
    size_t dist_words;
    size_t bytes;
};

MarginScratch margin_scratch(char* base, size_t bricks)
{
    Carver c{base};
    MarginScratch m{};
    m.state = c.take<uint8_t>(bricks);
    m.field = c.take<uint16_t>(bricks * 512);
    m.dist_words = bricks * 256;
    m.dist = c.take<uint32_t>(m.dist_words);
    m.bytes = c.off;
    return m;
}

// at least what `bricks` bricks need: a call that needs no more than an earlier one allocates nothing
int ensure_margin_scratch(tbrm_resources* r, size_t bricks)
{
    const size_t bytes = margin_scratch(nullptr, bricks).bytes;
    if (r->margin_bytes >= bytes) return TBRM_OK;
    HIP_TRY(hipStreamSynchronize(r->stream));
    if (r->d_margin) HIP_TRY(hipFree(r->d_margin));
    r->d_margin = nullptr;
    r->margin_bytes = 0;
    HIP_TRY(hipMalloc((void**) &r->d_margin, bytes));
    r->margin_bytes = bytes;
    return TBRM_OK;
}

// what both calls check of a desc before the handle's state; the box and the plan
int margin_arguments(const tbrm_resources* r, const tbrm_margin_desc* d, MorphParams& p, MarginPlan& plan)
{
    if (d->op < TBRM_MARGIN_EXPAND || d->op > TBRM_MARGIN_CLOSE) return fail(TBRM_ERR_INVALID_ARG, "op %d: must be TBRM_MARGIN_EXPAND .. TBRM_MARGIN_CLOSE", (int) d->op);
    if (d->new_label < -1 || d->new_label > 255) return fail(TBRM_ERR_INVALID_ARG, "new_label %d: must be 0 .. 255, or -1 to measure only", (int) d->new_label);
    if (d->erase_label < 0 || d->erase_label > 255) return fail(TBRM_ERR_INVALID_ARG, "erase_label %d: must be 0 .. 255", (int) d->erase_label);
    if (d->reserved != 0) return fail(TBRM_ERR_INVALID_ARG, "reserved = %d: must be 0", (int) d->reserved);
    int reach[3];
    if (!margin_reaches(d->weights, d->limit, reach))
        return fail(TBRM_ERR_INVALID_ARG, "weights (%u, %u, %u), limit %u: every weight must be >= 1, limit 1 .. 2^31 - 1, every reach isqrt(limit / weight) at most %d and one of them at least 1",
                    d->weights[0], d->weights[1], d->weights[2], d->limit, TBRM_MARGIN_MAX_REACH);
    const tbrm_resources::Dims dims = r->data_dims();
    const BoxVerdict v = box_resolve(dims, d->origin, d->extent, true, &p.box, nullptr);
    if (v.what != BOX_OK) return fail_box(v, true, dims, d->origin, d->extent);
    for (int c = 0; c < 3; ++c) p.dims[c] = dims[c];
    if (int e = begin_label_edit(r, "no label volume")) return e;
    if (!margin_plan(p.dims, p.box.origin, p.box.end, d->op, d->weights, d->limit, &plan)) return fail(TBRM_ERR_INVALID_ARG, "no plan for these arguments");
    return TBRM_OK;
}

// the parameters of the morphology kernels this call borrows (k_morph_load, k_morph_write) and of its own
void margin_params(const tbrm_resources* r, const tbrm_margin_desc* d, const MarginPlan& plan, const GrowScratch& g, const MarginScratch& m,
                   MorphParams& p, MarginParams& q)
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
    q.box = p.box;
    for (int c = 0; c < 3; ++c) {
        q.dims[c] = p.dims[c];
        q.w[c] = d->weights[c];
        q.reach[c] = plan.reach[c];
        q.kb[c] = (plan.reach[c] + kBrick - 1) / kBrick;
    }
    q.limit = d->limit;
    q.bits = g.bits;
    q.cls[0] = g.act[0];
    q.cls[1] = g.act[1];
    q.skip = tune(TUNE_MARGIN_SKIP) != 0;
    q.state = m.state;
    q.field = m.field;
    q.dist = m.dist;
    q.ctl = g.ctl;
}

} // namespace

extern "C" {

int tbrm_margin_abi_version(void) { return TBRM_MARGIN_ABI_VERSION; }

int tbrm_host_margin_weights(const double spacing[3], double radius, uint32_t weights[3], uint32_t* limit)
{
    if (!spacing || !weights || !limit) return fail(TBRM_ERR_INVALID_ARG, "null argument");
    if (!margin_weights(spacing, radius, weights, limit))
        return fail(TBRM_ERR_INVALID_ARG, "spacing (%g, %g, %g), radius %g: must be finite and > 0, and give a limit below 2^31 and reaches of at most %d voxels, one of them at least 1",
                    spacing[0], spacing[1], spacing[2], radius, TBRM_MARGIN_MAX_REACH);
    return TBRM_OK;
}

int tbrm_margin_counters(const tbrm_resources* r, uint64_t out[4])
{
    if (!r || !out) return fail(TBRM_ERR_INVALID_ARG, "null argument");
    for (int k = 0; k < 4; ++k) out[k] = r->margin_counters[k];
    return TBRM_OK;
}

int tbrm_margin_labels(tbrm_resources* r, const tbrm_margin_desc* d, tbrm_margin_result* out)
{
    if (!r || !d || !out) return fail(TBRM_ERR_INVALID_ARG, "null argument");
    if (int e = refuse_resident(r)) return e;
    MorphParams p{};
    MarginParams q{};
    MarginPlan plan;
    if (int e = margin_arguments(r, d, p, plan)) return e;
    if (int e = ensure_grow_scratch(r)) return e;
    const BrickRange range{{plan.b0[0], plan.b0[1], plan.b0[2]}, {plan.nb[0], plan.nb[1], plan.nb[2]}};
    const size_t bricks = (size_t) range_bricks(range);
    if (int e = ensure_margin_scratch(r, bricks)) return e;
    margin_params(r, d, plan, grow_scratch(r), margin_scratch(r->d_margin, bricks), p, q);

    int32_t ctl[MORPH_CTL_WORDS];
    ctl_start(ctl, MORPH_CTL_WORDS, MORPH_MIN_X, p.dims);
    HIP_TRY(hipMemcpyAsync(p.ctl, ctl, sizeof(ctl), hipMemcpyHostToDevice, r->stream));
    HIP_TRY(launch_morph_load(p, r->stream));
    for (int i = 0; i < plan.transforms; ++i) {
        q.from = i & 1;
        q.shrink = plan.shrink[i];
        HIP_TRY(launch_margin_states(q, r->stream));
        HIP_TRY(launch_margin_xy(q, r->stream));
        q.layer0 = 0;
        HIP_TRY(launch_margin_z(q, false, range.nb[2], r->stream));
    }
    p.from = plan.transforms & 1; // the board the last transform wrote
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
    out->launches = plan.transforms * kMarginLaunchesPerTransform;
    ++r->margin_counters[0];
    r->margin_counters[1] += (uint64_t) out->launches;
    r->margin_counters[2] += counts[MORPH_WINDOWS];
    r->margin_counters[3] += counts[MORPH_BRICKS_WRITTEN];

    if (d->new_label >= 0) return labels_changed(r, out->bbox_min, out->bbox_max); // (nothing joined or left: nothing to do)
    return TBRM_OK;
}

int tbrm_label_distance(tbrm_resources* r, const tbrm_margin_desc* d, int32_t inside, void* out_host, size_t out_bytes)
{
    if (!r || !d || !out_host) return fail(TBRM_ERR_INVALID_ARG, "null argument");
    if (int e = refuse_resident(r)) return e;
    MorphParams p{};
    MarginParams q{};
    MarginPlan plan;
    tbrm_margin_desc one = *d;
    if (int e = margin_arguments(r, &one, p, plan)) return e; // (the op is checked, then replaced: a map is one transform)
    one.op = inside ? TBRM_MARGIN_SHRINK : TBRM_MARGIN_EXPAND;
    if (!margin_plan(p.dims, p.box.origin, p.box.end, one.op, one.weights, one.limit, &plan)) return fail(TBRM_ERR_INVALID_ARG, "no plan for these arguments");
    const size_t ex = (size_t) (p.box.end[0] - p.box.origin[0]), ey = (size_t) (p.box.end[1] - p.box.origin[1]), ez = (size_t) (p.box.end[2] - p.box.origin[2]);
    if (out_bytes != ex * ey * ez * sizeof(uint32_t))
        return fail(TBRM_ERR_INVALID_ARG, "out_bytes = %zu: the box holds %zu x %zu x %zu voxels of 4 bytes", out_bytes, ex, ey, ez);
    if (int e = ensure_grow_scratch(r)) return e;
    const BrickRange range{{plan.b0[0], plan.b0[1], plan.b0[2]}, {plan.nb[0], plan.nb[1], plan.nb[2]}};
    const size_t bricks = (size_t) range_bricks(range);
    if (int e = ensure_margin_scratch(r, bricks)) return e;
    const MarginScratch m = margin_scratch(r->d_margin, bricks);
    margin_params(r, &one, plan, grow_scratch(r), m, p, q);

    int32_t ctl[MORPH_CTL_WORDS];
    ctl_start(ctl, MORPH_CTL_WORDS, MORPH_MIN_X, p.dims);
    HIP_TRY(hipMemcpyAsync(p.ctl, ctl, sizeof(ctl), hipMemcpyHostToDevice, r->stream));
    HIP_TRY(launch_morph_load(p, r->stream));
    q.from = 0;
    q.shrink = plan.shrink[0];
    HIP_TRY(launch_margin_states(q, r->stream));
    HIP_TRY(launch_margin_xy(q, r->stream));
    // the map leaves in chunks of whole z slices of the box that fit the staging (a range of nb bricks stages 256 nb words and a slice
    // of the box has at most 64 nb[0] nb[1]: at least four slices per brick layer fit)
    const size_t per_chunk = std::min(ez, m.dist_words / (ex * ey));
    int launches = 2;
    for (size_t z = 0; z < ez; z += per_chunk) {
        q.z0 = p.box.origin[2] + (int) z;
        q.z1 = p.box.origin[2] + (int) std::min(ez, z + per_chunk);
        q.layer0 = (q.z0 >> kBrickShift) - range.b0[2];
        const int layers = ((q.z1 - 1) >> kBrickShift) - (q.z0 >> kBrickShift) + 1;
        HIP_TRY(launch_margin_z(q, true, layers, r->stream));
        HIP_TRY(hipMemcpyAsync((uint32_t*) out_host + z * ex * ey, m.dist, (size_t) (q.z1 - q.z0) * ex * ey * sizeof(uint32_t), hipMemcpyDeviceToHost, r->stream));
        HIP_TRY(hipStreamSynchronize(r->stream)); // (the next chunk overwrites the staging)
        ++launches;
    }
    HIP_TRY(hipMemcpyAsync(ctl, p.ctl, sizeof(ctl), hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    uint64_t counts[MORPH_CTL_COUNTS];
    memcpy(counts, ctl, sizeof(counts));
    ++r->margin_counters[0];
    r->margin_counters[1] += (uint64_t) launches;
    r->margin_counters[2] += counts[MORPH_WINDOWS];
    return TBRM_OK;
}

} // extern "C"
