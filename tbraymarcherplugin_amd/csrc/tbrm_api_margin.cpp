// tbrm_api_margin.cpp — Euclidean margins of labels (include/tbrm_margin.h): validation, the plan (tbrm_margin_plan.h),
// the scratch and the counters around the kernels of tbrm_margin_kernels.hip.
//
// Between the frame's load and write (tbrm_board_edit.h): one or two transforms board -> board (k_margin_states,
// k_margin_xy, k_margin_z). The states, the field and a distance map's staging are the handle's d_margin. tbrm_label_distance takes
// the frame's load and ends on its own: one transform, the map out in chunks, nothing compared or written.
#include "tbrm_board_edit.h"
#include "tbrm_margin_kernels.h"
#include "tbrm_margin_plan.h"
#include "../../include/tbrm_margin.h"

#include <algorithm>

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

// what both calls check of a desc before the handle's state; the box and the plan
int margin_arguments(const tbrm_resources* r, const tbrm_margin_desc* d, BoardEdit& edit, MarginPlan& plan)
{
    if (d->op < TBRM_MARGIN_EXPAND || d->op > TBRM_MARGIN_CLOSE) return fail(TBRM_ERR_INVALID_ARG, "op %d: must be TBRM_MARGIN_EXPAND .. TBRM_MARGIN_CLOSE", (int) d->op);
    if (int e = label_codes(d->new_label, d->erase_label, d->reserved)) return e;
    int reach[3];
    if (!margin_reaches(d->weights, d->limit, reach))
        return fail(TBRM_ERR_INVALID_ARG, "weights (%u, %u, %u), limit %u: every weight must be >= 1, limit 1 .. 2^31 - 1, every reach isqrt(limit / weight) at most %d and one of them at least 1",
                    d->weights[0], d->weights[1], d->weights[2], d->limit, TBRM_MARGIN_MAX_REACH);
    if (int e = edit.begin(r, d->origin, d->extent)) return e;
    const MorphParams& p = edit.p;
    if (!margin_plan(p.dims, p.box.origin, p.box.end, d->op, d->weights, d->limit, &plan)) return fail(TBRM_ERR_INVALID_ARG, "no plan for these arguments");
    return TBRM_OK;
}

// the scratch of both kinds, the frame's bind, the plan's ranges and the parameters of the call's own kernels
int margin_params(tbrm_resources* r, const tbrm_margin_desc* d, const MarginPlan& plan, BoardEdit& edit, MarginScratch& m, MarginParams& q)
{
    MorphParams& p = edit.p;
    if (int e = edit.bind(r, d)) return e;
    edit.ranges(plan);
    const size_t bricks = (size_t) range_bricks(p.range);
    // (not counted in tbrm_path_counters [12], unlike the other operators' scratch)
    if (int e = ensure_bytes(r, r->d_margin, r->margin_bytes, margin_scratch(nullptr, bricks).bytes, nullptr)) return e;
    m = margin_scratch(r->d_margin, bricks);

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
    q.bits = p.bits;
    q.cls[0] = p.cls[0];
    q.cls[1] = p.cls[1];
    q.skip = tune(TUNE_MARGIN_SKIP) != 0;
    q.state = m.state;
    q.field = m.field;
    q.dist = m.dist;
    q.ctl = p.ctl;
    return TBRM_OK;
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

int tbrm_margin_counters(const tbrm_resources* r, uint64_t out[4]) { return copy_counters(r, &tbrm_resources::margin_counters, out); }

int tbrm_margin_labels(tbrm_resources* r, const tbrm_margin_desc* d, tbrm_margin_result* out)
{
    if (!r || !d || !out) return fail(TBRM_ERR_INVALID_ARG, "null argument");
    if (int e = refuse_resident(r)) return e;
    BoardEdit edit(MORPH_CTL_WORDS);
    MarginParams q{};
    MarginPlan plan;
    MarginScratch m;
    if (int e = margin_arguments(r, d, edit, plan)) return e;
    if (int e = margin_params(r, d, plan, edit, m, q)) return e;

    if (int e = edit.load(r)) return e;
    for (int i = 0; i < plan.transforms; ++i) {
        q.from = i & 1;
        q.shrink = plan.shrink[i];
        HIP_TRY(launch_margin_states(q, r->stream));
        HIP_TRY(launch_margin_xy(q, r->stream));
        q.layer0 = 0;
        HIP_TRY(launch_margin_z(q, false, q.range.nb[2], r->stream));
    }
    if (int e = edit.write(r, plan.transforms & 1)) return e; // the board the last transform wrote

    memset(out, 0, sizeof(*out));
    edit.result(out);
    for (int c = 0; c < 3; ++c) out->reach[c] = plan.reach[c];
    out->launches = plan.transforms * kMarginLaunchesPerTransform;
    return edit.end(r, r->margin_counters, out->launches);
}

int tbrm_label_distance(tbrm_resources* r, const tbrm_margin_desc* d, int32_t inside, void* out_host, size_t out_bytes)
{
    if (!r || !d || !out_host) return fail(TBRM_ERR_INVALID_ARG, "null argument");
    if (int e = refuse_resident(r)) return e;
    BoardEdit edit(MORPH_CTL_WORDS);
    const MorphParams& p = edit.p;
    MarginParams q{};
    MarginPlan plan;
    MarginScratch m;
    tbrm_margin_desc one = *d;
    if (int e = margin_arguments(r, &one, edit, plan)) return e; // (the op is checked, then replaced: a map is one transform)
    one.op = inside ? TBRM_MARGIN_SHRINK : TBRM_MARGIN_EXPAND;
    if (!margin_plan(p.dims, p.box.origin, p.box.end, one.op, one.weights, one.limit, &plan)) return fail(TBRM_ERR_INVALID_ARG, "no plan for these arguments");
    const size_t ex = (size_t) (p.box.end[0] - p.box.origin[0]), ey = (size_t) (p.box.end[1] - p.box.origin[1]), ez = (size_t) (p.box.end[2] - p.box.origin[2]);
    if (out_bytes != ex * ey * ez * sizeof(uint32_t))
        return fail(TBRM_ERR_INVALID_ARG, "out_bytes = %zu: the box holds %zu x %zu x %zu voxels of 4 bytes", out_bytes, ex, ey, ez);
    if (int e = margin_params(r, &one, plan, edit, m, q)) return e;

    if (int e = edit.load(r)) return e;
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
        q.layer0 = (q.z0 >> kBrickShift) - q.range.b0[2];
        const int layers = ((q.z1 - 1) >> kBrickShift) - (q.z0 >> kBrickShift) + 1;
        HIP_TRY(launch_margin_z(q, true, layers, r->stream));
        HIP_TRY(hipMemcpyAsync((uint32_t*) out_host + z * ex * ey, m.dist, (size_t) (q.z1 - q.z0) * ex * ey * sizeof(uint32_t), hipMemcpyDeviceToHost, r->stream));
        HIP_TRY(hipStreamSynchronize(r->stream)); // (the next chunk overwrites the staging)
        ++launches;
    }
    if (int e = edit.read_ctl(r)) return e;
    ++r->margin_counters[0];
    r->margin_counters[1] += (uint64_t) launches;
    r->margin_counters[2] += edit.count(MORPH_WINDOWS);
    return TBRM_OK;
}

} // extern "C"
