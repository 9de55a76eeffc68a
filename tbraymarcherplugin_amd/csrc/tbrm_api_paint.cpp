// tbrm_api_paint.cpp — the 3D paint brush (include/tbrm_paint.h): validation, the stroke's staging and the counters
// around the kernel of tbrm_paint_kernels.hip, and the two host functions (tbrm_paint_plan.h).
//
// Ahead of the frame's load (tbrm_board_edit.h): the plan of the stroke (segments, runs, the work box) on the host and
// into the handle's staging. Between load and write: k_paint board 0 -> board 1. The frame works on the work box: outside it M is
// empty and R = S, so cutting the box to it changes nothing but the cost.
#include "tbrm_board_edit.h"
#include "tbrm_paint_kernels.h"
#include "../../include/tbrm_paint.h"
#include "../../include/tbrm_margin.h"

using namespace tbrm;
using namespace tbrm_host;

static_assert(TBRM_PAINT_MAX_POINTS == kPaintMaxPoints && TBRM_PAINT_MAX_COORD == kPaintMaxCoord && TBRM_PAINT_MAX_DIM == kPaintMaxDim && TBRM_PAINT_MAX_WEIGHT == kPaintMaxWeight &&
              TBRM_PAINT_MAX_LIMIT == kPaintMaxLimit && TBRM_PAINT_MAX_REACH == kPaintMaxReach, "tbrm_paint_plan.h restates the header's constants");
static_assert(TBRM_PAINT_PAINT == PAINT_PAINT && TBRM_PAINT_ERASE == PAINT_ERASE, "tbrm_paint_plan.h restates the header's operators");
static_assert(kPaintMaxRuns <= 64, "k_paint gives every run a lane");

namespace {

// d_paint: [the segments][the runs], each part 256-byte aligned
struct PaintScratch {
    PaintSegment* segs;
    PaintRun* runs;
    size_t bytes;
};
PaintScratch paint_scratch(char* base, size_t n_segs, size_t n_runs)
{
    Carver c{base};
    PaintScratch s{};
    s.segs = c.take<PaintSegment>(n_segs);
    s.runs = c.take<PaintRun>(n_runs);
    s.bytes = c.off;
    return s;
}

// what the call checks of a desc and a stroke before the handle's state; the box
int paint_arguments_of(const tbrm_resources* r, const tbrm_paint_desc* d, const int32_t* points, size_t n_points, BoardEdit& edit)
{
    const tbrm_resources::Dims dims = r->data_dims();
    const int dd[3] = {dims[0], dims[1], dims[2]};
    const PaintVerdict v = paint_arguments(dd, d->op, d->gate, d->weights, d->limit, points, n_points);
    switch (v.what) {
    case PAINT_OK: break;
    case PAINT_DIMS: return fail(TBRM_ERR_UNSUPPORTED, "a volume of %d x %d x %d: the brush takes at most %d voxels along an axis", dd[0], dd[1], dd[2], TBRM_PAINT_MAX_DIM);
    case PAINT_N_POINTS: return fail(TBRM_ERR_INVALID_ARG, "n_points %zu: must be 1 .. %d", n_points, TBRM_PAINT_MAX_POINTS);
    case PAINT_OP: return fail(TBRM_ERR_INVALID_ARG, "op %d: must be 0 .. %d", (int) d->op, kPaintOps - 1);
    case PAINT_GATE: return fail(TBRM_ERR_INVALID_ARG, "gate %d: must be 0 or 1", (int) d->gate);
    case PAINT_WEIGHT: return fail(TBRM_ERR_INVALID_ARG, "weights[%d] = %u: must be 1 .. %d", v.axis, (unsigned) d->weights[v.axis], TBRM_PAINT_MAX_WEIGHT);
    case PAINT_LIMIT: return fail(TBRM_ERR_INVALID_ARG, "limit %u: must be 1 .. %u", (unsigned) d->limit, (unsigned) TBRM_PAINT_MAX_LIMIT);
    case PAINT_REACH:
        return fail(TBRM_ERR_INVALID_ARG, "limit %u with weights[%d] = %u: a reach of %d voxels, at most %d", (unsigned) d->limit, v.axis, (unsigned) d->weights[v.axis],
                    paint_reach_voxels(paint_reach8(d->limit, d->weights[v.axis])), TBRM_PAINT_MAX_REACH);
    case PAINT_COORD:
        return fail(TBRM_ERR_INVALID_ARG, "point %d: coordinate %d = %d, must be within +-%d eighths of a voxel", v.index, v.axis, (int) points[3 * (size_t) v.index + v.axis], TBRM_PAINT_MAX_COORD);
    case PAINT_SEGMENT: return fail(TBRM_ERR_INVALID_ARG, "segment %d: its squared length must be below 2^30 (tbrm_host_paint_stroke splits it)", v.index);
    }
    if (int e = label_codes(d->new_label, d->erase_label, 0)) return e; // (the desc has no reserved field)
    if (d->gate)
        if (int e = fail_value_range(r, d->lo, d->hi, false)) return e;
    return edit.begin(r, d->origin, d->extent);
}

// the staging, the frame's bind on the work box and the parameters of the call's own kernel
int paint_params(tbrm_resources* r, const tbrm_paint_desc* d, const PaintPlan& plan, BoardEdit& edit, PaintScratch& m, PaintParams& q)
{
    MorphParams& p = edit.p;
    if (int e = edit.bind(r, d)) return e;
    p.box = plan.work;
    p.range = plan.range;
    p.wrange = plan.range; // no reach: the bricks of the work box
    if (int e = ensure_bytes(r, r->d_paint, r->paint_bytes, paint_scratch(nullptr, plan.segs.size(), plan.runs.size()).bytes, "paint stroke staging")) return e;
    m = paint_scratch(r->d_paint, plan.segs.size(), plan.runs.size());

    q.bnx = p.bnx;
    q.bnxy = p.bnxy;
    for (int c = 0; c < 3; ++c) { q.dims[c] = p.dims[c]; q.w[c] = (int32_t) d->weights[c]; }
    q.work = plan.work;
    q.range = plan.range;
    q.limit = (int32_t) d->limit;
    q.op = d->op;
    q.skip = tune(TUNE_PAINT_SKIP) != 0;
    q.segs = m.segs;
    q.runs = m.runs;
    q.n_segs = (int) plan.segs.size();
    q.n_runs = (int) plan.runs.size();
    q.data = r->d_data;
    q.fmt = d->gate ? data_fmt(r) : kPaintNoGate;
    if (d->gate) {
        if (q.fmt == FMT_F32) { q.lo_f = (float) d->lo; q.hi_f = (float) d->hi; }
        else { q.lo_code = (uint32_t) d->lo; q.hi_code = (uint32_t) d->hi; }
    }
    q.bits = p.bits;
    q.cls[0] = p.cls[0];
    q.cls[1] = p.cls[1];
    q.ctl = p.ctl;
    return TBRM_OK;
}

} // namespace

extern "C" {

int tbrm_paint_abi_version(void) { return TBRM_PAINT_ABI_VERSION; }

int tbrm_host_paint_brush(const double spacing[3], double radius, uint32_t weights[3], uint32_t* limit)
{
    if (!spacing || !weights || !limit) return fail(TBRM_ERR_INVALID_ARG, "null argument");
    uint32_t w[3], margin_limit = 0;
    if (int e = tbrm_host_margin_weights(spacing, radius, w, &margin_limit)) return e;
    uint32_t l = 0;
    if (!paint_brush_admissible(w, margin_limit, &l))
        return fail(TBRM_ERR_INVALID_ARG, "spacing (%g, %g, %g), radius %g: must give weights of at most %d, a limit below 2^30 in eighths squared and reaches of at most %d voxels",
                    spacing[0], spacing[1], spacing[2], radius, TBRM_PAINT_MAX_WEIGHT, TBRM_PAINT_MAX_REACH);
    for (int c = 0; c < 3; ++c) weights[c] = w[c];
    *limit = l;
    return TBRM_OK;
}

int tbrm_host_paint_stroke(const int32_t dims[3], const float* uvw, size_t n, const uint32_t weights[3], int32_t* out_points, size_t capacity, size_t* n_out)
{
    if (!dims || !uvw || !weights || !n_out || (!out_points && capacity)) return fail(TBRM_ERR_INVALID_ARG, "null argument");
    *n_out = 0;
    for (int c = 0; c < 3; ++c) {
        if (dims[c] < 1 || dims[c] > TBRM_PAINT_MAX_DIM) return fail(TBRM_ERR_INVALID_ARG, "dims[%d] = %d: must be 1 .. %d", c, (int) dims[c], TBRM_PAINT_MAX_DIM);
        if (weights[c] < 1u || weights[c] > (uint32_t) TBRM_PAINT_MAX_WEIGHT) return fail(TBRM_ERR_INVALID_ARG, "weights[%d] = %u: must be 1 .. %d", c, (unsigned) weights[c], TBRM_PAINT_MAX_WEIGHT);
    }
    if (n < 1) return fail(TBRM_ERR_INVALID_ARG, "n %zu: a stroke has at least one position", n);
    std::vector<int32_t> points;
    paint_stroke(dims, uvw, n, weights, points);
    *n_out = points.size() / 3;
    if (*n_out > capacity) return fail(TBRM_ERR_INVALID_ARG, "capacity %zu: the stroke has %zu points", capacity, *n_out);
    memcpy(out_points, points.data(), points.size() * sizeof(int32_t));
    return TBRM_OK;
}

int tbrm_paint_counters(const tbrm_resources* r, uint64_t out[4]) { return copy_counters(r, &tbrm_resources::paint_counters, out); }

int tbrm_paint_labels(tbrm_resources* r, const tbrm_paint_desc* d, const int32_t* points_xyz, size_t n_points, tbrm_paint_result* out)
{
    if (!r || !d || !points_xyz || !out) return fail(TBRM_ERR_INVALID_ARG, "null argument");
    if (int e = refuse_resident(r)) return e;
    BoardEdit edit(PAINT_CTL_WORDS);
    const MorphParams& p = edit.p;
    PaintParams q{};
    PaintScratch m;
    if (int e = paint_arguments_of(r, d, points_xyz, n_points, edit)) return e;
    PaintPlan plan;
    paint_plan(p.box, d->weights, d->limit, points_xyz, n_points, plan);

    memset(out, 0, sizeof(*out));
    for (int c = 0; c < 3; ++c) { out->bbox_min[c] = p.dims[c]; out->bbox_max[c] = -1; }
    out->segments = (int32_t) plan.segs.size();
    ++r->paint_counters[0];
    if (plan.empty) return TBRM_OK; // the stroke misses the box: nothing is launched, nothing changes

    if (int e = paint_params(r, d, plan, edit, m, q)) return e;
    HIP_TRY(hipMemcpyAsync(m.segs, plan.segs.data(), plan.segs.size() * sizeof(PaintSegment), hipMemcpyHostToDevice, r->stream));
    HIP_TRY(hipMemcpyAsync(m.runs, plan.runs.data(), plan.runs.size() * sizeof(PaintRun), hipMemcpyHostToDevice, r->stream));
    if (int e = edit.load(r)) return e;
    HIP_TRY(launch_paint(q, r->stream));
    if (int e = edit.write(r, 1)) return e; // the board k_paint wrote (the wait also: the plan's vectors have been read)

    edit.changes(out);
    out->stamp_voxels = edit.count(PAINT_CTL_STAMP);
    out->bricks_whole = (int32_t) edit.count(PAINT_CTL_WHOLE);
    out->bricks_untouched = (int32_t) edit.count(PAINT_CTL_UNTOUCHED);
    out->bricks_evaluated = (int32_t) edit.count(MORPH_WINDOWS);
    out->launches = kPaintLaunches;
    return edit.end(r, r->paint_counters, kPaintLaunches, false); // (the call was counted above)
}

} // extern "C"
