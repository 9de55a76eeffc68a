// tbrm_api_paint.cpp — the 3D paint brush (include/tbrm_paint.h): validation, the stroke's staging and the counters
// around the kernel of tbrm_paint_kernels.hip, and the two host functions (tbrm_paint_plan.h).
//
// A call is: the plan of the stroke (segments, runs, the work box) on the host and into the handle's staging, the source set of the
// work box's bricks from the label bytes into board 0 (k_morph_load, as it stands), k_paint board 0 -> board 1, the comparison of
// board 1 with the label bytes inside the work box (k_morph_write, as it stands) and behind a write what every label write ends with
// (labels_changed). Outside the work box M is empty and R = S: cutting the box to it changes nothing but the cost. The
// boards, their classes and the control words are the scratch of region growing.
#include "tbrm_resources.h"
#include "tbrm_paint_kernels.h"
#include "../../include/tbrm_paint.h"
#include "../../include/tbrm_margin.h"

#include <cmath>
#include <cstring>

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

// only ever grown: a call with a stroke no longer than one before it allocates nothing
int ensure_paint_scratch(tbrm_resources* r, size_t n_segs, size_t n_runs)
{
    const size_t bytes = paint_scratch(nullptr, n_segs, n_runs).bytes;
    if (r->paint_bytes >= bytes) return TBRM_OK;
    HIP_TRY(hipStreamSynchronize(r->stream));
    (void) hipFree(r->d_paint);
    r->d_paint = nullptr;
    r->paint_bytes = 0;
    count_alloc(r, 1, "paint stroke staging");
    HIP_TRY(hipMalloc((void**) &r->d_paint, bytes));
    r->paint_bytes = bytes;
    return TBRM_OK;
}

// what the call checks of a desc and a stroke before the handle's state; the box
int paint_arguments_of(const tbrm_resources* r, const tbrm_paint_desc* d, const int32_t* points, size_t n_points, MorphParams& p)
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
    if (d->new_label < -1 || d->new_label > 255) return fail(TBRM_ERR_INVALID_ARG, "new_label %d: must be 0 .. 255, or -1 to measure only", (int) d->new_label);
    if (d->erase_label < 0 || d->erase_label > 255) return fail(TBRM_ERR_INVALID_ARG, "erase_label %d: must be 0 .. 255", (int) d->erase_label);
    if (d->gate) { // the rules of tbrm_grow_desc without relative_to_seed
        if (!(d->lo <= d->hi)) return fail(TBRM_ERR_INVALID_ARG, "range [%g, %g]: needs lo <= hi", d->lo, d->hi);
        if (r->desc.data_format == TBRM_FMT_R32_FLOAT) {
            if (!std::isfinite(d->lo) || !std::isfinite(d->hi) || !std::isfinite((float) d->lo) || !std::isfinite((float) d->hi))
                return fail(TBRM_ERR_INVALID_ARG, "range [%g, %g]: both must be finite as float32", d->lo, d->hi);
        } else {
            const double top = r->desc.data_format == TBRM_FMT_G8 ? 255.0 : 65535.0;
            if (!(d->lo >= 0.0 && d->hi <= top) || d->lo != std::floor(d->lo) || d->hi != std::floor(d->hi))
                return fail(TBRM_ERR_INVALID_ARG, "range [%g, %g]: needs integral codes with 0 <= lo <= hi <= %g", d->lo, d->hi, top);
        }
    }
    const BoxVerdict b = box_resolve(dims, d->origin, d->extent, true, &p.box, nullptr);
    if (b.what != BOX_OK) return fail_box(b, true, dims, d->origin, d->extent);
    for (int c = 0; c < 3; ++c) p.dims[c] = dims[c];
    return begin_label_edit(r, "no label volume");
}

// the parameters of the morphology kernels this call borrows (k_morph_load, k_morph_write) and of its own
void paint_params(const tbrm_resources* r, const tbrm_paint_desc* d, const PaintPlan& plan, const GrowScratch& g, const PaintScratch& m, MorphParams& p, PaintParams& q)
{
    p.labels = r->d_labels;
    p.bnx = r->dbn[0];
    p.bnxy = r->dbn[0] * r->dbn[1];
    p.box = plan.work;
    p.range = plan.range;
    p.wrange = plan.range; // no reach: the bricks of the work box
    for (int w = 0; w < 8; ++w) { p.source[w] = d->source[w]; p.writable[w] = d->writable[w]; }
    p.bits = g.bits;
    p.cls[0] = g.act[0];
    p.cls[1] = g.act[1];
    p.new_label = d->new_label;
    p.erase_label = d->erase_label;
    p.ctl = g.ctl;

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
    q.fmt = !d->gate ? kPaintNoGate : (r->desc.data_format == TBRM_FMT_G8 ? FMT_U8 : (r->desc.data_format == TBRM_FMT_G16 ? FMT_U16 : FMT_F32));
    if (d->gate) {
        if (q.fmt == FMT_F32) { q.lo_f = (float) d->lo; q.hi_f = (float) d->hi; }
        else { q.lo_code = (uint32_t) d->lo; q.hi_code = (uint32_t) d->hi; }
    }
    q.bits = g.bits;
    q.cls[0] = g.act[0];
    q.cls[1] = g.act[1];
    q.ctl = g.ctl;
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

int tbrm_paint_counters(const tbrm_resources* r, uint64_t out[4])
{
    if (!r || !out) return fail(TBRM_ERR_INVALID_ARG, "null argument");
    for (int k = 0; k < 4; ++k) out[k] = r->paint_counters[k];
    return TBRM_OK;
}

int tbrm_paint_labels(tbrm_resources* r, const tbrm_paint_desc* d, const int32_t* points_xyz, size_t n_points, tbrm_paint_result* out)
{
    if (!r || !d || !points_xyz || !out) return fail(TBRM_ERR_INVALID_ARG, "null argument");
    if (int e = refuse_resident(r)) return e;
    MorphParams p{};
    PaintParams q{};
    if (int e = paint_arguments_of(r, d, points_xyz, n_points, p)) return e;
    PaintPlan plan;
    paint_plan(p.box, d->weights, d->limit, points_xyz, n_points, plan);

    memset(out, 0, sizeof(*out));
    for (int c = 0; c < 3; ++c) { out->bbox_min[c] = p.dims[c]; out->bbox_max[c] = -1; }
    out->segments = (int32_t) plan.segs.size();
    ++r->paint_counters[0];
    if (plan.empty) return TBRM_OK; // the stroke misses the box: nothing is launched, nothing changes

    if (int e = ensure_grow_scratch(r)) return e;
    if (int e = ensure_paint_scratch(r, plan.segs.size(), plan.runs.size())) return e;
    const PaintScratch m = paint_scratch(r->d_paint, plan.segs.size(), plan.runs.size());
    paint_params(r, d, plan, grow_scratch(r), m, p, q);

    int32_t ctl[PAINT_CTL_WORDS];
    ctl_start(ctl, PAINT_CTL_WORDS, MORPH_MIN_X, p.dims);
    HIP_TRY(hipMemcpyAsync(p.ctl, ctl, sizeof(ctl), hipMemcpyHostToDevice, r->stream));
    HIP_TRY(hipMemcpyAsync(m.segs, plan.segs.data(), plan.segs.size() * sizeof(PaintSegment), hipMemcpyHostToDevice, r->stream));
    HIP_TRY(hipMemcpyAsync(m.runs, plan.runs.data(), plan.runs.size() * sizeof(PaintRun), hipMemcpyHostToDevice, r->stream));
    HIP_TRY(launch_morph_load(p, r->stream));
    HIP_TRY(launch_paint(q, r->stream));
    p.from = 1; // the board k_paint wrote
    HIP_TRY(launch_morph_write(p, r->stream));
    HIP_TRY(hipMemcpyAsync(ctl, p.ctl, sizeof(ctl), hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream)); // (also: the plan's vectors have been read)

    uint64_t counts[PAINT_CTL_WORDS / 2];
    memcpy(counts, ctl, sizeof(counts));
    out->stamp_voxels = counts[PAINT_CTL_STAMP];
    out->added = counts[MORPH_ADDED];
    out->removed = counts[MORPH_REMOVED];
    out->relabelled = counts[MORPH_RELABELLED];
    for (int c = 0; c < 3; ++c) { out->bbox_min[c] = ctl[MORPH_MIN_X + c]; out->bbox_max[c] = ctl[MORPH_MAX_X + c]; }
    out->bricks_whole = (int32_t) counts[PAINT_CTL_WHOLE];
    out->bricks_untouched = (int32_t) counts[PAINT_CTL_UNTOUCHED];
    out->bricks_evaluated = (int32_t) counts[MORPH_WINDOWS];
    out->launches = kPaintLaunches;
    r->paint_counters[1] += (uint64_t) kPaintLaunches;
    r->paint_counters[2] += counts[MORPH_WINDOWS];
    r->paint_counters[3] += counts[MORPH_BRICKS_WRITTEN];

    if (d->new_label >= 0) return labels_changed(r, out->bbox_min, out->bbox_max); // (nothing joined or left: nothing to do)
    return TBRM_OK;
}

} // extern "C"
