// tbrm_api_segment.cpp — seeded region growing into the label volume (include/tbrm_segment.h): validation, the
// scratch, the pass loop and the counters around the kernels of tbrm_segment_kernels.hip.
//
// A call is: the candidate bits of the box's bricks (the only pass over voxels and labels), the seeds, propagation passes until a
// pass changes no brick, the region's size and bounding box, and — a writing call — new_label into the bricks of that bounding box,
// followed by what every label write ends with (labels_changed).
// The passes are enqueued grow_batch at a time and their changed-bricks words read back together; passes behind the fixed point
// find no brick due and do nothing, so the result does not depend on the batch. Nothing on the data side is touched, nothing waits
// for the occlusion stream (it reads neither the label volume nor the scratch).
#include "tbrm_resources.h"
#include "../../include/tbrm_segment.h"

#include <cmath>
#include <cstring>

using namespace tbrm;
using namespace tbrm_host;

namespace {

size_t grow_bricks(const tbrm_resources* r) { return (size_t) r->dbn[0] * r->dbn[1] * r->dbn[2]; }

} // namespace

namespace tbrm_host {

// the scratch, in one allocation: [bits: 16 words per brick][activity: 2 words per brick][seeds][control words], each part 256-byte aligned
GrowScratch grow_scratch(const tbrm_resources* r)
{
    const size_t nb = grow_bricks(r);
    Carver c{r->d_grow};
    GrowScratch g{};
    g.bits = c.take<uint64_t>(nb * 16);
    g.act[0] = c.take<uint32_t>(nb);
    g.act[1] = c.take<uint32_t>(nb);
    g.seeds = c.take<int32_t>((size_t) kGrowMaxSeeds * 3);
    g.ctl = c.take<int32_t>(GROW_CTL_WORDS);
    g.bytes = c.off;
    return g;
}

int ensure_grow_scratch(tbrm_resources* r)
{
    if (r->d_grow) return TBRM_OK;
    count_alloc(r, 1, "region growing scratch");
    HIP_TRY(hipMalloc((void**) &r->d_grow, grow_scratch(r).bytes));
    return TBRM_OK;
}

} // namespace tbrm_host

namespace {

// the stored value of one voxel, as the double the header's units carry it in
int read_voxel(tbrm_resources* r, const int32_t xyz[3], double* out)
{
    const size_t b = ((size_t) (xyz[2] >> kBrickShift) * r->dbn[1] + (size_t) (xyz[1] >> kBrickShift)) * r->dbn[0] + (size_t) (xyz[0] >> kBrickShift);
    const size_t i = b * 512 + (size_t) (((xyz[2] & 7) << 6) | ((xyz[1] & 7) << 3) | (xyz[0] & 7));
    const size_t elem = format_bytes(r->desc.data_format);
    uint32_t raw = 0u;
    HIP_TRY(hipMemcpyAsync(&raw, (const char*) r->d_data + i * elem, elem, hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    if (r->desc.data_format == TBRM_FMT_R32_FLOAT) {
        float f;
        memcpy(&f, &raw, sizeof(f));
        *out = (double) f;
    } else *out = (double) raw; // (little-endian: the code's one or two bytes are the low ones)
    return TBRM_OK;
}

} // namespace

extern "C" {

int tbrm_segment_abi_version(void) { return TBRM_SEGMENT_ABI_VERSION; }

int tbrm_host_hit_voxel(const int32_t dims[3], const tbrm_hit* hit, int32_t out_xyz[3])
{
    if (!dims || !hit || !out_xyz) return fail(TBRM_ERR_INVALID_ARG, "null argument");
    if (hit->sample < 0) return fail(TBRM_ERR_INVALID_ARG, "the record holds no hit");
    for (int c = 0; c < 3; ++c)
        if (dims[c] < 1) return fail(TBRM_ERR_INVALID_ARG, "dims[%d] = %d: must be >= 1", c, (int) dims[c]);
    for (int c = 0; c < 3; ++c) { // the label step's voxel (k_raymarch_lit LABELS): float32, round half to even
        float u = hit->uvw[c];
        u = u < 0.0f ? 0.0f : (u > 1.0f ? 1.0f : u); // saturate; a NaN goes to 0 as the device's saturate does
        if (!(u == u)) u = 0.0f;
        const float t = (float) (dims[c] - 1) * u;
        out_xyz[c] = (int32_t) std::nearbyintf(t); // (the default rounding mode: to nearest, ties to even)
    }
    return TBRM_OK;
}

int tbrm_segment_counters(const tbrm_resources* r, uint64_t out[4]) { return copy_counters(r, &tbrm_resources::grow_counters, out); }

int tbrm_attach_empty_label_volume(tbrm_resources* r)
{
    if (!r) return fail(TBRM_ERR_INVALID_ARG, "null argument");
    if (r->resident) return fail(TBRM_ERR_UNSUPPORTED, "slab-resident handle: label volumes are not supported");
    if (int e = refuse_color(r, "tbrm_attach_empty_label_volume")) return e;
    if (r->d_labels) return TBRM_OK;
    if (int e = bind(r)) return e;
    if (int e = allocate_labels(r)) return e;
    HIP_TRY(hipMemsetAsync(r->d_labels, 0, grow_bricks(r) * 512, r->stream));
    const int b0[3] = {0, 0, 0}, b1[3] = {r->dbn[0], r->dbn[1], r->dbn[2]};
    if (int e = brick_masks(r, b0, b1)) return e;
    return refresh_live(r);
}

int tbrm_grow_region(tbrm_resources* r, const tbrm_grow_desc* d, const int32_t* seeds_xyz, int32_t n_seeds, tbrm_grow_result* out)
{
    if (!r || !d || !out || (n_seeds > 0 && !seeds_xyz)) return fail(TBRM_ERR_INVALID_ARG, "null argument");
    if (int e = refuse_resident(r)) return e;
    if (d->connectivity != 6 && d->connectivity != 26) return fail(TBRM_ERR_INVALID_ARG, "connectivity %d: must be 6 or 26", (int) d->connectivity);
    if (d->new_label < -1 || d->new_label > 255) return fail(TBRM_ERR_INVALID_ARG, "new_label %d: must be 0 .. 255, or -1 to measure only", (int) d->new_label);
    if (n_seeds < 0 || n_seeds > TBRM_GROW_MAX_SEEDS) return fail(TBRM_ERR_INVALID_ARG, "n_seeds %d: must be 0 .. %d", (int) n_seeds, TBRM_GROW_MAX_SEEDS);
    if (d->relative_to_seed && n_seeds < 1) return fail(TBRM_ERR_INVALID_ARG, "relative_to_seed needs a seed");
    const tbrm_resources::Dims dims = r->data_dims();
    for (int32_t s = 0; s < n_seeds; ++s)
        for (int c = 0; c < 3; ++c)
            if (seeds_xyz[3 * s + c] < 0 || seeds_xyz[3 * s + c] >= dims[c])
                return fail(TBRM_ERR_INVALID_ARG, "seed %d lies outside the volume: coordinate %d along axis %d of %d", (int) s, (int) seeds_xyz[3 * s + c], c, dims[c]);

    GrowParams p{};
    const BoxVerdict v = box_resolve(dims, d->origin, d->extent, true, &p.box, &p.range);
    if (v.what != BOX_OK) return fail_box(v, true, dims, d->origin, d->extent);
    uint64_t box_voxels = 1;
    for (int c = 0; c < 3; ++c) box_voxels *= (uint64_t) (p.box.end[c] - p.box.origin[c]);
    const bool is_float = r->desc.data_format == TBRM_FMT_R32_FLOAT;
    const double top = r->desc.data_format == TBRM_FMT_G8 ? 255.0 : 65535.0;
    if (int e = fail_value_range(r, d->lo, d->hi, d->relative_to_seed != 0)) return e;
    const bool writes = d->new_label >= 0;
    if (int e = begin_label_edit(r, writes ? "no label volume to write to" : nullptr)) return e;
    if (int e = ensure_grow_scratch(r)) return e;

    // the range in use
    double lo = d->lo, hi = d->hi;
    bool none = false; // no voxel can be a candidate
    if (d->relative_to_seed) {
        double v0 = 0.0;
        if (int e = read_voxel(r, seeds_xyz, &v0)) return e;
        if (v0 != v0) { none = true; lo = hi = v0; }
        else {
            lo = v0 + d->lo;
            hi = v0 + d->hi;
            if (!is_float) {
                none = lo > top || hi < 0.0;
                lo = std::min(std::max(lo, 0.0), top);
                hi = std::min(std::max(hi, 0.0), top);
            }
        }
    }
    if (is_float) { lo = (double) (float) lo; hi = (double) (float) hi; } // (what the kernel compares with, and what is reported)
    if (is_float) { p.lo_f = (float) lo; p.hi_f = (float) hi; }
    else { p.lo_code = (uint32_t) lo; p.hi_code = (uint32_t) hi; }
    if (none) { p.lo_f = 1.0f; p.hi_f = 0.0f; p.lo_code = 1u; p.hi_code = 0u; }

    const GrowScratch g = grow_scratch(r);
    p.data = r->d_data;
    p.labels = r->d_labels;
    p.fmt = data_fmt(r);
    p.bnx = r->dbn[0];
    p.bnxy = r->dbn[0] * r->dbn[1];
    for (int w = 0; w < 8; ++w) p.writable[w] = d->writable[w];
    p.all_join = n_seeds == 0;
    p.conn26 = d->connectivity == 26;
    p.bits = g.bits;
    p.act[0] = g.act[0];
    p.act[1] = g.act[1];
    p.seeds = g.seeds;
    p.n_seeds = n_seeds;
    p.new_label = d->new_label;
    p.ctl = g.ctl;

    int32_t ctl[GROW_CTL_WORDS];
    ctl_start(ctl, GROW_CTL_WORDS, GROW_MIN_X, dims);
    HIP_TRY(hipMemcpyAsync(g.ctl, ctl, sizeof(ctl), hipMemcpyHostToDevice, r->stream));
    if (n_seeds > 0) HIP_TRY(hipMemcpyAsync(g.seeds, seeds_xyz, (size_t) n_seeds * 3 * sizeof(int32_t), hipMemcpyHostToDevice, r->stream));
    HIP_TRY(launch_grow_candidates(p, r->stream));
    HIP_TRY(launch_grow_seeds(p, r->stream));

    // The passes. The first counts as a change whatever it does, every later one that changes a brick moves at least one more of the
    // box's voxels into the region (the seeds' are there already), and the pass after the last change changes nothing: box_voxels + 1
    // passes always hold a pass without a change. None among that many is a defect, reported instead of looped on.
    uint64_t passes = 0, visits = 0;
    if (n_seeds > 0) {
        const int batch = std::min(std::max(tune(TUNE_GROW_BATCH), 1), kGrowMaxBatch);
        int32_t changed[kGrowMaxBatch];
        uint64_t enqueued = 0;
        for (bool done = false; !done;) {
            if (enqueued >= box_voxels + 1) return fail(TBRM_ERR_NO_DEVICE, "region growing did not reach its fixed point within %llu passes", (unsigned long long) enqueued);
            if (enqueued) HIP_TRY(hipMemsetAsync(g.ctl + GROW_CHANGED, 0, (size_t) kGrowMaxBatch * sizeof(int32_t), r->stream));
            for (int i = 0; i < batch; ++i, ++enqueued) {
                p.first_pass = enqueued == 0;
                p.changed_word = GROW_CHANGED + i;
                p.act[0] = g.act[enqueued & 1];
                p.act[1] = g.act[(enqueued + 1) & 1];
                HIP_TRY(launch_grow_pass(p, r->stream));
            }
            HIP_TRY(hipMemcpyAsync(changed, g.ctl + GROW_CHANGED, (size_t) batch * sizeof(int32_t), hipMemcpyDeviceToHost, r->stream));
            HIP_TRY(hipStreamSynchronize(r->stream));
            for (int i = 0; i < batch && !done; ++i) {
                if (changed[i] == 0) done = true;
                else ++passes;
            }
        }
    }
    HIP_TRY(launch_grow_measure(p, r->stream));
    HIP_TRY(hipMemcpyAsync(ctl, g.ctl, GROW_CHANGED * sizeof(int32_t), hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    visits = (uint32_t) ctl[GROW_VISITS];

    memset(out, 0, sizeof(*out));
    out->voxels = (uint32_t) ctl[GROW_VOXELS];
    for (int c = 0; c < 3; ++c) { out->bbox_min[c] = ctl[GROW_MIN_X + c]; out->bbox_max[c] = ctl[GROW_MAX_X + c]; }
    out->passes = (int32_t) passes;
    out->seeds_taken = ctl[GROW_SEEDS_TAKEN];
    out->lo_used = lo;
    out->hi_used = hi;
    ++r->grow_counters[0];
    r->grow_counters[1] += passes;
    r->grow_counters[2] += visits;

    if (writes && out->voxels > 0) {
        BrickRange w; // the bricks the bounding box touches
        int wb1[3];
        bbox_bricks(out->bbox_min, out->bbox_max, w.b0, wb1);
        for (int c = 0; c < 3; ++c) w.nb[c] = wb1[c] - w.b0[c];
        HIP_TRY(launch_grow_write(p, w, r->stream));
        HIP_TRY(hipMemcpyAsync(ctl, g.ctl, GROW_CHANGED * sizeof(int32_t), hipMemcpyDeviceToHost, r->stream));
        if (int e = labels_changed(r, out->bbox_min, out->bbox_max)) return e; // (refresh_live waits for the stream: ctl has arrived)
        out->relabelled = (uint32_t) ctl[GROW_RELABELLED];
        r->grow_counters[3] += (uint32_t) ctl[GROW_BRICKS_WRITTEN];
    }
    return TBRM_OK;
}

} // extern "C"
