// tbrm_api_islands.cpp — the islands of a label (include/tbrm_islands.h): validation (tbrm_islands_rule.h), the scratch
// and the counters around the kernels of tbrm_islands_kernels.hip.
//
// A call is: the set's boards and the bricks' own components (k_islands_local), the scan of the local counts (read back: the slot
// tables are sized from it), the slots, the merge across brick faces, the roots (read back: the sort is sized from it), the order,
// the rule, and — a writing call, or one that wants the table's labels — the pass over the set's voxels (k_islands_write); behind a
// write that changed a byte what every label write ends with (labels_changed). Nothing on the data side is touched, nothing waits for the occlusion stream.
#include "tbrm_resources.h"
#include "tbrm_islands_kernels.h"
#include "../../include/tbrm_islands.h"

#include <cstring>
#include <vector>

using namespace tbrm;
using namespace tbrm_host;

static_assert(TBRM_ISLANDS_MEASURE == kIslandsMeasure && TBRM_ISLAND_KEPT == kIslandKept && TBRM_ISLAND_BORDER == kIslandBorder,
              "tbrm_islands_rule.h restates the header's constants");

namespace {

// one of the handle's three scratch buffers, at least `bytes` large: a call that needs no more than an earlier one allocates nothing
int ensure_islands_scratch(tbrm_resources* r, int which, size_t bytes)
{
    if (r->islands_bytes[which] >= bytes) return TBRM_OK;
    HIP_TRY(hipStreamSynchronize(r->stream));
    if (r->d_islands[which]) HIP_TRY(hipFree(r->d_islands[which]));
    r->d_islands[which] = nullptr;
    r->islands_bytes[which] = 0;
    HIP_TRY(hipMalloc((void**) &r->d_islands[which], bytes));
    r->islands_bytes[which] = bytes;
    ++r->islands_counters[5];
    return TBRM_OK;
}

void carve_bricks(IslandsParams& p, Carver& c)
{
    const size_t nb = p.nbox, tiles = (nb + kIslandsTile - 1) / kIslandsTile;
    p.ctl = c.take<int32_t>(ISL_CTL_WORDS);
    p.boards = c.take<uint64_t>(nb * 8);
    p.lid = c.take<uint8_t>(nb * 512);
    p.cnt = c.take<uint32_t>(nb);
    p.base = c.take<uint32_t>(nb);
    p.tile_sum = c.take<uint32_t>(tiles);
    p.tile_base = c.take<uint32_t>(tiles);
}

void carve_slots(IslandsParams& p, Carver& c)
{
    const size_t n = p.total;
    p.parent = c.take<uint32_t>(n);
    p.root = c.take<uint32_t>(n);
    p.size = c.take<uint32_t>(n);
    p.first = c.take<uint32_t>(n);
    p.border = c.take<uint32_t>(n);
    p.rank = c.take<uint32_t>(n);
    p.act = c.take<int32_t>(n);
    p.keys_in = c.take<uint64_t>(n);
    p.vals_in = c.take<uint32_t>(n);
}

void* carve_islands(IslandsParams& p, Carver& c, size_t sort_bytes)
{
    p.keys_out = c.take<uint64_t>(p.n_roots);
    p.vals_out = c.take<uint32_t>(p.n_roots);
    p.table = c.take<IslandsEntry>(p.table_cap);
    return c.take<char>(sort_bytes);
}

} // namespace

extern "C" {

int tbrm_islands_abi_version(void) { return TBRM_ISLANDS_ABI_VERSION; }

int tbrm_islands_counters(const tbrm_resources* r, uint64_t out[6])
{
    if (!r || !out) return fail(TBRM_ERR_INVALID_ARG, "null argument");
    for (int k = 0; k < 6; ++k) out[k] = r->islands_counters[k];
    out[4] = (uint64_t) (r->islands_bytes[0] + r->islands_bytes[1] + r->islands_bytes[2]);
    return TBRM_OK;
}

int tbrm_label_islands(tbrm_resources* r, const tbrm_islands_desc* d, tbrm_island* table, int32_t capacity, tbrm_islands_result* out)
{
    if (!r || !d || !out) return fail(TBRM_ERR_INVALID_ARG, "null argument");
    if (capacity < 0) return fail(TBRM_ERR_INVALID_ARG, "table capacity %d: must be >= 0", (int) capacity);
    if (capacity > 0 && !table) return fail(TBRM_ERR_INVALID_ARG, "null table with capacity %d", (int) capacity);
    if (int e = refuse_resident(r)) return e;
    const tbrm_resources::Dims dims = r->data_dims();
    IslandsParams p{};
    for (int c = 0; c < 3; ++c) p.dims[c] = dims[c];
    if (const char* what = islands_validate(p.dims, d->origin, d->extent, d->connectivity, d->max_islands, d->keep_label, d->label_step, d->drop_label,
                                            d->spare_border, d->flags, d->reserved, p.box.origin, p.box.end))
        return fail(TBRM_ERR_INVALID_ARG, "%s (connectivity %d, max_islands %d, keep_label %d, label_step %d, drop_label %d, spare_border %d, flags %u, reserved %u, box %d %d %d + %d %d %d in %d %d %d)",
                    what, (int) d->connectivity, (int) d->max_islands, (int) d->keep_label, (int) d->label_step, (int) d->drop_label, (int) d->spare_border,
                    (unsigned) d->flags, (unsigned) d->reserved, (int) d->origin[0], (int) d->origin[1], (int) d->origin[2], (int) d->extent[0], (int) d->extent[1],
                    (int) d->extent[2], dims[0], dims[1], dims[2]);
    if (int e = begin_label_edit(r, "no label volume")) return e;
    if ((uint64_t) dims[0] * (uint64_t) dims[1] * (uint64_t) dims[2] >= (1ull << 32))
        return fail(TBRM_ERR_UNSUPPORTED, "a volume of 2^32 voxels or more: an island's size and first voxel are 32-bit sort keys");

    const bool measure = (d->flags & TBRM_ISLANDS_MEASURE) != 0;
    p.labels = r->d_labels;
    p.bnx = r->dbn[0];
    p.bnxy = r->dbn[0] * r->dbn[1];
    for (int c = 0; c < 3; ++c) axis_bricks(p.box.origin[c], p.box.end[c], p.range.b0[c], p.range.nb[c]);
    p.nbox = (uint32_t) range_bricks(p.range); // (fewer than 2^32 voxels: fewer than 2^23 bricks)
    for (int w = 0; w < 8; ++w) p.source[w] = d->source[w];
    p.conn26 = d->connectivity == 26;
    p.spare = d->spare_border;
    p.write = !measure;
    p.rule.min_voxels = d->min_voxels;
    p.rule.max_islands = d->max_islands;
    p.rule.keep_label = d->keep_label;
    p.rule.label_step = d->label_step;
    p.rule.drop_label = d->drop_label;

    {
        Carver size{nullptr};
        carve_bricks(p, size);
        if (int e = ensure_islands_scratch(r, 0, size.off)) return e;
        Carver at{r->d_islands[0]};
        carve_bricks(p, at);
    }
    int32_t ctl[ISL_CTL_WORDS];
    ctl_start(ctl, ISL_CTL_WORDS, ISL_MIN_X, dims);
    HIP_TRY(hipMemcpyAsync(p.ctl, ctl, sizeof(ctl), hipMemcpyHostToDevice, r->stream));
    HIP_TRY(launch_islands_local(p, r->stream));
    HIP_TRY(launch_islands_scan(p, r->stream));
    HIP_TRY(hipMemcpyAsync(ctl, p.ctl, sizeof(ctl), hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    p.total = (uint32_t) ctl[ISL_TOTAL];

    std::vector<IslandsEntry> entries;
    if (p.total > 0) {
        {
            Carver size{nullptr};
            carve_slots(p, size);
            if (int e = ensure_islands_scratch(r, 1, size.off)) return e;
            Carver at{r->d_islands[1]};
            carve_slots(p, at);
        }
        HIP_TRY(launch_islands_slots(p, r->stream));
        HIP_TRY(launch_islands_merge(p, r->stream));
        HIP_TRY(launch_islands_flatten(p, r->stream));
        HIP_TRY(hipMemcpyAsync(ctl, p.ctl, sizeof(ctl), hipMemcpyDeviceToHost, r->stream));
        HIP_TRY(hipStreamSynchronize(r->stream));
        p.n_roots = (uint32_t) ctl[ISL_ROOTS];
        p.table_cap = (uint32_t) capacity < p.n_roots ? (uint32_t) capacity : p.n_roots;
        if (p.n_roots > 0) {
            size_t sort_bytes = 0;
            HIP_TRY(islands_sort_bytes(p.n_roots, &sort_bytes));
            Carver size{nullptr};
            carve_islands(p, size, sort_bytes);
            if (int e = ensure_islands_scratch(r, 2, size.off)) return e;
            Carver at{r->d_islands[2]};
            void* const temp = carve_islands(p, at, sort_bytes);
            HIP_TRY(launch_islands_sort(p, temp, sort_bytes, r->stream));
            HIP_TRY(launch_islands_rule(p, r->stream));
        }
        if (p.write || p.table_cap > 0) HIP_TRY(launch_islands_write(p, r->stream)); // (measuring: only the table's labels)
        HIP_TRY(hipMemcpyAsync(ctl, p.ctl, sizeof(ctl), hipMemcpyDeviceToHost, r->stream));
        if (p.table_cap > 0) {
            entries.resize(p.table_cap);
            HIP_TRY(hipMemcpyAsync(entries.data(), p.table, (size_t) p.table_cap * sizeof(IslandsEntry), hipMemcpyDeviceToHost, r->stream));
        }
        HIP_TRY(hipStreamSynchronize(r->stream));
    }

    uint64_t counts[ISL_CTL_COUNTS];
    memcpy(counts, ctl, sizeof(counts));
    memset(out, 0, sizeof(*out));
    out->set_voxels = counts[ISL_SET_VOXELS];
    out->islands = p.n_roots;
    out->spared = (uint32_t) ctl[ISL_SPARED];
    out->kept = counts[ISL_KEPT];
    out->dropped = counts[ISL_DROPPED];
    out->kept_voxels = counts[ISL_KEPT_VOXELS];
    out->dropped_voxels = counts[ISL_DROPPED_VOXELS];
    out->largest = (uint32_t) ctl[ISL_LARGEST];
    out->relabelled = counts[ISL_RELABELLED];
    for (int c = 0; c < 3; ++c) { out->bbox_min[c] = ctl[ISL_MIN_X + c]; out->bbox_max[c] = ctl[ISL_MAX_X + c]; }
    out->table_entries = (int32_t) p.table_cap;
    for (uint32_t i = 0; i < p.table_cap; ++i) {
        const IslandsEntry& e = entries[i];
        tbrm_island& t = table[i];
        memset(&t, 0, sizeof(t));
        t.voxels = e.voxels;
        t.first[0] = (int32_t) (e.first % (uint32_t) dims[0]);
        t.first[1] = (int32_t) ((e.first / (uint32_t) dims[0]) % (uint32_t) dims[1]);
        t.first[2] = (int32_t) (e.first / (uint32_t) dims[0] / (uint32_t) dims[1]);
        t.label = (!measure && e.label >= 0) ? e.label : (e.lo == e.hi ? (int32_t) e.lo : -1);
        t.flags = e.flags;
    }
    ++r->islands_counters[0];
    r->islands_counters[1] += out->islands + out->spared;
    r->islands_counters[2] += counts[ISL_BRICKS_WRITTEN];
    r->islands_counters[3] += p.total;

    if (!measure) return labels_changed(r, out->bbox_min, out->bbox_max); // (no byte changed: nothing to do)
    return TBRM_OK;
}

} // extern "C"
