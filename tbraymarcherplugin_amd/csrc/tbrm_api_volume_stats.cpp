// tbrm_api_volume_stats.cpp — statistics of the data volume (include/tbrm_volume_stats.h): the value histogram, the per-label
// statistics (k_volume_histogram / k_label_statistics, tbrm_stats_kernels.hip) and the percentile window, which is host arithmetic.
//
// The calls read the bricked data volume, and the label volume, and write the handle's statistics scratch only: no generation
// moves, no cache or metadata is touched, nothing waits for the occlusion stream (it never writes either volume). The scratch —
// n_bins + 4 histogram words, then the 256 label records — is taken once (ensure_stats_scratch) and freed with the handle.
#include "tbrm_resources.h"
#include "tbrm_stats_divisor.h"
#include "../../include/tbrm_volume_stats.h"

#include <cmath>
#include <cstring>
#include <limits>

using namespace tbrm;
using namespace tbrm_host;

namespace {

constexpr size_t kHistWords = kStatsMaxBins + 4;
constexpr size_t kLabelOffsetWords = (kHistWords + 63) / 64 * 64; // (256-byte aligned: the sums are 8-byte words)
constexpr size_t kScratchWords = kLabelOffsetWords + kStatsLabelWords;

// what every statistics call checks about the handle
int stats_handle(const tbrm_resources* r)
{
    if (int e = refuse_resident(r)) return e;
    if (!r->has_volume) return fail(TBRM_ERR_NOT_INITIALIZED, "no volume: upload one with tbrm_upload_volume");
    return TBRM_OK;
}

// the box against the volume; an all-zero extent (or no box at all) is the whole volume
int stats_box(const tbrm_resources* r, const int32_t* origin, const int32_t* extent, StatsParams& p)
{
    const tbrm_resources::Dims dims = r->data_dims();
    const BoxVerdict v = box_resolve(dims, origin, extent, true, &p.box, &p.range);
    if (v.what != BOX_OK) return fail_box(v, true, dims, origin, extent);
    p.data = r->d_data;
    p.fmt = data_fmt(r);
    p.bnx = r->dbn[0];
    p.bnxy = r->dbn[0] * r->dbn[1];
    return TBRM_OK;
}

int histogram_params(const tbrm_resources* r, const tbrm_histogram_desc* d, StatsParams& p)
{
    if (d->n_bins < 1 || d->n_bins > kStatsMaxBins) return fail(TBRM_ERR_INVALID_ARG, "n_bins %d: must be 1 .. %d", (int) d->n_bins, kStatsMaxBins);
    if (int e = stats_box(r, d->origin, d->extent, p)) return e;
    p.n_bins = (uint32_t) d->n_bins;
    if (p.fmt == FMT_F32) {
        const float lo = (float) d->lo, hi = (float) d->hi;
        if (!std::isfinite(d->lo) || !std::isfinite(d->hi) || !std::isfinite(lo) || !std::isfinite(hi) || !(lo < hi))
            return fail(TBRM_ERR_INVALID_ARG, "histogram range [%g, %g]: needs lo < hi, both finite as float32", d->lo, d->hi);
        const float width = hi - lo; // (separate statements: no contraction, no wider intermediate)
        p.lo_f = lo;
        p.hi_f = hi;
        p.scale = (float) d->n_bins / width;
    } else {
        const double top = p.fmt == FMT_U8 ? 255.0 : 65535.0;
        if (!(d->lo >= 0.0 && d->lo <= d->hi && d->hi <= top) || d->lo != std::floor(d->lo) || d->hi != std::floor(d->hi))
            return fail(TBRM_ERR_INVALID_ARG, "histogram range [%g, %g]: needs integral codes with 0 <= lo <= hi <= %g", d->lo, d->hi, top);
        p.lo_code = (uint32_t) d->lo;
        p.hi_code = (uint32_t) d->hi;
        stats_divisor(p.hi_code - p.lo_code + 1, p.div_mul, p.div_shift);
    }
    uint32_t copies = 1; // as many LDS copies as fit, 16 at most
    while (copies < 16 && copies * 2 * p.n_bins <= (uint32_t) kStatsMaxBins) copies *= 2;
    p.copies = copies;
    if (d->use_label_mask) {
        if (!r->d_labels) return fail(TBRM_ERR_NOT_INITIALIZED, "use_label_mask without a label volume: upload one with tbrm_upload_label_volume");
        p.labels = r->d_labels;
        for (int w = 0; w < 8; ++w) p.mask[w] = d->label_mask[w];
    }
    return TBRM_OK;
}

// A few workgroups per compute unit, never more than the bricks need (four waves, a brick each at a time). What a workgroup
// flushes grows with the bins: two per unit above 1024 bins, four below. Tunable stats_groups caps the grid (a test hook: a wave
// then takes many bricks of a small volume).
int stats_grid(const tbrm_resources* r, const StatsParams& p, int per_cu)
{
    const uint64_t bricks = range_bricks(p.range);
    uint64_t groups = (uint64_t) std::max(r->n_cus, 1) * (uint64_t) per_cu;
    if (tune(TUNE_STATS_GROUPS) > 0) groups = std::min<uint64_t>(groups, (uint64_t) tune(TUNE_STATS_GROUPS));
    return (int) std::min<uint64_t>((bricks + 3) / 4, groups);
}

void count_bricks(tbrm_resources* r, const StatsParams& p)
{
    uint64_t whole = 1, all = 1;
    for (int c = 0; c < 3; ++c) { // along an axis the whole bricks are those with [8b, 8b + 8) inside [origin, end)
        const int first = (p.box.origin[c] + kBrick - 1) >> kBrickShift, last = p.box.end[c] >> kBrickShift; // [first, last)
        whole *= (uint64_t) std::max(last - first, 0);
        all *= (uint64_t) p.range.nb[c];
    }
    r->stats_counters[2] += whole;
    r->stats_counters[3] += all - whole;
}

int enqueue_histogram(tbrm_resources* r, const StatsParams& p)
{
    HIP_TRY(launch_volume_histogram(p, p.labels != nullptr, stats_grid(r, p, p.n_bins > 1024 ? 2 : 4), r->stream));
    ++r->stats_counters[0];
    count_bricks(r, p);
    return TBRM_OK;
}

double key_to_value(uint32_t key, int fmt)
{
    if (fmt != FMT_F32) return (double) key;
    const uint32_t bits = (key & 0x80000000u) ? key ^ 0x80000000u : ~key;
    float v;
    memcpy(&v, &bits, sizeof(v));
    return (double) v;
}

} // namespace

namespace tbrm_host {

int ensure_stats_scratch(tbrm_resources* r, bool counted)
{
    if (r->d_stats) return TBRM_OK;
    if (counted) count_alloc(r, 1, "volume statistics scratch");
    HIP_TRY(hipMalloc((void**) &r->d_stats, kScratchWords * sizeof(uint32_t)));
    r->stats_host.assign(kScratchWords, 0u);
    return TBRM_OK;
}

} // namespace tbrm_host

extern "C" {

int tbrm_volume_stats_abi_version(void) { return TBRM_VOLUME_STATS_ABI_VERSION; }

int tbrm_volume_histogram_device(tbrm_resources* r, const tbrm_histogram_desc* desc, uint32_t* device_counts)
{
    if (!r || !desc || !device_counts) return fail(TBRM_ERR_INVALID_ARG, "null argument");
    if (int e = stats_handle(r)) return e;
    StatsParams p{};
    if (int e = histogram_params(r, desc, p)) return e;
    if (int e = bind(r)) return e;
    if (int e = ensure_stats_scratch(r)) return e; // (part of the contract: a handle's first statistics call takes the scratch)
    p.out = device_counts;
    return enqueue_histogram(r, p);
}

int tbrm_volume_histogram(tbrm_resources* r, const tbrm_histogram_desc* desc, uint64_t* out_counts, uint64_t out_tally[4])
{
    if (!r || !desc || !out_counts || !out_tally) return fail(TBRM_ERR_INVALID_ARG, "null argument");
    if (int e = stats_handle(r)) return e;
    StatsParams p{};
    if (int e = histogram_params(r, desc, p)) return e;
    if (int e = bind(r)) return e;
    if (int e = ensure_stats_scratch(r)) return e;
    const size_t words = (size_t) p.n_bins + 4;
    p.out = r->d_stats;
    HIP_TRY(hipMemsetAsync(r->d_stats, 0, words * sizeof(uint32_t), r->stream));
    if (int e = enqueue_histogram(r, p)) return e;
    HIP_TRY(hipMemcpyAsync(r->stats_host.data(), r->d_stats, words * sizeof(uint32_t), hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    for (uint32_t b = 0; b < p.n_bins; ++b) out_counts[b] = r->stats_host[b];
    for (int k = 0; k < 4; ++k) out_tally[k] = r->stats_host[p.n_bins + k];
    return TBRM_OK;
}

int tbrm_label_statistics(tbrm_resources* r, const int32_t origin[3], const int32_t extent[3], tbrm_label_stat out[256])
{
    if (!r || !out || (origin == nullptr) != (extent == nullptr)) return fail(TBRM_ERR_INVALID_ARG, "null argument");
    if (int e = stats_handle(r)) return e;
    StatsParams p{};
    if (int e = stats_box(r, origin, extent, p)) return e;
    if (int e = bind(r)) return e;
    if (int e = ensure_stats_scratch(r)) return e;
    p.labels = r->d_labels;
    p.out = r->d_stats + kLabelOffsetWords;
    HIP_TRY(hipMemsetAsync(p.out, 0, kStatsLabelWords * sizeof(uint32_t), r->stream));
    HIP_TRY(launch_label_statistics(p, stats_grid(r, p, 4), r->stream));
    ++r->stats_counters[1];
    count_bricks(r, p);
    uint32_t* const h = r->stats_host.data() + kLabelOffsetWords;
    HIP_TRY(hipMemcpyAsync(h, p.out, kStatsLabelWords * sizeof(uint32_t), hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    for (int l = 0; l < 256; ++l) {
        tbrm_label_stat& s = out[l];
        s.count = h[l];
        s.nan_count = h[256 + l];
        s.sum = 0.0;
        s.min = std::numeric_limits<double>::infinity();
        s.max = -std::numeric_limits<double>::infinity();
        if (s.count == s.nan_count) continue;
        s.min = key_to_value(~h[512 + l], p.fmt);
        s.max = key_to_value(h[768 + l], p.fmt);
        if (p.fmt == FMT_F32) memcpy(&s.sum, h + 1024 + 2 * l, sizeof(double));
        else {
            uint64_t sum;
            memcpy(&sum, h + 1024 + 2 * l, sizeof(sum));
            s.sum = (double) sum;
        }
    }
    return TBRM_OK;
}

int tbrm_host_window_from_histogram(const uint64_t* counts, int32_t n_bins, double lo_edge, double hi_edge, double p_low, double p_high,
                                    tbrm_windowing_params* out)
{
    if (!counts || !out) return fail(TBRM_ERR_INVALID_ARG, "null argument");
    if (n_bins < 1) return fail(TBRM_ERR_INVALID_ARG, "n_bins %d: must be >= 1", (int) n_bins);
    if (!std::isfinite(lo_edge) || !std::isfinite(hi_edge) || !(lo_edge < hi_edge))
        return fail(TBRM_ERR_INVALID_ARG, "histogram edges [%g, %g): need finite lo_edge < hi_edge", lo_edge, hi_edge);
    if (!(p_low >= 0.0 && p_low < p_high && p_high <= 1.0)) return fail(TBRM_ERR_INVALID_ARG, "percentiles %g, %g: need 0 <= p_low < p_high <= 1", p_low, p_high);
    uint64_t total = 0;
    for (int32_t k = 0; k < n_bins; ++k) total += counts[k];
    if (total == 0) return fail(TBRM_ERR_INVALID_ARG, "empty histogram");
    const double want_lo = p_low * (double) total, want_hi = p_high * (double) total;
    int32_t k_lo = -1, k_hi = -1;
    uint64_t cum = 0;
    for (int32_t k = 0; k < n_bins; ++k) {
        cum += counts[k];
        if (k_lo < 0 && (double) cum > want_lo) k_lo = k;
        if (k_hi < 0 && (double) cum >= want_hi) k_hi = k;
    }
    if (k_lo < 0) k_lo = n_bins - 1; // (not reached: cum ends at total > p_low * total)
    if (k_hi < 0) k_hi = n_bins - 1; // (only by rounding of p_high * total above total)
    const double w = (hi_edge - lo_edge) / (double) n_bins;
    const double lower = lo_edge + (double) k_lo * w, upper = lo_edge + (double) (k_hi + 1) * w;
    out->center = (float) ((lower + upper) / 2.0);
    out->width = (float) (upper - lower);
    out->low_cutoff = 1;
    out->high_cutoff = 1;
    return TBRM_OK;
}

int tbrm_volume_stats_counters(const tbrm_resources* r, uint64_t out[4]) { return copy_counters(r, &tbrm_resources::stats_counters, out); }

} // extern "C"
