/* tbrm_volume_stats.h — statistics of the data volume computed where it lives (C-ABI, libtbrm.so): a value histogram of the whole
 * volume, of a box or of the voxels of some labels; per-label count / sum / min / max; and a percentile window proposed from a
 * histogram. A window or transfer-function editor and a segmentation tool need these every frame; the only other way to them is
 * tbrm_download_volume_region of the whole volume and counting on the host.
 *
 * Units. Everything is in the data format's STORED units: the integer codes 0 .. 255 / 0 .. 65535 for UNORM8 / UNORM16 (as
 * doubles where a double carries them), the float itself for R32_FLOAT. The zero padding of ragged edge bricks is not data: a
 * voxel counts only if it lies inside the volume and inside the box.
 *
 * The binning rule (tests hold it bit for bit; n = n_bins):
 *   UNORM8 / UNORM16   lo, hi integral codes, 0 <= lo <= hi <= 255 | 65535. code < lo: below; code > hi: above; else
 *                      bin = ((code - lo) * n) / (hi - lo + 1), unsigned 32-bit, floor division.
 *   R32_FLOAT          lo < hi, both finite after narrowing to float32 (done on the host); scale = (float) n / (hi - lo) in float32
 *                      on the host. NaN: nan. v < lo: below. Else t = (v - lo) * scale, two float32 operations, no fma;
 *                      t < n: bin = (int) t; else v <= hi: the last bin; else above.
 *
 * Semantics. The calls behave as the download calls do: they are enqueued on the handle's stream behind everything issued before;
 * the host forms return with the result on the host, tbrm_volume_histogram_device returns once enqueued. The host forms wait for the
 * stream once, as a download does; that wait is the call's own and no light operator's, so tbrm_path_counters [12] / [13] do not
 * count it. Nothing of the handle's
 * state changes (generations, caches, skipping metadata, light volume): the frame after a statistics call is bit-identical to the
 * frame before it. A small scratch (bins, tallies, 256 label records, 24 KiB) is taken by the handle's first statistics call, or by
 * tbrm_resources_reserve, and freed with the handle; after that no statistics call allocates.
 * Colour handles and handles with a label volume accept; slab-resident handles refuse (TBRM_ERR_UNSUPPORTED).
 * TBRM_ERR_INVALID_ARG: a null argument, a box that leaves the volume, an extent <= 0 that is not all-zero, n_bins out of range, a
 * bad lo / hi. TBRM_ERR_NOT_INITIALIZED: no volume uploaded, or use_label_mask without a label volume. */
#ifndef TBRM_VOLUME_STATS_H
#define TBRM_VOLUME_STATS_H

#include "tbrm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TBRM_VOLUME_STATS_ABI_VERSION 1
#define TBRM_HISTOGRAM_MAX_BINS 4096

typedef struct tbrm_histogram_desc {
    int32_t origin[3], extent[3];   /* dense box [origin, origin + extent) of the data volume; extent = {0,0,0}: the whole volume (origin is then ignored) */
    int32_t n_bins;                 /* 1 .. 4096 */
    int32_t use_label_mask;         /* 0: every voxel of the box; 1: only voxels whose label L has bit (label_mask[L>>5] >> (L&31)) & 1 */
    double  lo, hi;                 /* value range, in stored units */
    uint32_t label_mask[8];
} tbrm_histogram_desc;

typedef struct tbrm_label_stat {    /* stored units: codes for UNORM8/16 (as double), the float itself for R32_FLOAT */
    uint64_t count;                 /* voxels of the box with this label (NaN voxels included) */
    uint64_t nan_count;             /* R32_FLOAT only; else 0 */
    double sum, min, max;           /* over the non-NaN voxels; sum = 0, min = +inf, max = -inf when there are none. Infinite voxels
                                     * count: the sum is then that infinity, or NaN when both signs occur */
} tbrm_label_stat;

TBRM_API int tbrm_volume_stats_abi_version(void);
/* out_counts: n_bins words. out_tally: [0] below, [1] above, [2] nan, [3] voxels visited — the voxels of the box that pass the
 * label mask, = [0] + [1] + [2] + the sum of out_counts. */
TBRM_API int tbrm_volume_histogram(tbrm_resources* res, const tbrm_histogram_desc* desc, uint64_t* out_counts, uint64_t out_tally[4]);
/* The same into device memory: n_bins + 4 uint32 words (4-byte aligned), the bins and then the four tallies. The call ADDS to what
 * the words hold: the caller zeroes them (once, for a histogram over several boxes or several calls). Counts fit 32 bits: a
 * volume has fewer than 2^32 voxels; sums over several calls are the caller's to keep below that. */
TBRM_API int tbrm_volume_histogram_device(tbrm_resources* res, const tbrm_histogram_desc* desc, uint32_t* device_counts);
/* Per label 0 .. 255 over the box (origin and extent both NULL, or an all-zero extent: the whole volume). Without a label volume
 * every voxel has label 0: out[0] is the volume's global count / sum / min / max. Integer formats: every field is exact and
 * deterministic (a sum of codes is below 2^53). R32_FLOAT: count, nan_count, min, max are exact; sum is accumulated in float64 in
 * an order that is not fixed, so it need not be bitwise reproducible from run to run. */
TBRM_API int tbrm_label_statistics(tbrm_resources* res, const int32_t origin[3], const int32_t extent[3], tbrm_label_stat out[256]);
/* Pure host code, double precision: a window from the percentiles p_low < p_high of a histogram whose n_bins equal bins span
 * [lo_edge, hi_edge), in the WINDOW's units (normalised value code / (2^n - 1) for UNORM data: the caller converts; the bins of a
 * full-range UNORM histogram span [0, (max_code + 1) / max_code)). With total = sum of counts and cum_k = counts_0 + .. + counts_k:
 * k_lo = the smallest k with cum_k > p_low * total, k_hi = the smallest k with cum_k >= p_high * total, w = (hi_edge - lo_edge) / n_bins,
 * lower = lo_edge + k_lo * w, upper = lo_edge + (k_hi + 1) * w; center = (lower + upper) / 2 and width = upper - lower, narrowed to
 * float; both cut-offs are set. TBRM_ERR_INVALID_ARG: a null argument, total == 0, not 0 <= p_low < p_high <= 1, n_bins < 1, edges
 * that are not finite with lo_edge < hi_edge. */
TBRM_API int tbrm_host_window_from_histogram(const uint64_t* counts, int32_t n_bins, double lo_edge, double hi_edge,
                                             double p_low, double p_high, tbrm_windowing_params* out);
/* Cumulative per handle: [0] histogram calls, [1] label-statistics calls, [2] bricks taken on the whole-brick path (inside the box
 * and the volume on all three axes: no per-voxel tests), [3] bricks taken on the cut path (cut by the box or by the volume's ragged edge). */
TBRM_API int tbrm_volume_stats_counters(const tbrm_resources* res, uint64_t out[4]);

#ifdef __cplusplus
}
#endif
#endif /* TBRM_VOLUME_STATS_H */
