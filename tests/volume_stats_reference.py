"""A plain numpy restatement of include/tbrm_volume_stats.h: the binning rule (integer arithmetic for the codes, np.float32
operations for float data), the per-label statistics and the percentile window (Python floats). Volumes are [z, y, x] arrays, boxes
(origin, extent) in (x, y, z); no padding exists here — a dense array has none."""
import math

import numpy as np

TALLY = ("below", "above", "nan", "visited")


def box_view(a, origin=None, extent=None):
    if extent is None:
        return a
    (ox, oy, oz), (ex, ey, ez) = origin, extent
    return a[oz:oz + ez, oy:oy + ey, ox:ox + ex]


def bins_of_codes(codes, n_bins, lo, hi):
    """(bin per code or -1, class per code: 0 binned, 1 below, 2 above) by the UNORM rule, in unsigned 64-bit numpy integers (the
    products stay below 2^32: 65535 * 4096)"""
    c = np.asarray(codes).astype(np.uint64)
    lo, hi = int(lo), int(hi)
    cls = np.where(c < lo, 1, np.where(c > hi, 2, 0))
    safe = np.where(cls == 0, c, lo) - np.uint64(lo)
    assert int(safe.max(initial=0)) * n_bins < 2 ** 32
    b = (safe * np.uint64(n_bins)) // np.uint64(hi - lo + 1)
    return np.where(cls == 0, b.astype(np.int64), -1), cls


def bins_of_floats(values, n_bins, lo, hi):
    """the R32_FLOAT rule: every operation a float32 operation; class 3 is NaN"""
    v = np.asarray(values, dtype=np.float32)
    lo32, hi32 = np.float32(lo), np.float32(hi)
    with np.errstate(all="ignore"):
        scale = np.float32(np.float32(n_bins) / np.float32(hi32 - lo32))
        t = ((v - lo32).astype(np.float32) * scale).astype(np.float32)
        nan = v != v
        below = ~nan & (v < lo32)
        inside = ~nan & ~below & (t < np.float32(n_bins))
        last = ~nan & ~below & ~inside & (v <= hi32)
        b = np.full(v.shape, -1, dtype=np.int64)
        b[inside] = t[inside].astype(np.int32)   # truncation, as (int) t
        b[last] = n_bins - 1
    cls = np.where(nan, 3, np.where(below, 1, np.where(inside | last, 0, 2)))
    return b, cls


def histogram(vol, n_bins, lo, hi, origin=None, extent=None, labels_vol=None, labels=None):
    """(counts uint64[n_bins], tally dict) of tbrm_volume_histogram"""
    v = box_view(vol, origin, extent).reshape(-1)
    if labels is not None:
        keep = np.isin(box_view(labels_vol, origin, extent).reshape(-1), np.asarray(list(labels), dtype=np.int64))
        v = v[keep]
    b, cls = (bins_of_floats if v.dtype == np.float32 else bins_of_codes)(v, n_bins, lo, hi)
    counts = np.bincount(b[cls == 0], minlength=n_bins).astype(np.uint64)
    tally = {"below": int((cls == 1).sum()), "above": int((cls == 2).sum()), "nan": int((cls == 3).sum()), "visited": int(v.size)}
    return counts, tally


def label_statistics(vol, labels_vol=None, origin=None, extent=None):
    """per label 0 .. 255: dicts count, nan_count, sum (math.fsum for floats, exact for codes), min, max, abs_sum (sum of |v|), and
    for float data n = count - nan_count"""
    v = box_view(vol, origin, extent).reshape(-1)
    l = np.zeros(v.shape, dtype=np.uint8) if labels_vol is None else box_view(labels_vol, origin, extent).reshape(-1)
    out = []
    for label in range(256):
        mine = v[l == label]
        nan = mine != mine if mine.dtype == np.float32 else np.zeros(mine.shape, dtype=bool)
        real = mine[~nan]
        rec = {"count": int(mine.size), "nan_count": int(nan.sum()), "sum": 0.0, "min": math.inf, "max": -math.inf, "abs_sum": 0.0}
        if real.size:
            if real.dtype == np.float32 and not np.isfinite(real).all():
                # infinite voxels: +inf, -inf, or NaN when both signs occur, in any order of summation (math.fsum refuses these)
                signs = {float(x) for x in real[~np.isfinite(real)]}
                rec["sum"] = math.nan if len(signs) == 2 else signs.pop()
                rec["abs_sum"] = math.inf
            elif real.dtype == np.float32:
                rec["sum"] = math.fsum(float(x) for x in real)
                rec["abs_sum"] = math.fsum(abs(float(x)) for x in real)
            else:
                rec["sum"] = float(int(real.astype(np.uint64).sum()))
                rec["abs_sum"] = rec["sum"]
            rec["min"], rec["max"] = float(real.min()), float(real.max())
        out.append(rec)
    return out


def window_from_histogram(counts, lo_edge, hi_edge, p_low, p_high):
    """(center, width) as float32 values, or None where tbrm_host_window_from_histogram answers TBRM_ERR_INVALID_ARG"""
    counts = [int(c) for c in counts]
    n = len(counts)
    total = sum(counts)
    if n < 1 or total == 0 or not (0.0 <= p_low < p_high <= 1.0):
        return None
    if not (math.isfinite(lo_edge) and math.isfinite(hi_edge) and lo_edge < hi_edge):
        return None
    cum, k_lo, k_hi = 0, None, None
    for k, c in enumerate(counts):
        cum += c
        if k_lo is None and float(cum) > p_low * float(total):
            k_lo = k
        if k_hi is None and float(cum) >= p_high * float(total):
            k_hi = k
    w = (hi_edge - lo_edge) / float(n)
    lower, upper = lo_edge + float(k_lo) * w, lo_edge + float(k_hi + 1) * w
    return np.float32((lower + upper) / 2.0), np.float32(upper - lower)
