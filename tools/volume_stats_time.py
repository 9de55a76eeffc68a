#!/usr/bin/env python3
"""What the volume statistics (include/tbrm_volume_stats.h) cost, on config 3's volume (512^3 UNORM16), once on uniformly random
voxels and once on a spike volume with 90 % of the voxels at one code (most of a CT is air):
  hist_256 / hist_4096   the whole-volume histogram at 256 and 4096 bins,
  hist_box64             a 64^3 box at the unaligned origin (203, 131, 77), 256 bins,
  hist_masked            the histogram of the voxels of two of four labels, 256 bins (reads the label volume too),
  label_stats            the per-label statistics with that label volume,
each as wall_ms (host wall time of the host form: enqueue, kernel, read-back) and gpu_ms (HIP events round the device form, or round
the host form's launch where there is no device form), with GBps = the bytes the kernel must read / gpu_ms, and, from the same run,
the only other route to the same numbers: download_volume_region of the whole volume plus np.bincount (download_ms, bincount_ms).
Every figure is the median of --reps repetitions after one that is thrown away. Reports the spike-to-uniform ratio of gpu_ms and
the speed-up of hist_256's wall_ms over the download route. Prints one JSON line.

    python tools/volume_stats_time.py [--reps 7]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch

    from tbraymarcherplugin_amd import abi, synthetic as S

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--n", type=int, default=0, help="volume edge (default: config 3's)")
    args = ap.parse_args()
    cfg = S.CONFIGS[3]
    n = args.n or cfg["n"]
    dims = (n, n, n)
    dtype = np.dtype(cfg["dtype"])
    assert dtype == np.uint16
    device = torch.device("cuda", 0)
    rng = np.random.default_rng(0x5EED0003)
    labels = np.zeros((n, n, n), dtype=np.uint8)   # four segments: octants of the lower half, background above
    labels[:n // 2, :n // 2, :n // 2] = 1
    labels[:n // 2, n // 2:, :n // 2] = 2
    labels[:n // 2, :, n // 2:] = 3
    origin, edge = (203 * n // 512, 131 * n // 512, 77 * n // 512), max(n // 8, 1)

    def median_ms(fn, sync):
        out = []
        for k in range(args.reps + 1):
            t0 = time.perf_counter()
            fn()
            sync()
            if k:
                out.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(out))

    def gpu_ms(fn):
        out = []
        for k in range(args.reps + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn()
            b.record(stream)
            b.synchronize()
            if k:
                out.append(a.elapsed_time(b))
        return float(np.median(out))

    results = {}
    for kind in ("uniform", "spike"):
        vol = rng.integers(0, 65536, size=(n, n, n), dtype=np.uint16)
        if kind == "spike":
            vol[rng.random((n, n, n), dtype=np.float32) < 0.9] = 1000
        res = abi.Resources(dims, abi.DTYPE_FMT[dtype], cfg["light_32bit"], False, 0)
        res.upload_volume(vol)
        res.upload_label_volume(labels)
        res.reserve(1)
        stream = torch.cuda.ExternalStream(res.stream(), device=device)
        buf = torch.zeros(4096 + 4, dtype=torch.int32, device=device)
        torch.cuda.synchronize()
        vox, box_vox = n ** 3, edge ** 3
        # bytes a kernel must read: the bricks the box touches (2 bytes a voxel, + 1 with labels)
        touched = 1
        for c in range(3):
            touched *= ((origin[c] + edge - 1) // 8 - origin[c] // 8 + 1) * 8
        cases = {
            "hist_256": (dict(n_bins=256, lo=0, hi=65535), 2 * vox),
            "hist_4096": (dict(n_bins=4096, lo=0, hi=65535), 2 * vox),
            "hist_box64": (dict(n_bins=256, lo=0, hi=65535, origin=origin, extent=(edge, edge, edge)), 2 * touched),
            "hist_masked": (dict(n_bins=256, lo=0, hi=65535, labels=[1, 3]), 3 * vox),
        }
        r = {}
        for name, (kw, nbytes) in cases.items():
            g = gpu_ms(lambda: res.volume_histogram_device(buf.data_ptr(), **kw))
            w = median_ms(lambda: res.volume_histogram(**kw), lambda: None)
            r[name] = {"wall_ms": round(w, 4), "gpu_ms": round(g, 4), "GBps": round(nbytes / (g * 1e-3) / 1e9, 1)}
        g = gpu_ms(lambda: res.label_statistics())   # (no device form: the events bracket the host form, read-back included)
        w = median_ms(lambda: res.label_statistics(), lambda: None)
        r["label_stats"] = {"wall_ms": round(w, 4), "gpu_ms": round(g, 4), "GBps": round(3 * vox / (g * 1e-3) / 1e9, 1)}
        # the route without this header: the whole volume to the host, counted there
        box = {}

        def download():
            box["v"] = res.download_volume_region((0, 0, 0), dims)

        r["download_ms"] = round(median_ms(download, lambda: None), 3)
        r["bincount_ms"] = round(median_ms(lambda: np.bincount(box["v"].reshape(-1) >> 8, minlength=256), lambda: None), 3)
        counts, _ = res.volume_histogram(256, 0, 65535)
        assert np.array_equal(counts, np.bincount(box["v"].reshape(-1) >> 8, minlength=256))
        r["speedup_over_download"] = round((r["download_ms"] + r["bincount_ms"]) / r["hist_256"]["wall_ms"], 1)
        r["counters"] = res.volume_stats_counters()
        results[kind] = r
        res.close()
    ratio = {k: round(results["spike"][k]["gpu_ms"] / results["uniform"][k]["gpu_ms"], 2)
             for k in ("hist_256", "hist_4096", "hist_box64", "hist_masked", "label_stats")}
    print(json.dumps({"tool": "volume_stats_time", "workload": f"{n}^3 uint16, four labels; box {edge}^3 at {list(origin)}",
                      "reps": args.reps, **results, "spike_to_uniform_gpu_ms": ratio}), flush=True)


if __name__ == "__main__":
    main()
