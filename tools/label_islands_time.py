#!/usr/bin/env python3
"""What the islands of a label (include/tbrm_islands.h) cost, on config 3's volume — 512^3 UNORM16 — with two labels there: the one
tools/region_grow_time.py's grow produces (the window's span in codes, grown 6-connected from the voxel under the image centre: one
island with holes) and the thresholded one (the same range with no seeds: the body plus its specks), against the route it replaces, in
the same process:
  keep1 / remove64 / split16 / fill    host wall time of one writing tbrm_label_islands call (complete on return), whole volume,
                                       6-connected, on the thresholded label (fill: on the grown label, holes of any size);
  keep1_c26                            the same at 26-connectivity;
  measure                              a measuring call with no table: everything but the pass over the voxels;
  transfers                            tbrm_download_label_volume plus tbrm_update_label_region of the bounding box of what keep1
                                       changed: what a host that labels on its own CPU moves, with NOTHING charged for its labelling;
  scipy (its own line)                 scipy.ndimage.label of the same mask on the host, once.
Every timed call starts from the same label volume (uploaded again before it, outside the timed span). A round takes the cases one after
the other, --reps rounds follow one that is thrown away, and the report is the median over the rounds with the smallest and the largest
round (the spread). Prints one JSON line, and with --table FILE writes the table of DESIGN.md §16.

    python tools/label_islands_time.py [--reps 7] [--n 512] [--table profiles/r12_label_islands.txt]
"""
import argparse
import json
import math
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
    ap.add_argument("--table", default="", help="write the text table here")
    ap.add_argument("--no-scipy", action="store_true", help="leave the host labelling out")
    args = ap.parse_args()
    cfg = S.CONFIGS[3]
    n = args.n or cfg["n"]
    device = torch.device("cuda", 0)
    res = abi.Resources((n, n, n), abi.DTYPE_FMT[np.dtype(cfg["dtype"])], cfg["light_32bit"], False, 0)
    vol = S.make_volume_torch((n, n, n), cfg["dtype"], S.seed_for_config(3), device)
    torch.cuda.synchronize()
    res.upload_volume_device(vol.data_ptr(), vol.numel() * vol.element_size())
    del vol
    res.set_tf_lut(abi.color_curve_to_lut(S.tf_keys(cfg["tf"])))
    res.set_windowing(abi.WindowingParams(*cfg["window"]))
    center, width = cfg["window"][0], cfg["window"][1]
    lo, hi = math.ceil((center - width / 2) * 65535), math.floor((center + width / 2) * 65535)   # the window's span, in codes
    world = S.default_world()
    fb = cfg["fb"] * n // cfg["n"]
    cam, rp = S.default_camera(fb, fb), abi.RaymarchParams(float(cfg["steps"]) * n / cfg["n"], -1, True)
    hit, _, _ = res.pick(cam, fb // 2, fb // 2, rp, world, 0.5)
    assert hit["sample"] >= 0, "the image centre meets nothing"
    seed = abi.hit_voxel((n, n, n), hit)
    res.attach_empty_labels()
    grown = res.grow_region([seed], lo, hi, 1, 6)
    grown_labels = res.download_label_volume()
    res.upload_label_volume(np.zeros_like(grown_labels))
    thresholded = res.grow_region([], lo, hi, 1, 6)
    thresholded_labels = res.download_label_volume()

    # name: (the label volume it starts from, the call)
    variants = {
        "keep1": (thresholded_labels, lambda: res.keep_largest_islands(1, 1)),
        "keep1_c26": (thresholded_labels, lambda: res.keep_largest_islands(1, 1, connectivity=26)),
        "remove64": (thresholded_labels, lambda: res.remove_small_islands(1, 64)),
        "split16": (thresholded_labels, lambda: res.split_islands(1, 1, 16)),
        "fill": (grown_labels, lambda: res.fill_label_holes(1)),
        "measure": (thresholded_labels, lambda: res.label_islands([1], 6, measure=True)),
    }
    info = {}
    for name, (start, call) in variants.items():   # what each case does, outside the timing
        res.upload_label_volume(start)
        c0 = res.islands_counters()
        got = call()
        c1 = res.islands_counters()
        info[name] = dict(islands=got["islands"], spared=got["spared"], kept=got["kept"], dropped=got["dropped"], set_voxels=got["set_voxels"],
                          largest=got["largest"], relabelled=got["relabelled"], local_components=c1["local_components"] - c0["local_components"],
                          bricks_written=c1["bricks_written"] - c0["bricks_written"], scratch_bytes=c1["scratch_bytes"],
                          bbox=[list(got["bbox_min"]), list(got["bbox_max"])])
    bmin, bmax = info["keep1"]["bbox"]
    extent = [b - a + 1 for a, b in zip(bmin, bmax)]
    box_labels = np.ones(extent[::-1], dtype=np.uint8)

    def transfers():
        res.download_label_volume()
        res.update_label_region(bmin, box_labels)

    cases = {"transfers": (thresholded_labels, transfers), **variants}
    rounds = {k: [] for k in cases}
    for r in range(args.reps + 1):
        for name, (start, fn) in cases.items():
            res.upload_label_volume(start)   # every case starts from the same label
            res.flush()
            t0 = time.perf_counter()
            fn()   # (every case is complete on return)
            if r:
                rounds[name].append((time.perf_counter() - t0) * 1e3)
    out = {k: {"ms": round(float(np.median(v)), 3), "min_ms": round(float(min(v)), 3), "max_ms": round(float(max(v)), 3)} for k, v in rounds.items()}
    host = None
    if not args.no_scipy:
        from scipy import ndimage
        mask = thresholded_labels == 1
        t0 = time.perf_counter()
        _, found = ndimage.label(mask)
        host = {"ms": round((time.perf_counter() - t0) * 1e3, 1), "islands": int(found)}
    result = {"tool": "label_islands_time",
              "workload": f"{n}^3 labels; grown: {grown['voxels']} voxels from {list(seed)} over codes {lo} .. {hi}; thresholded: {thresholded['voxels']} voxels",
              "reps": args.reps, **out, "cases": info, "scipy_label": host, "transfer_bytes": {"download": n ** 3, "upload": int(box_labels.size)}}
    print(json.dumps(result), flush=True)
    if args.table:
        with open(args.table, "w") as f:
            f.write(f"label islands, {result['workload']}; wall ms per call, median (min .. max) of {args.reps} rounds\n")
            for name in variants:
                o, i = out[name], info[name]
                f.write(f"  {name:10s} {o['ms']:8.3f} ({o['min_ms']:.3f} .. {o['max_ms']:.3f})  set {i['set_voxels']}, islands {i['islands']} (+{i['spared']} spared), largest {i['largest']}, "
                        f"kept {i['kept']}, dropped {i['dropped']}, {i['local_components']} local components, {i['relabelled']} bytes changed in {i['bricks_written']} bricks, "
                        f"scratch held {i['scratch_bytes']} bytes\n")
            o = out["transfers"]
            f.write(f"transfers alone (download {n ** 3} bytes, upload {box_labels.size} bytes, no labelling): {o['ms']:8.3f} ({o['min_ms']:.3f} .. {o['max_ms']:.3f})\n")
            if host:
                f.write(f"scipy.ndimage.label of the thresholded mask on the host, once: {host['ms']:.1f} ms, {host['islands']} islands\n")
    res.close()


if __name__ == "__main__":
    main()
