#!/usr/bin/env python3
"""What smoothing a label (include/tbrm_smooth.h) costs, on config 3's volume — 512^3 UNORM16 — and the label that
tools/region_grow_time.py's grow produces there (the window's span in codes, grown from the voxel under the image centre), against the
nearest existing operator and against the route it replaces, in the same process:
  median1 / median2 / median3 / median8 / median16, ..x3
                                 host wall time of one writing tbrm_smooth_labels call (complete on return) on label 1, whole volume,
                                 the median (1 / 2) at radius r on all three axes, 1 and 3 iterations, at the default smooth_skip (1);
  median_2mm                     the same with the radii of tbrm_host_smooth_radii for 0.7 x 0.7 x 2.5 mm voxels and 2 mm;
  .._noskip                      the same cases at smooth_skip = 0: every brick of the range computed;
  close1_c26 / close2_c26 ..     tbrm_morph_labels' closing by as many unit steps of the cube: the operator that shares the load, the
                                 write and labels_changed with it;
  transfers                      tbrm_download_label_volume plus tbrm_update_label_region of the bounding box of what median2 moved:
                                 what a host that runs its own median filter moves, with NOTHING charged for the filter.
Every timed call starts from the same label volume (uploaded again before it, outside the timed span). A round takes the cases one after
the other, --reps rounds follow one that is thrown away, and the report is the median over the rounds with the smallest and the largest
round (the spread). Bricks computed come from tbrm_smooth_counters [2]; bricks skipped are the rest of bricks x passes. Prints one
JSON line, and with --table FILE writes the table of DESIGN.md §19.

    python tools/label_smooth_time.py [--reps 7] [--n 512] [--table profiles/r16_label_smooth.txt]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RADII = (1, 2, 3, 8, 16)
ITERATIONS = (1, 3)
SPACING_MM, RADIUS_MM = (0.7, 0.7, 2.5), 2.0


def main():
    import torch

    from tbraymarcherplugin_amd import abi, synthetic as S

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--n", type=int, default=0, help="volume edge (default: config 3's)")
    ap.add_argument("--table", default="", help="write the text table here")
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
    labels = res.download_label_volume()
    bricks = ((n + 7) // 8) ** 3

    mm = abi.smooth_radii(SPACING_MM, RADIUS_MM)
    medians = [(f"median{r}" + ("" if k == 1 else f"x{k}"), (r, r, r), k) for r in RADII for k in ITERATIONS] + [("median_2mm", mm, 1)]
    variants = [(name, radius, k, 1) for name, radius, k in medians] + [(name + "_noskip", radius, k, 0) for name, radius, k in medians]
    morphs = [(f"close{r}_c26", r) for r in RADII]
    info = {}
    for name, radius, k, skip in variants:   # what each case does, outside the timing
        abi.set_tunable("smooth_skip", skip)
        res.upload_label_volume(labels)
        c0 = res.smooth_counters()
        got = res.smooth_labels(radius, [1], 1, iterations=k)
        c1 = res.smooth_counters()
        computed = c1["bricks_computed"] - c0["bricks_computed"]
        info[name] = dict(added=got["added"], removed=got["removed"], launches=got["launches"], radius=list(radius), reach=list(got["reach"]), computed=computed,
                          skipped=bricks * got["launches"] - computed, bricks_written=c1["bricks_written"] - c0["bricks_written"],
                          bbox=[list(got["bbox_min"]), list(got["bbox_max"])])
    abi.set_tunable("smooth_skip", 1)
    for name, r in morphs:
        res.upload_label_volume(labels)
        got = res.morph_labels("close", r, [1], 1, 26)
        info[name] = dict(added=got["added"], removed=got["removed"], launches=got["launches"])
    bmin, bmax = info["median2"]["bbox"]
    extent = [b - a + 1 for a, b in zip(bmin, bmax)]
    box_labels = np.ones(extent[::-1], dtype=np.uint8)

    def transfers():
        res.download_label_volume()
        res.update_label_region(bmin, box_labels)

    cases = {"transfers": (transfers, 1)}
    for name, radius, k, skip in variants:
        cases[name] = ((lambda radius=radius, k=k: res.smooth_labels(radius, [1], 1, iterations=k)), skip)
    for name, r in morphs:
        cases[name] = ((lambda r=r: res.morph_labels("close", r, [1], 1, 26)), 1)
    rounds = {k: [] for k in cases}
    for r in range(args.reps + 1):
        for name, (fn, skip) in cases.items():
            abi.set_tunable("smooth_skip", skip)
            res.upload_label_volume(labels)   # every case starts from the grown label
            res.flush()
            t0 = time.perf_counter()
            fn()   # (every case is complete on return)
            if r:
                rounds[name].append((time.perf_counter() - t0) * 1e3)
    abi.set_tunable("smooth_skip", 1)
    out = {k: {"ms": round(float(np.median(v)), 3), "min_ms": round(float(min(v)), 3), "max_ms": round(float(max(v)), 3)} for k, v in rounds.items()}
    result = {"tool": "label_smooth_time", "workload": f"{n}^3 labels, label 1 = {grown['voxels']} voxels grown from {list(seed)} over codes {lo} .. {hi}",
              "reps": args.reps, **out, "cases": info, "bricks": bricks, "mm": {"spacing": SPACING_MM, "radius": RADIUS_MM, "radii": mm},
              "transfer_bytes": {"download": n ** 3, "upload": int(box_labels.size)}}
    print(json.dumps(result), flush=True)
    if args.table:
        with open(args.table, "w") as f:
            f.write(f"Label smoothing (median), {result['workload']}; {bricks} bricks; wall ms per call, median (min .. max) of {args.reps} rounds\n")
            f.write(f"median_2mm: spacing {SPACING_MM} mm, radius {RADIUS_MM} mm -> radii {mm}\n")
            for name, _, _, skip in variants:
                o, i = out[name], info[name]
                f.write(f"  {name:20s} smooth_skip {skip}: {o['ms']:8.3f} ({o['min_ms']:.3f} .. {o['max_ms']:.3f})  radius {i['radius']}, {i['launches']} launches, bricks {i['computed']} computed / "
                        f"{i['skipped']} skipped, +{i['added']} -{i['removed']} voxels, {i['bricks_written']} bricks written\n")
            f.write("tbrm_morph_labels, closing by as many unit steps of the cube (connectivity 26), morph_steps 8:\n")
            for name, _ in morphs:
                o, i = out[name], info[name]
                f.write(f"  {name:20s} {o['ms']:8.3f} ({o['min_ms']:.3f} .. {o['max_ms']:.3f})  {i['launches']} launches, +{i['added']} -{i['removed']} voxels\n")
            o = out["transfers"]
            f.write(f"transfers alone (download {n ** 3} bytes, upload {box_labels.size} bytes, no filter): {o['ms']:8.3f} ({o['min_ms']:.3f} .. {o['max_ms']:.3f})\n")
    res.close()


if __name__ == "__main__":
    main()
