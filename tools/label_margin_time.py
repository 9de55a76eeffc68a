#!/usr/bin/env python3
"""What the Euclidean margins of labels (include/tbrm_margin.h) cost, on config 3's volume — 512^3 UNORM16 — and the label that
tools/region_grow_time.py's grow produces there (the window's span in codes, grown from the voxel under the image centre), against the
unit-step morphology at the same radius and against the route they replace, in the same process:
  expand2 / expand5 / expand16, shrink.., close..
                                 host wall time of one writing tbrm_margin_labels call (complete on return) on label 1, whole volume,
                                 isotropic weights, limit = reach^2, at the default margin_skip (1);
  expand_5mm                     the same with the weights of tbrm_host_margin_weights for 0.7 x 0.7 x 2.5 mm voxels and 5 mm;
  .._noskip                      the same cases at margin_skip = 0: every brick of the range computed;
  dilate2_c6 / dilate2_c26 ..    tbrm_morph_labels' dilation by as many unit steps (octahedron and cube), for comparison;
  transfers                      tbrm_download_label_volume plus tbrm_update_label_region of the bounding box of what expand5 moved:
                                 what a host that runs its own distance transform moves, with NOTHING charged for the transform.
Every timed call starts from the same label volume (uploaded again before it, outside the timed span). A round takes the cases one after
the other, --reps rounds follow one that is thrown away, and the report is the median over the rounds with the smallest and the largest
round (the spread). Bricks computed come from tbrm_margin_counters [2]; bricks skipped are the rest of bricks x transforms. Prints one
JSON line, and with --table FILE writes the table of DESIGN.md §18.

    python tools/label_margin_time.py [--reps 7] [--n 512] [--table profiles/r14_label_margin.txt]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

REACHES = (2, 5, 16)
OPS = ("expand", "shrink", "close")
SPACING_MM, RADIUS_MM = (0.7, 0.7, 2.5), 5.0


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

    mm = abi.margin_weights(SPACING_MM, RADIUS_MM)
    margins = [(f"{op}{r}", op, (1, 1, 1), r * r) for r in REACHES for op in OPS] + [("expand_5mm", "expand", mm[0], mm[1])]
    variants = [(name, op, w, limit, 1) for name, op, w, limit in margins] + [(name + "_noskip", op, w, limit, 0) for name, op, w, limit in margins]
    morphs = [(f"dilate{r}_c{conn}", r, conn) for r in REACHES for conn in (6, 26)]
    info = {}
    for name, op, w, limit, skip in variants:   # what each case does, outside the timing
        abi.set_tunable("margin_skip", skip)
        res.upload_label_volume(labels)
        c0 = res.margin_counters()
        got = res.margin_labels(op, w, limit, [1], 1)
        c1 = res.margin_counters()
        computed = c1["bricks_computed"] - c0["bricks_computed"]
        info[name] = dict(added=got["added"], removed=got["removed"], launches=got["launches"], reach=list(got["reach"]), computed=computed,
                          skipped=bricks * (got["launches"] // 3) - computed, bricks_written=c1["bricks_written"] - c0["bricks_written"],
                          bbox=[list(got["bbox_min"]), list(got["bbox_max"])])
    abi.set_tunable("margin_skip", 1)
    for name, r, conn in morphs:
        res.upload_label_volume(labels)
        got = res.morph_labels("dilate", r, [1], 1, conn)
        info[name] = dict(added=got["added"], removed=got["removed"], launches=got["launches"])
    bmin, bmax = info["expand5"]["bbox"]
    extent = [b - a + 1 for a, b in zip(bmin, bmax)]
    box_labels = np.ones(extent[::-1], dtype=np.uint8)

    def transfers():
        res.download_label_volume()
        res.update_label_region(bmin, box_labels)

    cases = {"transfers": (transfers, 1)}
    for name, op, w, limit, skip in variants:
        cases[name] = ((lambda op=op, w=w, limit=limit: res.margin_labels(op, w, limit, [1], 1)), skip)
    for name, r, conn in morphs:
        cases[name] = ((lambda r=r, conn=conn: res.morph_labels("dilate", r, [1], 1, conn)), 1)
    rounds = {k: [] for k in cases}
    for r in range(args.reps + 1):
        for name, (fn, skip) in cases.items():
            abi.set_tunable("margin_skip", skip)
            res.upload_label_volume(labels)   # every case starts from the grown label
            res.flush()
            t0 = time.perf_counter()
            fn()   # (every case is complete on return)
            if r:
                rounds[name].append((time.perf_counter() - t0) * 1e3)
    abi.set_tunable("margin_skip", 1)
    out = {k: {"ms": round(float(np.median(v)), 3), "min_ms": round(float(min(v)), 3), "max_ms": round(float(max(v)), 3)} for k, v in rounds.items()}
    result = {"tool": "label_margin_time", "workload": f"{n}^3 labels, label 1 = {grown['voxels']} voxels grown from {list(seed)} over codes {lo} .. {hi}",
              "reps": args.reps, **out, "cases": info, "bricks": bricks, "mm": {"spacing": SPACING_MM, "radius": RADIUS_MM, "weights": mm[0], "limit": mm[1]},
              "transfer_bytes": {"download": n ** 3, "upload": int(box_labels.size)}}
    print(json.dumps(result), flush=True)
    if args.table:
        with open(args.table, "w") as f:
            f.write(f"Euclidean label margins, {result['workload']}; {bricks} bricks; wall ms per call, median (min .. max) of {args.reps} rounds\n")
            f.write(f"expand_5mm: spacing {SPACING_MM} mm, radius {RADIUS_MM} mm -> weights {mm[0]}, limit {mm[1]}\n")
            for name, _, _, _, skip in variants:
                o, i = out[name], info[name]
                f.write(f"  {name:20s} margin_skip {skip}: {o['ms']:8.3f} ({o['min_ms']:.3f} .. {o['max_ms']:.3f})  reach {i['reach']}, {i['launches']} launches, bricks {i['computed']} computed / "
                        f"{i['skipped']} skipped, +{i['added']} -{i['removed']} voxels, {i['bricks_written']} bricks written\n")
            f.write("tbrm_morph_labels, dilation by as many unit steps (c6: octahedron, c26: cube), morph_steps 8:\n")
            for name, _, _ in morphs:
                o, i = out[name], info[name]
                f.write(f"  {name:20s} {o['ms']:8.3f} ({o['min_ms']:.3f} .. {o['max_ms']:.3f})  {i['launches']} launches, +{i['added']} voxels\n")
            o = out["transfers"]
            f.write(f"transfers alone (download {n ** 3} bytes, upload {box_labels.size} bytes, no distance transform): {o['ms']:8.3f} ({o['min_ms']:.3f} .. {o['max_ms']:.3f})\n")
    res.close()


if __name__ == "__main__":
    main()
