#!/usr/bin/env python3
"""What label morphology (include/tbrm_morphology.h) costs, on config 3's volume — 512^3 UNORM16 — and the label that
tools/region_grow_time.py's grow produces there (the window's span in codes, grown from the voxel under the image centre), against the
route it replaces, in the same process:
  close2_c6 / close2_c26, open1_c6 / open1_c26, dilate8_c6 / dilate8_c26
                                 host wall time of one writing tbrm_morph_labels call (complete on return) on label 1, whole volume,
                                 at the default morph_steps (8);
  dilate8_c6_s1 / dilate8_c26_s1 the same dilation at morph_steps = 1: a launch per unit step instead of one launch of 8 steps;
  transfers                      tbrm_download_label_volume plus tbrm_update_label_region of the bounding box of what close2_c6 moved:
                                 what a host that filters on its own CPU moves, with NOTHING charged for its filter.
Every timed call starts from the same label volume (uploaded again before it, outside the timed span). A round takes the cases one after
the other, --reps rounds follow one that is thrown away, and the report is the median over the rounds with the smallest and the largest
round (the spread). Windows computed come from tbrm_morph_counters [2]; windows skipped are the rest of bricks x launches. Prints one JSON
line, and with --table FILE writes the table of DESIGN.md §15.

    python tools/label_morph_time.py [--reps 7] [--n 512] [--table profiles/r11_label_morph.txt]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = [("close2", "close", 2), ("open1", "open", 1), ("dilate8", "dilate", 8)]


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

    variants = [(f"{name}_c{conn}", op, r, conn, 8) for name, op, r in CASES for conn in (6, 26)]
    variants += [(f"dilate8_c{conn}_s1", "dilate", 8, conn, 1) for conn in (6, 26)]
    info = {}
    for name, op, r, conn, steps in variants:   # what each case does, outside the timing
        abi.set_tunable("morph_steps", steps)
        res.upload_label_volume(labels)
        c0 = res.morph_counters()
        got = res.morph_labels(op, r, [1], 1, conn)
        c1 = res.morph_counters()
        windows = c1["windows"] - c0["windows"]
        info[name] = dict(added=got["added"], removed=got["removed"], launches=got["launches"], windows=windows,
                          skipped=bricks * got["launches"] - windows, bricks_written=c1["bricks_written"] - c0["bricks_written"],
                          bbox=[list(got["bbox_min"]), list(got["bbox_max"])])
    bmin, bmax = info["close2_c6"]["bbox"]
    extent = [b - a + 1 for a, b in zip(bmin, bmax)]
    box_labels = np.ones(extent[::-1], dtype=np.uint8)

    def transfers():
        res.download_label_volume()
        res.update_label_region(bmin, box_labels)

    def morph(op, r, conn, steps):
        def call():
            res.morph_labels(op, r, [1], 1, conn)
        return call, steps

    cases = {"transfers": (transfers, 8)}
    for name, op, r, conn, steps in variants:
        cases[name] = morph(op, r, conn, steps)
    rounds = {k: [] for k in cases}
    for r in range(args.reps + 1):
        for name, (fn, steps) in cases.items():
            abi.set_tunable("morph_steps", steps)
            res.upload_label_volume(labels)   # every case starts from the grown label
            res.flush()
            t0 = time.perf_counter()
            fn()   # (every case is complete on return)
            if r:
                rounds[name].append((time.perf_counter() - t0) * 1e3)
    abi.set_tunable("morph_steps", 8)
    out = {k: {"ms": round(float(np.median(v)), 3), "min_ms": round(float(min(v)), 3), "max_ms": round(float(max(v)), 3)} for k, v in rounds.items()}
    result = {"tool": "label_morph_time", "workload": f"{n}^3 labels, label 1 = {grown['voxels']} voxels grown from {list(seed)} over codes {lo} .. {hi}",
              "reps": args.reps, **out, "cases": info, "bricks": bricks, "transfer_bytes": {"download": n ** 3, "upload": int(box_labels.size)}}
    print(json.dumps(result), flush=True)
    if args.table:
        with open(args.table, "w") as f:
            f.write(f"label morphology, {result['workload']}; {bricks} bricks; wall ms per call, median (min .. max) of {args.reps} rounds\n")
            for name, _, _, _, steps in variants:
                o, i = out[name], info[name]
                f.write(f"  {name:15s} morph_steps {steps}: {o['ms']:8.3f} ({o['min_ms']:.3f} .. {o['max_ms']:.3f})  {i['launches']} launches, windows {i['windows']} computed / "
                        f"{i['skipped']} skipped, +{i['added']} -{i['removed']} voxels, {i['bricks_written']} bricks written\n")
            o = out["transfers"]
            f.write(f"transfers alone (download {n ** 3} bytes, upload {box_labels.size} bytes, no filter): {o['ms']:8.3f} ({o['min_ms']:.3f} .. {o['max_ms']:.3f})\n")
    res.close()


if __name__ == "__main__":
    main()
