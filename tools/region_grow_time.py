#!/usr/bin/env python3
"""What seeded region growing (include/tbrm_segment.h) costs, on config 3's volume — 512^3 UNORM16, the benchmark's window and
transfer function — against the route it replaces, in the same process:
  grow_c6_b<N> / grow_c26_b<N>   host wall time of one writing tbrm_grow_region call (complete on return), 6- / 26-connected, with
                                 grow_batch = N in {1, 4, 8, 16, 32}: range = the window's span in codes, seed = the voxel tbrm_pick finds
                                 under the image centre at threshold 0.5, new_label 1;
  transfers                      tbrm_download_volume_region of the whole volume plus tbrm_update_label_region of the grown region's
                                 bounding box: what a host that fills on its own CPU moves, with NOTHING charged for its fill.
A round takes the cases one after the other, --reps rounds follow one that is thrown away, and the report is the median over the rounds
with the smallest and the largest round (the spread). Passes, brick visits and voxels come from the call's result and
tbrm_segment_counters. Prints one JSON line, and with --table FILE writes the table of DESIGN.md §14.

    python tools/region_grow_time.py [--reps 7] [--n 512] [--table profiles/r10_region_grow.txt]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BATCHES = (1, 4, 8, 16, 32)


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

    info = {}
    for conn in (6, 26):
        c0 = res.segment_counters()
        r = res.grow_region([seed], lo, hi, 1, conn)
        c1 = res.segment_counters()
        info[conn] = dict(voxels=r["voxels"], passes=r["passes"], brick_visits=c1["brick_visits"] - c0["brick_visits"],
                          bricks_written=c1["bricks_written"] - c0["bricks_written"], bbox=[list(r["bbox_min"]), list(r["bbox_max"])])
    bmin, bmax = info[6]["bbox"]
    extent = [b - a + 1 for a, b in zip(bmin, bmax)]
    box_labels = np.ones(extent[::-1], dtype=np.uint8)

    def transfers():
        res.download_volume_region((0, 0, 0), (n, n, n))
        res.update_label_region(bmin, box_labels)

    cases = {"transfers": transfers}
    for conn in (6, 26):
        for b in BATCHES:
            def grow(conn=conn, b=b):
                abi.set_tunable("grow_batch", b)
                res.grow_region([seed], lo, hi, 1, conn)
            cases[f"grow_c{conn}_b{b}"] = grow
    rounds = {k: [] for k in cases}
    for r in range(args.reps + 1):
        for name, fn in cases.items():
            res.flush()
            t0 = time.perf_counter()
            fn()   # (every case is complete on return)
            if r:
                rounds[name].append((time.perf_counter() - t0) * 1e3)
    out = {k: {"ms": round(float(np.median(v)), 3), "min_ms": round(float(min(v)), 3), "max_ms": round(float(max(v)), 3)} for k, v in rounds.items()}
    best = {conn: min(BATCHES, key=lambda b: out[f"grow_c{conn}_b{b}"]["ms"]) for conn in (6, 26)}
    result = {"tool": "region_grow_time", "workload": f"{n}^3 uint16, codes {lo} .. {hi}, seed {list(seed)}", "reps": args.reps, **out,
              "region": {str(k): v for k, v in info.items()}, "best_batch": {str(k): v for k, v in best.items()},
              "transfer_bytes": {"download": n ** 3 * 2, "upload": int(box_labels.size)}}
    print(json.dumps(result), flush=True)
    if args.table:
        with open(args.table, "w") as f:
            f.write(f"region growing, {result['workload']}; wall ms per call, median (min .. max) of {args.reps} rounds\n")
            for conn in (6, 26):
                i = info[conn]
                f.write(f"{conn}-connected: {i['voxels']} voxels, {i['passes']} passes, {i['brick_visits']} brick visits, {i['bricks_written']} bricks written\n")
                for b in BATCHES:
                    o = out[f"grow_c{conn}_b{b}"]
                    f.write(f"  grow_batch {b:2d}: {o['ms']:8.3f} ({o['min_ms']:.3f} .. {o['max_ms']:.3f})\n")
            o = out["transfers"]
            f.write(f"transfers alone (download {n ** 3 * 2} bytes, upload {box_labels.size} bytes, no fill): {o['ms']:8.3f} ({o['min_ms']:.3f} .. {o['max_ms']:.3f})\n")
    res.close()


if __name__ == "__main__":
    main()
