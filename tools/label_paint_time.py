#!/usr/bin/env python3
"""What the paint brush (include/tbrm_paint.h) costs, on config 3's volume — 512^3 UNORM16 — with an empty label volume, against the
route it replaces, in the same process:
  ball_r4 / ball_r16             host wall time of one writing tbrm_paint_labels call (complete on return, the stroke's plan and
                                 upload included) that paints label 1: one point at the volume's centre, radius 4 / 16 voxels;
  stroke64_r.. / stroke1024_r..  a stroke of 64 / 1024 points along a closed curve through the middle of the volume;
  .._gated                       the same with the gate on the window's span of codes (the data volume is read);
  .._noskip                      the same cases at paint_skip = 0: every brick of the work box tests every voxel against every segment;
  transfers_..                   tbrm_download_label_volume plus tbrm_update_label_region of the bounding box of what the stroke
                                 painted: what a host that paints into its own copy moves, with NOTHING charged for the painting.
Every timed call starts from the empty label volume (uploaded again before it, outside the timed span). A round takes the cases one
after the other, --reps rounds follow one that is thrown away, and the report is the median over the rounds with the smallest and
the largest round (the spread). Prints one JSON line, and with --table FILE writes the table of DESIGN.md §22.

    python tools/label_paint_time.py [--reps 7] [--n 512] [--table profiles/r19_label_paint.txt]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def curve(n, points):
    """`points` points in eighths of a voxel along a closed curve through the middle half of a volume of edge n; one point: the centre"""
    if points == 1:
        return np.array([[4 * (n - 1)] * 3], dtype=np.int32)
    t = 2 * math.pi * np.arange(points) / points
    c, r = (n - 1) / 2, 0.25 * n
    xyz = np.stack([c + r * np.cos(t), c + r * np.sin(2 * t + 0.3), c + 0.6 * r * np.sin(3 * t + 1.1)], axis=1)
    return np.rint(8.0 * xyz).astype(np.int32)


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
    center, width = cfg["window"][0], cfg["window"][1]
    gate = (math.ceil((center - width / 2) * 65535), math.floor((center + width / 2) * 65535))   # the window's span, in codes
    res.attach_empty_labels()
    labels = np.zeros((n, n, n), dtype=np.uint8)

    base = []
    for points in (1, 64, 1024):
        for radius in (4, 16):
            weights, limit = abi.paint_brush((1.0, 1.0, 1.0), float(radius))
            name = ("ball" if points == 1 else f"stroke{points}") + f"_r{radius}"
            base.append((name, curve(n, points), weights, limit, None))
            base.append((name + "_gated", curve(n, points), weights, limit, gate))
    variants = [(name, p, w, l, g, 1) for name, p, w, l, g in base] + [(name + "_noskip", p, w, l, g, 0) for name, p, w, l, g in base]
    info = {}
    for name, p, w, l, g, skip in variants:   # what each case does, outside the timing
        abi.set_tunable("paint_skip", skip)
        res.upload_label_volume(labels)
        c0 = res.paint_counters()
        got = res.paint_labels(p, w, l, "paint", [1], 1, gate=g)
        c1 = res.paint_counters()
        info[name] = dict(points=int(len(p)), stamp=got["stamp_voxels"], added=got["added"], whole=got["bricks_whole"], untouched=got["bricks_untouched"],
                          evaluated=got["bricks_evaluated"], bricks_written=c1["bricks_written"] - c0["bricks_written"], launches=got["launches"],
                          bbox=[list(got["bbox_min"]), list(got["bbox_max"])])
    abi.set_tunable("paint_skip", 1)
    for name, p, w, l, g, skip in variants:   # the switch changes nothing but the bricks' verdicts
        if skip == 0:
            a, b = info[name], info[name[:-len("_noskip")]]
            assert (a["stamp"], a["added"], a["bbox"]) == (b["stamp"], b["added"], b["bbox"]), name

    cases = {}
    for name, p, w, l, g in base:
        if g is None:
            bmin, bmax = info[name]["bbox"]
            block = np.ones([b - a + 1 for a, b in zip(bmin, bmax)][::-1], dtype=np.uint8)
            info["transfers_" + name] = dict(download=n ** 3, upload=int(block.size))

            def transfers(bmin=bmin, block=block):
                res.download_label_volume()
                res.update_label_region(bmin, block)

            cases["transfers_" + name] = (transfers, 1)
    for name, p, w, l, g, skip in variants:
        cases[name] = ((lambda p=p, w=w, l=l, g=g: res.paint_labels(p, w, l, "paint", [1], 1, gate=g)), skip)
    rounds = {k: [] for k in cases}
    for r in range(args.reps + 1):
        for name, (fn, skip) in cases.items():
            abi.set_tunable("paint_skip", skip)
            res.upload_label_volume(labels)   # every case starts from the empty label volume
            res.flush()
            t0 = time.perf_counter()
            fn()   # (every case is complete on return)
            if r:
                rounds[name].append((time.perf_counter() - t0) * 1e3)
    abi.set_tunable("paint_skip", 1)
    out = {k: {"ms": round(float(np.median(v)), 3), "min_ms": round(float(min(v)), 3), "max_ms": round(float(max(v)), 3)} for k, v in rounds.items()}
    result = {"tool": "label_paint_time", "workload": f"{n}^3 empty labels over config 3's volume, label 1 painted, gate {gate[0]} .. {gate[1]}", "reps": args.reps, **out,
              "cases": info, "bricks": ((n + 7) // 8) ** 3}
    print(json.dumps(result), flush=True)
    if args.table:
        with open(args.table, "w") as f:
            f.write(f"The paint brush, {result['workload']}; {result['bricks']} bricks in the volume; wall ms per call, median (min .. max) of {args.reps} rounds\n")
            for name, _, _, _, _, skip in variants:
                o, i = out[name], info[name]
                f.write(f"  {name:32s} paint_skip {skip}: {o['ms']:9.3f} ({o['min_ms']:.3f} .. {o['max_ms']:.3f})  {i['points']} points, bricks {i['whole']} whole / {i['untouched']} untouched / "
                        f"{i['evaluated']} evaluated, stamp {i['stamp']} voxels, {i['bricks_written']} bricks written\n")
            for name in cases:
                if name.startswith("transfers_"):
                    o, i = out[name], info[name]
                    f.write(f"  {name:32s} (download {i['download']} bytes, upload {i['upload']} bytes, no painting): {o['ms']:9.3f} ({o['min_ms']:.3f} .. {o['max_ms']:.3f})\n")
    res.close()


if __name__ == "__main__":
    main()
