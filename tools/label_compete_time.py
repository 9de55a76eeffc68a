#!/usr/bin/env python3
"""What competitive growing from seed labels (include/tbrm_compete.h) costs, on config 3's volume — 512^3 UNORM16, the benchmark's
window — against the transfers of the route it replaces, in the same process:
  compete_<box>_b<N>   host wall time of one writing tbrm_compete_labels call (complete on return) over the whole volume or its lower
                       half, with grow_batch = N in {1, 16, 32}: three painted balls of labels 1, 2, 3, gate = the window's span in codes,
                       step cost 1 per axis, value_shift 6, no cost limit; the painted labels are uploaded again before every call
                       (not timed), so that every call does the same work;
  transfers_<box>      tbrm_download_volume_region of the box plus tbrm_update_label_region of the same box: what a host that solves on
                       its own CPU moves, with NOTHING charged for its solver.
A round takes the cases one after the other, --reps rounds follow one that is thrown away, and the report is the median over the rounds
with the smallest and the largest round (the spread). Passes, brick visits and claimed voxels come from the call's result and
tbrm_compete_counters. Prints one JSON line, and with --table FILE writes the table of DESIGN.md §21.

    python tools/label_compete_time.py [--reps 5] [--n 512] [--table profiles/r18_label_compete.txt]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BATCHES = (1, 16, 32)


def main():
    import torch

    from tbraymarcherplugin_amd import abi, synthetic as S

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
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
    lo, hi = math.ceil((center - width / 2) * 65535), math.floor((center + width / 2) * 65535)   # the window's span, in codes
    painted = np.zeros((n, n, n), dtype=np.uint8)
    r = max(n // 64, 1)
    z, y, x = np.ogrid[-r:r + 1, -r:r + 1, -r:r + 1]
    ball = x * x + y * y + z * z <= r * r
    for label, (cx, cy, cz) in ((1, (n // 4, n // 3, n // 4)), (2, (2 * n // 3, n // 2, n // 3)), (3, (n // 2, 2 * n // 3, 3 * n // 8))):
        painted[cz - r:cz + r + 1, cy - r:cy + r + 1, cx - r:cx + r + 1][ball] = label
    boxes = {"whole": ((0, 0, 0), (n, n, n)), "half": ((0, 0, 0), (n, n, n // 2))}
    kw = dict(step_cost=(1, 1, 1), value_shift=6)

    info = {}
    for name, (origin, extent) in boxes.items():
        res.upload_label_volume(painted)
        c0 = res.compete_counters()
        got = res.compete_labels([1, 2, 3], lo, hi, origin=origin, extent=extent, **kw)
        c1 = res.compete_counters()
        info[name] = dict(seed_voxels=got["seed_voxels"], claimable=got["claimable"], claimed=got["claimed"], max_cost=got["max_cost"], passes=got["passes"],
                          brick_visits=c1["brick_visits"] - c0["brick_visits"], bricks_written=c1["bricks_written"] - c0["bricks_written"],
                          bricks=math.prod(-(-e // 8) for e in extent))

    cases = {}
    for name, (origin, extent) in boxes.items():
        block = np.ones(extent[::-1], dtype=np.uint8)

        def transfers(origin=origin, extent=extent, block=block):
            res.download_volume_region(origin, extent)
            res.update_label_region(origin, block)
        cases[f"transfers_{name}"] = transfers
        for b in BATCHES:
            def compete(origin=origin, extent=extent, b=b):
                abi.set_tunable("grow_batch", b)
                res.compete_labels([1, 2, 3], lo, hi, origin=origin, extent=extent, **kw)
            cases[f"compete_{name}_b{b}"] = compete
    rounds = {k: [] for k in cases}
    for rep in range(args.reps + 1):
        for name, fn in cases.items():
            res.upload_label_volume(painted)   # (not timed: every call starts from the painted balls)
            res.flush()
            t0 = time.perf_counter()
            fn()   # (every case is complete on return)
            if rep:
                rounds[name].append((time.perf_counter() - t0) * 1e3)
    abi.set_tunable("grow_batch", 16)
    out = {k: {"ms": round(float(np.median(v)), 3), "min_ms": round(float(min(v)), 3), "max_ms": round(float(max(v)), 3)} for k, v in rounds.items()}
    result = {"tool": "label_compete_time", "workload": f"{n}^3 uint16, gate {lo} .. {hi}, three balls of radius {r}, step 1 1 1, shift 6", "reps": args.reps, **out,
              "boxes": info, "transfer_bytes": {k: {"download": math.prod(e) * 2, "upload": math.prod(e)} for k, (_, e) in boxes.items()}}
    print(json.dumps(result), flush=True)
    if args.table:
        with open(args.table, "w") as f:
            f.write(f"competitive growing, {result['workload']}; wall ms per call, median (min .. max) of {args.reps} rounds\n")
            for name, (_, extent) in boxes.items():
                i = info[name]
                f.write(f"{name} ({extent[0]} x {extent[1]} x {extent[2]}, {i['bricks']} bricks): {i['seed_voxels']} seed voxels, {i['claimable']} claimable, {i['claimed']} claimed, "
                        f"max cost {i['max_cost']}, {i['passes']} passes, {i['brick_visits']} brick visits, {i['bricks_written']} bricks written\n")
                for b in BATCHES:
                    o = out[f"compete_{name}_b{b}"]
                    f.write(f"  grow_batch {b:2d}: {o['ms']:9.3f} ({o['min_ms']:.3f} .. {o['max_ms']:.3f})\n")
                o = out[f"transfers_{name}"]
                t = result["transfer_bytes"][name]
                f.write(f"  transfers alone (download {t['download']} bytes, upload {t['upload']} bytes, no solver): {o['ms']:9.3f} ({o['min_ms']:.3f} .. {o['max_ms']:.3f})\n")
    res.close()


if __name__ == "__main__":
    main()
