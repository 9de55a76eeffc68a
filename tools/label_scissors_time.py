#!/usr/bin/env python3
"""What view-space scissors (include/tbrm_scissors.h) cost, on config 3's volume — 512^3 UNORM16 — and the label that
tools/region_grow_time.py's grow produces there (the window's span in codes, grown from the voxel under the image centre), under a
1024^2 view of the whole volume, against the route they replace, in the same process:
  disc_erase_inside / disc_erase_outside / disc_fill_inside / disc_fill_outside
                                 host wall time of one writing tbrm_scissors_labels call (complete on return, the mask's upload and
                                 summary included) on label 1, whole volume: a disc lasso of a quarter of the frame's area;
  polygon_erase_inside           a twelve-point concave polygon (tbrm_host_scissors_polygon);
  disc_to_surface                the disc with depth_max at the depth picked under the image centre: "cut down to the visible surface";
  clear_erase_inside             an all-clear mask: every brick is outside by its corners, the kernel projects nothing — what the
                                 load, the write and the call's fixed parts cost;
  .._noskip                      the same cases at scissors_skip = 0: every brick of the range projected voxel by voxel;
  transfers                      tbrm_download_label_volume plus tbrm_update_label_region of the bounding box of what
                                 disc_erase_inside moved: what a host that projects the voxels itself moves, with NOTHING charged
                                 for the projection.
Every timed call starts from the same label volume (uploaded again before it, outside the timed span). A round takes the cases one after
the other, --reps rounds follow one that is thrown away, and the report is the median over the rounds with the smallest and the largest
round (the spread). Prints one JSON line, and with --table FILE writes the table of DESIGN.md §20.

    python tools/label_scissors_time.py [--reps 7] [--n 512] [--table profiles/r17_label_scissors.txt]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

OPS = ("erase_inside", "erase_outside", "fill_inside", "fill_outside")


def disc_mask(width, height, share=0.25):
    """uint32 [height, ceil(width / 32)]: a centred disc of `share` of the frame's area"""
    r2 = share * width * height / math.pi
    y, x = np.indices((height, width))
    bits = (x + 0.5 - width / 2) ** 2 + (y + 0.5 - height / 2) ** 2 <= r2
    padded = np.zeros((height, (width + 31) // 32 * 32), dtype=np.uint64)
    padded[:, :width] = bits
    return (padded.reshape(height, -1, 32) << np.arange(32, dtype=np.uint64)[None, None, :]).sum(axis=2).astype(np.uint32)


def star(width, height, points=12):
    """a concave polygon of `points` points round the frame's centre, on multiples of 1 / 256"""
    out = []
    for k in range(points):
        r = (0.42 if k % 2 == 0 else 0.2) * min(width, height)
        a = 2 * math.pi * k / points + 0.1
        out.append((round((width / 2 + r * math.cos(a)) * 256) / 256, round((height / 2 + r * math.sin(a)) * 256) / 256))
    return out


def main():
    import torch

    from tbraymarcherplugin_amd import abi, synthetic as S

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--n", type=int, default=0, help="volume edge (default: config 3's)")
    ap.add_argument("--view", type=int, default=1024, help="the view's edge in pixels")
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
    view = args.view
    cam, rp = S.default_camera(view, view), abi.RaymarchParams(float(cfg["steps"]) * n / cfg["n"], -1, True)
    hit, _, depth = res.pick(cam, view // 2, view // 2, rp, world, 0.5)
    assert hit["sample"] >= 0, "the image centre meets nothing"
    seed = abi.hit_voxel((n, n, n), hit)
    res.attach_empty_labels()
    grown = res.grow_region([seed], lo, hi, 1, 6)
    labels = res.download_label_volume()
    bricks = ((n + 7) // 8) ** 3

    whole = abi.scissors_projection((n, n, n), world, cam)
    to_surface = abi.scissors_projection((n, n, n), world, cam, 0.0, float(depth))
    disc, polygon, clear = disc_mask(view, view), abi.scissors_polygon(star(view, view), view, view), np.zeros(abi.scissors_mask_shape(view, view), dtype=np.uint32)
    base = [(f"disc_{op}", whole, disc, op) for op in OPS] + [("polygon_erase_inside", whole, polygon, "erase_inside"), ("disc_to_surface", to_surface, disc, "erase_inside"),
                                                                ("clear_erase_inside", whole, clear, "erase_inside")]
    variants = [(name, p, m, op, 1) for name, p, m, op in base] + [(name + "_noskip", p, m, op, 0) for name, p, m, op in base]
    info = {}
    for name, p, m, op, skip in variants:   # what each case does, outside the timing
        abi.set_tunable("scissors_skip", skip)
        res.upload_label_volume(labels)
        c0 = res.scissors_counters()
        got = res.scissor_labels(p, m, op, [1], 1)
        c1 = res.scissors_counters()
        info[name] = dict(added=got["added"], removed=got["removed"], launches=got["launches"], inside=got["bricks_inside"], outside=got["bricks_outside"],
                          projected=got["bricks_projected"], by_source=bricks - got["bricks_inside"] - got["bricks_outside"] - got["bricks_projected"],
                          bricks_written=c1["bricks_written"] - c0["bricks_written"], bbox=[list(got["bbox_min"]), list(got["bbox_max"])])
    abi.set_tunable("scissors_skip", 1)
    bmin, bmax = info["disc_erase_inside"]["bbox"]
    extent = [b - a + 1 for a, b in zip(bmin, bmax)]
    box_labels = np.ones(extent[::-1], dtype=np.uint8)

    def transfers():
        res.download_label_volume()
        res.update_label_region(bmin, box_labels)

    cases = {"transfers": (transfers, 1)}
    for name, p, m, op, skip in variants:
        cases[name] = ((lambda p=p, m=m, op=op: res.scissor_labels(p, m, op, [1], 1)), skip)
    rounds = {k: [] for k in cases}
    for r in range(args.reps + 1):
        for name, (fn, skip) in cases.items():
            abi.set_tunable("scissors_skip", skip)
            res.upload_label_volume(labels)   # every case starts from the grown label
            res.flush()
            t0 = time.perf_counter()
            fn()   # (every case is complete on return)
            if r:
                rounds[name].append((time.perf_counter() - t0) * 1e3)
    abi.set_tunable("scissors_skip", 1)
    out = {k: {"ms": round(float(np.median(v)), 3), "min_ms": round(float(min(v)), 3), "max_ms": round(float(max(v)), 3)} for k, v in rounds.items()}
    result = {"tool": "label_scissors_time", "workload": f"{n}^3 labels, label 1 = {grown['voxels']} voxels grown from {list(seed)} over codes {lo} .. {hi}, a {view}^2 view",
              "reps": args.reps, **out, "cases": info, "bricks": bricks, "scale_log2": int(whole.scale_log2), "picked_depth": float(depth),
              "mask_pixels": {"disc": int(np.unpackbits(disc.view(np.uint8)).sum()), "polygon": int(np.unpackbits(polygon.view(np.uint8)).sum())},
              "transfer_bytes": {"download": n ** 3, "upload": int(box_labels.size)}}
    print(json.dumps(result), flush=True)
    if args.table:
        with open(args.table, "w") as f:
            f.write(f"View-space scissors, {result['workload']}; {bricks} bricks; rows scaled by 2^{result['scale_log2']}; wall ms per call, median (min .. max) of {args.reps} rounds\n")
            f.write(f"masks: disc {result['mask_pixels']['disc']} pixels, polygon {result['mask_pixels']['polygon']} pixels of {view * view}; disc_to_surface: depth_max {depth:.6g}\n")
            for name, _, _, _, skip in variants:
                o, i = out[name], info[name]
                f.write(f"  {name:28s} scissors_skip {skip}: {o['ms']:8.3f} ({o['min_ms']:.3f} .. {o['max_ms']:.3f})  bricks {i['inside']} inside / {i['outside']} outside / "
                        f"{i['projected']} projected / {i['by_source']} by the source set, +{i['added']} -{i['removed']} voxels, {i['bricks_written']} bricks written, {i['launches']} launches\n")
            o = out["transfers"]
            f.write(f"transfers alone (download {n ** 3} bytes, upload {box_labels.size} bytes, no projection): {o['ms']:8.3f} ({o['min_ms']:.3f} .. {o['max_ms']:.3f})\n")
    res.close()


if __name__ == "__main__":
    main()
