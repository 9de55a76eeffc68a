#!/usr/bin/env python3
"""What a data-volume region update (include/tbrm_volume_region.h) costs next to a whole upload, on config 3's volume (512^3
UNORM16): for boxes of 8^3, 64^3, 256^3 voxels at unaligned origins and for the whole volume as a box,
  update_ms    host wall time of update_volume_region_device + flush (the box is in HBM already),
  refresh_ms   what the next lit frame takes beyond a steady frame: the skipping metadata brought up to date
               (restricted k_brick_minmax per box, then k_brick_empty, the shell flag and the three k_brick_dist passes whole),
and, as the yardstick from the same run, the same two figures for upload_volume_device. Every figure is the median of --reps
repetitions after one that is thrown away; frames are small (256^2, 128 steps) so that the refresh is not lost in the march.
Prints one JSON line.

    python tools/volume_region_time.py [--reps 7]
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
    args = ap.parse_args()
    cfg = S.CONFIGS[3]
    n = cfg["n"]
    dims = (n, n, n)
    device = torch.device("cuda", 0)
    vol = S.make_volume_torch(dims, cfg["dtype"], S.seed_for_config(3), device)
    other = S.make_volume_torch(dims, cfg["dtype"], S.seed_for_config(5), device)   # where the boxes' voxels come from
    res = abi.Resources(dims, abi.DTYPE_FMT[np.dtype(cfg["dtype"])], cfg["light_32bit"], False, 0)
    torch.cuda.synchronize()
    nbytes = vol.numel() * vol.element_size()
    res.upload_volume_device(vol.data_ptr(), nbytes)
    res.set_tf_lut(abi.color_curve_to_lut(S.tf_keys(cfg["tf"])))
    res.set_windowing(abi.WindowingParams(*cfg["window"]))
    world = S.default_world()
    res.add_dir_light(S.light(0), True, world)
    res.flush()
    fb = 256
    cam, tile, rp = S.default_camera(fb, fb), abi.Tile(0, 0, fb, fb), abi.RaymarchParams(128.0, -1, True)
    out = torch.empty((fb, fb, 4), dtype=torch.float32, device=device)

    def wall_ms(fn):
        t0 = time.perf_counter()
        fn()
        res.flush()
        return (time.perf_counter() - t0) * 1e3

    def frame():
        res.raymarch_lit_device(cam, tile, rp, world, out.data_ptr())

    for _ in range(5):
        wall_ms(frame)
    steady = float(np.median([wall_ms(frame) for _ in range(20)]))

    def measure(write):
        upd, ref = [], []
        for k in range(args.reps + 1):
            u = wall_ms(lambda: write(k))
            f = wall_ms(frame) - steady
            if k:
                upd.append(u)
                ref.append(f)
        return {"update_ms": round(float(np.median(upd)), 4), "refresh_ms": round(float(np.median(ref)), 4)}

    results = {}
    for edge, origin in ((8, (203, 131, 77)), (64, (203, 131, 77)), (256, (203, 131, 77)), (n, (0, 0, 0))):
        boxes = [other, vol] if edge == n else [
            v[origin[2]:origin[2] + edge, origin[1]:origin[1] + edge, origin[0]:origin[0] + edge].contiguous() for v in (other, vol)]
        torch.cuda.synchronize()
        box_bytes = boxes[0].numel() * boxes[0].element_size()
        r = measure(lambda k: res.update_volume_region_device(origin, (edge, edge, edge), boxes[k & 1].data_ptr(), box_bytes))
        r["origin"] = list(origin)
        if edge == n:   # the scatter reads the box once and writes the bricks once
            r["scatter_GBps"] = round(2 * box_bytes / (r["update_ms"] * 1e-3) / 1e9, 1)
        results["full" if edge == n else f"{edge}^3"] = r
    sources = [other, vol]
    results["upload_volume_device"] = measure(lambda k: res.upload_volume_device(sources[k & 1].data_ptr(), nbytes))
    print(json.dumps({"tool": "volume_region_time", "workload": f"config 3 volume: {n}^3 uint16; frames {fb}^2, 128 steps, one light",
                      "reps": args.reps, "steady_frame_ms": round(steady, 4), "counters": res.volume_region_counters(), **results}), flush=True)
    res.close()


if __name__ == "__main__":
    main()
