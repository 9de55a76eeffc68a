#!/usr/bin/env python3
"""What the label overlay (include/tbrm_labels.h) costs the lit frame: config 3's frame (512^3 UNORM16, UNORM8 light volume lit by
its four lights, 1024^2 RGBA f32, 512 steps) timed like bench.py — HIP events on the library's stream around each frame, warm-up
frames first, then the mean — with no label volume, a label volume under an all-clear colour table, a sparse label (a few spheres,
~2 % of the voxels) and a dense one (~50 %), each with empty-space skipping on and off. The sparse and dense cases run twice: with
the reference's default colours (alpha 0.5: rays that enter a label soon take the early exit, so the frame can get cheaper) and
with faint ones (alpha 0.001: the label step's own cost, next to the same amount of data work). Prints one JSON line.

    python tools/label_overlay_time.py [--frames 20] [--warmup 5]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def spheres(n, centers, radius):
    """label 1 .. k in spheres of `radius` (fraction of n) around `centers` (fractions of n), 0 elsewhere"""
    z, y, x = np.ogrid[:n, :n, :n]
    lab = np.zeros((n, n, n), dtype=np.uint8)
    for k, (cx, cy, cz) in enumerate(centers):
        lab[(x - cx * n) ** 2 + (y - cy * n) ** 2 + (z - cz * n) ** 2 <= (radius * n) ** 2] = 1 + k % 2
    return lab


def main():
    import torch

    from tbraymarcherplugin_amd import abi, synthetic as S

    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    cfg = S.CONFIGS[3]
    n = cfg["n"]
    dims = (n, n, n)
    device = torch.device("cuda", 0)
    vol = S.make_volume_torch(dims, cfg["dtype"], S.seed_for_config(3), device)
    res = abi.Resources(dims, abi.DTYPE_FMT[np.dtype(cfg["dtype"])], cfg["light_32bit"], False, 0)
    torch.cuda.synchronize()
    res.upload_volume_device(vol.data_ptr(), vol.numel() * vol.element_size())
    res.set_tf_lut(abi.color_curve_to_lut(S.tf_keys(cfg["tf"])))
    res.set_windowing(abi.WindowingParams(*cfg["window"]))
    world = S.default_world()
    for i in cfg["lights"]:
        res.add_dir_light(S.light(i), True, world)
    res.flush()
    fb = cfg["fb"]
    cam = S.default_camera(fb, fb)
    tile = abi.Tile(0, 0, fb, fb)
    out = torch.empty((fb, fb, 4), dtype=torch.float32, device=device)
    stream = torch.cuda.ExternalStream(res.stream(), device=device)

    def frame_ms(skipping):
        rp = abi.RaymarchParams(float(cfg["steps"]), -1, skipping)
        for _ in range(args.warmup):
            res.raymarch_lit_device(cam, tile, rp, world, out.data_ptr())
        res.flush()
        times = []
        for _ in range(args.frames):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            res.raymarch_lit_device(cam, tile, rp, world, out.data_ptr())
            e1.record(stream)
            e1.synchronize()
            times.append(float(e0.elapsed_time(e1)))
        return round(float(np.mean(times)), 4)

    clear = np.zeros((256, 4), dtype=np.float32)
    overlay = abi.make_default_label_colors()
    faint = overlay.copy()
    faint[1:, 3] = 0.001
    rng = np.random.default_rng(3)
    sparse = spheres(n, rng.uniform(0.25, 0.75, size=(6, 3)), 0.095)
    dense = spheres(n, [(0.5, 0.5, 0.5)], 0.49)
    cases = {}
    for skipping in (True, False):
        key = "skip_on" if skipping else "skip_off"
        r = {"no_labels": frame_ms(skipping)}
        res.upload_label_volume(sparse)
        res.set_label_colors(clear)
        r["labels_all_clear"] = frame_ms(skipping)
        abi.set_tunable("ray_labels", 1)   # the same, through the label kernel (a label byte per live sample, nothing to add)
        r["labels_all_clear_label_kernel"] = frame_ms(skipping)
        abi.set_tunable("ray_labels", 0)
        res.set_label_colors(overlay)
        r["sparse"] = frame_ms(skipping)
        res.set_label_colors(faint)
        r["sparse_faint"] = frame_ms(skipping)
        res.upload_label_volume(dense)
        r["dense_faint"] = frame_ms(skipping)
        res.set_label_colors(overlay)
        r["dense"] = frame_ms(skipping)
        res.release_label_volume()
        cases[key] = r
    print(json.dumps({"tool": "label_overlay_time", "workload": f"config 3 lit frame: {n}^3 uint16, {fb}^2 RGBA f32, {cfg['steps']} steps",
                      "frames": args.frames, "warmup": args.warmup, "ms_per_frame": cases,
                      "label_fraction": {"sparse": round(float((sparse > 0).mean()), 4), "dense": round(float((dense > 0).mean()), 4)}}),
          flush=True)
    res.close()


if __name__ == "__main__":
    main()
