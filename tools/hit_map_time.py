#!/usr/bin/env python3
"""What a hit map (include/tbrm_hit.h) costs, on config 3 — 512^3 UNORM16, 1024 x 1024 rays, 512 steps, the benchmark's view, window,
transfer function and lights — against the lit march of the same view in the same process:
  lit        tbrm_raymarch_lit_device with view_cache_mb = 0 (every frame marches: k_raymarch_lit),
  hit_005    tbrm_raymarch_hits_device at threshold 0.05 (records and depth),
  hit_095    the same at threshold 0.95: per sample a strict subset of the lit march's work, over the same samples,
  hit_095_nd the same without the depth buffer.
Each figure is kernel time by HIP events round --launches back-to-back launches on the handle's stream, per launch; a round takes
the cases one after the other, --reps rounds follow one that is thrown away, and the report is the median over the rounds with the
smallest and the largest round (the spread). Also the host wall time of a 1 x 1 tbrm_pick round trip (launch, 32-byte copy, wait):
launch-bound, reported and not tuned. Checks first that the 0.95 map is the lit frame's alpha channel bit for bit. Prints one JSON line.

The waves per SIMD of k_raymarch_hit are a build-time choice (TBRM_HIT_WAVES, tbrm_kernels.hip); to compare values build one library
each (tools/build_variant.py NAME --only kernels_hit -DTBRM_HIT_WAVES=N) and run this once per library with TBRM_LIB_PATH set:

    python tools/hit_map_time.py [--reps 9] [--launches 40] [--note TEXT]
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
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--n", type=int, default=0, help="volume edge (default: config 3's)")
    ap.add_argument("--fb", type=int, default=0, help="framebuffer edge (default: config 3's)")
    ap.add_argument("--note", default="", help="copied into the result (which build this is)")
    args = ap.parse_args()
    cfg = S.CONFIGS[3]
    n, fb = args.n or cfg["n"], args.fb or cfg["fb"]
    steps = float(cfg["steps"]) * n / cfg["n"]
    device = torch.device("cuda", 0)
    abi.set_tunable("view_cache_mb", 0)
    abi.set_tunable("gpu_timing", 0)   # (no timing events of the library's own between the frames: the hit calls record none)
    res = abi.Resources((n, n, n), abi.DTYPE_FMT[np.dtype(cfg["dtype"])], cfg["light_32bit"], False, 0)
    vol = S.make_volume_torch((n, n, n), cfg["dtype"], S.seed_for_config(3), device)
    torch.cuda.synchronize()
    res.upload_volume_device(vol.data_ptr(), vol.numel() * vol.element_size())
    res.set_tf_lut(abi.color_curve_to_lut(S.tf_keys(cfg["tf"])))
    res.set_windowing(abi.WindowingParams(*cfg["window"]))
    world = S.default_world()
    res.clear_light_volume(0.0)
    for i in cfg["lights"]:
        res.add_dir_light(S.light(i), True, world)
    cam, tile, rp = S.default_camera(fb, fb), abi.Tile(0, 0, fb, fb), abi.RaymarchParams(steps, -1, True)
    stream = torch.cuda.ExternalStream(res.stream(), device=device)
    frame = torch.empty((fb, fb, 4), dtype=torch.float32, device=device)
    hits = torch.empty(fb * fb * 32, dtype=torch.uint8, device=device)
    depth = torch.empty(fb * fb, dtype=torch.float32, device=device)
    cases = {
        "lit": lambda: res.raymarch_lit_device(cam, tile, rp, world, frame.data_ptr()),
        "hit_005": lambda: res.raymarch_hits_device(cam, tile, rp, world, 0.05, hits.data_ptr(), depth.data_ptr()),
        "hit_095": lambda: res.raymarch_hits_device(cam, tile, rp, world, 0.95, hits.data_ptr(), depth.data_ptr()),
        "hit_095_nd": lambda: res.raymarch_hits_device(cam, tile, rp, world, 0.95, hits.data_ptr(), None),
    }
    # the same rays: the 0.95 map against the frame's alpha channel
    cases["lit"]()
    cases["hit_095"]()
    res.flush()
    rec = hits.cpu().numpy().view(abi.HIT_DTYPE).reshape(fb, fb)
    alpha = frame.cpu().numpy()[..., 3]
    in_full = (rec["sample"] >= 0) & (rec["sample"] < rec["full_steps"])
    tied = bool(np.array_equal(np.where(in_full, np.float32(1.0), rec["alpha"]).view(np.uint32), np.ascontiguousarray(alpha).view(np.uint32)))
    shares = {"hit_095": float((rec["sample"] >= 0).mean())}
    cases["hit_005"]()
    res.flush()
    shares["hit_005"] = float((hits.cpu().numpy().view(abi.HIT_DTYPE)["sample"] >= 0).mean())

    rounds = {k: [] for k in cases}
    for r in range(args.reps + 1):
        for name, fn in cases.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            for _ in range(args.launches):
                fn()
            b.record(stream)
            b.synchronize()
            if r:
                rounds[name].append(a.elapsed_time(b) / args.launches)
    out = {k: {"ms": round(float(np.median(v)), 4), "min_ms": round(float(min(v)), 4), "max_ms": round(float(max(v)), 4)} for k, v in rounds.items()}
    lit_spread = out["lit"]["max_ms"] - out["lit"]["min_ms"]

    walls = []
    for k in range(200 + 20):
        t0 = time.perf_counter()
        res.pick(cam, fb // 2, fb // 2, rp, world, 0.5)
        if k >= 20:
            walls.append((time.perf_counter() - t0) * 1e6)
    print(json.dumps({"tool": "hit_map_time", "note": args.note, "lib": os.path.basename(abi.LIB_PATH),
                      "workload": f"{n}^3 uint16, {fb} x {fb} rays, {steps:g} steps", "reps": args.reps, "launches": args.launches, **out,
                      "lit_spread_ms": round(lit_spread, 4), "hit_095_minus_lit_ms": round(out["hit_095"]["ms"] - out["lit"]["ms"], 4),
                      "hit_095_within_lit_spread": bool(out["hit_095"]["ms"] <= out["lit"]["ms"] + lit_spread),
                      "alpha_tied_to_lit": tied, "hit_share": {k: round(v, 4) for k, v in shares.items()},
                      "pick_wall_us": {"median": round(float(np.median(walls)), 1), "min": round(float(min(walls)), 1)},
                      "counters": res.hit_counters()}), flush=True)
    res.close()


if __name__ == "__main__":
    main()
