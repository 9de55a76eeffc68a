#!/usr/bin/env python3
"""What coloured lights (include/tbrm_color_lights.h) cost on config 3 (512^3 UNORM16, 1024^2 RGBA f32, 512 steps, four lights),
timed like bench.py — HIP events on the library's stream around each call, warm-up calls first, then the mean:

  * the lit frame on a mono handle against a colour handle that holds the same lights as white ones, for the UNORM8 and the
    float32 light volume;
  * ChangeDirLight (light 1 swinging 5 degrees about z and back) on the mono handle, and on the colour handle white -> white,
    white -> (1, 0.5, 0) (and back), and as a change of colour alone;
  * a coloured Add cold (the factor cache cleared before it) and warm (removed and added again: its factors are kept).

The yardstick of the coloured Change is three times the mono Change: three separate mono handles. Prints one JSON line.

    python tools/color_light_time.py [--calls 20] [--warmup 5]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch

    from tbraymarcherplugin_amd import abi, synthetic as S

    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    cfg = S.CONFIGS[3]
    n = cfg["n"]
    dims = (n, n, n)
    device = torch.device("cuda", 0)
    vol = S.make_volume_torch(dims, cfg["dtype"], S.seed_for_config(3), device)
    torch.cuda.synchronize()
    world = S.default_world()
    fb = cfg["fb"]
    cam = S.default_camera(fb, fb)
    tile = abi.Tile(0, 0, fb, fb)
    out = torch.empty((fb, fb, 4), dtype=torch.float32, device=device)
    rp = abi.RaymarchParams(float(cfg["steps"]), -1, True)

    def make(rgb, light32):
        res = abi.Resources(dims, abi.DTYPE_FMT[np.dtype(cfg["dtype"])], light32, False, 0, rgb=rgb)
        res.upload_volume_device(vol.data_ptr(), vol.numel() * vol.element_size())
        res.set_tf_lut(abi.color_curve_to_lut(S.tf_keys(cfg["tf"])))
        res.set_windowing(abi.WindowingParams(*cfg["window"]))
        res.reserve(len(cfg["lights"]))
        for i in cfg["lights"]:
            res.add_dir_light(S.light(i), True, world)   # (a colour handle: white)
        res.flush()
        return res

    def timed(res, calls):
        """mean ms of calls[k % len(calls)](), by events on the handle's stream"""
        stream = torch.cuda.ExternalStream(res.stream(), device=device)
        for k in range(args.warmup):
            calls[k % len(calls)]()
        res.flush()
        times = []
        for k in range(args.calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            calls[(args.warmup + k) % len(calls)]()
            e1.record(stream)
            e1.synchronize()
            times.append(float(e0.elapsed_time(e1)))
        res.flush()
        return round(float(np.mean(times)), 4)

    d0, i0 = S.LIGHTS[1]
    d1 = S.rotate_z(d0, 5.0)
    white, amber, teal = (1.0, 1.0, 1.0), (1.0, 0.5, 0.0), (0.2, 0.8, 1.0)
    result = {"frame_ms": {}, "change_ms": {}, "add_ms": {}}
    for light32 in (False, True):
        fmt = "float32_light" if light32 else "unorm8_light"
        mono, col = make(False, light32), make(True, light32)
        result["frame_ms"][fmt] = {
            "mono": timed(mono, [lambda: mono.raymarch_lit_device(cam, tile, rp, world, out.data_ptr())]),
            "colour_white_lights": timed(col, [lambda: col.raymarch_lit_device(cam, tile, rp, world, out.data_ptr())]),
        }
        if not light32:   # the operators on config 3's own light volume format
            ma, mb = abi.DirLightParams(d0, i0), abi.DirLightParams(d1, i0)
            ch = {"mono": timed(mono, [lambda: mono.change_dir_light(ma, mb, world), lambda: mono.change_dir_light(mb, ma, world)])}
            ch["mono_x3_yardstick"] = round(3 * ch["mono"], 4)

            def swing(ca, cb):
                a, b = abi.ColorDirLight(d0, i0, ca), abi.ColorDirLight(d1, i0, cb)
                return [lambda: col.change_color_dir_light(a, b, world), lambda: col.change_color_dir_light(b, a, world)]

            ch["colour_white_to_white"] = timed(col, swing(white, white))
            ch["colour_white_to_amber"] = timed(col, swing(white, amber))
            a, b = abi.ColorDirLight(d0, i0, white), abi.ColorDirLight(d0, i0, teal)
            ch["colour_only"] = timed(col, [lambda: col.change_color_dir_light(a, b, world), lambda: col.change_color_dir_light(b, a, world)])
            result["change_ms"] = ch
            extra = abi.ColorDirLight(S.LIGHTS[4][0], S.LIGHTS[4][1], amber)

            def cold():
                col.light_cache_clear()
                col.add_color_dir_light(extra, True, world)
                col.add_color_dir_light(extra, False, world)

            def warm():
                col.add_color_dir_light(extra, True, world)
                col.add_color_dir_light(extra, False, world)

            # (each call is an Add and its removal, so that the light volume stays what it was; the removal runs from kept factors)
            result["add_ms"] = {"cold_add_plus_warm_remove": timed(col, [cold]), "warm_add_plus_warm_remove": timed(col, [warm])}
        mono.close()
        col.close()
    print(json.dumps({"tool": "color_light_time", "workload": f"config 3: {n}^3 uint16, {fb}^2 RGBA f32, {cfg['steps']} steps, "
                      f"{len(cfg['lights'])} lights", "calls": args.calls, "warmup": args.warmup, **result}), flush=True)


if __name__ == "__main__":
    main()
