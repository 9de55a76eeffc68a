#!/usr/bin/env python3
"""What the label surface (include/tbrm_surface.h) costs, on config 3's volume — 512^3 UNORM16 — with the label grown from the picked
seed over the window's span (the label the other label tools time), against the route it replaces, in the same process:
  measure / measure_noskip         host wall time of one tbrm_label_surface call with TBRM_SURFACE_MEASURE (complete on return): the
                                   boards, the count, the scan, the read-back; surface_skip 1 / 0;
  quads / quads_noskip             a complete extraction onto device buffers: records, indices (4 per quad) and positions;
  triangles                        the same with 6 indices per quad;
  quads_no_positions               the same as quads without the positions;
  quads_to_host                    tbrm_label_surface onto host arrays: the extraction plus the copy of the mesh;
  download_label_volume            the host route's transfer alone: what a host mesher needs before it can begin, with NOTHING
                                   charged for the meshing.
A round takes the cases one after the other, each behind one untimed measuring call so that all have the same predecessor; --reps rounds
follow one that is thrown away, and the report is the median over the rounds with the smallest and the largest round (the spread). Prints one JSON line, and with --table FILE writes the table of DESIGN.md §23.

The floor — k_morph_load alone — and the split between the kernels are kernel times, which a host clock cannot give: run the tool
once more under `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o surface -- python tools/label_surface_time.py --reps 2` and pass the
kernel statistics it leaves to `--kernel-stats DIR/.../surface_kernel_stats.csv --table FILE` of a run that appends them to the table.

    python tools/label_surface_time.py [--reps 7] [--n 512] [--table profiles/r20_label_surface.txt] [--kernel-stats CSV]
"""
import argparse
import csv
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KERNELS = ("k_morph_load", "k_surface_count", "k_surface_scan_tiles", "k_surface_scan_top", "k_surface_emit")


def kernel_rows(path):
    """(name, calls, average ns) of the surface's kernels in a rocprofv3 kernel statistics CSV"""
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r.get("Name", "")
            for k in KERNELS:
                if name.startswith(k) or ("::" + k) in name:
                    rows.append((k, int(r["Calls"]), float(r["AverageNs"]), float(r["MinNs"]), float(r["MaxNs"])))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--n", type=int, default=0, help="volume edge (default: config 3's)")
    ap.add_argument("--table", default="", help="write the text table here")
    ap.add_argument("--kernel-stats", default="", help="a rocprofv3 kernel statistics CSV of this tool: append its kernel times to --table and stop")
    args = ap.parse_args()
    if args.kernel_stats:
        assert args.table, "--kernel-stats appends to --table"
        with open(args.table, "a") as f:
            f.write("Kernel times of the same calls in a run of their own under rocprofv3 --kernel-trace --stats (every variant above, mixed): calls, average us (min .. max)\n")
            for k, calls, avg, mn, mx in kernel_rows(args.kernel_stats):
                f.write(f"  {k:32s} {calls:5d} calls  {avg / 1e3:9.1f} ({mn / 1e3:.1f} .. {mx / 1e3:.1f})\n")
        return

    import torch

    from tbraymarcherplugin_amd import abi, synthetic as S

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

    info = {}
    for skip in (1, 0):
        abi.set_tunable("surface_skip", skip)
        m = res.measure_label_surface([1])
        info["skip%d" % skip] = {k: m[k] for k in ("set_voxels", "vertices", "quads", "blocks_evaluated", "blocks_skipped")}
    abi.set_tunable("surface_skip", 1)
    assert {k: v for k, v in info["skip0"].items() if not k.startswith("blocks")} == {k: v for k, v in info["skip1"].items() if not k.startswith("blocks")}
    nv, nq = m["vertices"], m["quads"]
    scale, offset = abi.surface_unit_cube((n, n, n))
    tv = torch.empty((nv, 5), dtype=torch.int32, device=device)
    ti = torch.empty((nq, 6), dtype=torch.int32, device=device)
    tp = torch.empty((nv, 3), dtype=torch.float32, device=device)
    hv, hi4, hp = np.zeros(nv, dtype=abi.SURFACE_VERTEX_DTYPE), np.zeros((nq, 4), dtype=np.uint32), np.zeros((nv, 3), dtype=np.float32)
    host_desc = res.surface_desc([1], scale=scale, offset=offset, vertex_capacity=nv, quad_capacity=nq)

    def to_host():
        out = abi.SURFACE_RESULT()
        abi.check(res.lib.tbrm_label_surface(res.handle, host_desc, hv.ctypes.data, hi4.ctypes.data, hp.ctypes.data, out))
        assert out.written == 1

    quads_view = ti.view(-1)[:nq * 4].view(nq, 4)
    cases = {
        "measure": (lambda: res.measure_label_surface([1]), 1),
        "measure_noskip": (lambda: res.measure_label_surface([1]), 0),
        "quads": (lambda: res.label_surface_device([1], tv, quads_view, tp, scale=scale, offset=offset), 1),
        "quads_noskip": (lambda: res.label_surface_device([1], tv, quads_view, tp, scale=scale, offset=offset), 0),
        "triangles": (lambda: res.label_surface_device([1], tv, ti, tp, triangles=True, scale=scale, offset=offset), 1),
        "quads_no_positions": (lambda: res.label_surface_device([1], tv, quads_view, None), 1),
        "quads_to_host": (to_host, 1),
        "download_label_volume": (lambda: res.download_label_volume(), 1),
    }
    rounds = {k: [] for k in cases}
    for r in range(args.reps + 1):
        for name, (fn, skip) in cases.items():
            abi.set_tunable("surface_skip", 1)
            res.measure_label_surface([1])   # every case follows the same call: what the case before it left in the caches is not its own
            abi.set_tunable("surface_skip", skip)
            res.flush()
            t0 = time.perf_counter()
            fn()   # (every case is complete on return)
            if r:
                rounds[name].append((time.perf_counter() - t0) * 1e3)
    abi.set_tunable("surface_skip", 1)
    # the mesh the timed calls left: the device form and the host form agree
    torch.cuda.synchronize()
    to_host()
    res.label_surface_device([1], tv, quads_view, tp, scale=scale, offset=offset)
    torch.cuda.synchronize()
    assert tv.cpu().numpy().tobytes() == hv.tobytes() and np.array_equal(quads_view.cpu().numpy().view(np.uint32), hi4) and tp.cpu().numpy().tobytes() == hp.tobytes()

    out = {k: {"ms": round(float(np.median(v)), 3), "min_ms": round(float(min(v)), 3), "max_ms": round(float(max(v)), 3)} for k, v in rounds.items()}
    mesh_bytes = {"quads": 20 * nv + 16 * nq + 12 * nv, "triangles": 20 * nv + 24 * nq + 12 * nv, "label_volume": n ** 3}
    result = {"tool": "label_surface_time", "workload": f"{n}^3, the label grown from the picked seed over the codes {lo} .. {hi}: {grown['voxels']} voxels", "reps": args.reps, **out,
              "cases": info, "bytes": mesh_bytes, "counters": res.surface_counters()}
    print(json.dumps(result), flush=True)
    if args.table:
        with open(args.table, "w") as f:
            i1, i0 = info["skip1"], info["skip0"]
            f.write(f"The label surface, {result['workload']}; wall ms per call, median (min .. max) of {args.reps} rounds\n")
            f.write(f"  the mesh: {nv} vertices, {nq} quads; {mesh_bytes['quads']} bytes as quads with positions, {mesh_bytes['triangles']} as triangles; the label volume: {n ** 3} bytes\n")
            f.write(f"  blocks of cells: surface_skip 1: {i1['blocks_evaluated']} evaluated / {i1['blocks_skipped']} skipped; surface_skip 0: {i0['blocks_evaluated']} / {i0['blocks_skipped']}\n")
            for name, (_, skip) in cases.items():
                o = out[name]
                f.write(f"  {name:32s} surface_skip {skip}: {o['ms']:9.3f} ({o['min_ms']:.3f} .. {o['max_ms']:.3f})\n")
    res.close()


if __name__ == "__main__":
    main()
