"""ARaymarchVolume::SmoothLabel / MedianLabel (include/tbrm_plugin.hpp) and examples/render_mhd.cpp --smooth: tests/cpp/smooth_test.cpp
builds against the C-ABI with plain g++; an actor without resources refuses both; on a GPU a ball of label voxels with a spur, a pit
and a speck on a volume with ElementSpacing 1 1 2.5 is smoothed by world radii and every label volume equals the program's own
brute-force restatement; the example prints what the binding's call gives for the same label volume."""
import os
import subprocess

import pytest

from test_facade import build_example

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "smooth_test.cpp")
LIB_DIR = os.path.join(ROOT, "tbraymarcherplugin_amd", "lib")


def build(tmp_path):
    exe = str(tmp_path / "smooth_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), SRC, "-o", exe,
                    "-L", LIB_DIR, "-ltbrm", "-lz", f"-Wl,-rpath,{LIB_DIR}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def test_smooth_facade_compiles_and_refuses_without_resources(tmp_path, abi_mod):
    out = subprocess.run([build(tmp_path), "nohandle"], check=True, capture_output=True, text=True).stdout
    assert out.strip() == "nohandle smooth=0 median=0 added=0 recompute=0 abi=1"


@pytest.mark.gpu
def test_smooth_label_through_the_facade_on_gpu(tmp_path, gpu):
    p = subprocess.run([build(tmp_path), str(tmp_path)], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), p.stdout + p.stderr
    lines = dict(l.split(" ", 1) for l in p.stdout.strip().splitlines() if " " in l)
    assert lines["spacing"] == "loaded=1"
    assert lines["nolabels"] == "refused=1"
    # world radii on 1 x 1 x 2.5 voxels: r_a = floor(radius / spacing_a + 0.5)
    assert lines["median"] == "wrong=0 counts=1 moved=1 radius=1,1,0 reach=1,1,0 launches=1"
    assert lines["median3"] == "wrong=0 counts=1 moved=1 radius=3,3,1 reach=3,3,1 launches=1"
    assert lines["twice"].startswith("wrong=0 counts=1 ") and lines["twice"].endswith(" radius=2,2,1 reach=4,4,2 launches=2")
    assert lines["third"] == "wrong=0 counts=1 moved=1 radius=2,2,1 reach=2,2,1 launches=1"
    assert lines["median_unit"] == "wrong=0 counts=1 moved=1 radius=2,2,2 reach=2,2,2 launches=1"   # no spacing: 2 voxels
    assert lines["features"] == "pit_filled=1 spur_cut=1 speck_removed=1 ball_kept=1"
    assert lines["measure"] == "added=1 relabelled=0 unchanged=1"
    assert lines["erase_label"] == "removed_got_it=1"
    assert lines["refused"] == "small=1 large=1 nan=1 iterations=1 reach=1 rank=1"
    assert lines["state"] == "frames=0 resets=0 recompute=0"        # a label edit is no frame and requests nothing
    assert lines["frame"] == "shows_change=1"
    assert lines["counters"] == "calls=7 launches=8"                # the refused calls never counted


@pytest.mark.gpu
def test_example_smooth_prints_the_bindings_result(tmp_path, gpu):
    import numpy as np
    from tbraymarcherplugin_amd import abi, synthetic as S

    dims = (48, 40, 36)
    vol = S.make_volume_numpy(dims, np.float32, 0x5EED0A00)
    (vol * 3000.0 - 1000.0).astype(np.int16).tofile(tmp_path / "ct.raw")
    (tmp_path / "ct.mhd").write_text("ObjectType = Image\nNDims = 3\nDimSize = 48 40 36\nElementSpacing = 0.7 0.7 2.5\n"
                                     "ElementType = MET_SHORT\nElementDataFile = ct.raw\n")
    example = build_example(tmp_path)
    args = [example, str(tmp_path / "ct.mhd"), str(tmp_path / "out.ppm"), "96", "64", "80"]
    p = subprocess.run(args + ["--grow", "48,32,3000,5", "--smooth", "2,2"], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    grow = [l for l in p.stdout.splitlines() if l.startswith("grow ")][0].split()
    got = [l for l in p.stdout.splitlines() if l.startswith("smooth ")]
    assert len(got) == 1 and p.stdout.index("grow ") < p.stdout.index("smooth "), p.stdout
    w = got[0].split()
    assert w[:6] == ["smooth", "2", "iterations", "2", "label", "5"] and w[6] == "radius" and w[10] == "reach"
    assert w[14::2][:4] == ["source", "result", "added", "removed"] and w[22] == "box" and w[30] == "launches"
    seed, lo, hi = tuple(int(v) for v in grow[3:6]), float(grow[7]), float(grow[9])
    radius = abi.smooth_radii((0.7, 0.7, 2.5), 2.0)
    assert [int(v) for v in w[7:10]] == list(radius) == [3, 3, 1]
    # the same grow and the same median through the binding on the volume the example loaded (the loader's normalisation restated)
    raw = np.fromfile(tmp_path / "ct.raw", dtype=np.int16).reshape(dims[::-1]).astype(np.float32)
    norm = (raw - np.float32(raw.min())) / np.float32(raw.max() - raw.min())
    codes = (norm * np.float32(65535.0)).astype(np.uint16)
    with abi.Resources(dims, abi.FMT_G16) as res:
        res.upload_volume(codes)
        res.attach_empty_labels()
        g = res.grow_region([seed], lo, hi, 5, 6)
        r = res.smooth_labels(radius, [5], 5, iterations=2)
    assert [int(v) for v in w[11:14]] == list(r["reach"]) == [6, 6, 2]
    assert int(w[15]) == g["voxels"] == r["source_voxels"]
    assert [int(w[17]), int(w[19]), int(w[21])] == [r["result_voxels"], r["added"], r["removed"]] and r["removed"] + r["added"] > 0
    assert [int(v) for v in w[23:26] + w[27:30]] == list(r["bbox_min"]) + list(r["bbox_max"]) and int(w[31]) == r["launches"] == 2
    # one pass by default and a label of its own choosing, a radius below half a voxel, and no label volume to work on
    p = subprocess.run(args + ["--grow", "48,32,3000,5", "--smooth", "0.7"], capture_output=True, text=True)
    assert p.returncode == 0 and "smooth 0.7 iterations 1 label 5 radius 1 1 0" in p.stdout, p.stdout + p.stderr
    p = subprocess.run(args + ["--grow", "48,32,3000,5", "--smooth", "2,1,5"], capture_output=True, text=True)
    assert p.returncode == 0 and "smooth 2 iterations 1 label 5 radius 3 3 1" in p.stdout, p.stdout + p.stderr
    p = subprocess.run(args + ["--grow", "48,32,3000,5", "--smooth", "0.3"], capture_output=True, text=True)
    assert p.returncode == 1 and "smooth failed" in p.stderr
    p = subprocess.run(args + ["--smooth", "1"], capture_output=True, text=True)
    assert p.returncode == 1 and "smooth failed" in p.stderr and "label volume" in p.stderr
