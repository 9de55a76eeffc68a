"""ARaymarchVolume::MarginLabel / ExpandLabelBy / ShrinkLabelBy / OpenLabelBy / CloseLabelBy (include/tbrm_plugin.hpp) and
examples/render_mhd.cpp --margin: tests/cpp/margin_test.cpp builds against the C-ABI with plain g++; an actor without resources
refuses all five; on a GPU a ball of label voxels on a volume with ElementSpacing 1 1 2.5 is closed, opened, expanded and shrunk by
world radii and every label volume equals the program's own brute-force restatement; the example prints what the binding's call gives
for the same label volume."""
import os
import subprocess

import pytest

from test_facade import build_example

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "margin_test.cpp")
LIB_DIR = os.path.join(ROOT, "tbraymarcherplugin_amd", "lib")


def build(tmp_path):
    exe = str(tmp_path / "margin_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), SRC, "-o", exe,
                    "-L", LIB_DIR, "-ltbrm", "-lz", f"-Wl,-rpath,{LIB_DIR}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def test_margin_facade_compiles_and_refuses_without_resources(tmp_path, abi_mod):
    out = subprocess.run([build(tmp_path), "nohandle"], check=True, capture_output=True, text=True).stdout
    assert out.strip() == "nohandle margin=0 expand=0 shrink=0 open=0 close=0 added=0 recompute=0 abi=1"


@pytest.mark.gpu
def test_margin_label_through_the_facade_on_gpu(tmp_path, gpu):
    p = subprocess.run([build(tmp_path), str(tmp_path)], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), p.stdout + p.stderr
    lines = dict(l.split(" ", 1) for l in p.stdout.strip().splitlines() if " " in l)
    assert lines["spacing"] == "loaded=1"
    assert lines["nolabels"] == "refused=1"
    for name in ("close", "open", "expand", "shrink", "expand_unit"):
        assert lines[name] == "wrong=0 counts=1 moved=1", (name, p.stdout)
    assert lines["pinhole"] == "filled=1"
    assert lines["speck"] == "removed=1 ball_kept=1"
    assert lines["quantised"] == "weights=256,256,1600 limit=2304 reach=3,3,1"    # 3 world units on 1 x 1 x 2.5 voxels
    assert lines["unit"] == "weights=256,256,256 limit=1024 reach=2,2,2"          # no spacing: 2 voxels
    assert lines["measure"] == "added=1 relabelled=0 unchanged=1"
    assert lines["erase_label"] == "removed_got_it=1"
    assert lines["refused"] == "small=1 large=1 nan=1"
    assert lines["state"] == "frames=0 resets=0 recompute=0"        # a label edit is no frame and requests nothing
    assert lines["frame"] == "shows_change=1"
    assert lines["counters"] == "calls=7 launches=27"               # the refused calls never counted


@pytest.mark.gpu
def test_example_margin_prints_the_bindings_result(tmp_path, gpu):
    import numpy as np
    from tbraymarcherplugin_amd import abi, synthetic as S

    dims = (48, 40, 36)
    vol = S.make_volume_numpy(dims, np.float32, 0x5EED0A00)
    (vol * 3000.0 - 1000.0).astype(np.int16).tofile(tmp_path / "ct.raw")
    (tmp_path / "ct.mhd").write_text("ObjectType = Image\nNDims = 3\nDimSize = 48 40 36\nElementSpacing = 0.7 0.7 2.5\n"
                                     "ElementType = MET_SHORT\nElementDataFile = ct.raw\n")
    example = build_example(tmp_path)
    args = [example, str(tmp_path / "ct.mhd"), str(tmp_path / "out.ppm"), "96", "64", "80"]
    p = subprocess.run(args + ["--grow", "48,32,3000,5", "--margin", "expand,3.5"], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    grow = [l for l in p.stdout.splitlines() if l.startswith("grow ")][0].split()
    got = [l for l in p.stdout.splitlines() if l.startswith("margin ")]
    assert len(got) == 1 and p.stdout.index("grow ") < p.stdout.index("margin "), p.stdout
    w = got[0].split()
    assert w[:5] == ["margin", "expand", "3.5", "label", "5"] and w[5] == "weights" and w[9] == "limit" and w[11] == "reach"
    assert w[15::2][:4] == ["source", "result", "added", "removed"] and w[23] == "box" and w[31] == "launches"
    seed, lo, hi = tuple(int(v) for v in grow[3:6]), float(grow[7]), float(grow[9])
    weights, limit = abi.margin_weights((0.7, 0.7, 2.5), 3.5)
    assert [int(v) for v in w[6:9]] == list(weights) == [256, 256, 3265] and int(w[10]) == limit == 6400
    # the same grow and the same margin through the binding on the volume the example loaded (the loader's normalisation restated)
    raw = np.fromfile(tmp_path / "ct.raw", dtype=np.int16).reshape(dims[::-1]).astype(np.float32)
    norm = (raw - np.float32(raw.min())) / np.float32(raw.max() - raw.min())
    codes = (norm * np.float32(65535.0)).astype(np.uint16)
    with abi.Resources(dims, abi.FMT_G16) as res:
        res.upload_volume(codes)
        res.attach_empty_labels()
        g = res.grow_region([seed], lo, hi, 5, 6)
        r = res.margin_labels("expand", weights, limit, [5], 5)
    assert [int(v) for v in w[12:15]] == list(r["reach"]) == [5, 5, 1]
    assert int(w[16]) == g["voxels"] == r["source_voxels"]
    assert [int(w[18]), int(w[20]), int(w[22])] == [r["result_voxels"], r["added"], r["removed"]] and r["removed"] == 0 and r["added"] > 0
    assert [int(v) for v in w[24:27] + w[28:31]] == list(r["bbox_min"]) + list(r["bbox_max"]) and int(w[32]) == r["launches"] == 3
    # a label of its own choosing, an operator that does not exist, a radius below one voxel, and no label volume to work on
    p = subprocess.run(args + ["--grow", "48,32,3000,5", "--margin", "shrink,0.7,5"], capture_output=True, text=True)
    assert p.returncode == 0 and " removed " in p.stdout and "margin shrink 0.7 label 5" in p.stdout, p.stdout + p.stderr
    p = subprocess.run(args + ["--grow", "48,32,3000,5", "--margin", "smooth,1"], capture_output=True, text=True)
    assert p.returncode == 1 and "margin failed" in p.stderr and "OP must be" in p.stderr
    p = subprocess.run(args + ["--grow", "48,32,3000,5", "--margin", "expand,0.5"], capture_output=True, text=True)
    assert p.returncode == 1 and "margin failed" in p.stderr
    p = subprocess.run(args + ["--margin", "open,1"], capture_output=True, text=True)
    assert p.returncode == 1 and "margin failed" in p.stderr and "label volume" in p.stderr
