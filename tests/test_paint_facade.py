"""ARaymarchVolume::PaintLabel / EraseLabel / PaintAlongHits (include/tbrm_plugin.hpp) and examples/render_mhd.cpp --paint:
tests/cpp/paint_test.cpp builds against the C-ABI with plain g++; an actor without resources refuses every call; on a GPU a ball, a
stroke and an erasure, a gated and boxed stroke and a stroke along hits are painted into the labels of an anisotropic volume and
every label volume equals the program's own restatement by loops; the example prints what the binding's call gives for the same
label volume."""
import os
import subprocess

import pytest

from test_facade import build_example

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "paint_test.cpp")
LIB_DIR = os.path.join(ROOT, "tbraymarcherplugin_amd", "lib")


def build(tmp_path):
    exe = str(tmp_path / "paint_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), SRC, "-o", exe,
                    "-L", LIB_DIR, "-ltbrm", "-lz", f"-Wl,-rpath,{LIB_DIR}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def test_paint_facade_compiles_and_refuses_without_resources(tmp_path, abi_mod):
    out = subprocess.run([build(tmp_path), "nohandle"], check=True, capture_output=True, text=True).stdout
    assert out.strip() == "nohandle paint=0 erase=0 hits=0 stroke=0 added=0 recompute=0 abi=1"


@pytest.mark.gpu
def test_paint_label_through_the_facade_on_gpu(tmp_path, gpu):
    p = subprocess.run([build(tmp_path), str(tmp_path)], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), p.stdout + p.stderr
    lines = dict(l.split(" ", 1) for l in p.stdout.strip().splitlines() if " " in l)
    assert lines["nolabels"] == "refused=1"
    assert lines["brush"] == "spacing=1 weights=256,256,1600 limit=147456"   # 64 * 256 * 3^2 in eighths squared
    for name in ("ball", "stroke", "erase"):   # each on the labels the one before left
        assert lines[name] == "wrong=0 counts=1 moved=1 brush=1", (name, lines[name])
    assert lines["measure"] == "added=1 relabelled=0 unchanged=1"
    assert lines["gated"] == "wrong=0 added=1"
    assert lines["hits"] == "wrong=0 points=3 segments=2 added=1 nohit=1"
    assert lines["pick"] == "hit=1 uvw=1 painted=1"
    assert lines["refused"] == "none=1 ragged=1 label=1 radius=1 op=1"
    assert lines["state"] == "frames=0 resets=0 recompute=0"        # a label edit is no frame and requests nothing
    assert lines["frame"] == "shows_change=1"
    assert lines["counters"] == "calls=7"                           # the refused calls never counted


@pytest.mark.gpu
def test_example_paint_prints_the_bindings_result(tmp_path, gpu):
    import numpy as np
    from tbraymarcherplugin_amd import abi, synthetic as S

    dims = (48, 40, 36)
    vol = S.make_volume_numpy(dims, np.float32, 0x5EED0A00)
    (vol * 3000.0 - 1000.0).astype(np.int16).tofile(tmp_path / "ct.raw")
    (tmp_path / "ct.mhd").write_text("ObjectType = Image\nNDims = 3\nDimSize = 48 40 36\nElementSpacing = 0.7 0.7 2.5\n"
                                     "ElementType = MET_SHORT\nElementDataFile = ct.raw\n")
    example = build_example(tmp_path)
    args = [example, str(tmp_path / "ct.mhd"), str(tmp_path / "out.ppm"), "96", "64", "80"]
    stroke = "10,8,6;30.5,20,18;40,33.25,30"
    p = subprocess.run(args + ["--paint", "5,4.0@" + stroke], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    got = [l for l in p.stdout.splitlines() if l.startswith("paint ")]
    assert len(got) == 1, p.stdout
    w = got[0].split()
    assert w[:6] == ["paint", "label", "5", "radius", "4", "points"] and w[7::2][:5] == ["segments", "stamp", "added", "removed", "relabelled"], w
    assert w[17] == "box" and w[25] == "bricks" and w[27::2][:3] == ["whole", "untouched", "evaluated"] and w[32] == "launches", w
    # the same stroke through the binding: the example's points are voxels, rounded to eighths
    points = np.rint(8.0 * np.array([[float(v) for v in q.split(",")] for q in stroke.split(";")])).astype(np.int32)
    weights, limit = abi.paint_brush((0.7, 0.7, 2.5), 4.0)
    with abi.Resources(dims, abi.FMT_G16) as res:
        res.upload_volume(np.zeros(dims[::-1], dtype=np.uint16))
        res.attach_empty_labels()
        r = res.paint_labels(points, weights, limit, "paint", [5], 5)
    assert [int(w[6]), int(w[8])] == [3, 2] == [len(points), r["segments"]]
    assert [int(w[10]), int(w[12]), int(w[14]), int(w[16])] == [r["stamp_voxels"], r["added"], r["removed"], r["relabelled"]] and r["added"] == r["stamp_voxels"] > 100
    assert [int(v) for v in w[18:21] + w[22:25]] == list(r["bbox_min"]) + list(r["bbox_max"])
    assert [int(w[26]), int(w[28]), int(w[30]), int(w[33])] == [r["bricks_whole"], r["bricks_untouched"], r["bricks_evaluated"], r["launches"]]
    # one point is a ball; a bad label, a missing radius and a point with two coordinates
    p = subprocess.run(args + ["--paint", "5,4.0@24,20,18"], capture_output=True, text=True)
    assert p.returncode == 0 and "paint label 5 radius 4 points 1 segments 1 " in p.stdout, p.stdout + p.stderr
    p = subprocess.run(args + ["--paint", "300,4.0@24,20,18"], capture_output=True, text=True)
    assert p.returncode == 1 and "paint failed" in p.stderr
    p = subprocess.run(args + ["--paint", "5@24,20,18"], capture_output=True, text=True)
    assert p.returncode == 2 and "usage" in p.stderr
    p = subprocess.run(args + ["--paint", "5,4.0@24,20"], capture_output=True, text=True)
    assert p.returncode == 2 and "usage" in p.stderr
