"""ARaymarchVolume::ScissorLabel / EraseInsideLasso / KeepInsideLasso / FillInsideLasso (include/tbrm_plugin.hpp) and
examples/render_mhd.cpp --scissors: tests/cpp/scissors_test.cpp builds against the C-ABI with plain g++; an actor without resources
refuses all four; on a GPU a slab of label voxels is cut and filled under a concave lasso on the example's camera and every label volume
equals the program's own restatement by loops; the example prints what the binding's call gives for the same label volume."""
import os
import subprocess

import pytest

from test_facade import build_example

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "scissors_test.cpp")
LIB_DIR = os.path.join(ROOT, "tbraymarcherplugin_amd", "lib")


def build(tmp_path):
    exe = str(tmp_path / "scissors_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), SRC, "-o", exe,
                    "-L", LIB_DIR, "-ltbrm", "-lz", f"-Wl,-rpath,{LIB_DIR}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def test_scissors_facade_compiles_and_refuses_without_resources(tmp_path, abi_mod):
    out = subprocess.run([build(tmp_path), "nohandle"], check=True, capture_output=True, text=True).stdout
    assert out.strip() == "nohandle scissor=0 erase=0 keep=0 fill=0 removed=0 recompute=0 abi=1"


@pytest.mark.gpu
def test_scissor_label_through_the_facade_on_gpu(tmp_path, gpu):
    p = subprocess.run([build(tmp_path), str(tmp_path)], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), p.stdout + p.stderr
    lines = dict(l.split(" ", 1) for l in p.stdout.strip().splitlines() if " " in l)
    assert lines["nolabels"] == "refused=1"
    for name in ("erase", "fill", "near", "keep", "fill_outside"):   # each on the labels the one before left
        assert lines[name] == "wrong=0 counts=1 moved=1 cut=1 pixels=1", (name, lines[name])
    assert lines["measure"] == "removed=1 relabelled=0 unchanged=1"
    assert lines["erase_label"] == "removed_got_it=1"
    assert lines["refused"] == "two=1 odd=1 label=1 op=1 depth=1"
    assert lines["state"] == "frames=0 resets=0 recompute=0"        # a label edit is no frame and requests nothing
    assert lines["frame"] == "shows_change=1"
    assert lines["counters"] == "calls=7"                           # the refused calls never counted


@pytest.mark.gpu
def test_example_scissors_prints_the_bindings_result(tmp_path, gpu):
    import numpy as np
    from tbraymarcherplugin_amd import abi, synthetic as S
    import label_scissors_reference as SR

    dims = (48, 40, 36)
    vol = S.make_volume_numpy(dims, np.float32, 0x5EED0A00)
    (vol * 3000.0 - 1000.0).astype(np.int16).tofile(tmp_path / "ct.raw")
    (tmp_path / "ct.mhd").write_text("ObjectType = Image\nNDims = 3\nDimSize = 48 40 36\nElementSpacing = 0.7 0.7 2.5\n"
                                     "ElementType = MET_SHORT\nElementDataFile = ct.raw\n")
    example = build_example(tmp_path)
    args = [example, str(tmp_path / "ct.mhd"), str(tmp_path / "out.ppm"), "96", "64", "80"]
    lasso = "20,10,70.5,14,50,30,66,58,24,50"
    p = subprocess.run(args + ["--grow", "48,32,3000,5", "--scissors", "erase_inside,5," + lasso], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    grow = [l for l in p.stdout.splitlines() if l.startswith("grow ")][0].split()
    got = [l for l in p.stdout.splitlines() if l.startswith("scissors ")]
    assert len(got) == 1 and p.stdout.index("grow ") < p.stdout.index("scissors "), p.stdout
    w = got[0].split()
    assert w[:6] == ["scissors", "erase_inside", "label", "5", "points", "5"] and w[6::2][:5] == ["pixels", "source", "result", "added", "removed"]
    assert w[16] == "box" and w[24] == "bricks" and w[26] == "inside" and w[28] == "outside" and w[30:32] == ["projected", "launches"]
    seed, lo, hi = tuple(int(v) for v in grow[3:6]), float(grow[7]), float(grow[9])
    # the same grow and the same cut through the binding on the volume the example loaded (the loader's normalisation and camera restated)
    raw = np.fromfile(tmp_path / "ct.raw", dtype=np.int16).reshape(dims[::-1]).astype(np.float32)
    norm = (raw - np.float32(raw.min())) / np.float32(raw.max() - raw.min())
    codes = (norm * np.float32(65535.0)).astype(np.uint16)
    cam = abi.look_at_camera((-145.0, -95.0, 80.0), (0.0, 0.0, 0.0), (0.0, 0.0, 1.0), 50.0, 96, 64)
    world = abi.make_world()
    points = np.array([float(v) for v in lasso.split(",")]).reshape(-1, 2)
    mask = abi.scissors_polygon(points, 96, 64)
    with abi.Resources(dims, abi.FMT_G16) as res:
        res.upload_volume(codes)
        res.attach_empty_labels()
        g = res.grow_region([seed], lo, hi, 5, 6)
        r = res.scissor_labels(abi.scissors_projection(dims, world, cam), mask, "erase_inside", [5], 5)
    assert int(w[7]) == int(SR.mask_bits(mask, 96).sum()) > 500
    assert int(w[9]) == g["voxels"] == r["source_voxels"]
    assert [int(w[11]), int(w[13]), int(w[15])] == [r["result_voxels"], r["added"], r["removed"]] and r["removed"] > 0 and r["result_voxels"] > 0
    assert [int(v) for v in w[17:20] + w[21:24]] == list(r["bbox_min"]) + list(r["bbox_max"])
    assert [int(w[23 + 2]), int(w[27]), int(w[29]), int(w[32])] == [r["bricks_inside"], r["bricks_outside"], r["bricks_projected"], r["launches"]]
    # the other operators by name, a bad operator, too few points, and no label volume to work on
    p = subprocess.run(args + ["--grow", "48,32,3000,5", "--scissors", "erase_outside,5," + lasso], capture_output=True, text=True)
    assert p.returncode == 0 and f"scissors erase_outside label 5 points 5 pixels {w[7]} source {w[9]} result {w[15]} added 0 removed {w[11]} " in p.stdout, p.stdout + p.stderr
    p = subprocess.run(args + ["--grow", "48,32,3000,5", "--scissors", "cut,5," + lasso], capture_output=True, text=True)
    assert p.returncode == 1 and "OP must be" in p.stderr
    p = subprocess.run(args + ["--scissors", "erase_inside,5,1,1,9,9"], capture_output=True, text=True)
    assert p.returncode == 2 and "usage" in p.stderr
    p = subprocess.run(args + ["--scissors", "fill_inside,5," + lasso], capture_output=True, text=True)
    assert p.returncode == 1 and "scissors failed" in p.stderr and "label volume" in p.stderr
