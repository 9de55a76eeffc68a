"""ARaymarchVolume::GrowFromSeeds / StepCostFromSpacing (include/tbrm_plugin.hpp) and examples/render_mhd.cpp --compete:
tests/cpp/compete_test.cpp builds against the C-ABI with plain g++; an actor without resources refuses; on a GPU two painted balls
in a two-phase volume split it where the program's own Dijkstra does; the example prints what the binding's call gives for the same
volume and the same painted balls."""
import os
import subprocess

import pytest

from test_facade import build_example

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "compete_test.cpp")
LIB_DIR = os.path.join(ROOT, "tbraymarcherplugin_amd", "lib")


def build(tmp_path):
    exe = str(tmp_path / "compete_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), SRC, "-o", exe,
                    "-L", LIB_DIR, "-ltbrm", "-lz", f"-Wl,-rpath,{LIB_DIR}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def test_compete_facade_compiles_and_refuses_without_resources(tmp_path, abi_mod):
    out = subprocess.run([build(tmp_path), "nohandle"], check=True, capture_output=True, text=True).stdout
    assert out.strip() == "nohandle grow=0 claimed=0 recompute=0 abi=1 unit=16,16,16 aniso=16,16,57"   # 16 * 2.5 / 0.7 = 57.1


@pytest.mark.gpu
def test_grow_from_seeds_through_the_facade_on_gpu(tmp_path, gpu):
    p = subprocess.run([build(tmp_path), str(tmp_path)], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), p.stdout + p.stderr
    lines = dict(l.split(" ", 1) for l in p.stdout.strip().splitlines() if " " in l)
    assert lines["nolabels"] == "refused=1"
    for name in ("measure", "limited", "whole"):   # each on the labels the one before left
        assert lines[name] == "wrong=0 costs=0 counts=1 both=1 steps=8,8,20", (name, lines[name])
    assert lines["split"] == "dense=1 thin=1"                       # the balls took their own phase
    assert lines["refused"] == "none=1 label=1 shift=1 cost=1"
    assert lines["state"] == "frames=0 resets=0 recompute=0"        # a label edit is no frame and requests nothing
    assert lines["counters"] == "calls=3"                           # the refused calls never counted


@pytest.mark.gpu
def test_example_compete_prints_the_bindings_result(tmp_path, gpu):
    import numpy as np
    from tbraymarcherplugin_amd import abi, synthetic as S

    dims = (48, 40, 36)
    vol = S.make_volume_numpy(dims, np.float32, 0x5EED0A00)
    (vol * 3000.0 - 1000.0).astype(np.int16).tofile(tmp_path / "ct.raw")
    (tmp_path / "ct.mhd").write_text("ObjectType = Image\nNDims = 3\nDimSize = 48 40 36\nElementSpacing = 0.7 0.7 2.5\n"
                                     "ElementType = MET_SHORT\nElementDataFile = ct.raw\n")
    example = build_example(tmp_path)
    args = [example, str(tmp_path / "ct.mhd"), str(tmp_path / "out.ppm"), "96", "64", "80"]
    balls = [(1, 10, 10, 10, 3), (2, 36, 28, 24, 2), (7, 24, 20, 4, 0)]
    spec = "4,5,3000," + ",".join("%d@%d,%d,%d,%d" % b for b in balls)
    p = subprocess.run(args + ["--compete", spec], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    got = [l for l in p.stdout.splitlines() if l.startswith("compete ")]
    assert len(got) == 1, p.stdout
    w = got[0].split()
    assert w[1:5] == ["step", "4", "4", "14"] and w[5:9] == ["shift", "5", "limit", "3000"]   # 4 * 2.5 / 0.7 = 14.3
    assert w[9::2][:5] == ["seeds", "claimable", "claimed", "relabelled", "max_cost"] and w[19] == "box" and w[27] == "passes" and w[29] == "per_label"
    # the same balls and the same call through the binding on the volume the example loaded (the loader's normalisation restated)
    raw = np.fromfile(tmp_path / "ct.raw", dtype=np.int16).reshape(dims[::-1]).astype(np.float32)
    norm = (raw - np.float32(raw.min())) / np.float32(raw.max() - raw.min())
    codes = (norm * np.float32(65535.0)).astype(np.uint16)
    labels = np.zeros(codes.shape, dtype=np.uint8)
    z, y, x = np.indices(labels.shape)
    for l, bx, by, bz, r in balls:
        labels[(x - bx) ** 2 + (y - by) ** 2 + (z - bz) ** 2 <= r * r] = l
    with abi.Resources(dims, abi.FMT_G16) as res:
        res.upload_volume(codes)
        res.upload_label_volume(labels)
        r = res.compete_labels([1, 2, 7], 0, 65535, step_cost=(4, 4, 14), value_shift=5, cost_limit=3000)
    assert [int(v) for v in w[10:19:2]] == [r["seed_voxels"], r["claimable"], r["claimed"], r["relabelled"], r["max_cost"]] and r["claimed"] > 1000
    assert [int(v) for v in w[20:23] + w[24:27]] == list(r["bbox_min"]) + list(r["bbox_max"])
    assert {int(k): int(v) for k, v in (t.split(":") for t in w[30:])} == r["claimed_per_label"] and len(r["claimed_per_label"]) == 3
    assert 1 <= int(w[28]) and r["max_cost"] <= 3000
    # what the example refuses: a bad spelling, a label out of range
    p = subprocess.run(args + ["--compete", "4,5"], capture_output=True, text=True)
    assert p.returncode == 2 and "usage" in p.stderr and "--compete COST,SHIFT,LIMIT,LABEL@X,Y,Z,R" in p.stderr
    p = subprocess.run(args + ["--compete", "4,5,0,0@3,3,3,1"], capture_output=True, text=True)
    assert p.returncode == 1 and "compete failed" in p.stderr
