"""ARaymarchVolume::PickVolume / RenderHitDepth (include/tbrm_plugin.hpp) and examples/render_mhd.cpp --pick: tests/cpp/hit_test.cpp
builds against the C-ABI with plain g++; an actor without resources refuses both; on a GPU the facade's answers are tbrm_pick's and
tbrm_raymarch_hits', they neither count as frames nor change the next one, and the example prints the hit the C-ABI call gives."""
import os
import subprocess

import pytest

from test_facade import build_example

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "hit_test.cpp")
LIB_DIR = os.path.join(ROOT, "tbraymarcherplugin_amd", "lib")


def build(tmp_path):
    exe = str(tmp_path / "hit_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), SRC, "-o", exe,
                    "-L", LIB_DIR, "-ltbrm", "-lz", f"-Wl,-rpath,{LIB_DIR}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def test_hit_facade_compiles_and_refuses_without_resources(tmp_path, abi_mod):
    out = subprocess.run([build(tmp_path), "nohandle"], check=True, capture_output=True, text=True).stdout
    assert out.strip() == "nohandle pick=0 depth=0 hit=0 untouched=1 recompute=0 abi=1"


@pytest.mark.gpu
def test_pick_and_hit_depth_through_the_facade_on_gpu(tmp_path, gpu):
    p = subprocess.run([build(tmp_path)], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), p.stdout + p.stderr
    lines = dict(l.split(" ", 1) for l in p.stdout.strip().splitlines() if " " in l)
    assert lines["depth"] == "equal=1 hits=1 misses=1"
    assert lines["pick"].startswith("same=1 on_depth=1 picks=100 hits=")
    n_hits = int(lines["pick"].rsplit("=", 1)[1])
    assert 8 <= n_hits <= 92                                      # the grid of picks meets the ball and misses it
    assert lines["labelled"] == "hit=1 label_in_range=1"
    assert lines["state"] == "frames=0 resets=0 recompute=0"      # a pick is no frame and requests nothing
    assert lines["frame"] == "identical=1"
    assert lines["counters"] == "maps=2 picks=101 launches=103"   # the 10 x 10 grid of picks and the labelled one; the map direct and through the facade


@pytest.mark.gpu
def test_example_pick_prints_the_abi_calls_hit(tmp_path, gpu):
    import numpy as np
    from tbraymarcherplugin_amd import synthetic as S

    vol = S.make_volume_numpy((48, 40, 36), np.float32, 0x5EED0A00)
    (vol * 3000.0 - 1000.0).astype(np.int16).tofile(tmp_path / "ct.raw")
    (tmp_path / "ct.mhd").write_text("ObjectType = Image\nNDims = 3\nDimSize = 48 40 36\nElementSpacing = 1 1 1.25\n"
                                     "ElementType = MET_SHORT\nElementDataFile = ct.raw\n")
    example, direct = build_example(tmp_path), build(tmp_path)
    kinds = set()
    for x, y in ((48, 32), (40, 28), (60, 40), (0, 0)):
        p = subprocess.run([example, str(tmp_path / "ct.mhd"), str(tmp_path / "out.ppm"), "96", "64", "80", "--pick", f"{x},{y}"],
                           capture_output=True, text=True)
        assert p.returncode == 0, p.stdout + p.stderr
        got = [l for l in p.stdout.splitlines() if l.startswith("pick ")]
        q = subprocess.run([direct, "mhd", str(tmp_path / "ct.mhd"), "96", "64", "80", f"{x},{y}"], capture_output=True, text=True)
        assert q.returncode == 0, q.stdout + q.stderr
        assert len(got) == 1 and got == [l for l in q.stdout.splitlines() if l.startswith("pick ")], (got, q.stdout)
        kinds.add(got[0].split()[2])
    assert kinds == {"hit", "miss"}
    p = subprocess.run([example, str(tmp_path / "ct.mhd"), str(tmp_path / "out.ppm"), "96", "64", "80", "--pick", "96,0"], capture_output=True, text=True)
    assert p.returncode == 1 and "pick failed" in p.stderr and "outside" in p.stderr
