"""ARaymarchVolume::MorphLabel / DilateLabel / ErodeLabel / OpenLabel / CloseLabel (include/tbrm_plugin.hpp) and
examples/render_mhd.cpp --morph: tests/cpp/morph_test.cpp builds against the C-ABI with plain g++; an actor without resources refuses
all five; on a GPU closing fills a pinhole, opening cuts a bridge and every label volume equals the program's own brute-force
restatement; the example prints what the binding's call gives for the same label volume."""
import os
import subprocess

import pytest

from test_facade import build_example

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "morph_test.cpp")
LIB_DIR = os.path.join(ROOT, "tbraymarcherplugin_amd", "lib")


def build(tmp_path):
    exe = str(tmp_path / "morph_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), SRC, "-o", exe,
                    "-L", LIB_DIR, "-ltbrm", "-lz", f"-Wl,-rpath,{LIB_DIR}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def test_morph_facade_compiles_and_refuses_without_resources(tmp_path, abi_mod):
    out = subprocess.run([build(tmp_path), "nohandle"], check=True, capture_output=True, text=True).stdout
    assert out.strip() == "nohandle morph=0 dilate=0 erode=0 open=0 close=0 added=0 recompute=0 abi=1"


@pytest.mark.gpu
def test_morph_label_through_the_facade_on_gpu(tmp_path, gpu):
    p = subprocess.run([build(tmp_path)], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), p.stdout + p.stderr
    lines = dict(l.split(" ", 1) for l in p.stdout.strip().splitlines() if " " in l)
    assert lines["nolabels"] == "refused=1"
    for name in ("close", "open", "dilate", "erode", "close26"):
        assert lines[name] == "wrong=0 counts=1 moved=1", (name, p.stdout)
    assert lines["pinhole"] == "filled=1"
    assert lines["bridge"] == "cut=1 blocks_kept=1"
    assert lines["measure"] == "added=1 relabelled=0 unchanged=1"
    assert lines["erase_label"] == "removed_got_it=1"
    assert lines["state"] == "frames=0 resets=0 recompute=0"        # a label edit is no frame and requests nothing
    assert lines["frame"] == "shows_change=1"
    assert lines["counters"] == "calls=7 launches=10"               # the refused call never counted


@pytest.mark.gpu
def test_example_morph_prints_the_bindings_result(tmp_path, gpu):
    import numpy as np
    from tbraymarcherplugin_amd import abi, synthetic as S

    dims = (48, 40, 36)
    vol = S.make_volume_numpy(dims, np.float32, 0x5EED0A00)
    (vol * 3000.0 - 1000.0).astype(np.int16).tofile(tmp_path / "ct.raw")
    (tmp_path / "ct.mhd").write_text("ObjectType = Image\nNDims = 3\nDimSize = 48 40 36\nElementSpacing = 1 1 1.25\n"
                                     "ElementType = MET_SHORT\nElementDataFile = ct.raw\n")
    example = build_example(tmp_path)
    args = [example, str(tmp_path / "ct.mhd"), str(tmp_path / "out.ppm"), "96", "64", "80"]
    p = subprocess.run(args + ["--grow", "48,32,3000,5", "--morph", "close,2"], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    grow = [l for l in p.stdout.splitlines() if l.startswith("grow ")][0].split()
    got = [l for l in p.stdout.splitlines() if l.startswith("morph ")]
    assert len(got) == 1 and p.stdout.index("grow ") < p.stdout.index("morph "), p.stdout
    w = got[0].split()
    assert w[:5] == ["morph", "close", "2", "label", "5"] and w[5::2][:4] == ["source", "result", "added", "removed"] and w[13] == "box" and w[21] == "launches"
    seed, lo, hi = tuple(int(v) for v in grow[3:6]), float(grow[7]), float(grow[9])
    # the same grow and the same closing through the binding on the volume the example loaded (the loader's normalisation restated)
    raw = np.fromfile(tmp_path / "ct.raw", dtype=np.int16).reshape(dims[::-1]).astype(np.float32)
    norm = (raw - np.float32(raw.min())) / np.float32(raw.max() - raw.min())
    codes = (norm * np.float32(65535.0)).astype(np.uint16)
    with abi.Resources(dims, abi.FMT_G16) as res:
        res.upload_volume(codes)
        res.attach_empty_labels()
        g = res.grow_region([seed], lo, hi, 5, 6)
        r = res.morph_labels("close", 2, [5], 5)
    assert int(w[6]) == g["voxels"] == r["source_voxels"]
    assert [int(w[8]), int(w[10]), int(w[12])] == [r["result_voxels"], r["added"], r["removed"]] and r["removed"] == 0
    assert [int(v) for v in w[14:17] + w[18:21]] == list(r["bbox_min"]) + list(r["bbox_max"]) and int(w[22]) == r["launches"] == 2
    # a label of its own choosing, an operator that does not exist, and no label volume to work on
    p = subprocess.run(args + ["--grow", "48,32,3000,5", "--morph", "erode,1,5"], capture_output=True, text=True)
    assert p.returncode == 0 and " removed " in p.stdout and "morph erode 1 label 5" in p.stdout, p.stdout + p.stderr
    p = subprocess.run(args + ["--grow", "48,32,3000,5", "--morph", "smooth,1"], capture_output=True, text=True)
    assert p.returncode == 1 and "morph failed" in p.stderr
    p = subprocess.run(args + ["--morph", "open,1"], capture_output=True, text=True)
    assert p.returncode == 1 and "morph failed" in p.stderr and "label volume" in p.stderr
