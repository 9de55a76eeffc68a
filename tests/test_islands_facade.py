"""ARaymarchVolume::KeepLargestIslands / RemoveSmallIslands / SplitIslands / FillLabelHoles (include/tbrm_plugin.hpp) and
examples/render_mhd.cpp --islands: tests/cpp/islands_test.cpp builds against the C-ABI with plain g++; an actor without resources
refuses all four; on a GPU keep-largest removes the specks and nothing else, fill-holes fills a cavity that CloseLabel with radius 1
leaves open, and every label volume equals the program's own brute force; the example prints what the binding's call gives for the
same label volume."""
import os
import subprocess

import pytest

from test_facade import build_example

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "islands_test.cpp")
LIB_DIR = os.path.join(ROOT, "tbraymarcherplugin_amd", "lib")


def build(tmp_path):
    exe = str(tmp_path / "islands_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), SRC, "-o", exe,
                    "-L", LIB_DIR, "-ltbrm", "-lz", f"-Wl,-rpath,{LIB_DIR}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def test_islands_facade_compiles_and_refuses_without_resources(tmp_path, abi_mod):
    out = subprocess.run([build(tmp_path), "nohandle"], check=True, capture_output=True, text=True).stdout
    assert out.strip() == "nohandle keep=0 remove=0 split=0 fill=0 islands=0 recompute=0 abi=1"


@pytest.mark.gpu
def test_islands_through_the_facade_on_gpu(tmp_path, gpu):
    p = subprocess.run([build(tmp_path)], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), p.stdout + p.stderr
    lines = dict(l.split(" ", 1) for l in p.stdout.strip().splitlines() if " " in l)
    assert lines["nolabels"] == "refused=1"
    assert lines["close"] == "cavity_open=1"
    assert lines["split"] == "wrong=0 counts=1"
    assert lines["remove"] == "wrong=0 counts=1 pair_kept=1"
    assert lines["keep"] == "wrong=0 specks_removed=1 nothing_else=1"
    assert lines["fill"] == "wrong=0 counts=1 cavity_filled=1"
    assert lines["fill_small"] == "wrong=0 kept=1"
    assert lines["state"] == "frames=0 resets=0 recompute=0"        # a label edit is no frame and requests nothing
    assert lines["frame"] == "shows_change=1"
    assert lines["counters"] == "calls=6"                           # the refused call never counted


@pytest.mark.gpu
def test_example_islands_prints_the_bindings_result(tmp_path, gpu):
    import numpy as np
    from tbraymarcherplugin_amd import abi, synthetic as S

    dims = (48, 40, 36)
    vol = S.make_volume_numpy(dims, np.float32, 0x5EED0A00)
    (vol * 3000.0 - 1000.0).astype(np.int16).tofile(tmp_path / "ct.raw")
    (tmp_path / "ct.mhd").write_text("ObjectType = Image\nNDims = 3\nDimSize = 48 40 36\nElementSpacing = 1 1 1.25\n"
                                     "ElementType = MET_SHORT\nElementDataFile = ct.raw\n")
    example = build_example(tmp_path)
    args = [example, str(tmp_path / "ct.mhd"), str(tmp_path / "out.ppm"), "96", "64", "80"]
    names = ["set", "islands", "spared", "kept", "dropped", "kept_voxels", "dropped_voxels", "largest", "relabelled"]
    fields = ["set_voxels", "islands", "spared", "kept", "dropped", "kept_voxels", "dropped_voxels", "largest", "relabelled"]
    raw = np.fromfile(tmp_path / "ct.raw", dtype=np.int16).reshape(dims[::-1]).astype(np.float32)
    norm = (raw - np.float32(raw.min())) / np.float32(raw.max() - raw.min())
    codes = (norm * np.float32(65535.0)).astype(np.uint16)   # the loader's normalisation restated
    moved = 0
    for op, n in (("keep", 1), ("remove", 4), ("split", 3), ("fill", 0), ("fill", 2)):
        # the grown label, opened by 2 so that it falls into pieces, then the tool
        p = subprocess.run(args + ["--grow", "48,32,3000,5", "--morph", "open,2", "--islands", f"{op},{n}"], capture_output=True, text=True)
        assert p.returncode == 0, p.stdout + p.stderr
        grow = [l for l in p.stdout.splitlines() if l.startswith("grow ")][0].split()
        got = [l for l in p.stdout.splitlines() if l.startswith("islands ")]
        assert len(got) == 1 and p.stdout.index("morph ") < p.stdout.index("islands "), p.stdout
        w = got[0].split()
        assert w[:5] == ["islands", op, str(n), "label", "5"] and w[5:23:2] == names and w[23] == "box", w
        seed, lo, hi = tuple(int(v) for v in grow[3:6]), float(grow[7]), float(grow[9])
        with abi.Resources(dims, abi.FMT_G16) as res:
            res.upload_volume(codes)
            res.attach_empty_labels()
            res.grow_region([seed], lo, hi, 5, 6)
            res.morph_labels("open", 2, [5], 5)
            r = {"keep": lambda: res.keep_largest_islands(5, n), "remove": lambda: res.remove_small_islands(5, n),
                 "split": lambda: res.split_islands(5, 5, n), "fill": lambda: res.fill_label_holes(5, n or None)}[op]()
        assert [int(v) for v in w[6:24:2]] == [r[k] for k in fields], (op, w, r)
        assert [int(v) for v in w[24:27] + w[28:31]] == list(r["bbox_min"]) + list(r["bbox_max"])
        moved += r["relabelled"]
    assert moved > 0
    # an operator that does not exist, and no label volume to work on
    p = subprocess.run(args + ["--grow", "48,32,3000,5", "--islands", "merge,1"], capture_output=True, text=True)
    assert p.returncode == 1 and "islands failed" in p.stderr
    p = subprocess.run(args + ["--islands", "keep,1"], capture_output=True, text=True)
    assert p.returncode == 1 and "islands failed" in p.stderr and "label volume" in p.stderr
