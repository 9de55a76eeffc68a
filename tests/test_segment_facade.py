"""ARaymarchVolume::GrowRegion / GrowRegionAt (include/tbrm_plugin.hpp) and examples/render_mhd.cpp --grow: tests/cpp/segment_test.cpp
builds against the C-ABI with plain g++; an actor without resources refuses both; on a GPU a click on a blob labels the blob under the
pixel and nothing else, and the example prints what the binding's call gives for the same seed."""
import os
import subprocess

import pytest

from test_facade import build_example

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "segment_test.cpp")
LIB_DIR = os.path.join(ROOT, "tbraymarcherplugin_amd", "lib")


def build(tmp_path):
    exe = str(tmp_path / "segment_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), SRC, "-o", exe,
                    "-L", LIB_DIR, "-ltbrm", "-lz", f"-Wl,-rpath,{LIB_DIR}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def r_mask(codes, seed, lo, hi):
    """the grown region by the numpy reference"""
    import region_grow_reference as GR

    return GR.grow(codes, [seed], lo, hi, -1, 6)[0]


def test_segment_facade_compiles_and_refuses_without_resources(tmp_path, abi_mod):
    out = subprocess.run([build(tmp_path), "nohandle"], check=True, capture_output=True, text=True).stdout
    assert out.strip() == "nohandle grow=0 at=0 seeded=0 voxels=0 recompute=0 abi=1"


@pytest.mark.gpu
def test_grow_region_at_through_the_facade_on_gpu(tmp_path, gpu):
    p = subprocess.run([build(tmp_path)], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), p.stdout + p.stderr
    lines = dict(l.split(" ", 1) for l in p.stdout.strip().splitlines() if " " in l)
    assert lines["miss"] == "seeded=0 voxels=0 labels=0"            # a click that meets nothing grows nothing and attaches nothing
    assert lines["grow"] == "seeded=1 seed_in_ball=1 voxels_are_the_ball=1 relabelled_all=1 wrong=0 corner_untouched=1 attached=1"
    assert lines["range"].startswith("lo=51900 hi=52100 box=11,9,5..28,26,22")   # the ball of radius 9 around (19.5, 17.5, 13.5)
    assert lines["stats"] == "count_is_voxels=1 mean=52000"
    assert lines["measure"] == "voxels_are_the_ball=1 relabelled=0"
    assert lines["state"] == "frames=0 resets=0 recompute=0"        # a label edit is no frame and requests nothing
    assert lines["frame"] == "shows_label=1"
    assert lines["cleared"] == "identical=1"                        # nothing but the labels changed
    assert lines["counters"] == "calls=2"                           # the miss never reached tbrm_grow_region


@pytest.mark.gpu
def test_example_grow_prints_the_bindings_result(tmp_path, gpu):
    import numpy as np
    from tbraymarcherplugin_amd import abi, synthetic as S

    dims = (48, 40, 36)
    vol = S.make_volume_numpy(dims, np.float32, 0x5EED0A00)
    (vol * 3000.0 - 1000.0).astype(np.int16).tofile(tmp_path / "ct.raw")
    (tmp_path / "ct.mhd").write_text("ObjectType = Image\nNDims = 3\nDimSize = 48 40 36\nElementSpacing = 1 1 1.25\n"
                                     "ElementType = MET_SHORT\nElementDataFile = ct.raw\n")
    example = build_example(tmp_path)
    p = subprocess.run([example, str(tmp_path / "ct.mhd"), str(tmp_path / "out.ppm"), "96", "64", "80", "--grow", "48,32,3000,5"],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    got = [l for l in p.stdout.splitlines() if l.startswith("grow ")]
    assert len(got) == 1, p.stdout
    w = got[0].split()
    assert w[:2] == ["grow", "48,32"] and w[2] == "seed" and w[6] == "range" and w[10] == "voxels" and w[12] == "box" and w[20] == "label" and w[22] == "mean"
    seed, voxels, label = tuple(int(v) for v in w[3:6]), int(w[11]), int(w[21])
    lo, hi, mean = float(w[7]), float(w[9]), float(w[23])
    assert label == 5 and voxels > 1 and hi - lo <= 6000 and lo <= mean <= hi
    # the same seed through the binding on the volume the example loaded (the loader's normalisation restated: float32, truncated)
    raw = np.fromfile(tmp_path / "ct.raw", dtype=np.int16).reshape(dims[::-1]).astype(np.float32)
    norm = (raw - np.float32(raw.min())) / np.float32(raw.max() - raw.min())
    codes = (norm * np.float32(65535.0)).astype(np.uint16)
    with abi.Resources(dims, abi.FMT_G16) as res:
        res.upload_volume(codes)
        r = res.grow_region([seed], -3000, 3000, -1, 6, relative=True)
    assert (r["lo_used"], r["hi_used"]) == (lo, hi)
    assert r["voxels"] == voxels and list(r["bbox_min"]) + list(r["bbox_max"]) == [int(v) for v in w[13:16] + w[17:20]]
    assert abs(float(codes[r_mask(codes, seed, lo, hi)].mean()) - mean) <= 1e-8 * mean   # (the example prints nine significant digits)
    p = subprocess.run([example, str(tmp_path / "ct.mhd"), str(tmp_path / "out.ppm"), "96", "64", "80", "--grow", "0,0,3000"], capture_output=True, text=True)
    assert p.returncode == 0 and "grow 0,0 miss" in p.stdout, p.stdout + p.stderr
    p = subprocess.run([example, str(tmp_path / "ct.mhd"), str(tmp_path / "out.ppm"), "96", "64", "80", "--grow", "96,0,10"], capture_output=True, text=True)
    assert p.returncode == 1 and "grow failed" in p.stderr and "outside" in p.stderr
