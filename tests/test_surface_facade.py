"""ARaymarchVolume::ExtractLabelSurface / MeasureLabelSurface (include/tbrm_plugin.hpp) and examples/render_mhd.cpp --surface:
tests/cpp/surface_test.cpp builds against the C-ABI with plain g++; an actor without resources refuses every call; on a GPU the
surfaces of a ball, of a slab that ends on the volume's faces and of a box of the ball are extracted from the labels of an anisotropic
volume and every mesh is held to the header's promises by the program's own loops; the example writes an OBJ whose counts are what
the binding's call gives for the same label volume."""
import os
import subprocess

import pytest

from test_facade import build_example

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "surface_test.cpp")
LIB_DIR = os.path.join(ROOT, "tbraymarcherplugin_amd", "lib")


def build(tmp_path):
    exe = str(tmp_path / "surface_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), SRC, "-o", exe,
                    "-L", LIB_DIR, "-ltbrm", "-lz", f"-Wl,-rpath,{LIB_DIR}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def test_surface_facade_compiles_and_refuses_without_resources(tmp_path, abi_mod):
    out = subprocess.run([build(tmp_path), "nohandle"], check=True, capture_output=True, text=True).stdout
    assert out.strip() == "nohandle extract=0 measure=0 vertices=0 recompute=0 abi=1"


@pytest.mark.gpu
def test_label_surface_through_the_facade_on_gpu(tmp_path, gpu):
    p = subprocess.run([build(tmp_path), str(tmp_path)], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), p.stdout + p.stderr
    lines = dict(l.split(" ", 1) for l in p.stdout.strip().splitlines() if " " in l)
    assert lines["nolabels"] == "refused=1"
    assert lines["ball"] == "counts=1" and lines["box"] == "counts=1" and lines["slab"] == "counts=1 faces=1"
    for name in ("ball_mesh", "slab_mesh", "box_mesh"):
        assert lines[name] == "ok=1 volume=1 edges=1 positions=1 normals=1", (name, lines[name])
    assert lines["measure"] == "same=1 empty=1"
    assert lines["refused"] == "none=1 leaves=1 label=1"
    assert lines["state"] == "frames=0 resets=0 recompute=0"        # a read is no frame and requests nothing
    assert lines["labels"] == "unchanged=1"
    assert lines["counters"] == "calls=9"                           # an extraction measures first; the refused calls never counted


@pytest.mark.gpu
def test_example_surface_writes_the_bindings_mesh(tmp_path, gpu):
    import numpy as np
    from tbraymarcherplugin_amd import abi, synthetic as S

    dims = (48, 40, 36)
    vol = S.make_volume_numpy(dims, np.float32, 0x5EED0A00)
    (vol * 3000.0 - 1000.0).astype(np.int16).tofile(tmp_path / "ct.raw")
    (tmp_path / "ct.mhd").write_text("ObjectType = Image\nNDims = 3\nDimSize = 48 40 36\nElementSpacing = 0.7 0.7 2.5\n"
                                     "ElementType = MET_SHORT\nElementDataFile = ct.raw\n")
    example = build_example(tmp_path)
    args = [example, str(tmp_path / "ct.mhd"), str(tmp_path / "out.ppm"), "96", "64", "80"]
    obj = tmp_path / "ball.obj"
    p = subprocess.run(args + ["--paint", "5,9.0@24,20,18", "--surface", f"5,{obj}"], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    got = [l for l in p.stdout.splitlines() if l.startswith("surface ")]
    assert len(got) == 1, p.stdout
    w = got[0].split()
    assert w[:3] == ["surface", "label", "5"] and w[3::2][:3] == ["voxels", "vertices", "quads"] and w[9] == "axis" and w[13] == "cells" and w[21] == "blocks", w
    # the same ball through the binding
    weights, limit = abi.paint_brush((0.7, 0.7, 2.5), 9.0)
    with abi.Resources(dims, abi.FMT_G16) as res:
        res.upload_volume(np.zeros(dims[::-1], dtype=np.uint16))
        res.attach_empty_labels()
        res.paint_labels([(8 * 24, 8 * 20, 8 * 18)], weights, limit, "paint", [5], 5)
        scale, offset = abi.surface_unit_cube(dims)
        r = res.label_surface([5], triangles=True, scale=scale, offset=offset)
    assert [int(w[4]), int(w[6]), int(w[8])] == [r["set_voxels"], r["vertices"], r["quads"]] and r["vertices"] > 100
    assert [int(v) for v in w[10:13]] == list(r["quads_axis"]) and [int(v) for v in w[14:17] + w[18:21]] == list(r["cell_min"]) + list(r["cell_max"])
    text = obj.read_text().splitlines()
    v = np.array([[float(c) for c in l.split()[1:]] for l in text if l.startswith("v ")])
    vn = np.array([[float(c) for c in l.split()[1:]] for l in text if l.startswith("vn ")])
    f = np.array([[int(c.split("//")[0]) for c in l.split()[1:]] for l in text if l.startswith("f ")])
    assert v.shape == (r["vertices"], 3) and vn.shape == v.shape and f.shape == (2 * r["quads"], 3)
    assert np.array_equal(f - 1, r["indices"].reshape(-1, 3))
    # positions: the unit cube back in the file's units, voxel i at i * spacing
    want = r["positions"].astype(np.float64) * (np.array(dims) - 1) * np.array([0.7, 0.7, 2.5])
    assert np.abs(v - want).max() < 1e-5
    assert np.abs(np.linalg.norm(vn, axis=1) - 1.0).max() < 1e-5   # a ball has no ambiguous cell
    centre = np.array([24, 20, 18]) * np.array([0.7, 0.7, 2.5])
    assert ((v - centre) * vn).sum(axis=1).min() > 0               # every normal points away from the centre
    # a label that is not there gives an empty mesh; a bad label and a missing file name are refused
    p = subprocess.run(args + ["--surface", f"7,{obj}"], capture_output=True, text=True)
    assert p.returncode == 1 and "surface failed" in p.stderr   # no label volume: nothing was painted
    p = subprocess.run(args + ["--paint", "5,4.0@24,20,18", "--surface", f"300,{obj}"], capture_output=True, text=True)
    assert p.returncode == 1 and "surface failed" in p.stderr
    p = subprocess.run(args + ["--surface", "5,"], capture_output=True, text=True)
    assert p.returncode == 2 and "usage" in p.stderr
