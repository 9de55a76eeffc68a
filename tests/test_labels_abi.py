"""The label overlay's C-ABI (include/tbrm_labels.h): exported and bound, null handles refused, the default colour table, the
C++ facade's forwards (no GPU needed)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from tbraymarcherplugin_amd import abi
import label_reference as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tbrm_labels.h")


def declared_symbols():
    return re.findall(r"TBRM_API\s+[\w\s\*]+?\b(tbrm_\w+)\s*\(", open(HEADER).read())


def test_header_symbols_are_exported_and_bound():
    lib = abi.load()
    declared = declared_symbols()
    assert sorted(declared) == sorted(abi.LABEL_SYMBOLS), set(declared) ^ set(abi.LABEL_SYMBOLS)
    assert not set(declared) & set(abi.SYMBOLS)
    for name in declared:
        assert hasattr(lib, name), f"{name} is declared in tbrm_labels.h but not exported by libtbrm.so"
    version = int(re.search(r"#define\s+TBRM_LABELS_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1))
    assert lib.tbrm_labels_abi_version() == version == abi.LABELS_ABI_VERSION


def test_every_handle_taking_entry_point_rejects_a_null_handle():
    lib = abi.load()
    z = C.c_void_p(None)
    buf = (C.c_float * 1024)()
    i3 = (C.c_int32 * 3)(0, 0, 0)
    e3 = (C.c_int32 * 3)(1, 1, 1)
    calls = {
        "tbrm_upload_label_volume": lambda: lib.tbrm_upload_label_volume(z, buf, 1),
        "tbrm_update_label_region": lambda: lib.tbrm_update_label_region(z, C.byref(i3), C.byref(e3), buf, 1),
        "tbrm_download_label_volume": lambda: lib.tbrm_download_label_volume(z, buf, 1),
        "tbrm_set_label_colors": lambda: lib.tbrm_set_label_colors(z, buf),
        "tbrm_release_label_volume": lambda: lib.tbrm_release_label_volume(z),
    }
    for name, call in calls.items():
        assert call() == abi.ERR_INVALID_ARG, name
        assert lib.tbrm_last_error(), name
    abi.set_tunable("ray_labels", 0)   # (clears nothing: only so that the next message is the query's own)
    assert lib.tbrm_has_label_volume(z) == 0 and b"null" in lib.tbrm_last_error()
    assert lib.tbrm_make_default_label_colors(None) == abi.ERR_INVALID_ARG
    free = {"tbrm_labels_abi_version", "tbrm_make_default_label_colors", "tbrm_has_label_volume"}
    assert set(abi.LABEL_SYMBOLS) == set(calls) | free


def test_default_label_colors_are_the_references():
    c = abi.make_default_label_colors()
    assert c.dtype == np.float32 and c.shape == (256, 4)
    assert np.array_equal(c[0], [0, 0, 0, 0])
    assert np.array_equal(c[1], [1, 0, 0, 0.5])
    assert np.array_equal(c[2], [0, 1, 0, 0.5])
    assert (c[3:] == [0, 0, 0, 1]).all()
    assert np.array_equal(c, LR.default_label_colors())


def test_ray_labels_tunable_exists():
    assert abi.get_tunable("ray_labels") == 0


def test_facade_label_forwards_compile_with_gxx(tmp_path, abi_mod):
    src = tmp_path / "labels_facade.cpp"
    src.write_text('#include "tbrm_plugin.hpp"\n#include "tbrm_labels.h"\n#include <cstdio>\n'
                   "int main() {\n"
                   "  tbrm_plugin::ARaymarchVolume v;\n"
                   "  unsigned char l[8] = {0};\n"
                   "  int32_t o[3] = {0, 0, 0}, e[3] = {1, 1, 1};\n"
                   "  float c[1024];\n"
                   "  tbrm_make_default_label_colors(c);\n"
                   "  const bool ok = !v.SetLabelVolume(l, 8) && !v.UpdateLabelRegion(o, e, l, 1) && !v.SetLabelColors(c) && !v.ClearLabelVolume();\n"
                   '  std::printf("%s %d\\n", ok ? "refused" : "accepted", (int) (c[4] == 1.0f && c[7] == 0.5f));\n'
                   "  return 0; }\n")
    exe = str(tmp_path / "labels_facade")
    lib_dir = os.path.join(ROOT, "tbraymarcherplugin_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe,
                    "-L", lib_dir, "-ltbrm", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert out.strip() == "refused 1"   # a volume without a handle refuses every label call
