"""The host-only pieces of tbraymarcherplugin_amd/csrc/tbrm_resources.h that state a layout or own memory — the DeviceScratch guard
(empty: no device needed) and Residency's layers() / bytes() / address() for a whole-volume, a first-slab and a last-slab handle —
in a stand-alone program (tests/cpp/resources_layout_test.cpp) under the address and undefined-behaviour sanitizers."""
import os
import subprocess

from tbraymarcherplugin_amd import build as tb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "resources_layout_test.cpp")


def test_guard_and_residency_under_sanitizers(tmp_path):
    exe = str(tmp_path / "resources_layout_test")
    subprocess.run([tb.hipcc_path(), "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unused-function", "-x", "hip", SRC,
                    "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip().splitlines()[-1] == "failures=0", p.stdout
