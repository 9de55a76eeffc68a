"""The index rules of a tile of the propagation sweep (tbrm_sweep_tile.h): hand-off words, the LDS plane, the staging of a brick layer and
a chained tile's dependency, checked by enumeration in a stand-alone program under the address and undefined-behaviour sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sweep_tile_rules_under_sanitizers(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "sweep_tile_test.cpp")
    exe = str(tmp_path / "sweep_tile_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", src, "-o", exe],
                   check=True)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip().splitlines()[-1] == "failures=0", p.stdout
