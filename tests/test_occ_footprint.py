"""The footprint rules of the light occlusion (tbrm_occ_footprint.h): texel split, sample coordinate, tap spans, brick ranges, the
staging decision, the staged block's layout and offsets, a pass's signature spans and the factor block, checked position by position
in a stand-alone program under the address and undefined-behaviour sanitizers (no contraction: the kernels' arithmetic)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_footprint_rules_under_sanitizers(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "occ_footprint_test.cpp")
    exe = str(tmp_path / "occ_footprint_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", src, "-o", exe],
                   check=True)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip().splitlines()[-1] == "failures=0", p.stdout
