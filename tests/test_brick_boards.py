"""The index rules the label tools share (tbrm_brick_boards.h) and the host's box rule (tbrm_box.h), pure integer code, checked voxel by
voxel in a stand-alone program under the address and undefined-behaviour sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_boards_and_box_rule_under_sanitizers(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "brick_boards_test.cpp")
    exe = str(tmp_path / "brick_boards_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", src, "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip().splitlines()[-1] == "failures=0", p.stdout
