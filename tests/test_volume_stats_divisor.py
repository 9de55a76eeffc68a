"""The multiply-shift that stands for the division of the UNORM binning rule (tbraymarcherplugin_amd/csrc/tbrm_stats_divisor.h),
on the host: tests/cpp/stats_divisor_test.cpp holds it against `/` for every divisor 1 .. 65536 at the dividends that decide."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "stats_divisor_test.cpp")


def test_multiply_shift_equals_the_division(tmp_path):
    exe = str(tmp_path / "stats_divisor_test")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", SRC, "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    last = p.stdout.strip().splitlines()[-1].split()
    assert last[1] == "wrong=0" and int(last[0].split("=")[1]) > 20_000_000, p.stdout
