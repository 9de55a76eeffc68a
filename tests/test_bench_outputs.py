"""bench.py --dump-outputs and the plain run: what the last timed step computed is written as float32 .npy files (large arrays as a
fixed, seeded sample), identical from run to run with the same arguments; a run without --full leaves the --full-only keys null."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_dump_outputs_writes_float32_and_a_seeded_sample_of_large_arrays(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_VALUES", {"frame": 1 << 10, "light_volume": 1 << 8})
    rng = np.random.default_rng(1)
    frame = rng.random((8, 16, 4), dtype=np.float32)
    light = rng.integers(0, 256, (16, 16, 16), dtype=np.uint8)
    written = bench.dump_outputs(str(tmp_path / "a"), {"frame": frame, "light_volume": light})
    assert written == {"frame.npy": [8, 16, 4], "light_volume_sample.npy": [1 << 8]}
    got = np.load(tmp_path / "a" / "frame.npy")
    assert got.dtype == np.float32 and np.array_equal(got, frame)
    sample = np.load(tmp_path / "a" / "light_volume_sample.npy")
    assert sample.dtype == np.float32
    assert np.isin(sample, light.reshape(-1).astype(np.float32)).all()
    # the same shapes give the same indices: a second dump of the same arrays is the same bytes
    bench.dump_outputs(str(tmp_path / "b"), {"frame": frame, "light_volume": light})
    for name in written:
        assert (tmp_path / "a" / name).read_bytes() == (tmp_path / "b" / name).read_bytes(), name


def test_dump_stays_under_64_mb():
    assert 4 * sum(bench.DUMP_MAX_VALUES.values()) <= 64 * 10 ** 6


def run_plain(dump_dir):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--config", "2",
                          "--dump-outputs", str(dump_dir)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_same_outputs_every_run(gpu, tmp_path):
    a, b = run_plain(tmp_path / "a"), run_plain(tmp_path / "b")
    for r in (a, b):
        assert r["full"] is False and r["steps"] == 3 and r["warmup"] == 1
        assert r["value"] > 0 and r["ms_per_step"] > 0 and r["unit"] == "Msamples/s" and r["higher_is_better"] is True and r["dtype"] == "f32"
        # one frame per timed step, and nothing that only --full measures
        assert r["light_paths_per_step"]["raymarch"] == 1.0, r["light_paths_per_step"]
        for key in ("gpu_ms", "gpu_ms_spread", "roofline", "cpu_baseline", "full_size_parity", "raymarch_only_msamples_per_s"):
            assert r[key] is None, key
    assert a["outputs_dumped"] == {"frame.npy": [512, 512, 4], "light_volume_sample.npy": [1 << 22]}, a["outputs_dumped"]
    for name in a["outputs_dumped"]:
        x, y = np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)
        assert x.dtype == np.float32 and np.array_equal(x, y), name
    frame = np.load(tmp_path / "a" / "frame.npy")
    assert np.isfinite(frame).all() and (frame[..., 3] > 0).any()
