"""Hit maps and picking (include/tbrm_hit.h) without a GPU: the float64 restatement of the hit march (tests/hit_reference.py) against
the restatement of the lit march where the two overlap, its monotony in the threshold, tbrm_host_hits_to_world against the
restatement's transforms, the header's symbols exported and bound, the record's layout, and the refusals that need no device."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from tbraymarcherplugin_amd import abi
import exact_reference as X
import exact_scenes as E
import hit_reference as H
from test_exact_reference import TAINT_CAP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tbrm_hit.h")


def declared_symbols(path=HEADER):
    return re.findall(r"TBRM_API\s+[\w\s\*]+?\b(tbrm_\w+)\s*\(", open(path).read())


def test_header_symbols_are_exported_and_bound():
    lib = abi.load()
    declared = declared_symbols()
    assert sorted(declared) == sorted(abi.HIT_SYMBOLS), set(declared) ^ set(abi.HIT_SYMBOLS)
    others = set(abi.SYMBOLS) | set(abi.LABEL_SYMBOLS) | set(abi.COLOR_LIGHT_SYMBOLS) | set(abi.VOLUME_REGION_SYMBOLS) | set(abi.VOLUME_STATS_SYMBOLS) | set(abi.VIEW_CACHE_SYMBOLS)
    assert not set(declared) & others
    for name in declared:
        assert hasattr(lib, name), f"{name} is declared in tbrm_hit.h but not exported by libtbrm.so"
    version = int(re.search(r"#define\s+TBRM_HIT_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1))
    assert lib.tbrm_hit_abi_version() == version == abi.HIT_ABI_VERSION == 1


def test_tbrm_h_is_unchanged():
    main = os.path.join(ROOT, "include", "tbrm.h")
    declared = declared_symbols(main)
    assert len(declared) == len(abi.SYMBOLS) == 62 and sorted(declared) == sorted(abi.SYMBOLS)
    assert int(re.search(r"#define\s+TBRM_ABI_VERSION\s+(\d+)", open(main).read()).group(1)) == abi.ABI_VERSION == abi.load().tbrm_abi_version() == 5


def test_record_layout():
    """sizeof(tbrm_hit) == 32, and the numpy record has the struct's fields at the struct's offsets"""
    text = open(HEADER).read()
    body = re.search(r"typedef struct tbrm_hit \{(.*?)\} tbrm_hit;", text, re.S).group(1)
    fields = re.findall(r"^\s*(float|int32_t)\s+(\w+)(?:\[(\d+)\])?;", body, re.M)
    assert [f[1] for f in fields] == list(abi.HIT_DTYPE.names) == ["uvw", "sample", "alpha", "value", "label", "full_steps"]
    offset = 0
    for ctype, name, count in fields:
        dt, off = abi.HIT_DTYPE.fields[name][:2]
        assert off == offset and dt.base == np.dtype(np.float32 if ctype == "float" else np.int32) and dt.shape == ((int(count),) if count else ())
        offset += 4 * int(count or 1)
    assert offset == abi.HIT_DTYPE.itemsize == 32


def test_null_arguments_and_bad_thresholds_are_refused_without_a_device():
    lib = abi.load()
    fake = C.c_void_p(8)   # never dereferenced: the pointer and threshold checks come first
    cam, tile, rp, world = abi.look_at_camera((0, -300, 0), (0, 0, 0), (0, 0, 1), 40.0, 16, 16), abi.Tile(0, 0, 16, 16), abi.RaymarchParams(), abi.make_world()
    out, out3 = C.c_void_p(256), (C.c_uint64 * 3)()
    args = [fake, C.byref(cam), C.byref(tile), C.byref(rp), C.byref(world)]
    for k in range(5):   # each of handle, camera, tile, params, world in turn
        a = list(args)
        a[k] = None
        assert lib.tbrm_raymarch_hits_device(*a, 0.5, None, out, None) == abi.ERR_INVALID_ARG and b"null" in lib.tbrm_last_error(), k
        assert lib.tbrm_raymarch_hits(*a, 0.5, out, None) == abi.ERR_INVALID_ARG and b"null" in lib.tbrm_last_error(), k
    assert lib.tbrm_raymarch_hits_device(*args, 0.5, None, None, None) == abi.ERR_INVALID_ARG
    assert lib.tbrm_raymarch_hits(*args, 0.5, None, None) == abi.ERR_INVALID_ARG
    pick = [fake, C.byref(cam), 3, 4, C.byref(rp), C.byref(world)]
    for k in (0, 1, 4, 5):
        a = list(pick)
        a[k] = None
        assert lib.tbrm_pick(*a, 0.5, out, None, None) == abi.ERR_INVALID_ARG and b"null" in lib.tbrm_last_error(), k
    assert lib.tbrm_pick(*pick, 0.5, None, None, None) == abi.ERR_INVALID_ARG
    for px, py in ((-1, 0), (0, -1), (16, 0), (0, 16)):
        assert lib.tbrm_pick(fake, C.byref(cam), px, py, C.byref(rp), C.byref(world), 0.5, out, None, None) == abi.ERR_INVALID_ARG
        assert b"outside" in lib.tbrm_last_error()
    for bad in (0.96, -0.01, 1.0, math.nan, math.inf):
        assert lib.tbrm_raymarch_hits_device(*args, bad, None, out, None) == abi.ERR_INVALID_ARG and b"threshold" in lib.tbrm_last_error(), bad
        assert lib.tbrm_raymarch_hits(*args, bad, out, None) == abi.ERR_INVALID_ARG and b"threshold" in lib.tbrm_last_error(), bad
        assert lib.tbrm_pick(*pick, bad, out, None, None) == abi.ERR_INVALID_ARG and b"threshold" in lib.tbrm_last_error(), bad
    assert lib.tbrm_hit_counters(None, C.byref(out3)) == abi.ERR_INVALID_ARG and lib.tbrm_hit_counters(fake, None) == abi.ERR_INVALID_ARG
    hits = np.zeros(2, dtype=abi.HIT_DTYPE)
    assert lib.tbrm_host_hits_to_world(None, C.byref(cam), hits.ctypes.data, 2, None, None) == abi.ERR_INVALID_ARG
    assert lib.tbrm_host_hits_to_world(C.byref(world), None, hits.ctypes.data, 2, None, None) == abi.ERR_INVALID_ARG
    assert lib.tbrm_host_hits_to_world(C.byref(world), C.byref(cam), None, 2, None, None) == abi.ERR_INVALID_ARG
    assert lib.tbrm_host_hits_to_world(C.byref(world), C.byref(cam), None, 0, None, None) == abi.OK


@pytest.mark.parametrize("name", ["outside-u16-jitter", "rotated-clip-bone", "depth-odd-tile-rowgroups", "inside-camera"])
def test_restatement_agrees_with_the_lit_march_at_095(name):
    """at threshold 0.95 a hit in the full steps is the lit march's early exit (alpha set to 1); everywhere else the alphas are equal"""
    s = H.scene_named(name)
    h = H.reference(name, 0.95)
    lit, _ = E.run_exact_ray(s, abi.host_bake_tf_lut(E.tf_lut(s["tf"])))
    in_full = (h["sample"] >= 0) & (h["sample"] < h["full_steps"])
    assert np.array_equal(in_full, lit[..., 3] == 1.0)
    assert np.array_equal(h["alpha"][~in_full], lit[..., 3][~in_full])
    assert np.all(h["alpha"][h["sample"] >= 0] > 0.95) and np.all(h["alpha"][h["sample"] < 0] <= 0.95)
    assert np.all(np.isinf(h["depth"][h["sample"] < 0])) and np.all(h["full_steps"][~h["crossing"]] == 0)


@pytest.mark.parametrize("name", H.HIT_SCENES)
def test_sample_is_monotone_in_the_threshold(name):
    lo, mid, hi = (H.reference(name, t) for t in H.THRESHOLDS)
    for a, b in ((lo, mid), (mid, hi)):
        assert np.array_equal(a["full_steps"], b["full_steps"])
        both = b["sample"] >= 0
        assert np.all(a["sample"][both] >= 0) and np.all(a["sample"][both] <= b["sample"][both])   # a higher bar is passed no sooner
        assert np.all(b["sample"][a["sample"] < 0] < 0)
        same = both & (a["sample"] == b["sample"])
        assert np.array_equal(a["uvw"][same], b["uvw"][same]) and np.array_equal(a["alpha"][same], b["alpha"][same])
    for r in (lo, mid, hi):
        assert r["taint"].mean() < TAINT_CAP
        assert np.all(r["sample"] <= r["full_steps"])


def test_the_scenes_have_hits_and_misses():
    """what the GPU comparisons' non-vacuity floors rest on: inside-camera hits everywhere at 0.5 and nowhere at 0.95"""
    assert (H.reference("inside-camera", 0.5)["sample"] >= 0).all() and (H.reference("inside-camera", 0.95)["sample"] < 0).all()
    for name in H.HIT_SCENES:
        n = sum(int(((H.reference(name, t)["sample"] >= 0) & ~H.reference(name, t)["taint"]).sum()) for t in H.THRESHOLDS)
        assert n >= 100, name


@pytest.mark.parametrize("name", ["rotated-clip-bone", "inside-camera"])
def test_host_hits_to_world_against_the_restatement(name):
    s = H.scene_named(name)
    r = H.reference(name, 0.5)
    hits = np.zeros(r["sample"].shape, dtype=abi.HIT_DTYPE)
    hits["uvw"] = r["uvw"].astype(np.float32)
    hits["sample"] = r["sample"]
    xyz, depth = abi.hits_to_world(s["world"], s["cam"], hits)
    hit = r["sample"] >= 0
    assert hit.sum() >= 100
    uvw32 = hits["uvw"].astype(np.float64)
    want = H.unit_cube_to_world(s["world"], uvw32)
    scale = max(abs(v) for v in X._v(s["world"].volume_transform.scale3d))
    assert np.abs(xyz[hit] - want[hit]).max() <= 1e-12 * scale
    assert np.abs(depth[hit] - H.depth_along_forward(s["world"], s["cam"], uvw32)[hit]).max() <= 1e-12 * scale * 10
    back = X.inverse_transform_position(s["world"].volume_transform, xyz[hit]) + 0.5   # the cube setup's own direction
    assert np.abs(back - uvw32[hit]).max() <= 1e-12
    assert np.all(xyz[~hit] == 0.0) and np.all(np.isinf(depth[~hit]) & (depth[~hit] > 0))
