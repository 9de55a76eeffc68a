"""Seeded region growing (include/tbrm_segment.h) without a GPU: the header's symbols exported and bound, the struct layouts, tbrm.h
left as it was, null arguments refused before anything is dereferenced, and tbrm_host_hit_voxel against the voxel rule of
tests/label_reference.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tbraymarcherplugin_amd import abi
import label_reference as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tbrm_segment.h")


def declared_symbols(path=HEADER):
    return re.findall(r"TBRM_API\s+[\w\s\*]+?\b(tbrm_\w+)\s*\(", open(path).read())


def test_header_symbols_are_exported_and_bound():
    lib = abi.load()
    declared = declared_symbols()
    assert sorted(declared) == sorted(abi.SEGMENT_SYMBOLS), set(declared) ^ set(abi.SEGMENT_SYMBOLS)
    others = (set(abi.SYMBOLS) | set(abi.LABEL_SYMBOLS) | set(abi.COLOR_LIGHT_SYMBOLS) | set(abi.VOLUME_REGION_SYMBOLS) | set(abi.VOLUME_STATS_SYMBOLS)
              | set(abi.VIEW_CACHE_SYMBOLS) | set(abi.HIT_SYMBOLS))
    assert not set(declared) & others
    for name in declared:
        assert hasattr(lib, name), f"{name} is declared in tbrm_segment.h but not exported by libtbrm.so"
    text = open(HEADER).read()
    version = int(re.search(r"#define\s+TBRM_SEGMENT_ABI_VERSION\s+(\d+)", text).group(1))
    assert lib.tbrm_segment_abi_version() == version == abi.SEGMENT_ABI_VERSION == 1
    assert int(re.search(r"#define\s+TBRM_GROW_MAX_SEEDS\s+(\d+)", text).group(1)) == abi.GROW_MAX_SEEDS == 4096


def test_struct_layouts():
    d, r = abi.GROW_DESC, abi.GROW_RESULT
    assert C.sizeof(d) == 88 and (d.connectivity.offset, d.new_label.offset, d.relative_to_seed.offset, d.lo.offset, d.hi.offset, d.writable.offset) == (24, 28, 32, 40, 48, 56)
    assert C.sizeof(r) == 64 and (r.relabelled.offset, r.bbox_min.offset, r.bbox_max.offset, r.passes.offset, r.seeds_taken.offset, r.lo_used.offset) == (8, 16, 28, 40, 44, 48)
    # the header's field order is the binding's
    text = open(HEADER).read()
    for struct, fields in (("tbrm_grow_desc", d._fields_), ("tbrm_grow_result", r._fields_)):
        body = re.search(r"typedef struct " + struct + r" \{(.*?)\} " + struct + ";", text, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = re.findall(r"(\w+)(?:\[\d+\])?\s*[,;]", body)
        assert names == [f[0] for f in fields], (struct, names)


def test_tbrm_h_is_unchanged():
    main = os.path.join(ROOT, "include", "tbrm.h")
    declared = declared_symbols(main)
    assert len(declared) == len(abi.SYMBOLS) == 62 and sorted(declared) == sorted(abi.SYMBOLS)
    assert int(re.search(r"#define\s+TBRM_ABI_VERSION\s+(\d+)", open(main).read()).group(1)) == abi.ABI_VERSION == abi.load().tbrm_abi_version() == 5


def test_grow_batch_is_a_tunable():
    assert abi.get_tunable("grow_batch") >= 1
    old = abi.get_tunable("grow_batch")
    abi.set_tunable("grow_batch", 1)
    assert abi.get_tunable("grow_batch") == 1
    abi.set_tunable("grow_batch", old)


def test_null_arguments_are_refused():
    lib = abi.load()
    z = C.c_void_p(None)
    fake = C.c_void_p(8)   # never dereferenced: the pointer checks come first
    desc = abi.GROW_DESC()
    desc.connectivity, desc.new_label, desc.hi = 6, -1, 255.0
    out, out4 = abi.GROW_RESULT(), (C.c_uint64 * 4)()
    seeds = (C.c_int32 * 3)(0, 0, 0)
    calls = {
        "tbrm_grow_region": [lambda: lib.tbrm_grow_region(z, C.byref(desc), seeds, 1, C.byref(out)),
                             lambda: lib.tbrm_grow_region(fake, None, seeds, 1, C.byref(out)),
                             lambda: lib.tbrm_grow_region(fake, C.byref(desc), None, 1, C.byref(out)),   # seeds announced, none given
                             lambda: lib.tbrm_grow_region(fake, C.byref(desc), seeds, 1, None)],
        "tbrm_attach_empty_label_volume": [lambda: lib.tbrm_attach_empty_label_volume(z)],
        "tbrm_segment_counters": [lambda: lib.tbrm_segment_counters(z, C.byref(out4)), lambda: lib.tbrm_segment_counters(fake, None)],
    }
    for name, variants in calls.items():
        for k, call in enumerate(variants):
            abi.set_tunable("ray_labels", 0)   # (a successful call in between: the next message is this call's own)
            assert call() == abi.ERR_INVALID_ARG, (name, k)
            assert b"null" in lib.tbrm_last_error(), (name, k)
    assert set(abi.SEGMENT_SYMBOLS) == set(calls) | {"tbrm_segment_abi_version", "tbrm_host_hit_voxel"}
    hit = np.zeros(1, dtype=abi.HIT_DTYPE)
    d3, o3 = (C.c_int32 * 3)(4, 4, 4), (C.c_int32 * 3)()
    assert lib.tbrm_host_hit_voxel(None, hit.ctypes.data, C.byref(o3)) == abi.ERR_INVALID_ARG
    assert lib.tbrm_host_hit_voxel(C.byref(d3), None, C.byref(o3)) == abi.ERR_INVALID_ARG
    assert lib.tbrm_host_hit_voxel(C.byref(d3), hit.ctypes.data, None) == abi.ERR_INVALID_ARG


# ---- tbrm_host_hit_voxel --------------------------------------------------------------------------------------------------------
DIMS = (5, 9, 3)   # N - 1 = 4, 8, 2: (N - 1) * u is exact in float32 and float64 for the dyadic u below


def reference_voxels(uvw):
    """the label step's voxel by label_reference.label_lookup: a label volume that numbers its voxels, a colour table that returns the number"""
    nx, ny, nz = DIMS
    labels = np.arange(nx * ny * nz, dtype=np.uint8).reshape(nz, ny, nx)
    colors = np.zeros((256, 4))
    colors[:, 0] = np.arange(256)
    col, _ = LR.label_lookup(labels, colors, np.asarray(uvw, dtype=np.float64), 0.0)
    n = col[:, 0].astype(np.int64)
    return np.stack([n % nx, (n // nx) % ny, n // (nx * ny)], axis=1)


def test_hit_voxel_follows_the_label_steps_rule():
    axis = [0.0, 1.0, 0.5, 0.125, 0.375, 0.625, 0.875, 0.25, 0.75, 0.0625, 0.1875, 0.3125, 0.4375, 0.5625, 0.6875, 0.8125, 0.9375,   # ties on some axis
            -0.5, 1.5, -1e-9, 1.0 + 1e-6, 0.3, 0.9, 0.51]                                                                                # outside [0, 1]; ordinary values
    axis = [float(np.float32(v)) for v in axis]
    rng = np.random.default_rng(5)
    uvw = np.array([[a, b, c] for a in axis for b, c in zip(rng.permutation(axis), rng.permutation(axis))])
    # keep the rows whose products are exact in float32, so that the float64 rule and the float32 rule see the same number
    exact = np.all((np.float32(uvw).clip(0, 1) * (np.float32(DIMS) - 1)).astype(np.float64) == uvw.clip(0, 1) * (np.array(DIMS) - 1.0), axis=1)
    uvw = uvw[exact]
    assert len(uvw) > 200
    want = reference_voxels(uvw)
    ties = 0
    for q, w in zip(uvw, want):
        hit = np.zeros((), dtype=abi.HIT_DTYPE)
        hit["uvw"], hit["sample"] = q, 3
        assert abi.hit_voxel(DIMS, hit) == tuple(w), q
        ties += int(any(((n - 1) * min(max(v, 0), 1)) % 1 == 0.5 for n, v in zip(DIMS, q)))
    assert ties > 100
    # spelled out: ties go to the even voxel, positions outside the cube to its faces
    hit = np.zeros((), dtype=abi.HIT_DTYPE)
    hit["sample"] = 0
    hit["uvw"] = (0.125, 0.3125, 0.75)     # 0.5, 2.5, 1.5
    assert abi.hit_voxel(DIMS, hit) == (0, 2, 2)
    hit["uvw"] = (0.375, 0.4375, 0.25)     # 1.5, 3.5, 0.5
    assert abi.hit_voxel(DIMS, hit) == (2, 4, 0)
    hit["uvw"] = (-3.0, 7.0, 1.0)
    assert abi.hit_voxel(DIMS, hit) == (0, 8, 2)
    assert abi.hit_voxel((1, 1, 1), hit) == (0, 0, 0)


def test_hit_voxel_refuses_a_record_without_a_hit():
    hit = np.zeros((), dtype=abi.HIT_DTYPE)
    hit["sample"] = -1
    with pytest.raises(abi.TbrmError) as e:
        abi.hit_voxel(DIMS, hit)
    assert e.value.code == abi.ERR_INVALID_ARG and "no hit" in str(e.value)
    hit["sample"] = 0
    with pytest.raises(abi.TbrmError) as e:
        abi.hit_voxel((4, 0, 4), hit)
    assert e.value.code == abi.ERR_INVALID_ARG
