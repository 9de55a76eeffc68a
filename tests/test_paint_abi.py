"""The paint brush (include/tbrm_paint.h) without a GPU: the header compiles as C, its symbols are exported and bound and belong to no
other list, the struct layouts match the ctypes mirrors, null and out-of-range arguments are refused with their field named,
paint_skip is a tunable, tbrm_host_paint_brush and tbrm_host_paint_stroke do what the header says (a split segment and n_out on a
short capacity among it), and the plan (tbrm_paint_plan.h: what the kernel runs, as host code) runs in a stand-alone program under
the address and undefined-behaviour sanitizers. What tbrm_paint_labels refuses of a desc needs a handle: tests/test_gpu_label_paint.py."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tbraymarcherplugin_amd import abi
import label_paint_reference as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "tbrm_paint.h")


def declared_symbols(path=HEADER):
    return re.findall(r"TBRM_API\s+[\w\s\*]+?\b(tbrm_\w+)\s*\(", open(path).read())


def test_header_symbols_are_exported_and_bound():
    lib = abi.load()
    declared = declared_symbols()
    assert sorted(declared) == sorted(abi.PAINT_SYMBOLS), set(declared) ^ set(abi.PAINT_SYMBOLS)
    others = (set(abi.SYMBOLS) | set(abi.LABEL_SYMBOLS) | set(abi.COLOR_LIGHT_SYMBOLS) | set(abi.VOLUME_REGION_SYMBOLS) | set(abi.VOLUME_STATS_SYMBOLS)
              | set(abi.VIEW_CACHE_SYMBOLS) | set(abi.HIT_SYMBOLS) | set(abi.SEGMENT_SYMBOLS) | set(abi.MORPH_SYMBOLS) | set(abi.ISLANDS_SYMBOLS)
              | set(abi.MARGIN_SYMBOLS) | set(abi.SMOOTH_SYMBOLS) | set(abi.SCISSORS_SYMBOLS) | set(abi.COMPETE_SYMBOLS))
    assert not set(declared) & others
    for name in declared:
        assert hasattr(lib, name), f"{name} is declared in tbrm_paint.h but not exported by libtbrm.so"
    text = open(HEADER).read()
    version = int(re.search(r"#define\s+TBRM_PAINT_ABI_VERSION\s+(\d+)", text).group(1))
    assert lib.tbrm_paint_abi_version() == version == abi.PAINT_ABI_VERSION == 1
    for name, value in (("MAX_POINTS", 4096), ("MAX_DIM", 16384), ("MAX_WEIGHT", 65535), ("MAX_REACH", 64)):
        assert int(re.search(r"#define\s+TBRM_PAINT_" + name + r"\s+(\d+)", text).group(1)) == getattr(abi, "PAINT_" + name) == getattr(PR, name) == value
    assert abi.PAINT_MAX_COORD == PR.MAX_COORD == 1 << 18 and abi.PAINT_MAX_LIMIT == PR.MAX_LIMIT == 2 ** 30 - 1
    for name, value in abi.PAINT_OPS.items():
        assert int(re.search(r"TBRM_PAINT_" + name.upper() + r"\s*=\s*(\d+)", text).group(1)) == value
    assert (PR.PAINT, PR.ERASE) == (0, 1) == tuple(abi.PAINT_OPS.values())


def test_header_compiles_as_c_and_the_layouts_match(tmp_path):
    d, r = abi.PAINT_DESC, abi.PAINT_RESULT
    assert C.sizeof(d) == 136
    assert (d.origin.offset, d.extent.offset, d.op.offset, d.new_label.offset, d.erase_label.offset, d.gate.offset, d.weights.offset, d.limit.offset, d.lo.offset, d.hi.offset,
            d.source.offset, d.writable.offset) == (0, 12, 24, 28, 32, 36, 40, 52, 56, 64, 72, 104)
    assert C.sizeof(r) == 80
    assert (r.stamp_voxels.offset, r.added.offset, r.removed.offset, r.relabelled.offset, r.bbox_min.offset, r.bbox_max.offset, r.segments.offset, r.bricks_whole.offset,
            r.bricks_untouched.offset, r.bricks_evaluated.offset, r.launches.offset, r.reserved.offset) == (0, 8, 16, 24, 32, 44, 56, 60, 64, 68, 72, 76)
    text = open(HEADER).read()
    for struct, fields in (("tbrm_paint_desc", d._fields_), ("tbrm_paint_result", r._fields_)):
        body = re.search(r"typedef struct " + struct + r" \{(.*?)\} " + struct + ";", text, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = re.findall(r"(\w+)(?:\[\d+\])?\s*[,;]", body)
        assert names == [f[0] for f in fields], (struct, names)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "tbrm_paint.h"\n'
                   "int main(void) {\n"
                   '  printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(tbrm_paint_desc), offsetof(tbrm_paint_desc, weights), offsetof(tbrm_paint_desc, lo),\n'
                   "         offsetof(tbrm_paint_desc, source), sizeof(tbrm_paint_result), offsetof(tbrm_paint_result, bbox_min), offsetof(tbrm_paint_result, launches));\n"
                   "  return TBRM_PAINT_MAX_POINTS == 4096 && TBRM_PAINT_MAX_COORD == 262144 && TBRM_PAINT_MAX_LIMIT == 1073741823u && TBRM_PAINT_ERASE == 1 ? 0 : 1;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", INCLUDE, str(src), "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.split() == ["136", "40", "56", "72", "80", "32", "72"], p.stdout


def test_the_other_label_headers_are_unchanged():
    for header, symbols, count, version in (("tbrm_scissors.h", abi.SCISSORS_SYMBOLS, 5, ("SCISSORS", abi.load().tbrm_scissors_abi_version())),
                                            ("tbrm_compete.h", abi.COMPETE_SYMBOLS, 4, ("COMPETE", abi.load().tbrm_compete_abi_version())),
                                            ("tbrm_margin.h", abi.MARGIN_SYMBOLS, 5, ("MARGIN", abi.load().tbrm_margin_abi_version()))):
        path = os.path.join(INCLUDE, header)
        assert sorted(declared_symbols(path)) == sorted(symbols) and len(symbols) == count, header
        assert int(re.search(r"#define\s+TBRM_" + version[0] + r"_ABI_VERSION\s+(\d+)", open(path).read()).group(1)) == version[1] == 1, header


def test_paint_skip_is_a_tunable():
    old = abi.get_tunable("paint_skip")
    assert old == 1
    try:
        abi.set_tunable("paint_skip", 0)
        assert abi.get_tunable("paint_skip") == 0
        assert abi.get_tunable("scissors_skip") == 1   # a tunable of its own
    finally:
        abi.set_tunable("paint_skip", old)


def test_null_arguments_are_refused():
    lib = abi.load()
    z = C.c_void_p(None)
    fake = C.c_void_p(8)   # never dereferenced: the pointer checks come first
    desc, out, out4 = abi.PAINT_DESC(), abi.PAINT_RESULT(), (C.c_uint64 * 4)()
    pts = (C.c_int32 * 3)()
    sp, w, limit = (C.c_double * 3)(1, 1, 1), (C.c_uint32 * 3)(1, 1, 1), C.c_uint32()
    dims, uvw, n_out = (C.c_int32 * 3)(8, 8, 8), (C.c_float * 3)(), C.c_size_t()
    calls = {
        "tbrm_paint_labels": [lambda: lib.tbrm_paint_labels(z, C.byref(desc), pts, 1, C.byref(out)), lambda: lib.tbrm_paint_labels(fake, None, pts, 1, C.byref(out)),
                              lambda: lib.tbrm_paint_labels(fake, C.byref(desc), None, 1, C.byref(out)), lambda: lib.tbrm_paint_labels(fake, C.byref(desc), pts, 1, None)],
        "tbrm_paint_counters": [lambda: lib.tbrm_paint_counters(z, C.byref(out4)), lambda: lib.tbrm_paint_counters(fake, None)],
        "tbrm_host_paint_brush": [lambda: lib.tbrm_host_paint_brush(None, 2.0, w, C.byref(limit)), lambda: lib.tbrm_host_paint_brush(sp, 2.0, None, C.byref(limit)),
                                  lambda: lib.tbrm_host_paint_brush(sp, 2.0, w, None)],
        "tbrm_host_paint_stroke": [lambda: lib.tbrm_host_paint_stroke(None, uvw, 1, w, pts, 1, C.byref(n_out)), lambda: lib.tbrm_host_paint_stroke(dims, None, 1, w, pts, 1, C.byref(n_out)),
                                   lambda: lib.tbrm_host_paint_stroke(dims, uvw, 1, None, pts, 1, C.byref(n_out)), lambda: lib.tbrm_host_paint_stroke(dims, uvw, 1, w, None, 1, C.byref(n_out)),
                                   lambda: lib.tbrm_host_paint_stroke(dims, uvw, 1, w, pts, 1, None)],
    }
    for name, variants in calls.items():
        for k, call in enumerate(variants):
            abi.set_tunable("ray_labels", 0)   # (a successful call in between: the next message is this call's own)
            assert call() == abi.ERR_INVALID_ARG, (name, k)
            assert b"null" in lib.tbrm_last_error(), (name, k)
    assert set(abi.PAINT_SYMBOLS) == set(calls) | {"tbrm_paint_abi_version"}


def test_the_brush_of_a_spacing_and_a_radius():
    for spacing, radius in (((1.0, 1.0, 1.0), 3.0), ((0.7, 0.7, 2.5), 2.0), ((0.5, 0.25, 0.25), 1.9)):
        weights, limit = abi.paint_brush(spacing, radius)
        assert (weights, limit) == (abi.margin_weights(spacing, radius)[0], 64 * abi.margin_weights(spacing, radius)[1])
        assert PR.admissible([(0, 0, 0)], weights, limit, (8, 8, 8))
    assert abi.paint_brush((1.0, 1.0, 1.0), 3.0) == ((256, 256, 256), 64 * 256 * 9)
    lib = abi.load()
    w, limit = (C.c_uint32 * 3)(7, 7, 7), C.c_uint32(7)
    for spacing, radius, names in (((1.0, 1.0, 1.0), 65.0, b"reaches"),        # 65 voxels
                                   ((1.0, 1.0, 17.0), 3.0, b"weights"),        # a weight of 256 * 289
                                   ((1.0, 0.0, 1.0), 3.0, b"spacing"), ((1.0, 1.0, 1.0), math.nan, b"radius"),
                                   ((1.0, 1.0, 1.0), 0.4, b"at least 1")):     # what tbrm_host_margin_weights refuses: no voxel within reach
        assert lib.tbrm_host_paint_brush((C.c_double * 3)(*spacing), radius, w, C.byref(limit)) == abi.ERR_INVALID_ARG, (spacing, radius)
        assert names in lib.tbrm_last_error(), lib.tbrm_last_error()
        assert tuple(w) == (7, 7, 7) and limit.value == 7   # a refusal leaves the outputs alone
    assert abi.paint_brush((1.0, 1.0, 1.0), 64.0)[1] == 64 * 256 * 64 * 64 == 2 ** 26   # the largest isotropic brush


def test_the_stroke_of_unit_cube_positions():
    dims = (41, 27, 19)
    uvw = [(0.0, 0.5, 1.0), (0.0, 0.5, 1.0), (-3.0, 0.5, 2.0), (0.25, 0.26, math.nan), (1.0, 1.0, 1.0)]
    got = abi.paint_stroke(dims, uvw, (1, 1, 1))
    assert got.dtype == np.int32 and got.tolist() == [[0, 104, 144], [80, 54, 0], [320, 208, 144]]
    # the rule, in double: nearbyint(8 (N - 1) clamp(u)), ties to even
    rng = np.random.default_rng(5)
    pos = rng.uniform(-0.2, 1.2, size=(200, 3)).astype(np.float32)
    pos[7] = (0.5, 1.5 / 208, 2.5 / 144)   # ties: 8 * 26 * u = 1.5 -> 2, 8 * 18 * u = 2.5 -> 2 (where the float32 holds them exactly)
    want = [tuple(int(np.rint(8.0 * (n - 1) * min(max(float(u), 0.0), 1.0))) for n, u in zip(dims, p)) for p in pos]
    want = [p for k, p in enumerate(want) if k == 0 or p != want[k - 1]]
    assert abi.paint_stroke(dims, pos, (1, 1, 1)).tolist() == [list(p) for p in want]
    # a voxel's centre is where tbrm_host_hit_voxel puts the hit: eight times the voxel
    for v in ((0, 0, 0), (40, 26, 18), (13, 7, 5)):
        u = [v[c] / (dims[c] - 1) for c in range(3)]
        assert abi.paint_stroke(dims, [u], (1, 1, 1)).tolist() == [[8 * c for c in v]]


def test_a_long_segment_is_split_and_a_short_capacity_says_what_is_needed():
    dims, heavy = (16384, 16384, 16384), (65535, 65535, 65535)
    ends = [(0.0, 0.0, 0.0), (1.0, 1.0, 0.5)]
    got = abi.paint_stroke(dims, ends, heavy)
    b = (8 * 16383, 8 * 16383, 65532)
    k = len(got) - 1
    assert k > 1 and got[0].tolist() == [0, 0, 0] and got[-1].tolist() == list(b)
    assert got.tolist() == [[j * c // k for c in b] for j in range(k + 1)]   # equal parts, the inserted points rounded down
    dd = lambda pts: max(sum(w * (int(q) - int(p)) ** 2 for w, p, q in zip(heavy, a, c)) for a, c in zip(pts[:-1], pts[1:]))
    assert dd(got.tolist()) < 2 ** 30 <= dd([[j * c // (k - 1) for c in b] for j in range(k)])   # the fewest
    # under light weights the same ends are one segment
    assert len(abi.paint_stroke((64, 64, 64), ends, (1, 1, 1))) == 2
    lib = abi.load()
    d, w = (C.c_int32 * 3)(*dims), (C.c_uint32 * 3)(*heavy)
    pos = np.asarray(ends, dtype=np.float32)
    out = np.full((k, 3), -5, dtype=np.int32)
    n_out = C.c_size_t(0)
    assert lib.tbrm_host_paint_stroke(d, pos.ctypes.data_as(C.c_void_p), 2, w, out.ctypes.data_as(C.c_void_p), k, C.byref(n_out)) == abi.ERR_INVALID_ARG
    assert b"capacity" in lib.tbrm_last_error() and n_out.value == k + 1 and (out == -5).all()
    with pytest.raises(abi.TbrmError, match="capacity"):
        abi.paint_stroke(dims, ends, heavy, capacity=k)
    assert np.array_equal(abi.paint_stroke(dims, ends, heavy, capacity=k + 7), got)
    for bad_dims, bad_w, names in (((0, 8, 8), (1, 1, 1), b"dims"), ((8, 16385, 8), (1, 1, 1), b"dims"), ((8, 8, 8), (1, 0, 1), b"weights"), ((8, 8, 8), (1, 1, 65536), b"weights")):
        assert lib.tbrm_host_paint_stroke((C.c_int32 * 3)(*bad_dims), pos.ctypes.data_as(C.c_void_p), 2, (C.c_uint32 * 3)(*bad_w), out.ctypes.data_as(C.c_void_p), k, C.byref(n_out)) == abi.ERR_INVALID_ARG
        assert names in lib.tbrm_last_error() and n_out.value == 0
    assert lib.tbrm_host_paint_stroke(d, pos.ctypes.data_as(C.c_void_p), 0, w, out.ctypes.data_as(C.c_void_p), k, C.byref(n_out)) == abi.ERR_INVALID_ARG and b"n 0" in lib.tbrm_last_error()


def test_plan_under_sanitizers(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "paint_plan_test.cpp")
    exe = str(tmp_path / "paint_plan_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", src, "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip().splitlines()[-1] == "failures=0", p.stdout
