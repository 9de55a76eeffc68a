"""The label surface (include/tbrm_surface.h) without a GPU: the header compiles as C, its symbols are exported and bound and belong to
no other list, the struct layouts match the ctypes mirrors (the vertex record is 20 bytes), null arguments are refused, surface_skip
is a tunable, tbrm_host_surface_unit_cube and tbrm_host_surface_positions do what the header says bit for bit, and the plan
(tbrm_surface_plan.h: what the kernels run, as host code) runs in a stand-alone program under the address and undefined-behaviour
sanitizers. What tbrm_label_surface refuses of a desc needs a handle: tests/test_gpu_label_surface.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tbraymarcherplugin_amd import abi
import label_surface_reference as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "tbrm_surface.h")


def declared_symbols(path=HEADER):
    return re.findall(r"TBRM_API\s+[\w\s\*]+?\b(tbrm_\w+)\s*\(", open(path).read())


def test_header_symbols_are_exported_and_bound():
    lib = abi.load()
    declared = declared_symbols()
    assert sorted(declared) == sorted(abi.SURFACE_SYMBOLS) and len(declared) == 6, set(declared) ^ set(abi.SURFACE_SYMBOLS)
    others = (set(abi.SYMBOLS) | set(abi.LABEL_SYMBOLS) | set(abi.COLOR_LIGHT_SYMBOLS) | set(abi.VOLUME_REGION_SYMBOLS) | set(abi.VOLUME_STATS_SYMBOLS)
              | set(abi.VIEW_CACHE_SYMBOLS) | set(abi.HIT_SYMBOLS) | set(abi.SEGMENT_SYMBOLS) | set(abi.MORPH_SYMBOLS) | set(abi.ISLANDS_SYMBOLS)
              | set(abi.MARGIN_SYMBOLS) | set(abi.SMOOTH_SYMBOLS) | set(abi.SCISSORS_SYMBOLS) | set(abi.COMPETE_SYMBOLS) | set(abi.PAINT_SYMBOLS))
    assert not set(declared) & others
    assert not set(declared) & set(declared_symbols(os.path.join(INCLUDE, "tbrm.h")))   # tbrm.h stays as it is
    for name in declared:
        assert hasattr(lib, name), f"{name} is declared in tbrm_surface.h but not exported by libtbrm.so"
    text = open(HEADER).read()
    version = int(re.search(r"#define\s+TBRM_SURFACE_ABI_VERSION\s+(\d+)", text).group(1))
    assert lib.tbrm_surface_abi_version() == version == abi.SURFACE_ABI_VERSION == 1
    assert abi.SURFACE_MAX_DIM == SR.MAX_DIM == 1 << 19 and re.search(r"#define\s+TBRM_SURFACE_MAX_DIM\s+\(1 << 19\)", text)
    assert re.search(r"TBRM_SURFACE_TRIANGLES\s*=\s*1\b", text) and re.search(r"TBRM_SURFACE_MEASURE\s*=\s*2\b", text)
    assert (abi.SURFACE_TRIANGLES, abi.SURFACE_MEASURE) == (1, 2)
    assert 24 * (abi.SURFACE_MAX_DIM - 1) + 12 < 2 ** 24   # the largest numerator of a position is exact in float32


def test_header_compiles_as_c_and_the_layouts_match(tmp_path):
    v, d, r = abi.SURFACE_VERTEX, abi.SURFACE_DESC, abi.SURFACE_RESULT
    assert C.sizeof(v) == 20 == abi.SURFACE_VERTEX_DTYPE.itemsize == SR.VERTEX_DTYPE.itemsize
    assert (v.cell.offset, v.sum.offset, v.edges.offset, v.normal.offset, v.corners.offset) == (0, 12, 15, 16, 19)
    assert abi.SURFACE_VERTEX_DTYPE == SR.VERTEX_DTYPE
    assert [abi.SURFACE_VERTEX_DTYPE.fields[f[0]][1] for f in v._fields_] == [0, 12, 15, 16, 19]
    assert C.sizeof(d) == 104
    assert (d.origin.offset, d.extent.offset, d.flags.offset, d.reserved.offset, d.vertex_capacity.offset, d.quad_capacity.offset, d.scale.offset, d.offset.offset,
            d.source.offset) == (0, 12, 24, 28, 32, 40, 48, 60, 72)
    assert C.sizeof(r) == 96
    assert (r.set_voxels.offset, r.vertices.offset, r.quads.offset, r.quads_axis.offset, r.cell_min.offset, r.cell_max.offset, r.blocks_evaluated.offset,
            r.blocks_skipped.offset, r.launches.offset, r.written.offset, r.reserved.offset) == (0, 8, 16, 24, 48, 60, 72, 76, 80, 84, 88)
    text = open(HEADER).read()
    for struct, fields in (("tbrm_surface_vertex", v._fields_), ("tbrm_surface_desc", d._fields_), ("tbrm_surface_result", r._fields_)):
        body = re.search(r"typedef struct " + struct + r" \{(.*?)\} " + struct + ";", text, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = re.findall(r"(\w+)(?:\[\d+\])?\s*[,;]", body)
        assert names == [f[0] for f in fields], (struct, names)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "tbrm_surface.h"\n'
                   "int main(void) {\n"
                   '  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(tbrm_surface_vertex), offsetof(tbrm_surface_vertex, edges), offsetof(tbrm_surface_vertex, corners),\n'
                   "         sizeof(tbrm_surface_desc), offsetof(tbrm_surface_desc, vertex_capacity), offsetof(tbrm_surface_desc, scale), offsetof(tbrm_surface_desc, source),\n"
                   "         sizeof(tbrm_surface_result), offsetof(tbrm_surface_result, cell_min), offsetof(tbrm_surface_result, written));\n"
                   "  return TBRM_SURFACE_ABI_VERSION == 1 && TBRM_SURFACE_MAX_DIM == 524288 && TBRM_SURFACE_TRIANGLES == 1 && TBRM_SURFACE_MEASURE == 2 ? 0 : 1;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", INCLUDE, str(src), "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.split() == ["20", "15", "19", "104", "32", "48", "72", "96", "48", "84"], p.stdout


def test_the_other_label_headers_are_unchanged():
    for header, symbols, count, version in (("tbrm_paint.h", abi.PAINT_SYMBOLS, 5, ("PAINT", abi.load().tbrm_paint_abi_version())),
                                            ("tbrm_islands.h", abi.ISLANDS_SYMBOLS, len(abi.ISLANDS_SYMBOLS), ("ISLANDS", abi.load().tbrm_islands_abi_version())),
                                            ("tbrm_morphology.h", abi.MORPH_SYMBOLS, len(abi.MORPH_SYMBOLS), ("MORPH", abi.load().tbrm_morph_abi_version()))):
        path = os.path.join(INCLUDE, header)
        assert sorted(declared_symbols(path)) == sorted(symbols) and len(symbols) == count, header
        assert int(re.search(r"#define\s+TBRM_" + version[0] + r"_ABI_VERSION\s+(\d+)", open(path).read()).group(1)) == version[1], header


def test_surface_skip_is_a_tunable():
    old = abi.get_tunable("surface_skip")
    assert old == 1
    try:
        abi.set_tunable("surface_skip", 0)
        assert abi.get_tunable("surface_skip") == 0
        assert abi.get_tunable("paint_skip") == 1   # a tunable of its own
    finally:
        abi.set_tunable("surface_skip", old)


def test_null_arguments_are_refused():
    lib = abi.load()
    z = C.c_void_p(None)
    fake = C.c_void_p(8)   # never dereferenced: the pointer checks come first
    desc, out, out6 = abi.SURFACE_DESC(), abi.SURFACE_RESULT(), (C.c_uint64 * 6)()
    one = (C.c_float * 3)(1, 1, 1)
    dims = (C.c_int32 * 3)(8, 8, 8)
    rec, pos = (abi.SURFACE_VERTEX * 1)(), (C.c_float * 3)()
    calls = {
        "tbrm_label_surface": [lambda: lib.tbrm_label_surface(z, C.byref(desc), None, None, None, C.byref(out)), lambda: lib.tbrm_label_surface(fake, None, None, None, None, C.byref(out)),
                               lambda: lib.tbrm_label_surface(fake, C.byref(desc), None, None, None, None)],
        "tbrm_label_surface_device": [lambda: lib.tbrm_label_surface_device(z, C.byref(desc), None, None, None, C.byref(out)),
                                      lambda: lib.tbrm_label_surface_device(fake, None, None, None, None, C.byref(out)),
                                      lambda: lib.tbrm_label_surface_device(fake, C.byref(desc), None, None, None, None)],
        "tbrm_surface_counters": [lambda: lib.tbrm_surface_counters(z, C.byref(out6)), lambda: lib.tbrm_surface_counters(fake, None)],
        "tbrm_host_surface_positions": [lambda: lib.tbrm_host_surface_positions(None, 1, one, one, pos), lambda: lib.tbrm_host_surface_positions(rec, 1, None, one, pos),
                                        lambda: lib.tbrm_host_surface_positions(rec, 1, one, None, pos), lambda: lib.tbrm_host_surface_positions(rec, 1, one, one, None)],
        "tbrm_host_surface_unit_cube": [lambda: lib.tbrm_host_surface_unit_cube(None, one, one), lambda: lib.tbrm_host_surface_unit_cube(dims, None, one),
                                        lambda: lib.tbrm_host_surface_unit_cube(dims, one, None)],
    }
    for name, variants in calls.items():
        for k, call in enumerate(variants):
            abi.set_tunable("ray_labels", 0)   # (a successful call in between: the next message is this call's own)
            assert call() == abi.ERR_INVALID_ARG, (name, k)
            assert b"null" in lib.tbrm_last_error(), (name, k)
    assert set(abi.SURFACE_SYMBOLS) == set(calls) | {"tbrm_surface_abi_version"}


def test_the_unit_cube():
    for dims in ((8, 8, 8), (40, 27, 19), (1, 2, 512), (524288, 3, 1)):
        scale, offset = abi.surface_unit_cube(dims)
        want_scale, want_offset = SR.unit_cube(dims)
        assert [np.float32(s).tobytes() for s in scale] == [np.float32(s).tobytes() for s in want_scale], dims
        assert offset == want_offset == (0.0, 0.0, 0.0)
        assert all(s == 0.0 for s, n in zip(scale, dims) if n == 1)
    lib = abi.load()
    s, o = (C.c_float * 3)(7, 7, 7), (C.c_float * 3)(7, 7, 7)
    for bad in ((0, 8, 8), (8, 8, -1)):
        assert lib.tbrm_host_surface_unit_cube((C.c_int32 * 3)(*bad), s, o) == abi.ERR_INVALID_ARG and b"dims" in lib.tbrm_last_error()
        assert tuple(s) == (7, 7, 7) and tuple(o) == (7, 7, 7)   # a refusal leaves the outputs alone


def test_the_positions_bit_for_bit():
    rng = np.random.default_rng(23)
    n = 4000
    v = np.zeros(n, dtype=abi.SURFACE_VERTEX_DTYPE)
    v["edges"] = rng.integers(3, 13, size=n)
    v["sum"] = (rng.random((n, 3)) * (2 * v["edges"][:, None] + 1)).astype(np.uint8)   # 0 .. 2 edges
    v["cell"] = rng.integers(-1, 600, size=(n, 3))
    v["cell"][:50] = -1                                             # a face at 0: the low corner lies outside
    v["cell"][50:100] = abi.SURFACE_MAX_DIM - 1                     # the largest numerator
    v["sum"][50:100] = 2 * v["edges"][50:100, None]
    for scale, offset in (((1.0, 1.0, 1.0), (0.0, 0.0, 0.0)), ((0.7, 0.7, 2.5), (-10.0, 3.25, 100.0)), ((1e-3, -3.0, 1.0 / 3.0), (1e6, -1e-6, 0.1)),
                          (*abi.surface_unit_cube((41, 1, 19)),)):
        got = abi.surface_positions(v, scale, offset)
        want = SR.positions_of(v, scale, offset)
        assert got.dtype == np.float32 and got.tobytes() == want.tobytes(), (scale, offset, np.argwhere(got != want)[:5])
    # N = 1: the scale is 0 and every position is the offset
    s, o = abi.surface_unit_cube((1, 1, 1))
    assert (abi.surface_positions(v[:10], s, o) == 0.0).all()
    assert abi.surface_positions(v[:0]).shape == (0, 3)
    lib = abi.load()
    out = np.full((2, 3), -5.0, dtype=np.float32)
    one = (C.c_float * 3)(1, 1, 1)
    for field, value, names in (("edges", 0, b"edges"), ("edges", 13, b"edges"), ("cell", -2, b"cell"), ("cell", abi.SURFACE_MAX_DIM, b"cell")):
        bad = v[:2].copy()
        bad[field][1] = value
        assert lib.tbrm_host_surface_positions(bad.ctypes.data_as(C.c_void_p), 2, one, one, out.ctypes.data_as(C.c_void_p)) == abi.ERR_INVALID_ARG
        assert names in lib.tbrm_last_error() and (out == -5.0).all()
    for bad_scale in ((np.inf, 1, 1), (1, np.nan, 1)):
        assert lib.tbrm_host_surface_positions(v.ctypes.data_as(C.c_void_p), 2, (C.c_float * 3)(*bad_scale), one, out.ctypes.data_as(C.c_void_p)) == abi.ERR_INVALID_ARG
        assert b"finite" in lib.tbrm_last_error() and (out == -5.0).all()


def test_plan_under_sanitizers(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "surface_plan_test.cpp")
    exe = str(tmp_path / "surface_plan_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", src, "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip().splitlines()[-1] == "failures=0", p.stdout
