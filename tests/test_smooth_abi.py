"""Smoothing of labels (include/tbrm_smooth.h) without a GPU: the header compiles as C, its symbols are exported and bound and belong to
no other list, the struct layouts match the ctypes mirrors, the other headers are as they were, null arguments are refused before
anything is dereferenced, smooth_skip is a tunable, tbrm_host_smooth_radii refuses what it must, and the plan (tbrm_smooth_plan.h: pure
host code) runs in a stand-alone program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import subprocess

from tbraymarcherplugin_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "tbrm_smooth.h")


def declared_symbols(path=HEADER):
    return re.findall(r"TBRM_API\s+[\w\s\*]+?\b(tbrm_\w+)\s*\(", open(path).read())


def test_header_symbols_are_exported_and_bound():
    lib = abi.load()
    declared = declared_symbols()
    assert sorted(declared) == sorted(abi.SMOOTH_SYMBOLS), set(declared) ^ set(abi.SMOOTH_SYMBOLS)
    others = (set(abi.SYMBOLS) | set(abi.LABEL_SYMBOLS) | set(abi.COLOR_LIGHT_SYMBOLS) | set(abi.VOLUME_REGION_SYMBOLS) | set(abi.VOLUME_STATS_SYMBOLS)
              | set(abi.VIEW_CACHE_SYMBOLS) | set(abi.HIT_SYMBOLS) | set(abi.SEGMENT_SYMBOLS) | set(abi.MORPH_SYMBOLS) | set(abi.ISLANDS_SYMBOLS)
              | set(abi.MARGIN_SYMBOLS))
    assert not set(declared) & others
    for name in declared:
        assert hasattr(lib, name), f"{name} is declared in tbrm_smooth.h but not exported by libtbrm.so"
    text = open(HEADER).read()
    version = int(re.search(r"#define\s+TBRM_SMOOTH_ABI_VERSION\s+(\d+)", text).group(1))
    assert lib.tbrm_smooth_abi_version() == version == abi.SMOOTH_ABI_VERSION == 1
    for name, value in (("MAX_RADIUS", 16), ("MAX_ITERATIONS", 64), ("MAX_REACH", 64), ("MAX_RANK_DEN", 256)):
        assert int(re.search(r"#define\s+TBRM_SMOOTH_" + name + r"\s+(\d+)", text).group(1)) == getattr(abi, "SMOOTH_" + name) == value
    assert abi.SMOOTH_MAX_REACH == abi.MARGIN_MAX_REACH == abi.MORPH_MAX_RADIUS


def test_header_compiles_as_c_and_the_layouts_match(tmp_path):
    d, r = abi.SMOOTH_DESC, abi.SMOOTH_RESULT
    assert C.sizeof(d) == 124
    assert (d.origin.offset, d.extent.offset, d.radius.offset, d.rank_num.offset, d.rank_den.offset, d.iterations.offset, d.new_label.offset,
            d.erase_label.offset, d.reserved.offset, d.source.offset, d.writable.offset) == (0, 12, 24, 36, 40, 44, 48, 52, 56, 60, 92)
    assert C.sizeof(r) == 80
    assert (r.source_voxels.offset, r.result_voxels.offset, r.added.offset, r.removed.offset, r.relabelled.offset, r.bbox_min.offset,
            r.bbox_max.offset, r.reach.offset, r.launches.offset) == (0, 8, 16, 24, 32, 40, 52, 64, 76)
    # the result is tbrm_morph_result's fields, where they are there, then tbrm_margin_result's
    m = abi.MORPH_RESULT
    for name in ("source_voxels", "result_voxels", "added", "removed", "relabelled", "bbox_min", "bbox_max"):
        assert getattr(r, name).offset == getattr(m, name).offset and getattr(r, name).size == getattr(m, name).size
    assert [(f[0], C.sizeof(f[1])) for f in r._fields_] == [(f[0], C.sizeof(f[1])) for f in abi.MARGIN_RESULT._fields_]
    # the header's field order is the binding's
    text = open(HEADER).read()
    for struct, fields in (("tbrm_smooth_desc", d._fields_), ("tbrm_smooth_result", r._fields_)):
        body = re.search(r"typedef struct " + struct + r" \{(.*?)\} " + struct + ";", text, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = re.findall(r"(\w+)(?:\[\d+\])?\s*[,;]", body)
        assert names == [f[0] for f in fields], (struct, names)
    # and a C compiler agrees
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "tbrm_smooth.h"\n'
                   "int main(void) {\n"
                   '  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(tbrm_smooth_desc), offsetof(tbrm_smooth_desc, radius), offsetof(tbrm_smooth_desc, rank_num),\n'
                   "         offsetof(tbrm_smooth_desc, iterations), offsetof(tbrm_smooth_desc, source), offsetof(tbrm_smooth_desc, writable), sizeof(tbrm_smooth_result),\n"
                   "         offsetof(tbrm_smooth_result, reach), offsetof(tbrm_smooth_result, launches));\n"
                   "  return TBRM_SMOOTH_MAX_RADIUS == 16 && TBRM_SMOOTH_MAX_RANK_DEN == 256 ? 0 : 1;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", INCLUDE, str(src), "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.split() == ["124", "24", "36", "44", "60", "92", "80", "64", "76"], p.stdout


def test_the_other_headers_are_unchanged():
    main = os.path.join(INCLUDE, "tbrm.h")
    declared = declared_symbols(main)
    assert len(declared) == len(abi.SYMBOLS) == 62 and sorted(declared) == sorted(abi.SYMBOLS)
    assert int(re.search(r"#define\s+TBRM_ABI_VERSION\s+(\d+)", open(main).read()).group(1)) == abi.ABI_VERSION == abi.load().tbrm_abi_version() == 5
    for header, symbols, count, version in (("tbrm_segment.h", abi.SEGMENT_SYMBOLS, 5, ("SEGMENT", abi.load().tbrm_segment_abi_version())),
                                            ("tbrm_morphology.h", abi.MORPH_SYMBOLS, 3, ("MORPH", abi.load().tbrm_morph_abi_version())),
                                            ("tbrm_islands.h", abi.ISLANDS_SYMBOLS, 3, ("ISLANDS", abi.load().tbrm_islands_abi_version())),
                                            ("tbrm_margin.h", abi.MARGIN_SYMBOLS, 5, ("MARGIN", abi.load().tbrm_margin_abi_version()))):
        path = os.path.join(INCLUDE, header)
        assert sorted(declared_symbols(path)) == sorted(symbols) and len(symbols) == count, header
        assert int(re.search(r"#define\s+TBRM_" + version[0] + r"_ABI_VERSION\s+(\d+)", open(path).read()).group(1)) == version[1] == 1, header
    assert C.sizeof(abi.MORPH_DESC) == 112 and C.sizeof(abi.MORPH_RESULT) == 72 and C.sizeof(abi.MARGIN_DESC) == 120 and C.sizeof(abi.MARGIN_RESULT) == 80


def test_smooth_skip_is_a_tunable():
    old = abi.get_tunable("smooth_skip")
    assert old == 1
    try:
        abi.set_tunable("smooth_skip", 0)
        assert abi.get_tunable("smooth_skip") == 0
        assert abi.get_tunable("margin_skip") == 1   # a tunable of its own
    finally:
        abi.set_tunable("smooth_skip", old)


def test_null_arguments_are_refused():
    lib = abi.load()
    z = C.c_void_p(None)
    fake = C.c_void_p(8)   # never dereferenced: the pointer checks come first
    desc = abi.SMOOTH_DESC()
    desc.radius[:] = [1, 1, 1]
    desc.rank_num, desc.rank_den, desc.iterations, desc.new_label = 1, 2, 1, -1
    out, out4 = abi.SMOOTH_RESULT(), (C.c_uint64 * 4)()
    sp, radii = (C.c_double * 3)(1, 1, 1), (C.c_int32 * 3)()
    calls = {
        "tbrm_smooth_labels": [lambda: lib.tbrm_smooth_labels(z, C.byref(desc), C.byref(out)),
                               lambda: lib.tbrm_smooth_labels(fake, None, C.byref(out)),
                               lambda: lib.tbrm_smooth_labels(fake, C.byref(desc), None)],
        "tbrm_host_smooth_radii": [lambda: lib.tbrm_host_smooth_radii(None, 1.0, radii), lambda: lib.tbrm_host_smooth_radii(sp, 1.0, None)],
        "tbrm_smooth_counters": [lambda: lib.tbrm_smooth_counters(z, C.byref(out4)), lambda: lib.tbrm_smooth_counters(fake, None)],
    }
    for name, variants in calls.items():
        for k, call in enumerate(variants):
            abi.set_tunable("ray_labels", 0)   # (a successful call in between: the next message is this call's own)
            assert call() == abi.ERR_INVALID_ARG, (name, k)
            assert b"null" in lib.tbrm_last_error(), (name, k)
    assert set(abi.SMOOTH_SYMBOLS) == set(calls) | {"tbrm_smooth_abi_version"}


def test_host_smooth_radii_errors():
    lib = abi.load()
    radii = (C.c_int32 * 3)(-7, -7, -7)
    for spacing, radius in (((0.0, 1, 1), 1.0), ((1, -1, 1), 1.0), ((1, 1, float("nan")), 1.0), ((1, 1, float("inf")), 1.0), ((1, 1, 1), 0.0), ((1, 1, 1), -2.0),
                            ((1, 1, 1), float("nan")), ((1, 1, 1), float("inf")), ((1, 1, 1), 16.5), ((1, 1, 0.1), 2.0), ((1, 1, 1), 0.4)):
        assert lib.tbrm_host_smooth_radii((C.c_double * 3)(*spacing), radius, radii) == abi.ERR_INVALID_ARG, (spacing, radius)
        assert b"radius" in lib.tbrm_last_error() and list(radii) == [-7, -7, -7]   # a refusal leaves the output alone
    assert lib.tbrm_host_smooth_radii((C.c_double * 3)(0.7, 0.7, 2.5), 2.0, radii) == abi.OK and list(radii) == [3, 3, 1]
    assert abi.smooth_radii((0.7, 0.7, 2.5), 2.0) == (3, 3, 1)


def test_plan_under_sanitizers(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "smooth_plan_test.cpp")
    exe = str(tmp_path / "smooth_plan_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", src, "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip().splitlines()[-1] == "failures=0", p.stdout
