"""Euclidean margins of labels (include/tbrm_margin.h) without a GPU: the header compiles as C, its symbols are exported and bound, the
struct layouts match the ctypes mirrors, the other headers are as they were, null arguments are refused before anything is
dereferenced, margin_skip is a tunable, and the plan (tbrm_margin_plan.h: pure host code) runs in a stand-alone program under the
address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import subprocess

from tbraymarcherplugin_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "tbrm_margin.h")


def declared_symbols(path=HEADER):
    return re.findall(r"TBRM_API\s+[\w\s\*]+?\b(tbrm_\w+)\s*\(", open(path).read())


def test_header_symbols_are_exported_and_bound():
    lib = abi.load()
    declared = declared_symbols()
    assert sorted(declared) == sorted(abi.MARGIN_SYMBOLS), set(declared) ^ set(abi.MARGIN_SYMBOLS)
    others = (set(abi.SYMBOLS) | set(abi.LABEL_SYMBOLS) | set(abi.COLOR_LIGHT_SYMBOLS) | set(abi.VOLUME_REGION_SYMBOLS) | set(abi.VOLUME_STATS_SYMBOLS)
              | set(abi.VIEW_CACHE_SYMBOLS) | set(abi.HIT_SYMBOLS) | set(abi.SEGMENT_SYMBOLS) | set(abi.MORPH_SYMBOLS) | set(abi.ISLANDS_SYMBOLS))
    assert not set(declared) & others
    for name in declared:
        assert hasattr(lib, name), f"{name} is declared in tbrm_margin.h but not exported by libtbrm.so"
    text = open(HEADER).read()
    version = int(re.search(r"#define\s+TBRM_MARGIN_ABI_VERSION\s+(\d+)", text).group(1))
    assert lib.tbrm_margin_abi_version() == version == abi.MARGIN_ABI_VERSION == 1
    assert int(re.search(r"#define\s+TBRM_MARGIN_MAX_REACH\s+(\d+)", text).group(1)) == abi.MARGIN_MAX_REACH == abi.MORPH_MAX_RADIUS == 64
    assert int(re.search(r"#define\s+TBRM_MARGIN_FAR\s+(0x[0-9A-Fa-f]+)u", text).group(1), 16) == abi.MARGIN_FAR == 2 ** 32 - 1
    ops = dict(re.findall(r"TBRM_MARGIN_(EXPAND|SHRINK|OPEN|CLOSE)\s*=\s*(\d)", text))
    assert {k.lower(): int(v) for k, v in ops.items()} == abi.MARGIN_OPS == {"expand": 0, "shrink": 1, "open": 2, "close": 3}


def test_header_compiles_as_c_and_the_layouts_match(tmp_path):
    d, r = abi.MARGIN_DESC, abi.MARGIN_RESULT
    assert C.sizeof(d) == 120
    assert (d.origin.offset, d.extent.offset, d.op.offset, d.new_label.offset, d.erase_label.offset, d.reserved.offset, d.weights.offset,
            d.limit.offset, d.source.offset, d.writable.offset) == (0, 12, 24, 28, 32, 36, 40, 52, 56, 88)
    assert C.sizeof(r) == 80
    assert (r.source_voxels.offset, r.result_voxels.offset, r.added.offset, r.removed.offset, r.relabelled.offset, r.bbox_min.offset,
            r.bbox_max.offset, r.reach.offset, r.launches.offset) == (0, 8, 16, 24, 32, 40, 52, 64, 76)
    # the result begins with tbrm_morph_result's fields, where they are there
    m = abi.MORPH_RESULT
    for name in ("source_voxels", "result_voxels", "added", "removed", "relabelled", "bbox_min", "bbox_max"):
        assert getattr(r, name).offset == getattr(m, name).offset and getattr(r, name).size == getattr(m, name).size
    # the header's field order is the binding's
    text = open(HEADER).read()
    for struct, fields in (("tbrm_margin_desc", d._fields_), ("tbrm_margin_result", r._fields_)):
        body = re.search(r"typedef struct " + struct + r" \{(.*?)\} " + struct + ";", text, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = re.findall(r"(\w+)(?:\[\d+\])?\s*[,;]", body)
        assert names == [f[0] for f in fields], (struct, names)
    # and a C compiler agrees
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "tbrm_margin.h"\n'
                   "int main(void) {\n"
                   '  printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(tbrm_margin_desc), offsetof(tbrm_margin_desc, weights), offsetof(tbrm_margin_desc, limit),\n'
                   "         offsetof(tbrm_margin_desc, source), offsetof(tbrm_margin_desc, writable), sizeof(tbrm_margin_result),\n"
                   "         offsetof(tbrm_margin_result, reach), offsetof(tbrm_margin_result, launches));\n"
                   "  return TBRM_MARGIN_FAR == 0xFFFFFFFFu && TBRM_MARGIN_CLOSE == 3 ? 0 : 1;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", INCLUDE, str(src), "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.split() == ["120", "40", "52", "56", "88", "80", "64", "76"], p.stdout


def test_the_other_headers_are_unchanged():
    main = os.path.join(INCLUDE, "tbrm.h")
    declared = declared_symbols(main)
    assert len(declared) == len(abi.SYMBOLS) == 62 and sorted(declared) == sorted(abi.SYMBOLS)
    assert int(re.search(r"#define\s+TBRM_ABI_VERSION\s+(\d+)", open(main).read()).group(1)) == abi.ABI_VERSION == abi.load().tbrm_abi_version() == 5
    for header, symbols, count, version in (("tbrm_segment.h", abi.SEGMENT_SYMBOLS, 5, ("SEGMENT", abi.load().tbrm_segment_abi_version())),
                                            ("tbrm_morphology.h", abi.MORPH_SYMBOLS, 3, ("MORPH", abi.load().tbrm_morph_abi_version())),
                                            ("tbrm_islands.h", abi.ISLANDS_SYMBOLS, 3, ("ISLANDS", abi.load().tbrm_islands_abi_version()))):
        path = os.path.join(INCLUDE, header)
        assert sorted(declared_symbols(path)) == sorted(symbols) and len(symbols) == count, header
        assert int(re.search(r"#define\s+TBRM_" + version[0] + r"_ABI_VERSION\s+(\d+)", open(path).read()).group(1)) == version[1] == 1, header
    assert C.sizeof(abi.MORPH_DESC) == 112 and C.sizeof(abi.MORPH_RESULT) == 72


def test_margin_skip_is_a_tunable():
    old = abi.get_tunable("margin_skip")
    assert old == 1
    try:
        abi.set_tunable("margin_skip", 0)
        assert abi.get_tunable("margin_skip") == 0
    finally:
        abi.set_tunable("margin_skip", old)


def test_null_arguments_are_refused():
    lib = abi.load()
    z = C.c_void_p(None)
    fake = C.c_void_p(8)   # never dereferenced: the pointer checks come first
    desc = abi.MARGIN_DESC()
    desc.op, desc.new_label, desc.limit = abi.MARGIN_CLOSE, -1, 4
    desc.weights[:] = [1, 1, 1]
    out, out4, buf = abi.MARGIN_RESULT(), (C.c_uint64 * 4)(), (C.c_uint32 * 8)()
    sp, w, limit = (C.c_double * 3)(1, 1, 1), (C.c_uint32 * 3)(), C.c_uint32()
    calls = {
        "tbrm_margin_labels": [lambda: lib.tbrm_margin_labels(z, C.byref(desc), C.byref(out)),
                               lambda: lib.tbrm_margin_labels(fake, None, C.byref(out)),
                               lambda: lib.tbrm_margin_labels(fake, C.byref(desc), None)],
        "tbrm_label_distance": [lambda: lib.tbrm_label_distance(z, C.byref(desc), 0, buf, 32),
                                lambda: lib.tbrm_label_distance(fake, None, 0, buf, 32),
                                lambda: lib.tbrm_label_distance(fake, C.byref(desc), 0, None, 32)],
        "tbrm_host_margin_weights": [lambda: lib.tbrm_host_margin_weights(None, 1.0, w, C.byref(limit)),
                                     lambda: lib.tbrm_host_margin_weights(sp, 1.0, None, C.byref(limit)),
                                     lambda: lib.tbrm_host_margin_weights(sp, 1.0, w, None)],
        "tbrm_margin_counters": [lambda: lib.tbrm_margin_counters(z, C.byref(out4)), lambda: lib.tbrm_margin_counters(fake, None)],
    }
    for name, variants in calls.items():
        for k, call in enumerate(variants):
            abi.set_tunable("ray_labels", 0)   # (a successful call in between: the next message is this call's own)
            assert call() == abi.ERR_INVALID_ARG, (name, k)
            assert b"null" in lib.tbrm_last_error(), (name, k)
    assert set(abi.MARGIN_SYMBOLS) == set(calls) | {"tbrm_margin_abi_version"}


def test_plan_under_sanitizers(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "margin_plan_test.cpp")
    exe = str(tmp_path / "margin_plan_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", src, "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip().splitlines()[-1] == "failures=0", p.stdout
