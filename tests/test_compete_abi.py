"""Competitive growing from seed labels (include/tbrm_compete.h) without a GPU: the header compiles as C, its symbols are exported and
bound and belong to no other list, the struct layouts match the ctypes mirrors, tbrm.h keeps its 62 symbols and tbrm_segment.h its 5,
null arguments are refused, tbrm_host_compete_float_range equals its restatement and refuses what has no codes, and the rules the
host and the kernels share (tbrm_compete_plan.h) run in a stand-alone program under the address and undefined-behaviour sanitizers.
The refusals that need a handle are in tests/test_gpu_label_compete.py."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np

from tbraymarcherplugin_amd import abi
import label_compete_reference as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "tbrm_compete.h")


def declared_symbols(path=HEADER):
    return re.findall(r"TBRM_API\s+[\w\s\*]+?\b(tbrm_\w+)\s*\(", open(path).read())


def test_header_symbols_are_exported_and_bound():
    lib = abi.load()
    declared = declared_symbols()
    assert sorted(declared) == sorted(abi.COMPETE_SYMBOLS), set(declared) ^ set(abi.COMPETE_SYMBOLS)
    others = (set(abi.SYMBOLS) | set(abi.LABEL_SYMBOLS) | set(abi.COLOR_LIGHT_SYMBOLS) | set(abi.VOLUME_REGION_SYMBOLS) | set(abi.VOLUME_STATS_SYMBOLS)
              | set(abi.VIEW_CACHE_SYMBOLS) | set(abi.HIT_SYMBOLS) | set(abi.SEGMENT_SYMBOLS) | set(abi.MORPH_SYMBOLS) | set(abi.ISLANDS_SYMBOLS)
              | set(abi.MARGIN_SYMBOLS) | set(abi.SMOOTH_SYMBOLS) | set(abi.SCISSORS_SYMBOLS))
    assert not set(declared) & others
    for name in declared:
        assert hasattr(lib, name), f"{name} is declared in tbrm_compete.h but not exported by libtbrm.so"
    text = open(HEADER).read()
    version = int(re.search(r"#define\s+TBRM_COMPETE_ABI_VERSION\s+(\d+)", text).group(1))
    assert lib.tbrm_compete_abi_version() == version == abi.COMPETE_ABI_VERSION == 1
    for name, value in (("MAX_COST", 0xFFFFFF), ("MAX_STEP_COST", 65535), ("MAX_SHIFT", 16), ("NO_COST", 0xFFFFFFFF)):
        assert int(re.search(r"#define\s+TBRM_COMPETE_" + name + r"\s+(\w+?)u?\s", text).group(1), 0) == getattr(abi, "COMPETE_" + name) == value
    assert (CR.MAX_COST, CR.UNREACHED) == (abi.COMPETE_MAX_COST, abi.COMPETE_NO_COST)


def test_header_compiles_as_c_and_the_layouts_match(tmp_path):
    d, r = abi.COMPETE_DESC, abi.COMPETE_RESULT
    assert C.sizeof(d) == 144
    assert (d.origin.offset, d.extent.offset, d.connectivity.offset, d.measure_only.offset, d.step_cost.offset, d.value_shift.offset, d.cost_limit.offset,
            d.reserved.offset, d.lo.offset, d.hi.offset, d.float_origin.offset, d.float_scale.offset, d.seeds.offset, d.writable.offset) == (
        0, 12, 24, 28, 32, 44, 48, 52, 56, 64, 72, 76, 80, 112)
    assert C.sizeof(r) == 2112
    assert (r.seed_voxels.offset, r.claimable.offset, r.claimed.offset, r.relabelled.offset, r.claimed_per_label.offset, r.max_cost.offset, r.passes.offset,
            r.bbox_min.offset, r.bbox_max.offset) == (0, 8, 16, 24, 32, 2080, 2084, 2088, 2100)
    text = open(HEADER).read()
    for struct, fields in (("tbrm_compete_desc", d._fields_), ("tbrm_compete_result", r._fields_)):
        body = re.search(r"typedef struct " + struct + r" \{(.*?)\} " + struct + ";", text, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = re.findall(r"(\w+)(?:\[\d+\])?\s*[,;]", body)
        assert names == [f[0] for f in fields], (struct, names)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "tbrm_compete.h"\n'
                   "int main(void) {\n"
                   '  printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(tbrm_compete_desc), offsetof(tbrm_compete_desc, cost_limit), offsetof(tbrm_compete_desc, lo),\n'
                   "         offsetof(tbrm_compete_desc, float_scale), offsetof(tbrm_compete_desc, writable), sizeof(tbrm_compete_result),\n"
                   "         offsetof(tbrm_compete_result, max_cost), offsetof(tbrm_compete_result, bbox_max));\n"
                   "  return TBRM_COMPETE_MAX_COST == 16777215u && TBRM_COMPETE_NO_COST == 4294967295u && TBRM_COMPETE_MAX_SHIFT == 16 ? 0 : 1;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", INCLUDE, str(src), "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.split() == ["144", "48", "56", "76", "112", "2112", "2080", "2100"], p.stdout


def test_the_other_headers_are_unchanged():
    main = os.path.join(INCLUDE, "tbrm.h")
    declared = declared_symbols(main)
    assert len(declared) == len(abi.SYMBOLS) == 62 and sorted(declared) == sorted(abi.SYMBOLS)
    assert int(re.search(r"#define\s+TBRM_ABI_VERSION\s+(\d+)", open(main).read()).group(1)) == abi.ABI_VERSION == abi.load().tbrm_abi_version() == 5
    segment = os.path.join(INCLUDE, "tbrm_segment.h")
    assert sorted(declared_symbols(segment)) == sorted(abi.SEGMENT_SYMBOLS) and len(abi.SEGMENT_SYMBOLS) == 5
    assert int(re.search(r"#define\s+TBRM_SEGMENT_ABI_VERSION\s+(\d+)", open(segment).read()).group(1)) == abi.load().tbrm_segment_abi_version() == 1
    assert abi.get_tunable("grow_batch") == 16   # the passes are batched by region growing's tunable: there is no new one


def test_null_arguments_are_refused():
    lib = abi.load()
    z = C.c_void_p(None)
    fake = C.c_void_p(8)   # never dereferenced: the pointer checks come first
    desc, out, out4 = abi.COMPETE_DESC(), abi.COMPETE_RESULT(), (C.c_uint64 * 4)()
    o, s = C.c_float(), C.c_float()
    calls = {
        "tbrm_compete_labels": [lambda: lib.tbrm_compete_labels(z, C.byref(desc), None, C.byref(out)),
                                lambda: lib.tbrm_compete_labels(fake, None, None, C.byref(out)),
                                lambda: lib.tbrm_compete_labels(fake, C.byref(desc), None, None)],
        "tbrm_compete_counters": [lambda: lib.tbrm_compete_counters(z, C.byref(out4)), lambda: lib.tbrm_compete_counters(fake, None)],
        "tbrm_host_compete_float_range": [lambda: lib.tbrm_host_compete_float_range(0.0, 1.0, None, C.byref(s)),
                                          lambda: lib.tbrm_host_compete_float_range(0.0, 1.0, C.byref(o), None)],
    }
    for name, variants in calls.items():
        for k, call in enumerate(variants):
            abi.set_tunable("ray_labels", 0)   # (a successful call in between: the next message is this call's own)
            assert call() == abi.ERR_INVALID_ARG, (name, k)
            assert b"null" in lib.tbrm_last_error(), (name, k)
    assert set(abi.COMPETE_SYMBOLS) == set(calls) | {"tbrm_compete_abi_version"}


def test_float_range():
    lib = abi.load()
    for lo, hi in ((-1000.0, 3000.0), (0.0, 1.0), (-1e-3, 1e-3), (1e30, 2e30), (-3e38, 1.5e38), (0.1, 0.1000001), (0.0, 65535.0)):
        assert abi.compete_float_range(lo, hi) == CR.float_range(lo, hi), (lo, hi)
    assert abi.compete_float_range(0.0, 65535.0) == (0.0, 1.0)
    o, s = C.c_float(-7.0), C.c_float(-7.0)
    for lo, hi in ((1.0, 1.0), (2.0, 1.0), (math.nan, 1.0), (0.0, math.nan), (0.0, math.inf), (-math.inf, 0.0), (0.0, 1e-320), (-1e300, 1e300), (1e39, 2e39)):
        assert lib.tbrm_host_compete_float_range(lo, hi, C.byref(o), C.byref(s)) == abi.ERR_INVALID_ARG, (lo, hi)
        assert b"range" in lib.tbrm_last_error() and (o.value, s.value) == (-7.0, -7.0)   # a refusal leaves the outputs alone
    # the codes of the ends of a range: 0 and 65535, and nothing outside
    fr = CR.float_range(-1000.0, 3000.0)
    c = CR.codes(np.array([-1000.0, 3000.0, -5000.0, 1e9, 1000.0], dtype=np.float32), fr)
    assert list(c[:4]) == [0, 65535, 0, 65535] and abs(int(c[4]) - 32768) <= 1


def test_plan_under_sanitizers(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "compete_plan_test.cpp")
    exe = str(tmp_path / "compete_plan_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", src, "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip().splitlines()[-1] == "failures=0", p.stdout
