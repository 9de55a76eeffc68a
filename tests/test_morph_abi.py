"""Label morphology (include/tbrm_morphology.h) without a GPU: the header's symbols exported and bound, the struct layouts, tbrm.h and
tbrm_segment.h left as they were, null arguments refused before anything is dereferenced, the morph_steps tunable, and the step plan
(tbrm_morph_plan.h: pure host code) in a stand-alone program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import subprocess

from tbraymarcherplugin_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tbrm_morphology.h")


def declared_symbols(path=HEADER):
    return re.findall(r"TBRM_API\s+[\w\s\*]+?\b(tbrm_\w+)\s*\(", open(path).read())


def test_header_symbols_are_exported_and_bound():
    lib = abi.load()
    declared = declared_symbols()
    assert sorted(declared) == sorted(abi.MORPH_SYMBOLS), set(declared) ^ set(abi.MORPH_SYMBOLS)
    others = (set(abi.SYMBOLS) | set(abi.LABEL_SYMBOLS) | set(abi.COLOR_LIGHT_SYMBOLS) | set(abi.VOLUME_REGION_SYMBOLS) | set(abi.VOLUME_STATS_SYMBOLS)
              | set(abi.VIEW_CACHE_SYMBOLS) | set(abi.HIT_SYMBOLS) | set(abi.SEGMENT_SYMBOLS))
    assert not set(declared) & others
    for name in declared:
        assert hasattr(lib, name), f"{name} is declared in tbrm_morphology.h but not exported by libtbrm.so"
    text = open(HEADER).read()
    version = int(re.search(r"#define\s+TBRM_MORPH_ABI_VERSION\s+(\d+)", text).group(1))
    assert lib.tbrm_morph_abi_version() == version == abi.MORPH_ABI_VERSION == 1
    assert int(re.search(r"#define\s+TBRM_MORPH_MAX_RADIUS\s+(\d+)", text).group(1)) == abi.MORPH_MAX_RADIUS == 64
    ops = dict(re.findall(r"TBRM_MORPH_(DILATE|ERODE|OPEN|CLOSE)\s*=\s*(\d)", text))
    assert {k.lower(): int(v) for k, v in ops.items()} == abi.MORPH_OPS == {"dilate": 0, "erode": 1, "open": 2, "close": 3}


def test_struct_layouts():
    d, r = abi.MORPH_DESC, abi.MORPH_RESULT
    assert C.sizeof(d) == 112
    assert (d.origin.offset, d.extent.offset, d.op.offset, d.radius.offset, d.connectivity.offset, d.new_label.offset, d.erase_label.offset,
            d.reserved.offset, d.source.offset, d.writable.offset) == (0, 12, 24, 28, 32, 36, 40, 44, 48, 80)
    assert C.sizeof(r) == 72
    assert (r.source_voxels.offset, r.result_voxels.offset, r.added.offset, r.removed.offset, r.relabelled.offset, r.bbox_min.offset,
            r.bbox_max.offset, r.launches.offset, r.reserved.offset) == (0, 8, 16, 24, 32, 40, 52, 64, 68)
    # the header's field order is the binding's
    text = open(HEADER).read()
    for struct, fields in (("tbrm_morph_desc", d._fields_), ("tbrm_morph_result", r._fields_)):
        body = re.search(r"typedef struct " + struct + r" \{(.*?)\} " + struct + ";", text, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = re.findall(r"(\w+)(?:\[\d+\])?\s*[,;]", body)
        assert names == [f[0] for f in fields], (struct, names)


def test_the_other_headers_are_unchanged():
    main = os.path.join(ROOT, "include", "tbrm.h")
    declared = declared_symbols(main)
    assert len(declared) == len(abi.SYMBOLS) == 62 and sorted(declared) == sorted(abi.SYMBOLS)
    assert int(re.search(r"#define\s+TBRM_ABI_VERSION\s+(\d+)", open(main).read()).group(1)) == abi.ABI_VERSION == abi.load().tbrm_abi_version() == 5
    segment = os.path.join(ROOT, "include", "tbrm_segment.h")
    assert sorted(declared_symbols(segment)) == sorted(abi.SEGMENT_SYMBOLS) and len(abi.SEGMENT_SYMBOLS) == 5
    assert int(re.search(r"#define\s+TBRM_SEGMENT_ABI_VERSION\s+(\d+)", open(segment).read()).group(1)) == abi.load().tbrm_segment_abi_version() == 1


def test_morph_steps_is_a_tunable():
    old = abi.get_tunable("morph_steps")
    assert 1 <= old <= 8
    try:
        abi.set_tunable("morph_steps", 1)
        assert abi.get_tunable("morph_steps") == 1
    finally:
        abi.set_tunable("morph_steps", old)


def test_null_arguments_are_refused():
    lib = abi.load()
    z = C.c_void_p(None)
    fake = C.c_void_p(8)   # never dereferenced: the pointer checks come first
    desc = abi.MORPH_DESC()
    desc.op, desc.radius, desc.connectivity, desc.new_label = abi.MORPH_CLOSE, 2, 6, -1
    out, out4 = abi.MORPH_RESULT(), (C.c_uint64 * 4)()
    calls = {
        "tbrm_morph_labels": [lambda: lib.tbrm_morph_labels(z, C.byref(desc), C.byref(out)),
                              lambda: lib.tbrm_morph_labels(fake, None, C.byref(out)),
                              lambda: lib.tbrm_morph_labels(fake, C.byref(desc), None)],
        "tbrm_morph_counters": [lambda: lib.tbrm_morph_counters(z, C.byref(out4)), lambda: lib.tbrm_morph_counters(fake, None)],
    }
    for name, variants in calls.items():
        for k, call in enumerate(variants):
            abi.set_tunable("ray_labels", 0)   # (a successful call in between: the next message is this call's own)
            assert call() == abi.ERR_INVALID_ARG, (name, k)
            assert b"null" in lib.tbrm_last_error(), (name, k)
    assert set(abi.MORPH_SYMBOLS) == set(calls) | {"tbrm_morph_abi_version"}


def test_step_plan_under_sanitizers(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "morph_plan_test.cpp")
    exe = str(tmp_path / "morph_plan_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", src, "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip().splitlines()[-1] == "failures=0", p.stdout
