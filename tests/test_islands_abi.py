"""The islands of a label (include/tbrm_islands.h) without a GPU: the header's symbols exported and bound, the struct layouts, the other
headers left as they were, null and invalid arguments refused before anything is dereferenced, and the rule with the argument
validation (tbrm_islands_rule.h: pure host code) in a stand-alone program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import subprocess

from tbraymarcherplugin_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tbrm_islands.h")


def declared_symbols(path=HEADER):
    return re.findall(r"TBRM_API\s+[\w\s\*]+?\b(tbrm_\w+)\s*\(", open(path).read())


def test_header_symbols_are_exported_and_bound():
    lib = abi.load()
    declared = declared_symbols()
    assert sorted(declared) == sorted(abi.ISLANDS_SYMBOLS), set(declared) ^ set(abi.ISLANDS_SYMBOLS)
    others = (set(abi.SYMBOLS) | set(abi.LABEL_SYMBOLS) | set(abi.COLOR_LIGHT_SYMBOLS) | set(abi.VOLUME_REGION_SYMBOLS) | set(abi.VOLUME_STATS_SYMBOLS)
              | set(abi.VIEW_CACHE_SYMBOLS) | set(abi.HIT_SYMBOLS) | set(abi.SEGMENT_SYMBOLS) | set(abi.MORPH_SYMBOLS))
    assert not set(declared) & others
    for name in declared:
        assert hasattr(lib, name), f"{name} is declared in tbrm_islands.h but not exported by libtbrm.so"
    text = open(HEADER).read()
    version = int(re.search(r"#define\s+TBRM_ISLANDS_ABI_VERSION\s+(\d+)", text).group(1))
    assert lib.tbrm_islands_abi_version() == version == abi.ISLANDS_ABI_VERSION == 1
    assert int(re.search(r"#define\s+TBRM_ISLANDS_MEASURE\s+(\d+)u", text).group(1)) == abi.ISLANDS_MEASURE == 1
    assert int(re.search(r"#define\s+TBRM_ISLAND_KEPT\s+(\d+)u", text).group(1)) == abi.ISLAND_KEPT == 1
    assert int(re.search(r"#define\s+TBRM_ISLAND_BORDER\s+(\d+)u", text).group(1)) == abi.ISLAND_BORDER == 2
    assert abi.ISLANDS_ANY_SIZE == 2 ** 64 - 1


def test_struct_layouts():
    d, r, i = abi.ISLANDS_DESC, abi.ISLANDS_RESULT, abi.ISLAND
    assert C.sizeof(d) == 96
    assert (d.origin.offset, d.extent.offset, d.connectivity.offset, d.max_islands.offset, d.min_voxels.offset, d.keep_label.offset, d.label_step.offset,
            d.drop_label.offset, d.spare_border.offset, d.flags.offset, d.reserved.offset, d.source.offset) == (0, 12, 24, 28, 32, 40, 44, 48, 52, 56, 60, 64)
    assert C.sizeof(r) == 104
    assert (r.set_voxels.offset, r.islands.offset, r.spared.offset, r.kept.offset, r.dropped.offset, r.kept_voxels.offset, r.dropped_voxels.offset,
            r.largest.offset, r.relabelled.offset, r.bbox_min.offset, r.bbox_max.offset, r.table_entries.offset, r.reserved.offset) == (
                0, 8, 16, 24, 32, 40, 48, 56, 64, 72, 84, 96, 100)
    assert C.sizeof(i) == 32
    assert (i.voxels.offset, i.first.offset, i.label.offset, i.flags.offset, i.reserved.offset) == (0, 8, 20, 24, 28)
    # the header's field order is the binding's
    text = open(HEADER).read()
    for struct, fields in (("tbrm_islands_desc", d._fields_), ("tbrm_islands_result", r._fields_), ("tbrm_island", i._fields_)):
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
    assert abi.load().tbrm_segment_abi_version() == 1
    morph = os.path.join(ROOT, "include", "tbrm_morphology.h")
    assert sorted(declared_symbols(morph)) == sorted(abi.MORPH_SYMBOLS) and len(abi.MORPH_SYMBOLS) == 3
    assert abi.load().tbrm_morph_abi_version() == 1


def test_null_and_invalid_arguments_are_refused():
    lib = abi.load()
    z = C.c_void_p(None)
    fake = C.c_void_p(8)   # never dereferenced: the pointer checks come first
    desc = abi.ISLANDS_DESC()
    desc.connectivity, desc.keep_label, desc.drop_label = 6, -1, 0
    out, out6, one = abi.ISLANDS_RESULT(), (C.c_uint64 * 6)(), (abi.ISLAND * 1)()
    calls = {
        "tbrm_label_islands": [lambda: lib.tbrm_label_islands(z, C.byref(desc), None, 0, C.byref(out)),
                               lambda: lib.tbrm_label_islands(fake, None, None, 0, C.byref(out)),
                               lambda: lib.tbrm_label_islands(fake, C.byref(desc), None, 0, None),
                               lambda: lib.tbrm_label_islands(fake, C.byref(desc), None, 1, C.byref(out))],
        "tbrm_islands_counters": [lambda: lib.tbrm_islands_counters(z, C.byref(out6)), lambda: lib.tbrm_islands_counters(fake, None)],
    }
    for name, variants in calls.items():
        for k, call in enumerate(variants):
            abi.set_tunable("ray_labels", 0)   # (a successful call in between: the next message is this call's own)
            assert call() == abi.ERR_INVALID_ARG, (name, k)
            assert b"null" in lib.tbrm_last_error(), (name, k)
    abi.set_tunable("ray_labels", 0)
    assert lib.tbrm_label_islands(fake, C.byref(desc), one, -1, C.byref(out)) == abi.ERR_INVALID_ARG and b"capacity" in lib.tbrm_last_error()
    assert set(abi.ISLANDS_SYMBOLS) == set(calls) | {"tbrm_islands_abi_version"}


def test_rule_and_validation_under_sanitizers(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "islands_rule_test.cpp")
    exe = str(tmp_path / "islands_rule_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", src, "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip().splitlines()[-1] == "failures=0", p.stdout
