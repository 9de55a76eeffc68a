"""Data-volume region updates (include/tbrm_volume_region.h) without a GPU: the header's symbols exported and bound, the argument
checks that need no handle (a handle needs a device: the box-against-volume and byte-count checks are in
tests/test_gpu_volume_region.py), tbrm.h left as it was, and the reach rule of the incremental min/max pass against a texel-by-texel
restatement of k_brick_minmax's loop."""
import ctypes as C
import os
import re

import pytest

from tbraymarcherplugin_amd import abi
import volume_region_reference as VR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tbrm_volume_region.h")


def declared_symbols(path=HEADER):
    return re.findall(r"TBRM_API\s+[\w\s\*]+?\b(tbrm_\w+)\s*\(", open(path).read())


def test_header_symbols_are_exported_and_bound():
    lib = abi.load()
    declared = declared_symbols()
    assert sorted(declared) == sorted(abi.VOLUME_REGION_SYMBOLS), set(declared) ^ set(abi.VOLUME_REGION_SYMBOLS)
    assert not set(declared) & (set(abi.SYMBOLS) | set(abi.LABEL_SYMBOLS) | set(abi.COLOR_LIGHT_SYMBOLS))
    for name in declared:
        assert hasattr(lib, name), f"{name} is declared in tbrm_volume_region.h but not exported by libtbrm.so"
    version = int(re.search(r"#define\s+TBRM_VOLUME_REGION_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1))
    assert lib.tbrm_volume_region_abi_version() == version == abi.VOLUME_REGION_ABI_VERSION == 1


def test_tbrm_h_is_unchanged():
    main = os.path.join(ROOT, "include", "tbrm.h")
    declared = declared_symbols(main)
    assert len(declared) == len(abi.SYMBOLS) == 62 and sorted(declared) == sorted(abi.SYMBOLS)
    assert int(re.search(r"#define\s+TBRM_ABI_VERSION\s+(\d+)", open(main).read()).group(1)) == abi.ABI_VERSION == abi.load().tbrm_abi_version() == 5


def region_calls(lib):
    return {"tbrm_update_volume_region": lib.tbrm_update_volume_region, "tbrm_update_volume_region_device": lib.tbrm_update_volume_region_device,
            "tbrm_download_volume_region": lib.tbrm_download_volume_region}


def test_null_arguments_are_refused():
    lib = abi.load()
    z = C.c_void_p(None)
    fake = C.c_void_p(8)   # never dereferenced: the pointer checks come first
    buf = (C.c_uint8 * 16)()
    o3, e3 = (C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(1, 1, 1)
    out4 = (C.c_uint64 * 4)()
    for name, call in region_calls(lib).items():
        for args in ((z, C.byref(o3), C.byref(e3), buf, 1), (fake, None, C.byref(e3), buf, 1), (fake, C.byref(o3), None, buf, 1),
                     (fake, C.byref(o3), C.byref(e3), None, 1)):
            abi.set_tunable("ray_labels", 0)   # (a successful call in between: the next message is this call's own)
            assert call(*args) == abi.ERR_INVALID_ARG, name
            assert b"null" in lib.tbrm_last_error(), name
    assert lib.tbrm_volume_region_counters(z, C.byref(out4)) == abi.ERR_INVALID_ARG and b"null" in lib.tbrm_last_error()
    assert lib.tbrm_volume_region_counters(fake, None) == abi.ERR_INVALID_ARG
    assert lib.tbrm_volume_skipping_digest(z, C.byref(out4)) == abi.ERR_INVALID_ARG and b"null" in lib.tbrm_last_error()
    assert lib.tbrm_volume_skipping_digest(fake, None) == abi.ERR_INVALID_ARG
    handle_taking = set(region_calls(lib)) | {"tbrm_volume_region_counters", "tbrm_volume_skipping_digest"}
    assert set(abi.VOLUME_REGION_SYMBOLS) == handle_taking | {"tbrm_volume_region_abi_version"}


@pytest.mark.parametrize("origin,extent,word", [((0, 0, 0), (0, 1, 1), b"extent"), ((0, 0, 0), (1, -3, 1), b"extent"), ((0, 0, 0), (1, 1, 0), b"extent"),
                                                ((-1, 0, 0), (2, 1, 1), b"leaves the volume"), ((0, 0, -8), (1, 1, 9), b"leaves the volume")])
def test_boxes_no_volume_can_hold_are_refused_before_the_handle_is_looked_at(origin, extent, word):
    lib = abi.load()
    buf = (C.c_uint8 * 16)()
    o3, e3 = (C.c_int32 * 3)(*origin), (C.c_int32 * 3)(*extent)
    for name, call in region_calls(lib).items():
        assert call(C.c_void_p(None), C.byref(o3), C.byref(e3), buf, 1) == abi.ERR_INVALID_ARG, name
        assert word in lib.tbrm_last_error(), (name, lib.tbrm_last_error())


DIMS = (24, 17, 10)   # bricks 3 x 3 x 2: x whole, y one texel into its last brick, z two
BOXES = [
    ((5, 3, 2), (1, 1, 1)),       # one voxel inside a brick
    ((8, 8, 8), (1, 1, 1)),       # a brick's first texel: the brick before reads it as its +8 tap
    ((7, 7, 7), (1, 1, 1)),       # a brick's last texel: nobody else's
    ((0, 0, 0), (1, 1, 1)),       # texel 0 of every axis: the last bricks under wrap
    ((0, 5, 3), (4, 2, 2)),       # texel 0 of x only
    ((3, 0, 1), (10, 4, 8)),      # texel 0 of y, across brick faces
    ((23, 16, 9), (1, 1, 1)),     # the last texel of every axis: what clamp sends the top tap to
    ((17, 16, 8), (3, 1, 2)),     # inside the ragged last bricks of y and z
    ((3, 5, 2), (10, 4, 8)),      # crosses brick faces
    ((16, 9, 0), (8, 7, 10)),     # up to a brick boundary
    ((0, 0, 0), (24, 17, 10)),    # the whole volume
]


@pytest.mark.parametrize("mode", [VR.WRAP, VR.CLAMP], ids=["wrap", "clamp"])
def test_reach_rule_matches_the_kernels_loop(mode):
    some_differ = False
    for origin, extent in BOXES:
        brute = VR.reached_bricks(DIMS, mode, origin, extent)
        assert VR.rule_bricks(DIMS, mode, origin, extent) == brute, (origin, extent, mode)
        touched = {(x // 8, y // 8, z // 8) for x in range(origin[0], origin[0] + extent[0]) for y in range(origin[1], origin[1] + extent[1])
                   for z in range(origin[2], origin[2] + extent[2])}
        assert touched <= brute
        some_differ = some_differ or touched != brute
    assert some_differ   # the apron matters: the reach is more than the bricks a box lies in
    # wrap and clamp differ exactly where a box holds texel 0
    assert (VR.reached_bricks(DIMS, VR.WRAP, (0, 5, 3), (4, 2, 2)) - VR.reached_bricks(DIMS, VR.CLAMP, (0, 5, 3), (4, 2, 2))) == {(2, 0, 0)}
    assert VR.reached_bricks(DIMS, VR.WRAP, (23, 16, 9), (1, 1, 1)) == VR.reached_bricks(DIMS, VR.CLAMP, (23, 16, 9), (1, 1, 1)) == {(2, 1, 1), (2, 2, 1)}
