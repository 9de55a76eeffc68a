"""Refusals keep their words and their order. The five board operators (tbrm_morph_labels, tbrm_margin_labels, tbrm_smooth_labels,
tbrm_scissors_labels, tbrm_paint_labels) check their label codes, their box and the handle through one frame (tbrm_board_edit.h); what
a call refuses, with which code and in which words, and which of two bad arguments it names, is held here as literal text, written
down from the sources before the frame existed. Every row changes fields of a call that succeeds as it stands, on a 9^3 volume."""
import ctypes as C

import numpy as np
import pytest

from tbraymarcherplugin_amd import abi

pytestmark = pytest.mark.gpu

DIMS = (9, 9, 9)
INVALID, NOT_INITIALIZED = abi.ERR_INVALID_ARG, abi.ERR_NOT_INITIALIZED
NO_LABELS = "no label volume: tbrm_attach_empty_label_volume or tbrm_upload_label_volume"
NEW_LABEL = "new_label %d: must be 0 .. 255, or -1 to measure only"
ERASE_LABEL = "erase_label %d: must be 0 .. 255"
RESERVED = "reserved = %d: must be 0"
LEAVES = "the box leaves the volume: [0, 0 + 10) along axis 0 of a volume 9 wide"
EMPTY = "box extent: must be > 0 along every axis (or all three 0: the whole volume): [0, 0 + 0) along axis 1 of a volume 9 wide"
BOX_LEAVES = {"origin": (0, 0, 0), "extent": (10, 1, 1)}
BOX_EMPTY = {"origin": (0, 0, 0), "extent": (1, 0, 1)}

# what every one of the five refuses alike: (changed fields, code, the message begins with); paint has no reserved field
CODES = [
    ({"new_label": 256}, INVALID, NEW_LABEL % 256),
    ({"new_label": -2}, INVALID, NEW_LABEL % -2),
    ({"erase_label": -1}, INVALID, ERASE_LABEL % -1),
    ({"erase_label": 256}, INVALID, ERASE_LABEL % 256),
    (BOX_LEAVES, INVALID, LEAVES),
    (BOX_EMPTY, INVALID, EMPTY),
    ({"new_label": 300, "erase_label": 300}, INVALID, NEW_LABEL % 300),
    ({"erase_label": 300, **BOX_LEAVES}, INVALID, ERASE_LABEL % 300),
]
WITH_RESERVED = [
    ({"reserved": 7}, INVALID, RESERVED % 7),
    ({"erase_label": -5, "reserved": 1}, INVALID, ERASE_LABEL % -5),
    ({"reserved": -1, **BOX_EMPTY}, INVALID, RESERVED % -1),
]
TABLE = {
    "morph": CODES + WITH_RESERVED + [
        ({"op": 4}, INVALID, "op 4: must be TBRM_MORPH_DILATE .. TBRM_MORPH_CLOSE"),
        ({"radius": 0}, INVALID, "radius 0: must be 1 .. "),
        ({"connectivity": 18}, INVALID, "connectivity 18: must be 6 or 26"),
        ({"connectivity": 8, "new_label": 999}, INVALID, "connectivity 8: must be 6 or 26"),
        ({"op": -1, "radius": 0}, INVALID, "op -1: must be TBRM_MORPH_DILATE .. TBRM_MORPH_CLOSE"),
    ],
    "margin": CODES + WITH_RESERVED + [
        ({"op": 4}, INVALID, "op 4: must be TBRM_MARGIN_EXPAND .. TBRM_MARGIN_CLOSE"),
        ({"weights": (0, 1, 1)}, INVALID, "weights (0, 1, 1), limit 4: every weight must be >= 1, limit 1 .. 2^31 - 1, every reach isqrt(limit / weight) at most "),
        ({"limit": 0}, INVALID, "weights (1, 1, 1), limit 0: every weight must be >= 1"),
        ({"op": 9, "new_label": 999}, INVALID, "op 9: must be TBRM_MARGIN_EXPAND .. TBRM_MARGIN_CLOSE"),
        ({"reserved": 3, "weights": (1, 0, 1)}, INVALID, RESERVED % 3),
        ({"limit": 0, **BOX_LEAVES}, INVALID, "weights (1, 1, 1), limit 0: every weight must be >= 1"),
    ],
    "smooth": CODES + WITH_RESERVED + [
        ({"radius": (-1, 1, 1)}, INVALID, "radius[0] = -1: must be 0 .. "),
        ({"radius": (0, 0, 0)}, INVALID, "radius (0, 0, 0): one radius must be at least 1"),
        ({"iterations": 0}, INVALID, "iterations 0: must be 1 .. "),
        ({"rank_den": 0}, INVALID, "rank_den 0: must be 1 .. "),
        ({"rank_num": 2}, INVALID, "rank_num 2: must be 0 .. rank_den - 1 = 1"),
        ({"iterations": 0, "new_label": 999}, INVALID, "iterations 0: must be 1 .. "),
        ({"rank_num": -1, "reserved": 2}, INVALID, "rank_num -1: must be 0 .. rank_den - 1 = 1"),
    ],
    "scissors": CODES + WITH_RESERVED + [
        ({"projection.width": 0}, INVALID, "width 0: must be 1 .. "),
        ({"projection.w_min": 0}, INVALID, "w_min 0: must be at least 1"),
        ({"op": 4}, INVALID, "op 4: must be 0 .. 3"),
        ({"n_words": 15}, INVALID, "n_words 15: a mask of width 16 and height 16 has 16 words"),
        ({"stray_row": 5}, INVALID, "mask_words: row 5 has a bit at or beyond width 16"),
        ({"stray_row": 2, "new_label": 999}, INVALID, "mask_words: row 2 has a bit at or beyond width 16"),
        ({"op": 7, "stray_row": 2}, INVALID, "op 7: must be 0 .. 3"),
        ({"new_label": 999, **BOX_LEAVES}, INVALID, NEW_LABEL % 999),
    ],
    "paint": CODES + [
        ({"op": 2}, INVALID, "op 2: must be 0 .. 1"),
        ({"gate": 2}, INVALID, "gate 2: must be 0 or 1"),
        ({"weights": (1, 0, 1)}, INVALID, "weights[1] = 0: must be 1 .. "),
        ({"limit": 0}, INVALID, "limit 0: must be 1 .. "),
        ({"points": [(1 << 19, 0, 0)]}, INVALID, "point 0: coordinate 0 = 524288, must be within +-"),
        ({"gate": 1, "lo": 5.0, "hi": 3.0}, INVALID, "range [5, 3]: needs lo <= hi"),
        ({"gate": 1, "lo": 1.5, "hi": 3.0}, INVALID, "range [1.5, 3]: needs integral codes with 0 <= lo <= hi <= 255"),
        ({"gate": 1, "lo": 0.0, "hi": 256.0}, INVALID, "range [0, 256]: needs integral codes with 0 <= lo <= hi <= 255"),
        ({"gate": 0, "lo": 5.0, "hi": 3.0}, abi.OK, ""),                                                  # without a gate the range is not read
        ({"weights": (0, 1, 1), "new_label": 999}, INVALID, "weights[0] = 0: must be 1 .. "),              # the stroke before the label codes
        ({"new_label": 999, "gate": 1, "lo": 5.0, "hi": 3.0}, INVALID, NEW_LABEL % 999),                  # ... and the gate range after them
        ({"gate": 1, "lo": 5.0, "hi": 3.0, **BOX_LEAVES}, INVALID, "range [5, 3]: needs lo <= hi"),        # ... and before the box
    ],
}


def a_call(res, name):
    """(desc, call): a desc of `name` that the handle accepts, and call(desc, extra) -> the entry point's return code"""
    lib, h = res.lib, res.handle
    if name == "morph":
        d, out = res.morph_desc("dilate", 1, [1], -1), abi.MORPH_RESULT()
        return d, lambda d, extra: lib.tbrm_morph_labels(h, C.byref(d), C.byref(out))
    if name == "margin":
        d, out = res.margin_desc("expand", (1, 1, 1), 4, [1], -1), abi.MARGIN_RESULT()
        return d, lambda d, extra: lib.tbrm_margin_labels(h, C.byref(d), C.byref(out))
    if name == "smooth":
        d, out = res.smooth_desc((1, 1, 1), [1], -1), abi.SMOOTH_RESULT()
        return d, lambda d, extra: lib.tbrm_smooth_labels(h, C.byref(d), C.byref(out))
    if name == "scissors":
        proj = abi.make_scissors_projection((1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 0, 1), 1, 1, 16, 16)   # pixel (x, y) of every voxel
        d, out = res.scissors_desc(proj, "erase_inside", [1], -1), abi.SCISSORS_RESULT()

        def call(d, extra):
            mask = np.full((16, 1), 0x0000FFFF, dtype=np.uint32)
            if "stray_row" in extra:
                mask[extra["stray_row"], 0] |= 1 << 16
            return lib.tbrm_scissors_labels(h, C.byref(d), mask.ctypes.data_as(C.c_void_p), extra.get("n_words", mask.size), C.byref(out))
        return d, call
    d, out = res.paint_desc((1, 1, 1), 24 * 24, "paint", [1], -1), abi.PAINT_RESULT()

    def call(d, extra):
        pts = np.ascontiguousarray(np.asarray(extra.get("points", [(36, 36, 36)]), dtype=np.int32).reshape(-1, 3))
        return lib.tbrm_paint_labels(h, C.byref(d), pts.ctypes.data_as(C.c_void_p), pts.shape[0], C.byref(out))
    return d, call


def refusal(res, name, changes):
    """(code, message) of the call of `name` with `changes`: fields of the desc (a.b: of a struct inside it), or what a_call takes"""
    d, call = a_call(res, name)
    extra = {}
    for path, value in changes.items():
        if path in ("n_words", "stray_row", "points"):
            extra[path] = value
            continue
        at, *rest = path.split(".")
        obj = d
        while rest:
            obj, at, rest = getattr(obj, at), rest[0], rest[1:]
        if isinstance(value, tuple):
            getattr(obj, at)[:] = list(value)
        else:
            setattr(obj, at, value)
    code = call(d, extra)
    return code, (abi.load().tbrm_last_error().decode() if code != abi.OK else "")


@pytest.fixture(scope="module")
def handles(gpu):
    labels = np.zeros(DIMS[::-1], dtype=np.uint8)
    labels[3:6, 3:6, 3:6] = 1
    vol = np.arange(9 ** 3, dtype=np.uint32).astype(np.uint8).reshape(DIMS[::-1])
    with abi.Resources(DIMS, abi.FMT_G8, False, False, 0) as with_labels, abi.Resources(DIMS, abi.FMT_G8, False, False, 0) as without:
        with_labels.upload_volume(vol)
        with_labels.upload_label_volume(labels)
        without.upload_volume(vol)
        yield with_labels, without, labels


@pytest.mark.parametrize("name", sorted(TABLE))
def test_refusals_keep_their_words_and_their_order(handles, name):
    res, without, labels = handles
    assert refusal(res, name, {}) == (abi.OK, ""), "the call every row starts from"
    for changes, code, begins in TABLE[name]:
        got = refusal(res, name, changes)
        assert got[0] == code and got[1].startswith(begins) and (begins or not got[1]), (name, changes, got, begins)
    # a handle without a label volume: after the arguments and the box, whatever the call would write
    assert refusal(without, name, {}) == (NOT_INITIALIZED, NO_LABELS)
    assert refusal(without, name, {"new_label": 1}) == (NOT_INITIALIZED, NO_LABELS)
    got = refusal(without, name, dict(BOX_LEAVES))
    assert got[0] == INVALID and got[1].startswith(LEAVES), got
    assert np.array_equal(res.download_label_volume(), labels)   # nothing here wrote: every call measured or was refused
