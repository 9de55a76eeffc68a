"""The label surface (include/tbrm_surface.h) on the GPU against tests/label_surface_reference.py. The results are integers, bytes and
float32 bit patterns: every comparison is exact equality — of every field of the result, the vertex records, the indices and the
positions. Every case runs under surface_skip 1 and 0. The reference is judged without a GPU in tests/test_label_surface_reference.py."""
import numpy as np
import pytest
import torch

from tbraymarcherplugin_amd import abi, synthetic as S
import label_surface_reference as SR

pytestmark = pytest.mark.gpu

RAGGED = (40, 27, 19)
_REFERENCES = {}


def make_res(dims, labels=None):
    res = abi.Resources(dims, abi.FMT_G8, False, False, 0)
    res.upload_volume(np.zeros(dims[::-1], dtype=np.uint8))   # the surface never reads the data
    if labels is not None:
        res.upload_label_volume(labels)
    return res


def reference(key, labels, source, origin=None, extent=None):
    """the reference's quads and records, computed once per case (key names the labels)"""
    k = (key, tuple(source), origin, extent)
    if k not in _REFERENCES:
        _REFERENCES[k] = SR.surface(labels, source, origin, extent)
    return _REFERENCES[k]


def blocks_of(dims, origin, extent):
    o, e = SR.resolve_box(dims, origin, extent)
    return int(np.prod([(e[c] >> 3) - (o[c] >> 3) + 1 for c in range(3)]))


def check(got, want, dims, origin, extent, triangles, scale, offset, where):
    for k in SR.FIELDS:
        assert got[k] == want[k], (k, got[k], want[k], where)
    assert got["blocks_evaluated"] + got["blocks_skipped"] == blocks_of(dims, origin, extent), (got, where)
    assert got["written"] == (1 if want["vertices"] else 0) and got["launches"] == (5 if want["vertices"] else 4), (got, where)
    assert got["vertex"].dtype == SR.VERTEX_DTYPE and got["vertex"].tobytes() == want["vertex"].tobytes(), (where, np.argwhere(got["vertex"] != want["vertex"])[:5])
    q = want["indices"]
    indices = q[:, [0, 1, 2, 0, 2, 3]] if triangles else q
    assert got["indices"].dtype == np.uint32 and got["indices"].shape == indices.shape and np.array_equal(got["indices"], indices), where
    pos = SR.positions_of(want["vertex"], scale or (1.0, 1.0, 1.0), offset or (0.0, 0.0, 0.0))
    assert got["positions"].dtype == np.float32 and got["positions"].tobytes() == pos.tobytes(), (where, np.argwhere(got["positions"] != pos)[:5])


def either_way(tunables, res, key, labels, source, origin=None, extent=None, triangles=False, scale=None, offset=None):
    """the extraction under surface_skip 1 and 0 against the reference; under 0 every block of the range is evaluated. Returns the
    result under 1"""
    want = reference(key, labels, source, origin, extent)
    dims = labels.shape[::-1]
    out = []
    try:
        for skip in (1, 0):
            tunables("surface_skip", skip)
            got = res.label_surface(source, origin, extent, triangles=triangles, scale=scale, offset=offset)
            check(got, want, dims, origin, extent, triangles, scale, offset, (key, source, origin, extent, triangles, skip))
            m = res.measure_label_surface(source, origin, extent)
            assert m["written"] == 0 and m["launches"] == 4 and all(m[k] == want[k] for k in SR.FIELDS)
            out.append(got)
    finally:
        tunables("surface_skip", 1)
    assert out[1]["blocks_skipped"] == 0
    return out[0]


# ---- one brick ----------------------------------------------------------------------------------------------------------------------------
def one_voxel(at):
    labels = np.zeros((8, 8, 8), dtype=np.uint8)
    labels[at[2], at[1], at[0]] = 3
    return labels


@pytest.mark.parametrize("name,labels", [("corner", one_voxel((0, 0, 0))), ("far_corner", one_voxel((7, 7, 7))), ("middle", one_voxel((3, 4, 5))),
                                         ("full", np.full((8, 8, 8), 3, dtype=np.uint8))])
def test_one_brick(gpu, tunables, name, labels):
    with make_res((8, 8, 8), labels) as res:
        got = either_way(tunables, res, "brick_" + name, labels, [3])
        if name == "full":
            assert (got["vertices"], got["quads"], got["set_voxels"]) == (9 ** 3 - 7 ** 3, 6 * 64, 512)
        else:
            assert (got["vertices"], got["quads"], got["set_voxels"]) == (8, 6, 1) and (got["vertex"]["edges"] == 3).all()
        either_way(tunables, res, "brick_" + name, labels, [3], triangles=True)


def test_the_empty_set(gpu, tunables):
    labels = np.zeros((8, 8, 8), dtype=np.uint8)
    labels[2, 2, 2] = 9   # another label
    with make_res((8, 8, 8), labels) as res:
        got = either_way(tunables, res, "empty", labels, [3])
        assert got["vertices"] == got["quads"] == got["written"] == 0 and got["cell_min"] == (8, 8, 8) and got["cell_max"] == (-1, -1, -1)
        assert got["vertex"].shape == (0,) and got["indices"].shape == (0, 4)
        # nothing is written: buffers offered to a call with nothing to say stay as they are
        d = res.surface_desc([3], vertex_capacity=4, quad_capacity=4)
        v, i, p = (np.full(n, 0xAB, dtype=np.uint8) for n in (80, 64, 48))
        out = abi.SURFACE_RESULT()
        abi.check(res.lib.tbrm_label_surface(res.handle, d, v.ctypes.data, i.ctypes.data, p.ctypes.data, out))
        assert out.written == 0 and all((a == 0xAB).all() for a in (v, i, p))
        assert res.surface_counters()["vertices_written"] == 0


# ---- the densest case ---------------------------------------------------------------------------------------------------------------------
def test_checkerboard(gpu, tunables):
    dims = (16, 16, 16)
    labels = SR.checkerboard_labels(dims)
    with make_res(dims, labels) as res:
        got = either_way(tunables, res, "checkerboard", labels, [3])
        # every cell is active but the four at corners of the volume whose one voxel is not in S; every lattice edge between two
        # voxels is a quad, and so is every edge that leaves the volume from a voxel of S (half of 16 x 16 per face)
        assert got["vertices"] == 17 ** 3 - 4 and got["quads"] == 3 * (15 * 256 + 2 * 128)
        assert got["blocks_skipped"] == 0
        either_way(tunables, res, "checkerboard", labels, [3], triangles=True, scale=(0.5, 2.0, 1.25), offset=(1.0, -2.0, 0.125))


# ---- the ragged volume --------------------------------------------------------------------------------------------------------------------
BOXES = {
    "whole": (None, None),
    "odd_origin_ends_inside_a_brick": ((3, 5, 1), (30, 17, 13)),
    "one_voxel_thick": ((14, 9, 11), (1, 15, 7)),
    "ends_on_the_ragged_face": ((9, 10, 3), (31, 17, 16)),
}


def ragged_labels(kind):
    if kind == "random":
        return SR.random_labels(RAGGED, 0.5, 77, labels=(3, 9, 200))
    return SR.ball_labels(RAGGED, (21, 12, 9), 9.3)


@pytest.mark.parametrize("box", list(BOXES))
@pytest.mark.parametrize("kind", ["random", "ball"])
def test_ragged(gpu, tunables, kind, box):
    labels = ragged_labels(kind)
    origin, extent = BOXES[box]
    with make_res(RAGGED, labels) as res:
        got = either_way(tunables, res, "ragged_" + kind, labels, [3], origin, extent)
        assert got["vertices"] > 0
        if kind == "ball" and box == "whole":
            assert got["blocks_skipped"] > 0   # the corners of the volume hold nothing


def test_several_labels_triangles_and_a_transform(gpu, tunables):
    labels = ragged_labels("random")
    with make_res(RAGGED, labels) as res:
        two = either_way(tunables, res, "ragged_random", labels, [3, 200])
        one = either_way(tunables, res, "ragged_random", labels, [3])
        assert two["set_voxels"] > one["set_voxels"]
        either_way(tunables, res, "ragged_random", labels, [3, 200], triangles=True)
        either_way(tunables, res, "ragged_random", labels, [3, 200], (3, 5, 1), (30, 17, 13), triangles=True, scale=(0.7, 0.7, 2.5), offset=(-10.0, 3.25, 100.0))
        scale, offset = abi.surface_unit_cube(RAGGED)
        got = either_way(tunables, res, "ragged_random", labels, [3], scale=scale, offset=offset)
        assert got["positions"].min() >= -1.0 / 18 and got["positions"].max() <= 1.0 + 1.0 / 18
        assert got["positions"].tobytes() == abi.surface_positions(got["vertex"], scale, offset).tobytes()   # the host helper on the downloaded records


def blocks_without_a_vertex(want, dims):
    held = {tuple(b) for b in ((want["vertex"]["cell"].astype(np.int64) + 1) >> 3).tolist()}
    return blocks_of(dims, None, None) - len(held)


@pytest.mark.parametrize("dims", [(17, 9, 24), (17, 17, 24), (24, 24, 24)])
def test_the_whole_volume_is_a_box(gpu, tunables, dims):
    """S the whole volume: the surface is the box only, and every interior block — every block of the range that holds no active
    cell — is skipped; under surface_skip 0 none is (either_way). In (17, 9, 24) every block of the range touches a face of the box
    (9 voxels along y are two blocks of cells, one with the face y = 0 and one with the face y = 9): there is no interior block
    and blocks_skipped is 0 by the definition, so blocks_skipped > 0 is asserted on the two shapes that have interior blocks."""
    nx, ny, nz = dims
    labels = np.full(dims[::-1], 3, dtype=np.uint8)
    with make_res(dims, labels) as res:
        got = either_way(tunables, res, "solid%d_%d_%d" % dims, labels, [3])
        assert got["set_voxels"] == nx * ny * nz and got["quads"] == 2 * (nx * ny + ny * nz + nx * nz) and got["vertices"] == got["quads"] + 2
        interior = blocks_without_a_vertex(reference("solid%d_%d_%d" % dims, labels, [3]), dims)
        assert got["blocks_skipped"] == interior == {(17, 9, 24): 0, (17, 17, 24): 2, (24, 24, 24): 8}[dims]


# ---- capacities ---------------------------------------------------------------------------------------------------------------------------
def test_short_capacities(gpu):
    labels = ragged_labels("ball")
    want = reference("ragged_ball", labels, [3])
    nv, nq = want["vertices"], want["quads"]
    with make_res(RAGGED, labels) as res:
        before = res.surface_counters()
        for vcap, qcap, names in ((nv - 1, nq, b"vertex_capacity"), (nv, nq - 1, b"quad_capacity"), (0, 0, b"vertex_capacity")):
            v, i, p = np.full(nv * 20, 0xAB, dtype=np.uint8), np.full(nq * 16, 0xAB, dtype=np.uint8), np.full(nv * 12, 0xAB, dtype=np.uint8)
            d = res.surface_desc([3], vertex_capacity=vcap, quad_capacity=qcap)
            out = abi.SURFACE_RESULT()
            assert res.lib.tbrm_label_surface(res.handle, d, v.ctypes.data, i.ctypes.data, p.ctypes.data, out) == abi.ERR_INVALID_ARG
            assert names in res.lib.tbrm_last_error(), res.lib.tbrm_last_error()
            assert (out.vertices, out.quads, out.written) == (nv, nq, 0) and out.set_voxels == want["set_voxels"]   # both counts are still reported
            assert all((a == 0xAB).all() for a in (v, i, p))
            # the device form, onto torch tensors
            tv = torch.full((max(vcap, 1), 20), 0xAB, dtype=torch.uint8, device="cuda")
            ti = torch.full((max(qcap, 1), 4), -7, dtype=torch.int32, device="cuda")
            d = res.surface_desc([3], vertex_capacity=vcap, quad_capacity=qcap)
            assert res.lib.tbrm_label_surface_device(res.handle, d, tv.data_ptr(), ti.data_ptr(), None, out) == abi.ERR_INVALID_ARG
            assert (out.vertices, out.quads, out.written) == (nv, nq, 0)
            torch.cuda.synchronize()
            assert bool((tv == 0xAB).all()) and bool((ti == -7).all())
        after = res.surface_counters()
        assert after["surface_calls"] == before["surface_calls"] + 6 and after["vertices_written"] == before["vertices_written"] == 0
        # null outputs hold nothing; exactly enough is enough
        d = res.surface_desc([3], vertex_capacity=nv, quad_capacity=nq)
        out = abi.SURFACE_RESULT()
        assert res.lib.tbrm_label_surface(res.handle, d, None, None, None, out) == abi.ERR_INVALID_ARG and out.vertices == nv
        got = res.label_surface([3])
        assert got["written"] == 1 and got["vertex"].tobytes() == want["vertex"].tobytes()


def test_refusals(gpu):
    labels = ragged_labels("ball")
    with make_res(RAGGED, labels) as res:
        out = abi.SURFACE_RESULT()
        for change, names in ((dict(flags=4), b"flags"), (dict(reserved=1), b"reserved"), (dict(scale=(1.0, np.inf, 1.0)), b"finite"), (dict(offset=(np.nan, 0.0, 0.0)), b"finite"),
                              (dict(origin=(0, 0, 0), extent=(41, 27, 19)), b"leaves"), (dict(origin=(0, -1, 0), extent=(4, 4, 4)), b"leaves"), (dict(origin=(0, 0, 0), extent=(4, 0, 4)), b"extent")):
            d = res.surface_desc([3], origin=change.get("origin"), extent=change.get("extent"), scale=change.get("scale"), offset=change.get("offset"), measure=True)
            d.flags |= change.get("flags", 0)
            d.reserved = change.get("reserved", 0)
            assert res.lib.tbrm_label_surface(res.handle, d, None, None, None, out) == abi.ERR_INVALID_ARG, change
            assert names in res.lib.tbrm_last_error(), (change, res.lib.tbrm_last_error())
        assert res.surface_counters()["surface_calls"] == 0
    with make_res(RAGGED) as bare:   # no label volume
        with pytest.raises(abi.TbrmError, match="label volume"):
            bare.measure_label_surface([3])
        assert bare.surface_counters()["surface_calls"] == 0


# ---- the device form ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("triangles", [False, True])
def test_device_form_equals_the_host_form(gpu, triangles):
    labels = ragged_labels("random")
    scale, offset = (0.7, 0.7, 2.5), (-10.0, 3.25, 100.0)
    with make_res(RAGGED, labels) as res:
        host = res.label_surface([3, 9], (3, 5, 1), (30, 17, 13), triangles=triangles, scale=scale, offset=offset)
        nv, nq = host["vertices"], host["quads"]
        tv = torch.full((nv + 3, 5), -7, dtype=torch.int32, device="cuda")
        ti = torch.full((nq + 2, 6 if triangles else 4), -7, dtype=torch.int32, device="cuda")
        tp = torch.full((nv + 3, 3), -7.0, dtype=torch.float32, device="cuda")
        got = res.label_surface_device([3, 9], tv, ti, tp, (3, 5, 1), (30, 17, 13), triangles=triangles, scale=scale, offset=offset)
        torch.cuda.synchronize()
        assert all(got[k] == host[k] for k in list(SR.FIELDS) + ["written", "launches"])
        assert tv[:nv].cpu().numpy().tobytes() == host["vertex"].tobytes() and bool((tv[nv:] == -7).all())
        assert np.array_equal(ti[:nq].cpu().numpy().view(np.uint32), host["indices"]) and bool((ti[nq:] == -7).all())
        assert tp[:nv].cpu().numpy().tobytes() == host["positions"].tobytes() and bool((tp[nv:] == -7.0).all())
        # without positions
        tv.fill_(-7)
        got = res.label_surface_device([3, 9], tv, ti, None, (3, 5, 1), (30, 17, 13), triangles=triangles)
        torch.cuda.synchronize()
        assert tv[:nv].cpu().numpy().tobytes() == host["vertex"].tobytes()


# ---- state --------------------------------------------------------------------------------------------------------------------------------
CAM = S.default_camera(64, 48)
TILE = abi.Tile(0, 0, 64, 48)
OTHER_COUNTERS = ("volume_region_counters", "volume_stats_counters", "hit_counters", "segment_counters", "morph_counters", "margin_counters", "smooth_counters",
                  "scissors_counters", "compete_counters", "paint_counters", "islands_counters", "launch_counters")


def test_state(gpu):
    dims = (48, 40, 44)
    vol = S.make_volume_numpy(dims, np.uint16, 0x5EED0002)
    labels = np.where(vol >= np.percentile(vol, 50), 1, 0).astype(np.uint8)   # label 1: red, half transparent
    rp = abi.RaymarchParams(100.0, 1, True)
    world = S.default_world()
    res = abi.Resources(dims, abi.FMT_G16)
    with res:
        res.upload_volume(vol)
        res.set_tf_lut(abi.color_curve_to_lut(S.tf_keys("A")))
        res.set_windowing(abi.WindowingParams(0.5, 0.9, True, False))
        res.upload_label_volume(labels)
        for i in (0, 1):
            res.add_dir_light(S.light(i), True, S.default_world())
        frame = res.raymarch_lit(CAM, TILE, rp, world)
        light = res.download_light_volume()
        stats = res.label_statistics()
        others = {name: getattr(res, name)() for name in OTHER_COUNTERS}
        path = res.path_counters()
        assert res.surface_counters() == dict.fromkeys(abi.Resources.SURFACE_COUNTERS, 0)

        got = res.label_surface([1], triangles=True)
        want = reference("state", labels, [1])
        check(got, want, dims, None, None, True, None, None, "state")
        c1 = res.surface_counters()
        assert c1["surface_calls"] == 2 and c1["vertices_written"] == want["vertices"] and c1["quads_written"] == want["quads"]   # (the binding measures, then extracts)
        assert c1["scratch_bytes"] > 0 and 1 <= c1["scratch_allocations"] <= 2

        assert np.array_equal(res.download_label_volume(), labels)
        assert {name: getattr(res, name)() for name in OTHER_COUNTERS} == others
        grew = res.path_counters()
        assert {k: v for k, v in grew.items() if k != "operator_alloc_calls"} == {k: v for k, v in path.items() if k != "operator_alloc_calls"}
        assert np.array_equal(res.raymarch_lit(CAM, TILE, rp, world), frame)
        assert np.array_equal(res.download_light_volume(), light) and np.array_equal(res.label_statistics(), stats)

        # a second, smaller call takes no scratch, and neither does the same call again
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        allocs = res.path_counters()["operator_alloc_calls"]
        small = res.label_surface([1], (5, 6, 7), (20, 21, 22))
        check(small, reference("state", labels, [1], (5, 6, 7), (20, 21, 22)), dims, (5, 6, 7), (20, 21, 22), False, None, None, "state, a box")
        again = res.label_surface([1], triangles=True)
        assert again["vertex"].tobytes() == got["vertex"].tobytes() and np.array_equal(again["indices"], got["indices"])
        c2 = res.surface_counters()
        assert c2["scratch_allocations"] == c1["scratch_allocations"] and c2["scratch_bytes"] == c1["scratch_bytes"] and c2["surface_calls"] == 6
        assert res.path_counters()["operator_alloc_calls"] == allocs
        torch.cuda.synchronize()
        assert torch.cuda.mem_get_info()[0] == free0
        # the label tools find their scratch usable after the surface worked in it
        m = res.morph_labels("dilate", 1, [1], -1)
        assert m["source_voxels"] == want["set_voxels"]


def test_after_an_edit(gpu, tunables):
    labels = ragged_labels("random")
    with make_res(RAGGED, labels) as res:
        first = res.measure_label_surface([5])
        assert first["vertices"] == 0
        weights, limit = abi.paint_brush((1.0, 1.0, 1.0), 6.0)
        res.paint_labels([(8 * 20, 8 * 13, 8 * 9), (8 * 30, 8 * 15, 8 * 12)], weights, limit, "paint", [5], 5)
        edited = res.download_label_volume()
        assert (edited == 5).sum() > 500
        got = either_way(tunables, res, "edited", edited, [5])   # the boards come from the current bytes
        assert got["set_voxels"] == int((edited == 5).sum())
        either_way(tunables, res, "edited", edited, [3, 5], (3, 5, 1), (30, 17, 13), triangles=True)
