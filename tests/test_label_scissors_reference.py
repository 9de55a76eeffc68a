"""The inputs of tests/test_gpu_label_scissors.py judged without a GPU, so that no GPU case is vacuous: every case cuts its volume in
two, the lattice cases have voxels whose U is an exact multiple of W, the verdict cases have bricks in all three states by the
reference's own voxels, the bound cases reach 2^45, and the reference's int64 arithmetic agrees with Python's integers."""
import numpy as np

import label_scissors_reference as SR


def test_every_case_is_admissible_and_cuts_its_volume():
    names = set()
    for name, dims, p, mask in SR.gpu_cases():
        assert name not in names
        names.add(name)
        assert SR.admissible(p, dims), name
        assert mask.shape == (p["height"], (p["width"] + 31) // 32) and mask.dtype == np.uint32, name
        assert np.array_equal(SR.mask_words(SR.mask_bits(mask, p["width"])), mask), name   # no bit at or beyond the width
        M = SR.in_M(p, mask, dims)
        assert 0 < M.sum() < M.size, (name, int(M.sum()))
        if name in SR.BOX_CASES:   # ... and every box of the box test but the one-voxel box
            for origin, extent in SR.BOXES:
                part = M[SR.box_mask(M.shape, origin, extent)]
                assert extent == (1, 1, 1) or 0 < part.sum() < part.size, (name, origin)
    assert set(SR.BOX_CASES) <= names
    assert len(names) >= 18


def test_int64_agrees_with_python_integers():
    rng = np.random.default_rng(3)
    for name, dims, p, mask in SR.gpu_cases():
        voxels = [tuple(int(rng.integers(0, d)) for d in dims) for _ in range(200)] + [(0, 0, 0), tuple(d - 1 for d in dims)]
        M = SR.in_M(p, mask, dims)
        assert SR.in_M_slowly(p, mask, dims, voxels) == [bool(M[z, y, x]) for x, y, z in voxels], name


def test_lattice_cases_land_on_pixel_edges():
    for name, dims, p, mask in SR.lattice_cases():
        U, V, W = SR.rows_at(p, dims)
        on_edge = (W > 0) & (U % np.where(W > 0, W, 1) == 0)
        assert on_edge.sum() >= U.size // 8, (name, int(on_edge.sum()))
        if name.startswith("along"):
            assert on_edge.all() and (V % W == 0).all(), name
    U, _, _ = SR.rows_at(SR.lattice_cases()[4][2], SR.SHAPES[0])
    assert SR.lattice_cases()[4][0] == "shear" and (U < 0).sum() > 1000 and (U >= 0).sum() > 1000


def test_perspective_cases_have_what_they_are_for():
    cases = {name: (dims, p, mask) for name, dims, p, mask in SR.perspective_cases()}
    dims, p, _ = cases["camera_inside"]
    _, _, W = SR.rows_at(p, dims)
    assert (W <= 0).sum() > 100 and (W > 0).sum() > 100
    straddling = 0
    for bz in range(0, dims[2], 8):
        for by in range(0, dims[1], 8):
            for bx in range(0, dims[0], 8):
                part = W[bz:bz + 8, by:by + 8, bx:bx + 8]
                straddling += bool((part <= 0).any() and (part > 0).any())
    assert straddling >= 3
    dims, p, _ = cases["depth_slab"]
    _, _, W = SR.rows_at(p, dims)
    assert ((W < p["w_min"]).sum() > 500 and (W > p["w_max"]).sum() > 500 and SR.brick_states(p, SR.all_set(77, 53), dims)["mixed"] > 10)
    assert cases["one_depth"][1]["w_min"] == cases["one_depth"][1]["w_max"]


def test_verdict_cases_have_bricks_in_all_three_states():
    name, dims, p, mask = SR.verdict_cases()[0]
    states = SR.brick_states(p, mask, dims)
    assert min(states.values()) >= 5, states
    assert SR.brick_states(*SR.verdict_cases()[1][2:], dims) == {"inside": 45, "outside": 0, "mixed": 0}
    assert SR.brick_states(*SR.verdict_cases()[2][2:], dims) == {"inside": 0, "outside": 45, "mixed": 0}
    for case in SR.perspective_cases()[:1] + SR.mask_cases()[1:2] + SR.bound_cases()[1:]:   # oblique, half_plane, deep
        assert min(SR.brick_states(case[2], case[3], case[1]).values()) >= 1, case[0]


def test_bound_cases_reach_the_limit():
    for name, dims, p, mask in SR.bound_cases():
        assert p["width"] == SR.MAX_IMAGE
        reach = max(SR.row_reach(p[k], dims) for k in "uvw")
        assert 2 ** 46 - 2 ** 20 < reach < 2 ** 46, (name, reach)
        U, V, W = SR.rows_at(p, dims)
        assert max(int(np.abs(U).max()), int(np.abs(V).max()), int(W.max())) >= 2 ** 45, name
    _, dims, p, _ = SR.bound_cases()[0]
    _, px, _ = SR.pixels(p, dims)
    assert px.max() >= SR.MAX_IMAGE - 500 and px.min() == 0
    _, dims, p, _ = SR.bound_cases()[1]
    U, _, W = SR.rows_at(p, dims)
    assert p["width"] * int(W.max()) > 2 ** 59 and (U < 0).any()


def test_operators_and_counts_of_the_reference():
    dims = SR.SHAPES[0]
    labels = SR.blob_labels(dims)
    name, _, p, mask = SR.verdict_cases()[0]
    M = SR.in_M(p, mask, dims)
    S = labels == 3
    for op, want in ((SR.ERASE_INSIDE, S & ~M), (SR.ERASE_OUTSIDE, S & M), (SR.FILL_INSIDE, S | M), (SR.FILL_OUTSIDE, S | ~M)):
        R, result, after = SR.scissors(labels, p, mask, op, [3], 3, erase_label=9)
        assert np.array_equal(R, want)
        assert result["added"] == (want & ~S).sum() and result["removed"] == (S & ~want).sum() and result["added"] + result["removed"] > 0
        assert np.array_equal(after == 3, want) and (after == 9).sum() == result["removed"]
        _, measured, same = SR.scissors(labels, p, mask, op, [3], -1)
        assert np.array_equal(same, labels) and measured["relabelled"] == 0 and measured["added"] == result["added"]
    assert SR.box_bricks(dims) == 45 and SR.box_bricks(dims, (8, 8, 8), (8, 8, 8)) == 1 and SR.box_bricks(dims, (3, 2, 16), (30, 20, 3)) == 5 * 3 * 1
