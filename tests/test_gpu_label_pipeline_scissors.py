"""Scissors among the other label writers on ONE handle: random sequences of twelve steps — six scissors calls alternating with region
updates, seeded growing, morphology, islands and Euclidean margins, whose generators and interpreter are
tests/label_pipeline_reference.py's — held to the references step by step: every field of every result, every label byte behind
every step, and the label statistics at the end. The shared scratch (the boards of region growing) and the lazily merged label
metadata pass from one operator to the next."""
import numpy as np
import pytest

from tbraymarcherplugin_amd import abi, synthetic as S
import label_pipeline_reference as P
import label_scissors_reference as SR

pytestmark = pytest.mark.gpu

SEEDS = (1, 2, 3, 5)   # blobs and empty starts, three data types, three shapes (label_pipeline_reference.setup)
OTHERS = ("grow", "morph", "region", "islands", "margin", "morph")
WORLD = S.default_world()


def gen_scissors(rng, labels, dims, k):
    """a scissors step: a random oblique camera (every third one inside the volume), a mask of one of four kinds, any operator"""
    width, height = [(77, 53), (64, 48), (33, 40)][k % 3]
    world, cam = SR.random_cameras(1, dims, width, height, seed=int(rng.integers(1 << 30)), inside=k % 3 == 2)[0]
    depth = (0.0, float("inf")) if rng.random() < 0.6 else (float(rng.uniform(150.0, 300.0)), float(rng.uniform(300.0, 420.0)))
    p = SR.of_struct(abi.scissors_projection(dims, world, cam, *depth))
    kind = P.pick(rng, ("disc", "half_plane", "polygon", "checkerboard"))
    if kind == "disc":
        mask = SR.disc(width, height, int(rng.integers(width // 4, 3 * width // 4)), int(rng.integers(height // 4, 3 * height // 4)), int(rng.integers(4, 20)))
    elif kind == "half_plane":
        mask = SR.half_plane(width, height, int(rng.integers(width // 4, 3 * width // 4)))
    elif kind == "polygon":
        mask = abi.scissors_polygon(np.round(rng.uniform(-5.0, max(width, height) + 5.0, size=(int(rng.integers(3, 8)), 2)) * 256) / 256, width, height)
    else:
        mask = SR.checkerboard(width, height)
    source = P.source_of(rng, labels)
    args = {"op": P.pick(rng, SR.OPS), "source": source, "new_label": P.new_label_of(rng, source), "erase_label": P.pick(rng, (0, 0, 4))}
    boxed = P.draw_box(rng, dims, P.pick(rng, ("brick", "medium", "large"))) if rng.random() < 0.4 else None
    return {"kind": "scissors", "p": p, "mask": mask, "args": P.mask_args(rng, labels, args, boxed)}


@pytest.mark.parametrize("seed", SEEDS)
def test_twelve_steps_with_the_other_writers(gpu, seed):
    su = P.setup(seed)
    dims = su["dims"]
    rng = np.random.default_rng(7000 + seed)
    vol, labels, colors = P.initial(su)
    plan = {"dims": dims, "boxed": {"islands": 0, "margin": 0}, "holes": False, "attempt": 0, "data_modes": []}
    others = [OTHERS[i] for i in rng.permutation(len(OTHERS))]
    moved = 0
    with abi.Resources(dims, abi.DTYPE_FMT[vol.dtype]) as res:
        res.upload_volume(vol)
        res.upload_label_volume(labels)
        for i in range(12):
            if i % 2:
                step = gen_scissors(rng, labels, dims, i // 2)
                got = res.scissor_labels(abi.make_scissors_projection(**step["p"]), step["mask"], **step["args"])
                _, want, labels = SR.scissors(labels, step["p"], step["mask"], **step["args"])
                fields = SR.FIELDS
                moved += want["added"] + want["removed"]
            else:
                step = P.GENERATORS[others[i // 2]](rng, vol, labels, plan)
                after = P.apply(step, vol, labels, colors)
                name, args = P.call_of(step) if "call" in step else (None, None)
                if step["kind"] == "region":
                    got = res.update_label_region(step["origin"], P.region_block(step))
                else:
                    got = {"grow": res.grow_region, "morph": res.morph_labels, "islands": res.label_islands, "margin": res.margin_labels}[name](**args)
                want, labels, fields = after.result, after.labels, P.FIELDS.get(step.get("call"), ())
            for k in fields:
                assert got[k] == want[k], (i, step["kind"], k, got[k], want[k])
            down = res.download_label_volume()
            assert np.array_equal(down, labels), (i, step["kind"], int((down != labels).sum()), np.argwhere(down != labels)[:5])
        stats = res.label_statistics()
        for l in range(256):
            assert stats[l]["count"] == int((labels == l).sum()), l
        assert res.scissors_counters()["scissors_calls"] == 6
    assert moved > 0
