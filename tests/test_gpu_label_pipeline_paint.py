"""The paint brush among the other label writers on ONE handle: random sequences of twelve steps — six brush strokes alternating with
region updates, seeded growing, morphology, islands and Euclidean margins, whose generators and interpreter are
tests/label_pipeline_reference.py's — held to the references step by step: every field of every result, every label byte behind
every step, and the label statistics at the end. The stroke's staging is a handle's own; the boards are region growing's, shared with
the morphology and the margins; the lazily merged label metadata passes from one operator to the next."""
import numpy as np
import pytest

from tbraymarcherplugin_amd import abi
import label_paint_reference as PR
import label_pipeline_reference as P

pytestmark = pytest.mark.gpu

SEEDS = (1, 2, 3, 5)   # blobs and empty starts, three data types, three shapes (label_pipeline_reference.setup)
OTHERS = ("grow", "morph", "region", "islands", "margin", "morph")
BRUSHES = (((1, 1, 1), 24 * 24), ((1, 1, 1), 300), ((256, 256, 3265), 133696), ((3, 2, 5), 2000), ((1, 1, 1), 50 * 50))


def gen_paint(rng, vol, labels, dims, k):
    """a stroke: a ball, a few segments or a wandering stroke of a hundred points, ends outside the volume now and then; paint or
    erase; one of five brushes; every third call measuring, two in five boxed, two in five gated over part of the range"""
    present = [int(l) for l in np.unique(labels) if l != 0]
    weights, limit = P.pick(rng, BRUSHES)
    n = int(P.pick(rng, (1, 2, 3, 5, 100)))
    if n == 100:
        points = PR.wiggle(dims, n, seed=int(rng.integers(1 << 30)), step=14)
    else:
        points = [tuple(int(rng.integers(-24, 8 * d + 24)) for d in dims) for _ in range(n)]
    source = [int(l) for l in rng.permutation(present)[:int(rng.integers(1, 3))]] if present and rng.random() < 0.85 else [int(rng.integers(200, 256))]
    args = {"points": points, "weights": weights, "limit": limit, "op": int(rng.integers(0, 2)), "source": source,
            "new_label": -1 if k % 3 == 2 else source[0], "erase_label": int(P.pick(rng, (0, 0, 9))),
            "writable": P.pick(rng, (None, None, [0], [0] + [l for l in present if l not in source][:2]))}
    if rng.random() < 0.4:
        args["origin"], args["extent"] = P.draw_box(rng, dims, P.pick(rng, ("brick", "medium", "large")))
    if rng.random() < 0.4:
        if vol.dtype == np.float32:
            finite = vol[np.isfinite(vol)]
            a, b = float(finite.min()), float(finite.max())
            args["gate"] = (float(np.float32(a + (b - a) * rng.uniform(0.0, 0.3))), float(np.float32(a + (b - a) * rng.uniform(0.6, 1.0))))
        else:
            top = 255 if vol.dtype == np.uint8 else 65535
            args["gate"] = (int(top * rng.uniform(0.0, 0.3)), int(top * rng.uniform(0.6, 1.0)))
    return args


@pytest.mark.parametrize("seed", SEEDS)
def test_twelve_steps_with_the_other_writers(gpu, seed):
    su = P.setup(seed)
    dims = su["dims"]
    rng = np.random.default_rng(9100 + seed)
    vol, labels, colors = P.initial(su)
    plan = {"dims": dims, "boxed": {"islands": 0, "margin": 0}, "holes": False, "attempt": 0, "data_modes": []}
    others = [OTHERS[i] for i in rng.permutation(len(OTHERS))]
    moved = 0
    with abi.Resources(dims, abi.DTYPE_FMT[vol.dtype]) as res:
        res.upload_volume(vol)
        res.upload_label_volume(labels)
        for i in range(12):
            if i % 2:
                args = gen_paint(rng, vol, labels, dims, i // 2)
                assert PR.admissible(args["points"], args["weights"], args["limit"], dims)
                got = res.paint_labels(**args)
                _, want, labels = PR.paint(labels, vol, **args)
                fields, kind = PR.FIELDS, "paint"
                bricks = PR.work_bricks(args["points"], args["weights"], args["limit"], dims, args.get("origin"), args.get("extent"))
                assert got["bricks_whole"] + got["bricks_untouched"] + got["bricks_evaluated"] == bricks and got["launches"] == (3 if bricks else 0), (i, got, bricks)
                moved += want["added"] + want["removed"]
            else:
                step = P.GENERATORS[others[i // 2]](rng, vol, labels, plan)
                after = P.apply(step, vol, labels, colors)
                name, args = P.call_of(step) if "call" in step else (None, None)
                if step["kind"] == "region":
                    got = res.update_label_region(step["origin"], P.region_block(step))
                else:
                    got = {"grow": res.grow_region, "morph": res.morph_labels, "islands": res.label_islands, "margin": res.margin_labels}[name](**args)
                want, labels, fields, kind = after.result, after.labels, P.FIELDS.get(step.get("call"), ()), step["kind"]
            for k in fields:
                assert got[k] == want[k], (i, kind, k, got[k], want[k], args)
            down = res.download_label_volume()
            assert np.array_equal(down, labels), (i, kind, int((down != labels).sum()), np.argwhere(down != labels)[:5])
        stats = res.label_statistics()
        for l in range(256):
            assert stats[l]["count"] == int((labels == l).sum()), l
        assert res.paint_counters()["paint_calls"] == 6
    assert moved > 0
