"""Competitive growing among the other label writers on ONE handle: random sequences of twelve steps — six compete calls alternating
with region updates, seeded growing, morphology, islands and Euclidean margins, whose generators and interpreter are
tests/label_pipeline_reference.py's — held to the references step by step: every field of every result (the costs of the box
included), every label byte behind every step, and the label statistics at the end. The compete scratch is a handle's own; the
lazily merged label metadata passes from one operator to the next."""
import numpy as np
import pytest

from tbraymarcherplugin_amd import abi
import label_compete_reference as CR
import label_pipeline_reference as P

pytestmark = pytest.mark.gpu

SEEDS = (1, 2, 3, 5)   # blobs and empty starts, three data types, three shapes (label_pipeline_reference.setup)
OTHERS = ("grow", "morph", "region", "islands", "margin", "morph")


def gen_compete(rng, vol, labels, dims, k):
    """a compete step: one to three of the labels present (or one that is absent) as seeds, a gate over part of the range, any step
    costs, every third call measuring, two in five boxed, a limit that may bind"""
    present = [int(l) for l in np.unique(labels) if l != 0]
    n = int(rng.integers(1, 4))
    seeds = [int(l) for l in rng.permutation(present)[:n]] if present and rng.random() < 0.9 else [int(rng.integers(200, 256))]
    if vol.dtype == np.float32:
        finite = vol[np.isfinite(vol)]
        a, b = float(finite.min()), float(finite.max())
        lo, hi = float(np.float32(a + (b - a) * rng.uniform(0.0, 0.3))), float(np.float32(a + (b - a) * rng.uniform(0.6, 1.0)))
        frange = CR.float_range(a, b)
    else:
        top = 255 if vol.dtype == np.uint8 else 65535
        lo, hi = int(top * rng.uniform(0.0, 0.3)), int(top * rng.uniform(0.6, 1.0))
        frange = None
    args = {"seeds": seeds, "lo": lo, "hi": hi, "step_cost": tuple(int(v) for v in rng.integers(0, 6, size=3)), "value_shift": int(rng.integers(0, 9)),
            "cost_limit": P.pick(rng, (0, 0, int(rng.integers(1, 400)), int(rng.integers(400, 40000)))), "measure_only": k % 3 == 2,
            "writable": P.pick(rng, (None, [0], [0] + [l for l in present if l not in seeds][:2]))}
    if rng.random() < 0.4:
        args["origin"], args["extent"] = P.draw_box(rng, dims, P.pick(rng, ("brick", "medium", "large")))
    return args, frange


@pytest.mark.parametrize("seed", SEEDS)
def test_twelve_steps_with_the_other_writers(gpu, seed):
    su = P.setup(seed)
    dims = su["dims"]
    rng = np.random.default_rng(9000 + seed)
    vol, labels, colors = P.initial(su)
    plan = {"dims": dims, "boxed": {"islands": 0, "margin": 0}, "holes": False, "attempt": 0, "data_modes": []}
    others = [OTHERS[i] for i in rng.permutation(len(OTHERS))]
    claimed = 0
    with abi.Resources(dims, abi.DTYPE_FMT[vol.dtype]) as res:
        res.upload_volume(vol)
        res.upload_label_volume(labels)
        for i in range(12):
            if i % 2:
                args, frange = gen_compete(rng, vol, labels, dims, i // 2)
                got, costs = res.compete_labels(float_range=frange, costs=True, **args)
                want, labels, want_costs, _ = CR.compete(vol, labels, frange=frange, **args)
                fields, kind = CR.FIELDS, "compete"
                assert np.array_equal(costs, want_costs), (i, args, int((costs != want_costs).sum()))
                assert (got["passes"] >= 1) == (want["claimed"] > 0), (i, got)
                claimed += want["claimed"]
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
        assert res.compete_counters()["compete_calls"] == 6
    assert claimed > 0
