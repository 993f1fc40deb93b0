"""fcn8s_tensorflow_amd/class_mix.py on the CPU: `mix_numpy` and `select_classes` against tests/golden/class_mix_cases.npz (written by plain
Python loops, tests/golden/make_class_mix_cases.py) with `==`, ClassMix's count ceil(k / 2) for every k, the balance of the selection over many
draws, and what `validate` refuses."""
import functools
import os
import types

import numpy as np
import pytest

from fcn8s_tensorflow_amd import class_mix as CM

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "class_mix_cases.npz")
FIELDS = ("N", "P", "C", "src", "seed", "draw", "images", "labels", "out_images", "out_labels", "selected", "note")


@functools.lru_cache(maxsize=None)
def golden():
    """The fixture's cases as dicts; N, P, C, seed, draw as Python ints."""
    z = np.load(GOLDEN)
    cases = []
    for i in range(int(z["count"])):
        c = {f: z["c%02d_%s" % (i, f)] for f in FIELDS}
        for f in ("N", "P", "C", "seed", "draw"):
            c[f] = int(c[f])
        c["note"] = str(c["note"])
        cases.append(c)
    return tuple(cases)


def case_ids():
    return ["%d-%dx%d-C%d-%s" % (i, c["N"], c["P"], c["C"], c["note"].split(",")[0].replace(" ", "_")) for i, c in enumerate(golden())]


def pick(P, Cn, N=2):
    return [c for c in golden() if (c["N"], c["P"], c["C"]) == (N, P, Cn)][0]


def test_the_fixture_has_the_cases_the_definition_needs():
    cs = golden()
    assert {c["P"] for c in cs} >= {1, 15, 16, 17, 255, 256, 257, 1023, 1025} and {c["C"] for c in cs} >= {2, 19, 20, 21, 64, 255}
    assert any(c["N"] == 3 and c["P"] == 300 for c in cs)
    assert any(c["draw"] == (1 << 48) - 1 for c in cs)
    assert any((c["src"] == np.arange(c["N"])).all() for c in cs) and any(len(set(c["src"].tolist())) < c["N"] for c in cs)
    a, b = [c for c in cs if "same input" in c["note"]][:2]
    assert (a["images"] == b["images"]).all() and (a["labels"] == b["labels"]).all() and (a["selected"] != b["selected"]).any()


@pytest.mark.parametrize("i", range(len(golden())), ids=case_ids())
def test_mix_numpy_and_select_classes_equal_the_fixture(i):
    c = golden()[i]
    oi, ol, sel = CM.mix_numpy(c["images"], c["labels"], c["src"], c["C"], c["seed"], c["draw"])
    assert (oi == c["out_images"]).all() and (ol == c["out_labels"]).all() and (sel == c["selected"]).all()
    for n in range(c["N"]):
        assert (CM.select_classes(c["labels"][c["src"][n]], c["C"], c["seed"], c["draw"], n) == c["selected"][n]).all()


def test_philox_matches_the_dropout_masks_restatement():
    """The first words of a few counters against values computed with Python ints."""
    M = 0xFFFFFFFF

    def ref(idx, seed, stream):
        c = [idx & M, idx >> 32, stream, 0x9E3779B9]
        k = [seed & M, seed >> 32]
        for _ in range(10):
            p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
            c = [((p1 >> 32) ^ c[1] ^ k[0]) & M, p1 & M, ((p0 >> 32) ^ c[3] ^ k[1]) & M, p0 & M]
            k = [(k[0] + 0x9E3779B9) & M, (k[1] + 0xBB67AE85) & M]
        return c[0]
    idx = [0, 1, 255, (1 << 32) - 1, 1 << 32, ((1 << 48) - 1 << 16) + (255 << 8) + 254]
    for seed in (0, 5, (1 << 64) - 1):
        got = CM.philox_u32(np.array(idx, np.uint64), seed, CM.STREAM)
        assert got.dtype == np.uint32 and got.tolist() == [ref(i, seed, CM.STREAM) for i in idx]


@pytest.mark.parametrize("Cn", [2, 20, 255])
def test_exactly_half_of_the_present_classes_rounded_up_are_selected(Cn):
    rng = np.random.default_rng(Cn)
    for k in range(Cn + 1):
        present = rng.choice(Cn, size=k, replace=False).astype(np.uint8)
        labels = np.concatenate([present, present, np.array([Cn, 255], np.uint8)])
        sel = CM.select_classes(labels, Cn, seed=3, draw=k, n=1)
        assert sel.sum() == (k + 1) // 2 and not sel[Cn:].any()
        assert set(np.flatnonzero(sel)) <= set(present.tolist())


def test_every_present_class_is_selected_about_half_of_the_time():
    """k = 10 of 20 classes present, 1000 draws: a class's count is Binomial(1000, 1/2) (5 of 10 are taken, by symmetry each with probability
    1/2), standard deviation sqrt(250) = 15.8; five of them are 79."""
    present = np.array([0, 2, 3, 5, 8, 11, 13, 14, 17, 19], np.uint8)
    count = np.zeros(256, np.int64)
    for draw in range(1000):
        count += CM.select_classes(present, 20, seed=12345, draw=draw, n=0)
    assert (np.abs(count[present] - 500) <= 79).all(), count[present]
    assert count.sum() == 5000 and not np.delete(count, present).any()


def test_a_source_out_of_range_counts_as_the_image_itself():
    c = pick(300, 20, 3)
    for bad in (-1, 3, 1 << 20):
        src = c["src"].copy(); src[1] = bad
        want = CM.mix_numpy(c["images"], c["labels"], np.where(np.arange(3) == 1, 1, c["src"]), 20, c["seed"], c["draw"])
        got = CM.mix_numpy(c["images"], c["labels"], src, 20, c["seed"], c["draw"])
        assert all((g == w).all() for g, w in zip(got, want))
        assert (got[0][1] == c["images"][1]).all() and (got[1][1] == c["labels"][1]).all()


def model(classes=20, device="cuda:0"):
    m = types.SimpleNamespace(engine=types.SimpleNamespace(logical_classes=classes, device=device))
    return m


def test_validate_takes_and_normalises_the_facades_arguments():
    v = CM.validate(20, thresholds=0.9)
    assert v["thresholds"].dtype == np.float32 and v["thresholds"].shape == (20,) and (v["thresholds"] == np.float32(0.9)).all()
    assert v["mix"] is True and v["seed"] == 0 and v["predict"] == {} and v["labeler"] == 'self'
    thr = np.linspace(0.5, 0.95, 20)
    assert (CM.validate(20, thresholds=thr)["thresholds"] == thr.astype(np.float32)).all()
    assert (CM.validate(20, model_thresholds=thr)["thresholds"] == thr.astype(np.float32)).all()
    assert CM.validate(20, labeler='ema', thresholds=0.5, has_average=True)["labeler"] == 'ema'
    other, student = model(), model()
    assert CM.validate(20, labeler=other, thresholds=0.5, student=student)["labeler"] is other
    assert CM.validate(20, thresholds=0.5, predict=dict(scales=(1.0, 0.5), flip=True), mix=False, seed=7)["mix"] is False


def test_validate_refuses_what_the_facade_must_refuse():
    student = model()
    bad = [dict(teacher=object()),                                              # together with teacher=
           dict(labeler='ema'),                                                 # no average
           dict(labeler='student'), dict(labeler=None), dict(labeler=3),
           dict(labeler=model(device="cuda:1"), student=student),               # another device
           dict(labeler=model(classes=19), student=student),                    # another class count
           dict(labeler=student, student=student),                              # the student itself
           dict(thresholds=None),                                               # none given and none fitted
           dict(thresholds=[0.5] * 19), dict(thresholds=float('nan')), dict(thresholds=True),
           dict(predict=dict(argmax=True)), dict(predict=dict(min_region=5)),
           dict(mix=1), dict(mix=None),
           dict(seed=-1), dict(seed=1.5), dict(seed=True), dict(seed=1 << 63)]
    for kw in bad:
        with pytest.raises(ValueError):
            CM.validate(20, **{**dict(thresholds=0.5), **kw})
    for Cn in (1, 256):
        with pytest.raises(ValueError):
            CM.validate(Cn, thresholds=0.5)


def test_the_op_level_arguments_are_checked_on_the_host_too():
    lab = np.zeros((1, 4), np.uint8)
    for kw in (dict(C=1), dict(C=256), dict(draw=1 << 48), dict(draw=-1), dict(seed=-1), dict(seed=1 << 64)):
        with pytest.raises(ValueError):
            CM.select_classes(lab, **{**dict(C=20, seed=0, draw=0, n=0), **kw})
    with pytest.raises(ValueError):
        CM.mix_numpy(np.zeros((1, 4, 3), np.uint8), np.zeros((1, 5), np.uint8), [0], 20, 0, 0)
