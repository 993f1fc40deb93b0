"""fcn8s_tensorflow_amd/strong_augment.py on the CPU: `augment_numpy` and `params_numpy` against tests/golden/strong_augment_cases.npz (written
by plain Python loops, tests/golden/make_strong_augment_cases.py) with `==`, the tap table's invariants, how often the two gates open over many
draws, and what `validate` and the op-level checks refuse."""
import functools
import os

import numpy as np
import pytest

from fcn8s_tensorflow_amd import strong_augment as SA

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "strong_augment_cases.npz")
FIELDS = ("N", "H", "W", "seed", "draw", "jitter", "blur_gate", "taps", "images", "out_images", "params", "note")
ONE = 65536


@functools.lru_cache(maxsize=None)
def golden():
    """The fixture's cases as dicts; N, H, W, seed, draw as Python ints, `jitter` None or int32[5], `blur` None or (gate, taps [Q, R + 1])."""
    z = np.load(GOLDEN)
    cases = []
    for i in range(int(z["count"])):
        c = {f: z["c%02d_%s" % (i, f)] for f in FIELDS}
        for f in ("N", "H", "W", "seed", "draw"):
            c[f] = int(c[f])
        c["note"] = str(c["note"])
        c["jitter"] = c["jitter"] if c["jitter"].size else None
        c["blur"] = (int(c["blur_gate"]), c["taps"]) if int(c["blur_gate"]) >= 0 else None
        cases.append(c)
    return tuple(cases)


def case_ids():
    return ["%d-%dx%dx%d-%s" % (i, c["N"], c["H"], c["W"], c["note"].split(",")[0].split(":")[0].replace(" ", "_")) for i, c in enumerate(golden())]


def pick(note):
    return [c for c in golden() if c["note"].startswith(note)][0]


def test_the_fixture_has_the_cases_the_definition_needs():
    cs = golden()
    shapes = {(c["H"], c["W"]) for c in cs}
    assert {h for h, _ in shapes} >= {2, 5, 8, 15, 16, 17, 33} and {w for _, w in shapes} >= {2, 5, 8, 31, 32, 33, 63, 64, 65, 129}
    for R in (1, 4, 7):                                          # H = R + 1 and W = R + 1 under a blur of radius R
        assert any(c["blur"] is not None and c["taps"].shape[1] - 1 == R and c["H"] == R + 1 for c in cs)
        assert any(c["blur"] is not None and c["taps"].shape[1] - 1 == R and c["W"] == R + 1 for c in cs)
    assert any((c["N"], c["H"], c["W"]) == (3, 48, 80) and len(set(c["params"][:, 0])) == 2 and len(set(c["params"][:, 6])) == 2 for c in cs)
    assert any(c["draw"] == (1 << 48) - 1 for c in cs)
    assert any(c["jitter"] is None and c["blur"] is None for c in cs) and any(c["jitter"] is None and c["blur"] is not None for c in cs)
    assert {c["taps"].shape[0] for c in cs if c["blur"] is not None} >= {1, 16}
    assert {0, 131072} <= {int(c["params"][0, 1]) for c in cs}
    assert (pick("strengths 0")["out_images"] == pick("strengths 0")["images"]).all() and pick("strengths 0")["params"][:, 0].all()
    assert any((c["params"][:, 4] > 0).any() for c in cs) and any((c["params"][:, 4] < 0).any() for c in cs)


@pytest.mark.parametrize("i", range(len(golden())), ids=case_ids())
def test_augment_numpy_and_params_numpy_equal_the_fixture(i):
    c = golden()[i]
    out, par = SA.augment_numpy(c["images"], c["seed"], c["draw"], c["jitter"], c["blur"])
    assert out.dtype == np.uint8 and (out == c["out_images"]).all()
    assert par.dtype == np.int32 and (par == c["params"]).all()
    assert (SA.params_numpy(c["images"], c["seed"], c["draw"], c["jitter"], c["blur"]) == c["params"]).all()


def test_the_draws_are_the_librarys_philox_on_its_own_stream():
    M = 0xFFFFFFFF

    def ref(idx, seed, stream):
        c = [idx & M, idx >> 32, stream, 0x9E3779B9]
        k = [seed & M, seed >> 32]
        for _ in range(10):
            p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
            c = [((p1 >> 32) ^ c[1] ^ k[0]) & M, p1 & M, ((p0 >> 32) ^ c[3] ^ k[1]) & M, p0 & M]
            k = [(k[0] + 0x9E3779B9) & M, (k[1] + 0xBB67AE85) & M]
        return c[0]
    for seed, draw in ((0, 0), (5, 77), ((1 << 64) - 1, (1 << 48) - 1)):
        u = SA.draws(3, seed, draw)
        assert u.dtype == np.uint32 and u.shape == (3, 7)
        assert u.tolist() == [[ref((draw << 16) + (n << 8) + j, seed, 0x53415547) for j in range(7)] for n in range(3)]


@pytest.mark.parametrize("args", [(0.15, 1.15, 16, 4), (0.3, 0.6, 3, 1), (0.5, 2.0, 16, 7), (1.0, 1.0, 1, 4), (0.8, 0.8, 2, 2)])
def test_the_rows_of_a_tap_table_sum_to_2048_and_do_not_increase(args):
    t = SA.taps_table(*args)
    assert t.dtype == np.uint16 and t.shape == (args[2], args[3] + 1)
    w = t.astype(np.int64)
    assert (w[:, 0] + 2 * w[:, 1:].sum(1) == 2048).all() and (np.diff(w, axis=1) <= 0).all()
    i = np.arange(1, args[3] + 1)
    for q, sigma in enumerate(np.linspace(args[0], args[1], args[2])):                       # the rounded Gaussian itself
        g = np.exp(-np.arange(-args[3], args[3] + 1) ** 2 / (2.0 * sigma * sigma))
        assert (w[q, 1:] == np.rint(2048 * np.exp(-i * i / (2.0 * sigma * sigma)) / g.sum())).all()


def test_the_lowest_sigma_is_the_identity_and_a_sigma_too_wide_is_refused():
    t = SA.taps_table(0.15, 1.15, 16, 4)
    assert t[0].tolist() == [2048, 0, 0, 0, 0] and t[15, 1] > 0
    img = np.random.default_rng(0).integers(0, 256, (1, 9, 11, 3), dtype=np.uint8)
    out, par = SA.augment_numpy(img, 0, 0, None, (ONE, t[:1]))
    assert par[0, 6] == 1 and (out == img).all()
    # (a box: every tap rounds to 683 and the centre, 2048 - 2 * 683 = 682, falls below them)
    for bad in ((100.0, 100.0, 1, 1), (0.0, 1.0, 4, 4), (1.0, 0.5, 4, 4), (0.5, 1.0, 0, 4), (0.5, 1.0, 17, 4), (0.5, 1.0, 4, 0), (0.5, 1.0, 4, 8),
                (0.5, float('inf'), 4, 4)):
        with pytest.raises(ValueError):
            SA.taps_table(*bad)


@pytest.mark.parametrize("seed", [0, 1, 12345])
def test_the_gates_open_as_often_as_their_probabilities_say(seed):
    """1000 draws: the colour gate at 52429 / 65536 = 0.8 opens Binomial(1000, 0.8) times (standard deviation 12.6, five of them 64), the blur
    gate at 1/2 Binomial(1000, 0.5) times (15.8, 79)."""
    img = np.zeros((1, 2, 2, 3), np.uint8)
    taps = SA.taps_table(0.5, 0.5, 1, 1)
    jit = bl = 0
    for draw in range(1000):
        p = SA.params_numpy(img, seed, draw, [52429, 0, 0, 0, 0], (32768, taps))
        jit += int(p[0, 0]); bl += int(p[0, 6])
    assert abs(jit - 800) <= 64 and abs(bl - 500) <= 79, (jit, bl)


def test_the_uniform_integers_cover_their_range_and_no_more():
    S = 3
    vals = {SA._uniform(u, S) for u in range(0, 1 << 32, (1 << 32) // 997)} | {SA._uniform(0, S), SA._uniform((1 << 32) - 1, S)}
    assert vals == set(range(-S, S + 1))
    assert SA._uniform(12345, 0) == 0 and SA._uniform((1 << 32) - 1, 65536) == 65536 and SA._uniform(0, 65536) == -65536


def test_validate_takes_and_normalises_the_facades_argument():
    assert SA.validate(None) is None and SA.validate(None, has_generator=False) is None
    v = SA.validate(True)
    assert v["jitter"].dtype == np.int32 and v["jitter"].tolist() == [52429, 16384, 16384, 16384, 22]
    assert v["blur"][0] == 32768 and (v["blur"][1] == SA.taps_table(0.15, 1.15, 16, 4)).all()
    assert SA.validate({})["jitter"].tolist() == v["jitter"].tolist()
    v = SA.validate(dict(jitter_p=1.0, hue=0.0, blur_p=0.0))
    assert v["blur"] is None and v["jitter"].tolist() == [ONE, 16384, 16384, 16384, 0]
    v = SA.validate(dict(jitter_p=0, sigma=(1.0, 1.0), levels=1, radius=3))
    assert v["jitter"] is None and v["blur"][1].shape == (1, 4)


def test_validate_refuses_what_the_facade_must_refuse():
    with pytest.raises(ValueError):
        SA.validate(True, has_generator=False)
    for bad in (1, 0.5, "on", [1, 2], dict(gamma=1.0), dict(jitter_p=1.5), dict(jitter_p=-0.1), dict(contrast=2.0), dict(hue=True),
                dict(brightness="x"), dict(blur_p=float('nan')), dict(sigma=1.0), dict(sigma=(0.0, 1.0)), dict(sigma=(2.0, 1.0)),
                dict(sigma=(100.0, 100.0), radius=1), dict(levels=0), dict(levels=17), dict(levels=2.0), dict(radius=8), dict(radius=0),
                dict(jitter_p=0, blur_p=0)):
        with pytest.raises(ValueError):
            SA.validate(bad)


def test_the_op_level_arguments_are_checked_on_the_host_too():
    img = np.zeros((1, 6, 6, 3), np.uint8)
    t = SA.taps_table(0.5, 1.0, 2, 2)
    ok = dict(seed=0, draw=0, jitter=[ONE, 1, 2, 3, 4], blur=(ONE, t))
    SA.augment_numpy(img, **ok)
    up = t.astype(np.int64); d = up[1, 0] - up[1, 1]; up[1, 0] -= 2 * d; up[1, 1] += d        # the same sum, but w[1] > w[0]
    assert up[1, 0] >= 0 and up[1, 0] + 2 * up[1, 1:].sum() == 2048 and up[1, 1] > up[1, 0]
    off = t.copy(); off[1, 0] += 2
    for kw in (dict(draw=1 << 48), dict(draw=-1), dict(seed=-1), dict(seed=1 << 64),
               dict(jitter=[ONE + 1, 0, 0, 0, 0]), dict(jitter=[-1, 0, 0, 0, 0]), dict(jitter=[ONE, ONE + 1, 0, 0, 0]), dict(jitter=[ONE, 0, ONE + 1, 0, 0]),
               dict(jitter=[ONE, 0, 0, ONE + 1, 0]), dict(jitter=[ONE, 0, 0, 0, 91]), dict(jitter=[ONE, 0, 0, -1, 0]), dict(jitter=[ONE, 0, 0, 0]),
               dict(jitter=[1.0, 0, 0, 0, 0]),
               dict(blur=(ONE + 1, t)), dict(blur=(-1, t)), dict(blur=(ONE, up)), dict(blur=(ONE, off)), dict(blur=(ONE, t[0])), dict(blur=t),
               dict(blur=(ONE, np.zeros((17, 3), np.uint16))), dict(blur=(ONE, SA.taps_table(0.5, 0.5, 1, 1)[:, :1])),
               dict(blur=(ONE, np.concatenate([t, np.zeros((2, 6), np.uint16)], 1)))):
        with pytest.raises(ValueError):
            SA.augment_numpy(img, **{**ok, **kw})
    with pytest.raises(ValueError):
        SA.augment_numpy(np.zeros((1, 2, 6, 3), np.uint8), **ok)                             # H <= R
    with pytest.raises(ValueError):
        SA.augment_numpy(np.zeros((1, 6, 6), np.uint8), **ok)
    with pytest.raises(ValueError):
        SA.augment_numpy(img.astype(np.float32), **ok)
