"""Monte-Carlo dropout inference, host side (fcn8s_tensorflow_amd/mc_dropout.py): what `validate` refuses, the counter streams of
`stream_ids` against training's, and the properties of `restate`, the definition the GPU tests compare against."""
import numpy as np
import pytest

from fcn8s_tensorflow_amd import mc_dropout as mc


def test_validate_accepts_the_range_and_returns_plain_types():
    assert mc.validate(20, 0.5, 0) == (20, 0.5, 0)
    assert mc.validate(1, 1.0, (1 << 30) - 1) == (1, 1.0, (1 << 30) - 1)
    assert mc.validate(np.int64(256), np.float32(0.25), np.int32(7)) == (256, 0.25, 7)


@pytest.mark.parametrize("args", [(0, 0.5, 0), (257, 0.5, 0), (-1, 0.5, 0),
                                  (4, 0.0, 0), (4, -0.1, 0), (4, 1.5, 0), (4, float("nan"), 0),
                                  (4, 0.5, -1), (4, 0.5, (1 << 30) - 3), (1, 0.5, 1 << 30)])
def test_validate_refuses(args):
    with pytest.raises(ValueError):
        mc.validate(*args)


@pytest.mark.parametrize("args", [(2.0, 0.5, 0), (True, 0.5, 0), (4, 0.5, 1.0), ("4", 0.5, 0)])
def test_validate_refuses_non_integers(args):
    with pytest.raises(TypeError):
        mc.validate(*args)


def test_stream_ids_are_disjoint_from_training_and_injective():
    # training: streams 2 step and 2 step + 1, step < 2^30, i.e. every id below 2^31; Monte-Carlo samples: everything from 2^31 on
    top_training = 2 * ((1 << 30) - 1) + 1
    assert top_training < mc.STREAM_BASE
    ks = [0, 1, 2, 3, 255, 256, 12345, (1 << 29), (1 << 30) - 2, (1 << 30) - 1]
    seen = set()
    for k in ks:
        a, b = mc.stream_ids(k, 0)
        assert (a, b) == mc.stream_ids(0, k) == mc.stream_ids(k // 2, k - k // 2)      # a function of offset + s alone
        assert b == a + 1 and a == 0x80000000 + 2 * k
        assert top_training < a and b <= 0xFFFFFFFF                                      # above every training stream, still 32-bit
        assert a not in seen and b not in seen
        seen.update((a, b))
    # injective in (offset + s): a and b are strictly increasing in it, and even / odd
    a = np.array([mc.stream_ids(0, k)[0] for k in range(0, 4096)], np.int64)
    assert (np.diff(a) == 2).all() and (a % 2 == 0).all()
    for bad in (-1, 1 << 30):
        with pytest.raises(ValueError):
            mc.stream_ids(bad, 0)


def test_restate_identical_samples_have_no_mutual_information():
    rng = np.random.default_rng(0)
    one = rng.normal(0, 3, (1, 4, 5, 7)).astype(np.float32)
    for S in (1, 2, 4, 5):
        for dt in (np.float64, np.float32):
            mean, ent, mi, am = mc.restate(np.repeat(one, S, 0), dtype=dt)
            assert mean.dtype == dt and ent.dtype == dt and mi.dtype == dt and am.dtype == np.int64
            assert np.abs(mi).max() <= (1e-12 if dt == np.float64 else 1e-6)
            m1, e1, _, a1 = mc.restate(one, dtype=dt)
            assert np.allclose(mean, m1, atol=1e-6) and np.allclose(ent, e1, atol=1e-6) and (am == a1).all()
    # ... exactly none in the device's order at S = 1, 2, 4 (sums of equal terms are exact there)
    for S in (1, 2, 4):
        assert (mc.restate(np.repeat(one, S, 0), dtype=np.float32)[2] == 0).all()


@pytest.mark.parametrize("C", [2, 4, 19, 20])
def test_restate_uniform_logits_have_entropy_log_c(C):
    x = np.full((3, 2, 2, C), 1.25, np.float32)
    mean, ent, mi, am = mc.restate(x)
    assert np.allclose(mean, 1.0 / C) and np.allclose(ent, np.log(C), atol=1e-12) and np.allclose(mi, 0, atol=1e-12) and (am == 0).all()


def test_restate_confident_disagreement_is_all_epistemic():
    C, S = 5, 5
    x = np.full((S, 3, C), -40.0, np.float32)
    for s in range(S):
        x[s, :, s] = 40.0                   # every sample is sure, each of another class
    mean, ent, mi, am = mc.restate(x)
    assert np.allclose(mean, 1.0 / S) and np.allclose(ent, np.log(S))
    assert np.allclose(mi, ent, atol=1e-9)
    # two against one: entropy of (2/3, 1/3), still all of it mutual information
    y = np.full((3, 1, 3), -40.0, np.float32); y[0, 0, 0] = y[1, 0, 0] = y[2, 0, 2] = 40.0
    mean, ent, mi, am = mc.restate(y)
    h = -(2 / 3 * np.log(2 / 3) + 1 / 3 * np.log(1 / 3))
    assert np.allclose(ent, h) and np.allclose(mi, h, atol=1e-9) and am[0] == 0


def test_restate_mutual_information_is_bounded_by_entropy_and_argmax_ties_go_low():
    rng = np.random.default_rng(1)
    for scale in (1.0, 30.0):
        x = (rng.normal(0, 1, (6, 8, 9, 20)) * scale).astype(np.float32)
        for dt in (np.float64, np.float32):
            mean, ent, mi, am = mc.restate(x, dtype=dt)
            assert (mi >= 0).all() and (mi <= ent + 1e-6).all() and (ent <= np.log(20) + 1e-6).all()
            assert np.allclose(mean.sum(-1), 1, atol=1e-5)
    t = np.zeros((2, 1, 4), np.float32); t[:, 0, 1] = t[:, 0, 3] = 2.0
    assert mc.restate(t)[3][0] == 1 and mc.restate(t, np.float32)[3][0] == 1


def test_restate_float32_stays_close_to_float64():
    rng = np.random.default_rng(2)
    for scale in (1.0, 30.0):
        x = (rng.normal(0, 1, (8, 16, 16, 20)) * scale).astype(np.float32)
        ref, got = mc.restate(x), mc.restate(x, dtype=np.float32)
        for r, g in zip(ref[:3], got[:3]):
            d = np.abs(g.astype(np.float64) - r).max()
            assert np.isfinite(d) and d < 5e-6, d          # a handful of roundings of numbers <= log 20: a few 1e-7


def test_restate_refuses_a_missing_sample_axis():
    with pytest.raises(ValueError):
        mc.restate(np.zeros((4,), np.float32))
    with pytest.raises(ValueError):
        mc.restate(np.zeros((0, 2, 3), np.float32))
