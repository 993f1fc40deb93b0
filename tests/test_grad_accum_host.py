"""optim.py on the host: the float64 / float32 restatements of the update's global norm, clip, accumulation order and guarded optimizer
steps (include/fcn8s_hip.h, "the update"), and the validation of FCN8s.train's `accumulation_steps` / `clip_global_norm`.  No GPU.

Reference: TensorFlow's tf.clip_by_global_norm for the clip coefficient; the reference itself updates once per batch without a clip
(fcn8s_tensorflow.py:256)."""
import math

import numpy as np
import pytest

from fcn8s_tensorflow_amd import optim

ULP32 = float(np.finfo(np.float32).eps)


def grads(seed=0, n=1237):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 3, n)).astype(np.float32)


def test_global_norm_is_the_float64_sum_rounded_once():
    g = grads()
    want = math.sqrt(sum(float(x) * float(x) for x in g))                # a plain Python float64 loop
    for gs in (1.0, 0.25, -0.5):
        got = optim.global_norm(g, gs)
        assert isinstance(got, np.float32)
        assert abs(float(got) - abs(gs) * want) <= ULP32 * abs(gs) * want          # one rounding to float (0.5 ulp) + the sum's order
    # a dict or a list of tensors is the flat buffer
    parts = {"a": g[:100].reshape(10, 10), "b": g[100:]}
    assert optim.global_norm(parts) == optim.global_norm(g) == optim.global_norm(list(parts.values()))
    assert optim.global_norm(np.zeros(5, np.float32)) == 0.0


def test_clip_matches_a_direct_float64_evaluation():
    g = grads(1)
    for gs in (1.0, 0.5):
        n = float(optim.global_norm(g, gs))
        for mx in (n * 0.5, n * 0.999, n * 1e-3, 1e-3):
            c, s, ok = optim.clip_scale(n, gs, mx)
            mx32 = float(np.float32(mx))
            want = mx32 / max(n, mx32)
            assert ok and isinstance(c, np.float32) and isinstance(s, np.float32)
            assert abs(float(c) - want) <= ULP32 * want                              # one float32 division
            assert abs(float(s) - gs * want) <= 2 * ULP32 * abs(gs * want)          # ... and one multiplication
            assert float(c) < 1.0


def test_a_clip_that_does_not_bite_changes_no_bit():
    g = grads(2)
    for gs in (1.0, 1.0 / 3.0, 0.125):
        n = optim.global_norm(g, gs)
        for mx in (float(n), float(n) * 1.5, 1e30, float("inf")):
            c, s, ok = optim.clip_scale(n, gs, mx)
            assert ok and c == np.float32(1.0)
            assert s.tobytes() == np.float32(gs).tobytes()
    # just above max_norm it bites
    n = np.float32(2.0)
    c, _, _ = optim.clip_scale(np.nextafter(n, np.float32(3.0)), 1.0, 2.0)
    assert c < 1.0
    # off
    c, s, ok = optim.clip_scale(5.0, 0.5, 0.0)
    assert c == 1.0 and s == np.float32(0.5) and ok


def test_accumulation_order_is_left_to_right_in_float32():
    rng = np.random.default_rng(3)
    g1, g2, g3 = (rng.standard_normal(4001).astype(np.float32) * np.float32(10.0 ** k) for k in (0, 3, -3))
    got = optim.accumulate([g1, g2, g3])
    want = np.empty_like(g1)
    for i in range(g1.size):                                             # element by element, each add rounded to float32
        want[i] = np.float32(np.float32(g1[i] + g2[i]) + g3[i])
    assert got.dtype == np.float32 and np.array_equal(got, want)
    assert not np.array_equal(got, optim.accumulate([g3, g2, g1]))        # the order is part of the definition
    assert not np.array_equal(got, (g1.astype(np.float64) + g2 + g3).astype(np.float32))
    single = optim.accumulate([g1])
    assert np.array_equal(single, g1) and single is not g1


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_a_non_finite_gradient_fails_the_guard_and_leaves_the_state(bad):
    g = grads(4, 257)
    for where in (0, 128, 256):
        h = g.copy(); h[where] = bad
        st = optim.update_stats(h, 0.5, 1.0)
        assert st["ok"] is False and not np.isfinite(st["norm"])
        for inf_clip in (1.0, float("inf")):
            _, s, ok = optim.clip_scale(st["norm"], 0.5, inf_clip)
            assert not ok
            th, m, v = g.copy(), g.copy() * 0.1, np.abs(g)
            th2, m2, v2 = optim.adam_step(th, h, m, v, 3, 1e-3, s, ok)
            assert np.array_equal(th2, th) and np.array_equal(m2, m) and np.array_equal(v2, v) and th2 is not th
            th3, b3 = optim.sgd_step(th, h, m, 1e-2, s, ok)
            assert np.array_equal(th3, th) and np.array_equal(b3, m)


def test_guarded_steps_are_the_plain_steps_at_the_clipped_scale():
    from oracle import fcn8s_oracle as orc
    rng = np.random.default_rng(5)
    n = 513
    th = rng.standard_normal(n).astype(np.float32); m = np.zeros(n, np.float32); v = np.zeros(n, np.float32)
    th_o, m_o, v_o = th.copy(), m.copy(), v.copy()
    for t in range(1, 4):
        g = rng.standard_normal(n).astype(np.float32)
        st = optim.update_stats(g, 0.5, 0.25 * float(optim.global_norm(g, 0.5)))
        assert st["ok"] and abs(float(st["clip_coef"]) - 0.25) < 1e-6
        th, m, v = optim.adam_step(th, g, m, v, t, 1e-3, st["scale"], st["ok"])
        th_o, m_o, v_o = orc.tf_adam_step(th_o, g * st["scale"], m_o, v_o, t, 1e-3)          # the oracle's Adam on the pre-scaled gradient
        assert np.abs(th - th_o).max() < 2e-6 and np.abs(m - m_o).max() < 1e-6 and np.abs(v - v_o).max() < 1e-6
    buf = np.zeros(n, np.float32)
    g = rng.standard_normal(n).astype(np.float32)
    th2, buf2 = optim.sgd_step(th, g, buf, 1e-2, np.float32(0.125))
    assert np.array_equal(buf2, g * np.float32(0.125)) and np.array_equal(th2, th - np.float32(1e-2) * buf2)


def test_train_argument_validation():
    assert optim.validate() == (1, 0.0)
    assert optim.validate(4, 1.0) == (4, 1.0)
    assert optim.validate(np.int64(2), float("inf")) == (2, float("inf"))
    for a in (0, -1, 1.5, "2", None, True):
        with pytest.raises(ValueError, match="accumulation_steps"):
            optim.validate(a, None)
    for c in (0, 0.0, -1.0, float("nan"), -float("inf"), "x", True):
        with pytest.raises(ValueError, match="clip_global_norm|max_norm"):
            optim.validate(1, c)
    # the engine's setter: None and 0 switch the clip off, the rest as fcn8s_set_grad_clip
    assert optim.validate_clip(None) == 0.0 and optim.validate_clip(0) == 0.0 and optim.validate_clip(float("inf")) == float("inf")
    for c in (-1e-3, float("nan")):
        with pytest.raises(ValueError):
            optim.validate_clip(c)
