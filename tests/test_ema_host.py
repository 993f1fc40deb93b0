"""The parameter average's host side (fcn8s_tensorflow_amd/optim.py, tf_bundle.py): the decay schedule against hand values, the float64
restatement of the update, the validation, and the names the shadow tensors travel under in a TensorFlow bundle.  No GPU."""
import numpy as np
import pytest

from fcn8s_tensorflow_amd import optim, tf_bundle


def test_decay_schedule_hand_values():
    # TensorFlow's num_updates rule: min(decay, (1 + t) / (10 + t))
    assert optim.ema_decay_at(0.999, 1, True) == 2.0 / 11.0
    assert optim.ema_decay_at(0.999, 2, True) == 3.0 / 12.0
    assert optim.ema_decay_at(0.999, 90, True) == 91.0 / 100.0
    assert optim.ema_decay_at(0.5, 1, True) == 2.0 / 11.0           # the ramp is still below 0.5 ...
    assert optim.ema_decay_at(0.5, 8, True) == 0.5                  # ... 9 / 18 reaches it
    assert optim.ema_decay_at(0.5, 1000, True) == 0.5
    assert optim.ema_decay_at(0.999, 8000, True) == 8001.0 / 8010.0 < 0.999
    assert optim.ema_decay_at(0.999, 8991, True) == 0.999           # 8992 / 9001 > 0.999
    for t in (1, 2, 1000):
        assert optim.ema_decay_at(0.999, t, False) == 0.999
    # omega is the float32 the device multiplies by
    w = optim.ema_omega(0.999, 1, True)
    assert w.dtype == np.float32 and w == np.float32(9.0 / 11.0)
    assert optim.ema_omega(0.999, 1, False) == np.float32(1.0 - 0.999)


def test_ema_step_is_float64():
    s = np.array([1.0, -2.0, 1e-6, 1e3], np.float32)
    th = np.array([0.5, -2.0, -1e-6, 999.0], np.float32)
    w = np.float32(0.1)
    out = optim.ema_step(s, th, w)
    assert out.dtype == np.float64
    want = s.astype(np.float64) - float(w) * (s.astype(np.float64) - th.astype(np.float64))
    assert np.array_equal(out, want)
    assert out[1] == -2.0                                            # s == theta stays put exactly
    assert np.array_equal(optim.ema_step(s, th, 1.0), th.astype(np.float64))      # w = 1: the parameters
    assert np.array_equal(optim.ema_step(s, th, 0.0), s.astype(np.float64))       # w = 0: the shadow
    # the recursion over four steps with warm-up, by hand
    x = 1.0
    thetas = (2.0, 3.0, 4.0, 5.0)
    acc = np.float64(x)
    for t, th_t in enumerate(thetas, 1):
        acc = optim.ema_step(acc, th_t, optim.ema_omega(0.999, t, True))
        x = x - float(np.float32(1.0 - min(0.999, (1.0 + t) / (10.0 + t)))) * (x - th_t)
    assert float(acc) == x


@pytest.mark.parametrize("bad", [float("nan"), -0.1, 1.0, 1.5, "x", True, float("inf")])
def test_validate_ema_refuses(bad):
    with pytest.raises(ValueError):
        optim.validate_ema(bad)


def test_validate_ema_accepts():
    assert optim.validate_ema(None) == (0.0, True)
    assert optim.validate_ema(0) == (0.0, True)
    assert optim.validate_ema(0.999, False) == (0.999, False)
    assert optim.validate_ema(np.float64(0.5), 1) == (0.5, True)


def test_tf_suffix_and_bundle_round_trip(tmp_path):
    assert tf_bundle.EMA_SUFFIX == "/ExponentialMovingAverage"
    rng = np.random.default_rng(0)
    names = ("conv1_1/filter", "conv1_1/biases", "fc7_pool4_pool3_conv2d_trans/bias")
    tensors = {}
    for k, shape in zip(names, ((3, 3, 3, 8), (8,), (19,))):
        tensors[k] = rng.standard_normal(shape).astype(np.float32)
        tensors[k + tf_bundle.EMA_SUFFIX] = rng.standard_normal(shape).astype(np.float32)
    prefix = str(tmp_path / "variables")
    tf_bundle.write_bundle(prefix, tensors)
    back = tf_bundle.read_bundle(prefix)
    for k in names:
        name = k + "/ExponentialMovingAverage"
        assert name in back
        assert np.array_equal(back[name], tensors[name]) and back[name].shape == tensors[name].shape
        assert np.array_equal(back[k], tensors[k])
