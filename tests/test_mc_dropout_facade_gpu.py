"""FCN8s.predict_uncertainty: the engine's Monte-Carlo dropout triple for host and device inputs, and inside averaged_weights() the
result of a model that was loaded with the averaged weights."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SMALL = (8, 16, 32, 64, 64, 128, 128)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def model():
    from fcn8s_tensorflow_amd.fcn8s import FCN8s
    m = FCN8s(vgg16_dir='synthetic:3', num_classes=19, widths=SMALL)
    m.engine.set_option("deterministic", 1)
    return m


def images(n, h, w, seed=3):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def test_predict_uncertainty_is_the_engines_triple_for_host_and_device_inputs():
    import torch
    m = model()
    img = images(2, 64, 96)
    pred, ent, mi = m.predict_uncertainty(img, samples=4, keep_prob=0.5)
    want = m.engine.predict_mc(img, samples=4, keep_prob=0.5, sample_offset=0, argmax=True, entropy=True, mutual_information=True)
    assert pred.dtype == np.int64 and pred.shape == (2, 64, 96) and ent.dtype == np.float32 and mi.shape == (2, 64, 96)
    for u, v in zip((pred, ent, mi), want):
        assert same_bits(u, v)
    assert pred.max() < 19 and (mi >= 0).all() and (mi <= ent + 1e-5).all() and ent.max() <= np.log(19) + 1e-5 and mi.max() > 0
    # a list of HWC arrays, as `predict` takes
    again = m.predict_uncertainty([img[0], img[1]], samples=4, keep_prob=0.5)
    for u, v in zip((pred, ent, mi), again):
        assert same_bits(u, v)
    # the mean softmax: the 19 logical classes, its argmax is the prediction; another offset, other samples
    sm, ent2, mi2 = m.predict_uncertainty(img, samples=4, keep_prob=0.5, argmax=False)
    assert sm.shape == (2, 64, 96, 19) and same_bits(np.argmax(sm, -1).astype(np.int64), pred) and same_bits(ent2, ent) and same_bits(mi2, mi)
    assert np.abs(sm.sum(-1) - 1).max() < 1e-5
    other = m.predict_uncertainty(img, samples=4, keep_prob=0.5, argmax=False, sample_offset=4)
    assert not same_bits(other[0], sm)
    # device in, device out
    d = m.predict_uncertainty(torch.from_numpy(img).cuda(), samples=4, keep_prob=0.5, argmax=False)
    for u, v in zip((sm, ent, mi), d):
        assert v.is_cuda and same_bits(u, v.cpu().numpy())
    # images of any size
    p, e2, _ = m.predict_uncertainty(images(1, 40, 72), samples=2)
    assert p.shape == (1, 40, 72) and e2.shape == (1, 40, 72)
    with pytest.raises(ValueError):
        m.predict_uncertainty(img, samples=0)
    m.close()


def test_predict_uncertainty_inside_averaged_weights():
    m = model()
    rng = np.random.default_rng(90)
    batch = (rng.integers(0, 256, (2, 64, 64, 3), dtype=np.uint8), rng.integers(0, 19, (2, 64, 64), dtype=np.uint8))
    m.engine.set_ema(0.5, warmup=False)
    for _ in range(3):
        m.engine.train_step(batch[0], batch[1], 1e-3, keep_prob=0.5)
    img = images(2, 64, 96)
    raw = m.predict_uncertainty(img, samples=3, argmax=False)
    with m.averaged_weights():
        avg = m.predict_uncertainty(img, samples=3, argmax=False)
    after = m.predict_uncertainty(img, samples=3, argmax=False)
    assert not same_bits(avg[0], raw[0])
    for u, v in zip(raw, after):
        assert same_bits(u, v)                       # the raw weights are live again
    # a model loaded with the averaged weights
    shadow = m.engine.get_ema()
    other = model()
    other.engine.flat_params.copy_(other.engine.torch.from_numpy(shadow).to(other.engine.flat_params.device))
    other.engine.freeze(False)
    want = other.predict_uncertainty(img, samples=3, argmax=False)
    for u, v in zip(avg, want):
        assert same_bits(u, v)
    m.close(); other.close()
