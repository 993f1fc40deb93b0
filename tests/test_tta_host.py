"""Host side of multi-scale / flip prediction (fcn8s_tensorflow_amd/tta.py): the pass-shape rule, argument validation and the float64
composition the GPU tests compare against, checked here against a brute-force per-pixel loop and torch's F.interpolate."""
import math

import numpy as np
import pytest

from fcn8s_tensorflow_amd import tta


def test_pass_shape_rule():
    assert tta.pass_shape(64, 96, 1.0) == (64, 96, 64, 96)
    assert tta.pass_shape(50, 70, 1.0) == (50, 70, 64, 96)
    assert tta.pass_shape(375, 1242, 1.0) == (375, 1242, 384, 1248)
    assert tta.pass_shape(375, 1242, 0.5) == (188, 621, 192, 640)        # floor(187.5 + 0.5) = 188
    assert tta.pass_shape(37, 53, 0.75) == (28, 40, 32, 64)              # 27.75 -> 28, 39.75 -> 40
    assert tta.pass_shape(37, 53, 1.5) == (56, 80, 64, 96)               # 55.5 -> 56, 79.5 -> 80
    assert tta.pass_shape(1024, 2048, 1.25) == (1280, 2560, 1280, 2560)
    assert tta.pass_shape(1, 1, 1.0) == (1, 1, 32, 32)
    assert tta.pass_shape(1, 1, 0.1) == (1, 1, 32, 32)                   # never below one pixel
    assert tta.pass_shape(1, 1, 4.0) == (4, 4, 32, 32)
    assert tta.pass_shape(33, 31, 4.0) == (132, 124, 160, 128)


def test_passes_order_and_identity():
    ps = tta.passes(50, 70, (0.5, 1.0), flip=True)
    assert [(p[0], p[1]) for p in ps] == [(0.5, False), (0.5, True), (1.0, False), (1.0, True)]
    assert ps[0][2:] == (25, 35, 32, 64)
    assert tta.is_identity(64, 96, (1.0,))
    assert not tta.is_identity(64, 96, (1.0,), flip=True)
    assert not tta.is_identity(50, 70, (1.0,))
    assert not tta.is_identity(64, 96, (1.0, 1.0))
    assert tta.resizes(64, 96, (0.5,)) and not tta.resizes(50, 70, (1.0,))


@pytest.mark.parametrize("bad", [(), [1.0] * 9, (0.0,), (-1.0,), (4.5,), (float("nan"),), (float("inf"),), (1.0, 0.0), "abc", 3.0])
def test_validation_rejects(bad):
    with pytest.raises(ValueError):
        tta.validate(bad)


def test_validation_accepts_and_rounds_to_float32():
    assert tta.validate((0.5, 1.0, 4.0)) == (0.5, 1.0, 4.0)
    assert tta.validate([1.1])[0] == float(np.float32(1.1))
    assert len(tta.validate([1.0] * 8)) == 8


def _brute_force(pass_logits, flips, H, W):
    """Per output pixel, per pass: the four half-pixel taps of the un-mirrored logits, softmax, mean -- written as plain loops."""
    N, C = pass_logits[0].shape[0], pass_logits[0].shape[3]
    out = np.zeros((N, H, W, C))
    for lg, f in zip(pass_logits, flips):
        Hs, Ws = lg.shape[1:3]
        for n in range(N):
            for y in range(H):
                ry = max((y + 0.5) * Hs / H - 0.5, 0.0)
                y0 = min(int(math.floor(ry)), Hs - 1); y1 = min(y0 + 1, Hs - 1); wy = ry - y0
                for x in range(W):
                    rx = max((x + 0.5) * Ws / W - 0.5, 0.0)
                    x0 = min(int(math.floor(rx)), Ws - 1); x1 = min(x0 + 1, Ws - 1); wx = rx - x0
                    col = (lambda c: Ws - 1 - c) if f else (lambda c: c)
                    v = ((1 - wy) * ((1 - wx) * lg[n, y0, col(x0)] + wx * lg[n, y0, col(x1)])
                         + wy * ((1 - wx) * lg[n, y1, col(x0)] + wx * lg[n, y1, col(x1)]))
                    e = np.exp(v - v.max())
                    out[n, y, x] += e / e.sum()
    return out / len(pass_logits)


def test_composition_against_brute_force():
    rng = np.random.default_rng(0)
    H, W, C = 7, 9, 5
    shapes = [(4, 5), (4, 5), (7, 9), (11, 13)]
    flips = [False, True, False, True]
    lgs = [rng.normal(0, 3, (2, h, w, C)) for h, w in shapes]
    got = tta.compose(lgs, flips, H, W)
    ref = _brute_force(lgs, flips, H, W)
    assert got.shape == (2, H, W, C)
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-12)
    np.testing.assert_allclose(got.sum(-1), 1.0, atol=1e-12)


def test_resize_matches_torch_interpolate():
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(1)
    for (h, w), (H, W) in [((5, 7), (11, 3)), ((16, 16), (16, 16)), ((9, 4), (3, 8)), ((1, 1), (4, 5))]:
        x = rng.normal(size=(2, h, w, 3))
        ref = torch.nn.functional.interpolate(torch.from_numpy(x).permute(0, 3, 1, 2), size=(H, W), mode="bilinear",
                                              align_corners=False).permute(0, 2, 3, 1).numpy()
        np.testing.assert_allclose(tta.resize_bilinear(x, H, W), ref, rtol=0, atol=1e-12)
