"""The NumPy restatement of the mean-field CRF (fcn8s_tensorflow_amd/crf.py) is the yardstick of the device kernel, so it is pinned here
first: against an independent per-pixel, per-tap transcription of the definition in include/fcn8s_hip.h, and by the identities the
definition implies (normalisation, mirrors, class permutations, dilation = sub-images, tiny images).  No GPU."""
import math

import numpy as np
import pytest

from fcn8s_tensorflow_amd import crf

FLT_MIN = 1.17549435e-38


def scene(H, W, C, seed=0):
    p, img, _ = crf.synthetic_scene(H, W, C, seed=seed, cell=4)
    return p, img


def loops(P, I, iterations, radius, dilation, w_appearance, w_smooth, theta_alpha, theta_beta, theta_gamma):
    """the definition, one pixel and one tap at a time (float64; thetas and weights as float32)"""
    H, W, C = P.shape
    ta, tb, tg = (float(np.float32(t)) for t in (theta_alpha, theta_beta, theta_gamma))
    wa, ws = float(np.float32(w_appearance)), float(np.float32(w_smooth))
    Q = [[[float(P[y, x, l]) for l in range(C)] for x in range(W)] for y in range(H)]
    U = [[[math.log(max(float(P[y, x, l]), FLT_MIN)) for l in range(C)] for x in range(W)] for y in range(H)]
    for _ in range(iterations):
        Qn = [[None] * W for _ in range(H)]
        for y in range(H):
            for x in range(W):
                mk = [0.0] * C; mg = [0.0] * C; sa = 0.0; sg = 0.0
                for ty in range(-radius, radius + 1):
                    for tx in range(-radius, radius + 1):
                        dy, dx = ty * dilation, tx * dilation
                        yy, xx = y + dy, x + dx
                        if (dy == 0 and dx == 0) or yy < 0 or yy >= H or xx < 0 or xx >= W:
                            continue
                        s2 = dy * dy + dx * dx
                        c2 = sum((int(I[y, x, c]) - int(I[yy, xx, c])) ** 2 for c in range(3))
                        a = math.exp(-s2 / (2 * ta * ta))
                        k = math.exp(-s2 / (2 * ta * ta) - c2 / (2 * tb * tb))
                        g = math.exp(-s2 / (2 * tg * tg))
                        sa += a; sg += g
                        for l in range(C):
                            mk[l] += k * Q[yy][xx][l]; mg[l] += g * Q[yy][xx][l]
                z = [U[y][x][l] + ((wa * mk[l] / sa + ws * mg[l] / sg) if sa > 0 else 0.0) for l in range(C)]
                mx = max(z)
                e = [math.exp(v - mx) for v in z]
                s = sum(e)
                Qn[y][x] = [v / s for v in e]
        Q = Qn
    return np.array(Q)


@pytest.mark.parametrize("d", [1, 2])
def test_restatement_equals_the_per_tap_loops(d):
    P, I = scene(9, 11, 4, seed=d)
    kw = dict(iterations=2, radius=2, dilation=d, w_appearance=4.0, w_smooth=2.0, theta_alpha=8.0, theta_beta=13.0, theta_gamma=3.0)
    got = crf.meanfield(P, I, crf.Params(**kw))
    assert got.dtype == np.float64
    assert np.abs(got - loops(P, I, **kw)).max() <= 1e-12
    # ... and with other weights and thetas, radius 1
    kw = dict(iterations=3, radius=1, dilation=d, w_appearance=10.0, w_smooth=0.5, theta_alpha=2.5, theta_beta=30.0, theta_gamma=1.25)
    assert np.abs(crf.meanfield(P, I, kw) - loops(P, I, **kw)).max() <= 1e-12


def test_rows_sum_to_one_and_zero_iterations_returns_p_itself():
    P, I = scene(20, 17, 8)
    q = crf.meanfield(P, I, crf.Params(iterations=3))
    assert np.abs(q.sum(-1) - 1).max() <= 1e-12 and (q >= 0).all()
    assert crf.meanfield(P, I, crf.Params(iterations=0)) is P
    q32 = crf.meanfield(P, I, crf.Params(iterations=3), dtype=np.float32)
    assert q32.dtype == np.float32 and np.abs(q32 - q).max() < 1e-5


def test_zero_weights_return_the_normalised_p():
    P, I = scene(12, 13, 8)
    q = crf.meanfield(P, I, crf.Params(iterations=4, w_appearance=0.0, w_smooth=0.0))
    P64 = P.astype(np.float64)
    assert np.abs(q - P64 / P64.sum(-1, keepdims=True)).max() <= 1e-12


def test_batches_are_independent_images():
    a, ia = scene(10, 12, 4, seed=1)
    b, ib = scene(10, 12, 4, seed=2)
    q = crf.meanfield(np.stack([a, b]), np.stack([ia, ib]))
    assert np.array_equal(q[0], crf.meanfield(a, ia)) and np.array_equal(q[1], crf.meanfield(b, ib))


def test_mirrors_and_class_permutations_commute():
    P, I = scene(13, 18, 8, seed=3)
    p = crf.Params(iterations=3, radius=2, dilation=2)
    q = crf.meanfield(P, I, p)
    lr = crf.meanfield(np.ascontiguousarray(P[:, ::-1]), np.ascontiguousarray(I[:, ::-1]), p)
    assert np.abs(lr[:, ::-1] - q).max() <= 1e-12
    tb = crf.meanfield(np.ascontiguousarray(P[::-1]), np.ascontiguousarray(I[::-1]), p)
    assert np.abs(tb[::-1] - q).max() <= 1e-12
    perm = np.random.default_rng(0).permutation(8)
    assert np.abs(crf.meanfield(np.ascontiguousarray(P[..., perm]), I, p) - q[..., perm]).max() <= 1e-12


@pytest.mark.parametrize("d,H,W", [(2, 14, 17), (3, 16, 20), (2, 12, 12), (3, 13, 11)])
def test_dilation_is_dilation_one_on_the_sub_images(d, H, W):
    """theta_alpha = 6, theta_gamma = 3: their quotients by 2 and 3 are exact in float32"""
    P, I = scene(H, W, 4, seed=d)
    q = crf.meanfield(P, I, crf.Params(iterations=3, radius=2, dilation=d, theta_alpha=6.0, theta_gamma=3.0))
    sub = crf.Params(iterations=3, radius=2, dilation=1, theta_alpha=6.0 / d, theta_gamma=3.0 / d)
    for y0 in range(d):
        for x0 in range(d):
            qs = crf.meanfield(np.ascontiguousarray(P[y0::d, x0::d]), np.ascontiguousarray(I[y0::d, x0::d]), sub)
            assert np.abs(qs - q[y0::d, x0::d]).max() <= 1e-12


def test_images_smaller_than_the_window():
    P, I = scene(5, 7, 4, seed=5)
    kw = dict(iterations=2, radius=3, dilation=2, w_appearance=4.0, w_smooth=2.0, theta_alpha=8.0, theta_beta=13.0, theta_gamma=3.0)
    assert np.abs(crf.meanfield(P, I, kw) - loops(P, I, **kw)).max() <= 1e-12
    # no neighbour inside the image at all: m = 0, Q = P / sum P
    for shape, d in (((1, 1), 1), ((1, 9), 8)):
        P, I = scene(shape[0], shape[1], 4, seed=6)
        q = crf.meanfield(P, I, crf.Params(iterations=3, radius=1, dilation=d))
        kw = dict(crf.Params(iterations=3, radius=1, dilation=d).as_dict())
        assert np.abs(q - loops(P, I, **kw)).max() <= 1e-12
        if shape == (1, 1):
            P64 = P.astype(np.float64)
            assert np.abs(q - P64 / P64.sum(-1, keepdims=True)).max() <= 1e-12
    # 1 x 9 at d = 8: only the two end pixels see each other
    P, I = scene(1, 9, 4, seed=7)
    q = crf.meanfield(P, I, crf.Params(iterations=1, radius=1, dilation=8))
    P64 = P.astype(np.float64)
    assert np.abs(q[0, 1:8] - (P64 / P64.sum(-1, keepdims=True))[0, 1:8]).max() <= 1e-12
    assert np.abs(q[0, 0] - (P64 / P64.sum(-1, keepdims=True))[0, 0]).max() > 1e-6


BAD = [("iterations", -1), ("iterations", 33), ("iterations", 2.5), ("iterations", float("nan")), ("radius", 0), ("radius", 8),
       ("dilation", 0), ("dilation", 9), ("w_appearance", -0.1), ("w_appearance", float("nan")), ("w_appearance", float("inf")),
       ("w_smooth", -1.0), ("w_smooth", float("nan")), ("w_smooth", float("inf")), ("theta_alpha", 0.0), ("theta_alpha", -1.0),
       ("theta_alpha", float("nan")), ("theta_alpha", float("inf")), ("theta_beta", 0.0), ("theta_beta", float("nan")),
       ("theta_beta", float("inf")), ("theta_gamma", 0.0), ("theta_gamma", float("nan")), ("theta_gamma", float("inf")),
       ("theta_gamma", "wide")]


@pytest.mark.parametrize("field,value", BAD)
def test_validate_rejects(field, value):
    with pytest.raises(ValueError, match=field):
        crf.validate(crf.Params(**{field: value}))
    with pytest.raises(ValueError, match=field):
        crf.resolve({field: value})


def test_params_defaults_and_resolve():
    p = crf.Params()
    assert p.as_dict() == dict(iterations=5, radius=3, dilation=1, w_appearance=4.0, w_smooth=2.0, theta_alpha=8.0, theta_beta=13.0, theta_gamma=3.0)
    assert crf.resolve(None) is None and crf.resolve(False) is None
    assert crf.resolve(True) == p and crf.resolve({}) == p
    assert crf.resolve(dict(radius=5)).radius == 5 and crf.resolve(crf.Params(dilation=2)).dilation == 2
    # the ranges' ends are accepted
    crf.validate(crf.Params(iterations=0, radius=1, dilation=1, w_appearance=0.0, w_smooth=0.0))
    crf.validate(crf.Params(iterations=32, radius=7, dilation=8))
    with pytest.raises(ValueError, match="sigma"):
        crf.Params(sigma=1.0)
    with pytest.raises(ValueError):
        crf.resolve(3)


def test_the_generator_gives_the_crf_something_to_do():
    """the share of pixels whose argmax the float64 restatement changes, and the agreement with the label map the logits came from"""
    for H, W, C, r, d, T, wa, ws in [(96, 128, 20, 3, 1, 5, 4, 2), (64, 64, 4, 5, 1, 5, 10, 3)]:
        P, I, lab = crf.synthetic_scene(H, W, C, seed=1)
        q = crf.meanfield(P, I, crf.Params(iterations=T, radius=r, dilation=d, w_appearance=wa, w_smooth=ws))
        changed = (q.argmax(-1) != P.argmax(-1)).mean()
        before, after = (P.argmax(-1) == lab).mean(), (q.argmax(-1) == lab).mean()
        assert changed > 0.10 and after > before + 0.10, (changed, before, after)
