"""Mean-field CRF refinement of a softmax: parameters, their validation, and the definition restated in NumPy.

The device code is csrc/crf.hip behind fcn8s_predict_crf / fcn8s_op_crf_meanfield; the definition is written out in
include/fcn8s_hip.h at fcn8s_crf_params.  `meanfield` below restates it with whole-array shifts, in float64 (the yardstick
of the tests) or in float32 (the same expressions in the device's number format: the yardstick for rounding).  No torch,
no device.

The defaults are a starting point in the usual range of the dense-CRF literature; their effect on a trained model's
mean IoU has not been measured.
"""
from __future__ import annotations

import math

import numpy as np

FLT_MIN = 1.17549435e-38
FIELDS = ("iterations", "radius", "dilation", "w_appearance", "w_smooth", "theta_alpha", "theta_beta", "theta_gamma")
DEFAULTS = dict(iterations=5, radius=3, dilation=1, w_appearance=4.0, w_smooth=2.0, theta_alpha=8.0, theta_beta=13.0, theta_gamma=3.0)
_INT_RANGES = dict(iterations=(0, 32), radius=(1, 7), dilation=(1, 8))


class Params:
    """The fields of fcn8s_crf_params with their defaults; Params(radius=5) overrides one."""
    __slots__ = FIELDS

    def __init__(self, **kw):
        unknown = sorted(set(kw) - set(FIELDS))
        if unknown:
            raise ValueError("unknown CRF parameter(s) %s; the fields are %s" % (", ".join(unknown), ", ".join(FIELDS)))
        for k in FIELDS:
            setattr(self, k, kw.get(k, DEFAULTS[k]))

    def as_dict(self):
        return {k: getattr(self, k) for k in FIELDS}

    def __repr__(self):
        return "crf.Params(%s)" % ", ".join("%s=%r" % kv for kv in self.as_dict().items())

    def __eq__(self, other):
        return isinstance(other, Params) and self.as_dict() == other.as_dict()


def resolve(crf):
    """The `crf=` argument of the prediction calls: None / False -> None (no CRF), True -> the defaults, a dict overrides fields,
    a Params is taken as it is.  The result is validated."""
    if crf is None or crf is False:
        return None
    if crf is True:
        p = Params()
    elif isinstance(crf, Params):
        p = crf
    elif isinstance(crf, dict):
        p = Params(**crf)
    else:
        raise ValueError("crf must be None, a bool, a dict of fields or a crf.Params, not %r" % type(crf).__name__)
    return validate(p)


def validate(params):
    """ValueError for every value the library rejects (FCN8S_ERR_BAD_ARG); returns a Params with ints and floats of the C struct's types."""
    p = params if isinstance(params, Params) else Params(**dict(params))
    out = Params()
    for k, (lo, hi) in _INT_RANGES.items():
        v = getattr(p, k)
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
            raise ValueError("crf %s must be an integer in %d..%d, got %r" % (k, lo, hi, v))
        setattr(out, k, int(v))
    for k in ("w_appearance", "w_smooth", "theta_alpha", "theta_beta", "theta_gamma"):
        v = getattr(p, k)
        try:
            f = float(np.float32(v))                  # as the C ABI receives it
        except (TypeError, ValueError):
            raise ValueError("crf %s must be a number, got %r" % (k, v))
        if isinstance(v, bool) or not math.isfinite(f):
            raise ValueError("crf %s must be finite, got %r" % (k, v))
        if k.startswith("w_") and not f >= 0.0:
            raise ValueError("crf %s must be >= 0, got %r" % (k, v))
        if k.startswith("theta_") and not f > 0.0:
            raise ValueError("crf %s must be > 0, got %r" % (k, v))
        setattr(out, k, f)
    return out


def _offsets(r, d):
    return [(ty * d, tx * d) for ty in range(-r, r + 1) for tx in range(-r, r + 1) if (ty, tx) != (0, 0)]


def _views(H, W, dy, dx):
    """slices (dst rows, dst cols, src rows, src cols) of the pixels i whose neighbour i + (dy, dx) lies inside the image; None if there are none"""
    y0, y1 = max(0, -dy), min(H, H - dy)
    x0, x1 = max(0, -dx), min(W, W - dx)
    if y0 >= y1 or x0 >= x1:
        return None
    return slice(y0, y1), slice(x0, x1), slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx)


def meanfield(prob, images, params=None, dtype=np.float64):
    """Q^T of the definition for prob [..., H, W, C] (float32) and uint8 images [..., H, W, 3]; computed in `dtype`, returned in it.
    iterations = 0 returns `prob` itself."""
    p = validate(params if params is not None else Params())
    prob = np.asarray(prob)
    images = np.asarray(images)
    if images.dtype != np.uint8 or images.shape != prob.shape[:-1] + (3,):
        raise ValueError("images must be uint8 of shape %s, got %s %s" % (prob.shape[:-1] + (3,), images.dtype, images.shape))
    if p.iterations == 0:
        return prob
    if prob.ndim > 3:
        return np.stack([meanfield(prob[i], images[i], p, dtype) for i in range(prob.shape[0])])
    f = np.dtype(dtype).type
    H, W, _ = prob.shape
    ia = f(1) / (f(2) * f(np.float32(p.theta_alpha)) * f(np.float32(p.theta_alpha)))
    ib = f(1) / (f(2) * f(np.float32(p.theta_beta)) * f(np.float32(p.theta_beta)))
    ig = f(1) / (f(2) * f(np.float32(p.theta_gamma)) * f(np.float32(p.theta_gamma)))
    wa, ws = f(np.float32(p.w_appearance)), f(np.float32(p.w_smooth))
    I = images.astype(np.int64)
    # per tap: the pixels it reaches, its appearance weights k (an [h, w] array) and its two position-only scalars
    taps = []
    den_a = np.zeros((H, W), dtype)
    den_g = np.zeros((H, W), dtype)
    for dy, dx in _offsets(p.radius, p.dilation):
        v = _views(H, W, dy, dx)
        if v is None:
            continue
        ys, xs, yn, xn = v
        s2 = f(dy * dy + dx * dx)
        c2 = ((I[ys, xs] - I[yn, xn]) ** 2).sum(-1).astype(dtype)
        a = np.exp(-(s2 * ia))
        g = np.exp(-(s2 * ig))
        k = np.exp(-(s2 * ia) - c2 * ib)
        den_a[ys, xs] += a
        den_g[ys, xs] += g
        taps.append((v, k.astype(dtype), f(g)))
    U = np.log(np.maximum(prob.astype(dtype), f(FLT_MIN)))
    Q = prob.astype(dtype)
    some = den_a > 0
    for _ in range(p.iterations):
        num_k = np.zeros_like(Q)
        num_g = np.zeros_like(Q)
        for (ys, xs, yn, xn), k, g in taps:
            Qn = Q[yn, xn]
            num_k[ys, xs] += k[..., None] * Qn
            num_g[ys, xs] += g * Qn
        m = np.zeros_like(Q)
        m[some] = wa * num_k[some] / den_a[some][:, None] + ws * num_g[some] / den_g[some][:, None]
        x = U + m
        x = np.exp(x - x.max(-1, keepdims=True))
        Q = (x / x.sum(-1, keepdims=True)).astype(dtype)
    return Q


def synthetic_scene(H, W, C, seed=0, cell=16, shift=3, noise=12.0):
    """A seeded input with structure for tests and tools/crf_bench.py (uniform noise gives the CRF almost nothing to do): labels constant
    on cell x cell squares, image = one random palette colour per label + N(0, noise) clipped to uint8, logits = 1.5 N(0, 1) + 3 on the
    class of the label map shifted `shift` pixels sideways.  Returns (prob float32 [H,W,C], image uint8 [H,W,3], labels int64 [H,W])."""
    rng = np.random.default_rng(seed)
    cells = rng.integers(0, C, ((H + cell - 1) // cell, (W + cell - 1) // cell))
    labels = np.repeat(np.repeat(cells, cell, 0), cell, 1)[:H, :W].astype(np.int64)
    palette = rng.integers(0, 256, (C, 3)).astype(np.float64)
    image = np.clip(np.rint(palette[labels] + rng.normal(0.0, noise, (H, W, 3))), 0, 255).astype(np.uint8)
    shifted = np.roll(labels, shift, axis=1)
    logits = 1.5 * rng.normal(0.0, 1.0, (H, W, C))
    logits[np.arange(H)[:, None], np.arange(W)[None, :], shifted] += 3.0
    logits = logits.astype(np.float32)
    e = np.exp(logits - logits.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(np.float32), image, labels
