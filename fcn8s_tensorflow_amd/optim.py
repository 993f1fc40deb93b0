"""Gradient accumulation over micro-batches, the global-norm clip and the non-finite guard of the update (fcn8s_accumulate_bucket,
fcn8s_set_grad_clip; definitions in include/fcn8s_hip.h): argument validation shared with the engine and the facade, and NumPy
restatements for the tests -- float64 where the library sums in double, float32 where it rounds to float.

Accumulation: after A micro-batches the gradient buffer holds fl(fl(g1 + g2) + g3) ... (one fp32 add per element and micro-batch);
the caller's grad_scale carries the 1 / A.
Clip: S = sum (double)g_i^2; norm = float32(|grad_scale| sqrt(S)); c = max_norm / max(norm, max_norm) in float32 (c = 1 for
max_norm = inf, or 0 = off); s = float32(grad_scale * c); ok = isfinite(norm).  The optimizer computes g * s where it computes
g * grad_scale without a clip; if not ok it touches neither the parameters nor its slots.

The average (fcn8s_set_ema): a shadow s of the parameters, s = theta when it is first switched on.  After every applied update, with t
the new global step: d_t = min(d, (1 + t) / (10 + t)) with warm-up, else d, in double (tf.train.ExponentialMovingAverage's num_updates
rule); w = float32(1 - d_t); s <- s - w (s - theta) in float32 (assign_moving_average without zero-debias).  A skipped update leaves s
alone, accumulation never touches it, replicas hold the same s.  d in (0, 1); 0 or None = off.
"""
import math

import numpy as np


def validate_clip(max_norm):
    """-> float max_norm as the C ABI receives it (0.0 = off; None means off); ValueError for what fcn8s_set_grad_clip rejects."""
    if max_norm is None:
        return 0.0
    try:
        v = float(np.float32(max_norm))
    except (TypeError, ValueError):
        raise ValueError("the clip's `max_norm` must be a number in (0, inf], 0 or None (off), got {!r}".format(max_norm))
    if isinstance(max_norm, bool) or math.isnan(v) or v < 0.0:
        raise ValueError("the clip's `max_norm` must be in (0, inf], 0 or None (off), got {!r}".format(max_norm))
    return v


def validate(accumulation_steps=1, clip_global_norm=None):
    """The two arguments of FCN8s.train -> (int accumulation_steps >= 1, float max_norm, 0.0 = off).  ValueError otherwise: a
    `clip_global_norm` that is given must be positive (inf allowed: the guard alone)."""
    a = accumulation_steps
    if isinstance(a, bool) or not isinstance(a, (int, np.integer)) or a < 1:
        raise ValueError("`accumulation_steps` must be an integer >= 1, got {!r}".format(a))
    if clip_global_norm is None:
        return int(a), 0.0
    v = validate_clip(clip_global_norm)
    if not v > 0.0:
        raise ValueError("`clip_global_norm` must be positive (inf = guard only) or None, got {!r}".format(clip_global_norm))
    return int(a), v


def validate_ema(ema_decay=None, ema_warmup=True):
    """-> (float decay as the C ABI receives it, 0.0 = off (None means off), bool warmup); ValueError for what fcn8s_set_ema rejects:
    a decay that is not a number, NaN, negative or >= 1."""
    if ema_decay is None:
        return 0.0, bool(ema_warmup)
    try:
        d = float(ema_decay)
    except (TypeError, ValueError):
        raise ValueError("`ema_decay` must be a number in (0, 1), 0 or None (off), got {!r}".format(ema_decay))
    if isinstance(ema_decay, bool) or math.isnan(d) or d < 0.0 or d >= 1.0:
        raise ValueError("`ema_decay` must be in (0, 1), 0 or None (off), got {!r}".format(ema_decay))
    return d, bool(ema_warmup)


def ema_decay_at(decay, t, warmup=True):
    """d_t of the update that makes the global step t (>= 1), in float64: min(decay, (1 + t) / (10 + t)) with warm-up, else decay."""
    d = float(decay)
    return min(d, (1.0 + float(t)) / (10.0 + float(t))) if warmup else d


def ema_omega(decay, t, warmup=True):
    """w = float32(1 - d_t): the weight of the new parameters in the update that makes the global step t."""
    return np.float32(1.0 - ema_decay_at(decay, t, warmup))


def ema_step(s, theta, omega):
    """s - w (s - theta) in float64 with w = float64(float32(omega)) (the device: float32, one subtraction and one fused multiply-add)."""
    s = np.asarray(s, np.float64); theta = np.asarray(theta, np.float64)
    return s - float(np.float32(omega)) * (s - theta)


def _flat(g):
    if isinstance(g, dict):
        g = list(g.values())
    if isinstance(g, (list, tuple)):
        return np.concatenate([np.asarray(a, np.float32).reshape(-1) for a in g]) if g else np.zeros(0, np.float32)
    return np.asarray(g, np.float32).reshape(-1)


def global_norm(g, grad_scale=1.0):
    """float32(|grad_scale| sqrt(sum float64(g)^2)) of an array, a list or a dict of arrays (np.float32 scalar)."""
    x = _flat(g).astype(np.float64)
    with np.errstate(over='ignore', invalid='ignore'):
        return np.float32(abs(float(np.float32(grad_scale))) * math.sqrt(float(np.sum(x * x))))


def clip_scale(norm, grad_scale, max_norm):
    """-> (c, s, ok): float32 c = max_norm / max(norm, max_norm) (1 for max_norm 0 or inf), float32 s = grad_scale * c, bool ok."""
    norm = np.float32(norm); gs = np.float32(grad_scale); mx = np.float32(max_norm)
    if mx > 0 and not np.isinf(mx):
        big = mx if np.isnan(norm) else np.maximum(norm, mx)        # fmaxf: a NaN norm gives max_norm
        with np.errstate(invalid='ignore'):
            c = np.float32(mx / big)
    else:
        c = np.float32(1.0)
    with np.errstate(invalid='ignore', over='ignore'):
        s = np.float32(gs * c)
    return c, s, bool(np.isfinite(norm))


def update_stats(g, grad_scale, max_norm):
    """What fcn8s_get_update_stats reports for the gradient g: dict(norm, clip_coef, scale, ok)."""
    n = global_norm(g, grad_scale)
    c, s, ok = clip_scale(n, grad_scale, max_norm)
    return dict(norm=n, clip_coef=c, scale=s, ok=ok)


def accumulate(micro_grads):
    """fl(fl(g1 + g2) + g3) ... in float32, the order of fold, fold, ..., flush."""
    it = iter(micro_grads)
    acc = np.array(next(it), dtype=np.float32, copy=True)
    for g in it:
        acc = (acc + np.asarray(g, np.float32)).astype(np.float32)
    return acc


def adam_step(theta, g, m, v, t, lr, s, ok=True, beta1=0.9, beta2=0.999, eps=1e-8):
    """The guarded TF-Adam step in float32 (fcn8s_op_tf_adam's expressions with grad_scale = s, each operation rounded to float32; the
    device may contract a multiply-add): -> new (theta, m, v); unchanged copies if not ok.  t = the step number after the update (>= 1)."""
    f = np.float32
    theta, g, m, v = (np.array(a, dtype=f, copy=True) for a in (theta, g, m, v))
    if not ok:
        return theta, m, v
    b1, b2, e = f(beta1), f(beta2), f(eps)
    lr_t = f(lr) * f(math.sqrt(1.0 - float(b2) ** t)) / f(1.0 - float(b1) ** t)
    gr = g * f(s)
    m = b1 * m + (f(1) - b1) * gr
    v = b2 * v + (f(1) - b2) * gr * gr
    theta = theta - lr_t * m / (np.sqrt(v) + e)
    return theta.astype(f), m.astype(f), v.astype(f)


def sgd_step(theta, g, buf, lr, s, ok=True, momentum=0.9):
    """The guarded SGD-momentum step in float32: buf = momentum * buf + g * s; theta -= lr * buf -> new (theta, buf)."""
    f = np.float32
    theta, g, buf = (np.array(a, dtype=f, copy=True) for a in (theta, g, buf))
    if not ok:
        return theta, buf
    buf = f(momentum) * buf + g * f(s)
    theta = theta - f(lr) * buf
    return theta.astype(f), buf.astype(f)
