"""The host side of temperature scaling (fcn8s_tensorflow_amd/temperature.py): the float32 restatement of the definition against the float64
one (the yardstick of the GPU tests: `e_units`), beta = 1 as the cross-entropy, the two-pass grid fit against a float64 golden-section
minimiser of the exact NLL, the grid ends, and the refusals."""
import functools
import math

import numpy as np
import pytest

from fcn8s_tensorflow_amd import temperature as ts

f32 = np.float32
IDENTITY = np.arange(256, dtype=np.uint8)


def softmax32(x):
    x = np.asarray(x, np.float64)
    e = np.exp(x - x.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(f32)


@functools.lru_cache(maxsize=None)
def case(N, P, Cn, seed=0, spoil=True, wrong_hot=False):
    """Random softmaxes at mixed sharpness (confidences from 1 / C to 1.0), among them rows with exact zeros and one-hot rows (the FLT_MIN
    clamp); labels that are mostly valid classes with some ignored (255) and some >= C; with `spoil`, rows holding a NaN, an inf, a negative
    entry.  The clamped entries are the true class (nll = 87.3 beta there, and E grows with it) only with `wrong_hot`.  Read-only; shared by
    the tests."""
    rng = np.random.default_rng([seed, N, P, Cn])
    temp = rng.choice(np.array([0.3, 1.0, 4.0, 40.0], f32), (N, P, 1))
    prob = softmax32(rng.normal(0, 1, (N, P, Cn)).astype(f32) * temp)
    r = rng.random((N, P))
    gt = rng.integers(0, Cn, (N, P)).astype(np.uint8)
    zero = r < 0.05                                                      # some entries exactly 0 (the row no longer sums to 1: any row is taken)
    other = (gt[zero] + rng.integers(1, Cn, int(zero.sum()))) % Cn
    prob[zero, rng.integers(0, Cn, int(zero.sum())) if wrong_hot else other] = 0.0
    hot = (r >= 0.05) & (r < 0.08)
    k = rng.integers(0, Cn, int(hot.sum()))
    prob[hot] = 0.0
    prob[hot, k] = 1.0
    gt[hot] = np.where(rng.random(int(hot.sum())) < (0.7 if wrong_hot else 2.0), k, gt[hot]).astype(np.uint8)
    r = rng.random((N, P))
    gt[r < 0.10] = 255
    gt[(r >= 0.10) & (r < 0.13)] = Cn + 1 if Cn + 1 < 255 else Cn
    if spoil:
        r = rng.random((N, P))
        prob[r < 0.01, 0] = np.nan
        prob[(r >= 0.01) & (r < 0.02), Cn - 1] = np.inf
        prob[(r >= 0.02) & (r < 0.03), 1] = -np.inf
        neg = (r >= 0.03) & (r < 0.05)
        prob[neg, Cn // 2 if wrong_hot else (gt[neg].astype(np.int64) + 1) % Cn] = -0.25
    for a in (prob, gt):
        a.setflags(write=False)
    return prob, gt


def grid_betas(K):
    """K candidates that always hold beta = 1: T log-spaced over [1/4, 4] (the range the issue's prototype measured E on)."""
    if K < 3:
        return np.array([1.0, 0.5][:K], f32)
    return ts.betas_of(ts.candidate_grid(0.25, 4.0, K))


def e_units(prob, gt, lut, betas):
    """E: the largest per-pixel |float32 restatement - float64 restatement| in units of 2^-16, and both restatements' results."""
    r32 = ts.nll_numpy(prob, gt, lut, betas, np.float32)
    r64 = ts.nll_numpy(prob, gt, lut, betas, np.float64)
    E = float(np.abs(r32[0].astype(np.float64) - r64[0]).max() * ts.Q_NLL) if r64[2] else 0.0
    return E, r32, r64


def exact_nll(prob, t, beta):
    """Mean NLL of the calibrated distribution at a float64 beta: log-sum-exp of beta log p minus beta log p_t."""
    l = np.log(np.fmax(prob.astype(np.float64), float(np.finfo(np.float32).tiny)))
    x = beta * (l - l.max(-1, keepdims=True))
    return float((np.log(np.exp(x).sum(-1)) - x[np.arange(len(t)), t]).mean())


def golden_section_temperature(prob, t, lo=2.0 ** -6, hi=2.0 ** 6, iters=80):
    """argmin over T of exact_nll(1 / T), searched in log T (the NLL is convex in beta, hence unimodal in log T)."""
    g = (math.sqrt(5) - 1) / 2
    a, b = math.log(lo), math.log(hi)
    f = lambda u: exact_nll(prob, t, math.exp(-u))
    c, d = b - g * (b - a), a + g * (b - a)
    fc, fd = f(c), f(d)
    for _ in range(iters):
        if fc < fd:
            b, d, fd = d, c, fc
            c = b - g * (b - a); fc = f(c)
        else:
            a, c, fc = c, d, fd
            d = a + g * (b - a); fd = f(d)
    return math.exp((a + b) / 2)


def host_sweep(prob, gt, lut=IDENTITY):
    return lambda betas: ts.nll_numpy(prob, gt, lut, betas, np.float32)[1:]


@pytest.mark.parametrize("Cn", [20, 19, 4, 2, 67])
def test_float32_restatement_against_float64(Cn):
    """The float32 restatement stays within the rounding budget of its own operations: with u = 2^-24, a term moves by at most
    8 u (C + 20 + nll + 2 beta (|l_t| + 2 |m|)) -- the fold over C classes, the exponent's argument of every class that still counts
    (beta |l_c| <= beta |m| + 20), the final subtraction, and beta d_t with both logarithms' errors."""
    prob, gt = case(3, 4099, Cn, wrong_hot=Cn in (20, 2))
    betas = grid_betas(8)
    E, r32, r64 = e_units(prob, gt, IDENTITY, betas)
    assert r32[2] == r64[2] > 0 and (r32[3] == r64[3]).all() and r32[3].min() > 0
    t = IDENTITY[gt.reshape(-1)].astype(np.int64)
    sel = t < Cn
    p = prob.reshape(-1, Cn)[sel]
    fin = np.isfinite(p).all(-1)
    p, t = p[fin].astype(np.float64), t[sel][fin]
    l = np.log(np.fmax(p, float(np.finfo(f32).tiny)))
    bound = 8 * 2.0 ** -24 * (Cn + 20 + r64[0] + 2 * betas[None, :].astype(np.float64) * (np.abs(l[np.arange(len(t)), t]) + 2 * np.abs(l.max(-1)))[:, None])
    d = np.abs(r32[0].astype(np.float64) - r64[0])
    print("C %d: E = %.3f units of 2^-16 over %d pixels x %d candidates" % (Cn, E, r64[2], betas.size))
    assert (d <= bound).all(), float((d / bound).max())
    assert (r64[0] >= -1e-12).all() and (r32[0] >= 0).all()              # s >= 1 and d_t <= 0
    # the integer tables are the rounded terms
    assert (r32[1] == np.rint(r32[0] * f32(ts.Q_NLL)).astype(np.int64).sum(0)).all()


def test_beta_one_is_the_cross_entropy():
    rng = np.random.default_rng(5)
    prob = softmax32(rng.normal(0, 2, (1, 5000, 20)))
    gt = rng.integers(0, 20, (1, 5000)).astype(np.uint8)
    terms = ts.nll_numpy(prob, gt, IDENTITY, [1.0], np.float64)[0][:, 0]
    p = prob[0].astype(np.float64)
    p = p / p.sum(-1, keepdims=True)                                     # the float32 row sums to 1 only up to rounding: normalise
    want = -np.log(p[np.arange(5000), gt[0]])
    assert np.abs(terms - want).max() <= 1e-12 * (1 + want.max())


def test_apply_numpy_is_the_distribution_whose_nll_is_summed():
    prob, gt = case(1, 517, 20)
    beta = 0.7
    q, h = ts.apply_numpy(prob, beta, np.float64)
    terms = ts.nll_numpy(prob, gt, IDENTITY, [beta], np.float64)[0][:, 0]
    t = IDENTITY[gt.reshape(-1)].astype(np.int64)
    keep = np.flatnonzero(t < 20)
    keep = keep[np.isfinite(prob.reshape(-1, 20)[keep]).all(-1)]
    qt = q.reshape(-1, 20)[keep, t[keep]]
    assert np.abs(-np.log(np.fmax(qt, 1e-300)) - terms).max() <= 1e-9 * (1 + terms.max())
    bad_rows = ~np.isfinite(prob).all(-1)
    assert bad_rows.any() and np.isnan(q[bad_rows]).all() and np.isnan(h[bad_rows]).all() and np.isfinite(q[~bad_rows]).all()
    assert np.abs(q[~bad_rows].sum(-1) - 1).max() < 1e-12
    assert (q[~bad_rows].argmax(-1) == np.where(np.isfinite(prob), prob, -1)[~bad_rows].argmax(-1)).mean() > 0.99   # ties of equal p_c aside


@pytest.mark.parametrize("T0", [0.5, 1.0, 2.5])
def test_two_pass_fit_recovers_a_known_temperature(T0):
    """Labels drawn from softmax(z0); the model presents softmax(T0 z0), whose calibrated form at T = T0 is softmax(z0).  The fit's T lies
    within one step ratio of the second grid of the float64 golden-section optimum of the exact NLL."""
    rng = np.random.default_rng(11)
    n, Cn = 20000, 20
    z0 = rng.normal(0, 2, (n, Cn))
    p0 = softmax32(z0).astype(np.float64)
    p0 /= p0.sum(-1, keepdims=True)
    t = (rng.random(n)[:, None] > np.cumsum(p0, -1)).sum(-1).clip(0, Cn - 1)
    prob = softmax32(T0 * z0)[None]
    gt = t.astype(np.uint8)[None]
    res = ts.fit(host_sweep(prob, gt), passes=2, candidates=32, t_min=0.125, t_max=8.0)
    best = golden_section_temperature(prob[0], t)
    ratio = max(res["temperature"] / best, best / res["temperature"])
    print("T0 %.2f: fit %.4f, golden section %.4f (ratio %.5f), nll %.5f -> %.5f" % (T0, res["temperature"], best, ratio, res["nllBefore"], res["nllAfter"]))
    assert ratio <= 1.0073
    assert abs(best / T0 - 1) < 0.03                                     # the sample's optimum is the generating temperature up to sampling noise
    assert not res["atBound"] and res["pixels"] == n and len(res["candidates"]) == 2 and all(len(c) == 32 for c in res["candidates"])
    assert res["nllAfter"] <= res["nllBefore"] and abs(res["nllBefore"] - exact_nll(prob[0], t, 1.0)) < 1e-4
    assert any(T == 1.0 for T, _ in res["candidates"][0])
    second = [T for T, _ in res["candidates"][1]]
    assert second[0] < res["temperature"] < second[-1] or res["temperature"] in (second[0], second[-1])


def test_an_optimum_outside_the_range_returns_the_bound():
    rng = np.random.default_rng(3)
    z0 = rng.normal(0, 2, (4000, 20))
    p0 = softmax32(z0).astype(np.float64)
    p0 /= p0.sum(-1, keepdims=True)
    t = (rng.random(4000)[:, None] > np.cumsum(p0, -1)).sum(-1).clip(0, 19)
    gt = t.astype(np.uint8)[None]
    res = ts.fit(host_sweep(softmax32(6.0 * z0)[None], gt), passes=2, candidates=16, t_min=0.5, t_max=2.0)     # optimum 6
    assert res["atBound"] and res["temperature"] == 2.0
    res = ts.fit(host_sweep(softmax32(0.2 * z0)[None], gt), passes=3, candidates=16, t_min=0.5, t_max=2.0)     # optimum 0.2
    assert res["atBound"] and res["temperature"] == 0.5
    res = ts.fit(host_sweep(softmax32(1.9 * z0)[None], gt), passes=2, candidates=16, t_min=0.5, t_max=2.0)     # inside the last interval
    assert not res["atBound"] and 1.7 < res["temperature"] < 2.0


def test_grids():
    g = ts.candidate_grid(0.125, 8.0, 32)
    assert len(g) == 32 and g[0] == 0.125 and g[-1] == 8.0 and (np.diff(g) > 0).all() and (g == 1.0).sum() == 1
    for lo, hi, k in [(2.0, 8.0, 5), (0.1, 0.5, 4), (1.0, 4.0, 3), (0.25, 1.0, 3), (0.9, 30.0, 6)]:
        g = ts.candidate_grid(lo, hi, k)
        assert len(g) <= k and (np.diff(g) > 0).all() and (g == 1.0).sum() == 1 and g.min() == min(lo, 1.0) and g.max() == max(hi, 1.0)
    T = np.array([0.5, 1.0, 2.0, 4.0])
    g, end = ts.refine(T, [3, 1, 2, 5], 5)
    assert end is None and g[0] == 0.5 and g[-1] == 2.0 and len(g) == 5 and abs(g[2] - 1.0) < 1e-12
    g, end = ts.refine(T, [1, 2, 3, 4], 4)
    assert end == 'min' and g[0] == 0.5 and g[-1] == 1.0
    g, end = ts.refine(T, [4, 3, 2, 1], 4)
    assert end == 'max' and g[0] == 2.0 and g[-1] == 4.0
    assert ts.betas_of([1.0, 2.0, 0.125]).tolist() == [1.0, 0.5, 8.0] and ts.betas_of([3.0]).dtype == np.float32


def test_validate_refusals(tmp_path):
    assert ts.validate([1.0, 0.5]).dtype == np.float32
    for bad in ([], [1.0] * 33, [0.0], [-1.0], [float('nan')], [float('inf')], [2.0 ** -7], [65.0]):
        with pytest.raises(ValueError):
            ts.validate(bad)
    assert ts.validate([2.0 ** -6, 2.0 ** 6]).tolist() == [2.0 ** -6, 2.0 ** 6]
    for bad in (0, -1.0, float('nan'), float('inf'), 1e-3, 100.0, "warm", None):
        with pytest.raises(ValueError):
            ts.validate_temperature(bad)
    for kw in (dict(passes=0), dict(passes=9), dict(passes=1.5), dict(candidates=2), dict(candidates=33), dict(t_min=2.0, t_max=1.0),
               dict(t_min=1.0, t_max=1.0), dict(t_min=0.0), dict(t_max=1000.0)):
        with pytest.raises(ValueError):
            ts.validate_fit(**{**dict(passes=2, candidates=32, t_min=0.125, t_max=8.0), **kw})
    prob, gt = case(1, 65, 20)
    with pytest.raises(ValueError):
        ts.nll_numpy(prob.astype(np.float64), gt, IDENTITY, [1.0])
    with pytest.raises(ValueError):
        ts.nll_numpy(prob, gt[:, :64], IDENTITY, [1.0])
    with pytest.raises(ValueError):
        ts.nll_numpy(prob, gt, IDENTITY[:255], [1.0])
    with pytest.raises(ValueError):
        ts.nll_numpy(prob[..., :1], gt, IDENTITY, [1.0])
    with pytest.raises(ValueError):                                      # a spoilt validation set is refused by the fit, as evaluate_reliability refuses it
        ts.fit(host_sweep(prob, gt), passes=1, candidates=4)
    with pytest.raises(ValueError):
        ts.fit(host_sweep(prob, np.full_like(gt, 255)), passes=1, candidates=4)
    path = str(tmp_path / "sub" / "t.json")
    clean, cgt = case(1, 257, 20, spoil=False)
    res = ts.fit(host_sweep(clean, np.where(cgt >= 20, 255, cgt).astype(np.uint8)), passes=1, candidates=4)
    ts.write_result_json(res, path)
    import json
    assert json.load(open(path))["temperature"] == res["temperature"]
