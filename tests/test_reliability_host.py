"""reliability.py on the host: `counts_numpy` on hand-made pixels whose bins are known, the measures against independent per-pixel
formulations in exact rational arithmetic, the Cityscapes look-up table against labels.py's table, validation and the JSON round trip."""
import json
import math
from fractions import Fraction

import numpy as np
import pytest

from fcn8s_tensorflow_amd import cityscapes_eval as ce, reliability as rel

M = rel.SCORE_BINS
f32 = np.float32


def edge_case():
    """Eleven pixels of 4 classes, every value dyadic (so every product below is exact), B = 16, one score with score_max = 2 (scale 512).
    Returns (prob, gt, lut, [score], [scale], bins, expected) with expected = {pixel: (b, ok, u_bin, s_bin)} for the counted pixels."""
    rows = [
        # p                            gt   score         what
        ([0.0, 1.0, 0.0, 0.0],         1,   0.0),         # conf exactly 1.0: int(1.0 * 16) = 16 is clamped into bin 15; u = 0 and s = 0 -> bin 0
        ([0.5, 0.25, 0.25, 0.0],       0,   0.5),         # conf exactly 0.5 with B = 16: the edge belongs to bin 8; u = 0.5 -> 512; s -> 256
        ([0.25, 0.375, 0.375, 0.0],    2,   1.0),         # two-way tie of the maximum: k = 1, the lowest index, so t = 2 is WRONG; conf 0.375 -> bin 6
        ([0.25, 0.25, 0.25, 0.25],     255, 0.25),        # t = 255: ignored
        ([0.25, 0.25, 0.25, 0.25],     7,   0.25),        # t >= C: bad[0]
        ([0.5, 0.5, 0.0, 0.0],         0,   float('nan')),  # a NaN score: bad[1]
        ([0.125, 0.125, 0.125, 0.625], 3,   5.0),         # a score above score_max: the last bin; conf 0.625 -> bin 10
        ([0.75, 0.25, 0.0, 0.0],       1,   -1.0),        # a negative score: bin 0; wrong; conf 0.75 -> bin 12
        ([float('nan'), 0.5, 0.5, 0.0], 1,  0.5),         # NaN at class 0 stays the running maximum: conf NaN, bad[1]
        ([0.5, 0.5, 0.0, 0.0],         1,   float('inf')),  # an infinite score: bad[1]
        ([0.0, 0.0, 0.0, 1.0],         3,   2.0),         # s exactly score_max: int(1024) clamped to 1023
    ]
    prob = np.array([r[0] for r in rows], f32)
    gt = np.array([r[1] for r in rows], np.uint8)
    score = np.array([r[2] for r in rows], f32)
    expected = {0: (15, True, 0, 0), 1: (8, True, 512, 256), 2: (6, False, 640, 512), 6: (10, True, 384, 1023), 7: (12, False, 256, 0),
                10: (15, True, 0, 1023)}
    return prob, gt, rel.identity_lut(), [score], [f32(M) / f32(2.0)], 16, expected


def edge_tables():
    """The tables of edge_case() written out by hand from `expected`, with scalar arithmetic only."""
    prob, gt, lut, (score,), _, B, expected = edge_case()
    calib, sums, hist, bad = rel.new_tables(B, 1)
    for i, (b, ok, ub, sb) in expected.items():
        p = [float(v) for v in prob[i]]
        t = int(gt[i])
        conf = max(p)
        calib[b] += (1, int(ok), int(round(conf * 2 ** 24)))
        nll = f32(-math.log(max(p[t], 1e-38)))
        brier = sum((v - (1.0 if c == t else 0.0)) ** 2 for c, v in enumerate(p))          # dyadic: exact in float64 and in float32
        sums += (1, int(ok), int(np.rint(f32(nll * f32(65536.0)))), int(round(brier * 2 ** 23)))
        hist[0, ub, 0 if ok else 1] += 1
        hist[1, sb, 0 if ok else 1] += 1
    bad[:] = (1, 3)
    return calib, sums, hist, bad


def test_hand_made_pixels_land_in_their_known_bins():
    prob, gt, lut, scores, scales, B, _ = edge_case()
    got = rel.counts_numpy(prob, gt, lut, scores, scales, B)
    want = edge_tables()
    for g, w, name in zip(got, want, ("calib", "sums", "hist", "bad")):
        if name == "sums":      # q_nll: the hand computation rounds a float64 log to float32 -- one unit per pixel at the most
            assert (g[[0, 1, 3]] == w[[0, 1, 3]]).all() and abs(int(g[2]) - int(w[2])) <= int(w[0])
        else:
            assert (g == w).all(), name
    assert got[0][:, 0].sum() == got[1][0] == got[2][0].sum() == got[2][1].sum() == 6
    # each pixel alone, as a batch of one: the same bins
    for i, (b, ok, ub, sb) in edge_case()[6].items():
        c, s, h, bd = rel.counts_numpy(prob[i:i + 1], gt[i:i + 1], lut, [scores[0][i:i + 1]], scales, B)
        assert c[b, 0] == 1 and c[b, 1] == int(ok) and h[0, ub, 0 if ok else 1] == 1 and h[1, sb, 0 if ok else 1] == 1 and not bd.any()


def test_counts_accept_any_leading_shape_and_no_scores():
    rng = np.random.default_rng(5)
    x = rng.normal(0, 2, (2, 7, 9, 5)).astype(f32)
    p = np.exp(x); p /= p.sum(-1, keepdims=True)
    gt = rng.integers(0, 7, (2, 7, 9), dtype=np.uint8)
    a = rel.counts_numpy(p, gt, rel.identity_lut(), bins=15)
    b = rel.counts_numpy(p.reshape(-1, 5), gt.reshape(-1), rel.identity_lut(), bins=15)
    assert all((u == v).all() for u, v in zip(a, b))
    assert a[2].shape == (1, M, 2) and a[3][0] == int((gt >= 5).sum()) and a[1][0] == int((gt < 5).sum())
    # the argmax rule is np.argmax's on finite rows, and correct pixels are those it hits
    sel = gt < 5
    assert a[1][1] == int((np.argmax(p, -1)[sel] == gt[sel]).sum())


# ---- the measures against per-pixel formulations in exact rational arithmetic --------------------------------------------------
def random_hist(rng, nbins_used, per_bin_max):
    h = np.zeros((M, 2), np.int64)
    at = rng.choice(M, nbins_used, replace=False)
    h[at] = rng.integers(0, per_bin_max + 1, (nbins_used, 2))
    return h


def samples_of(h):
    """[(bin, wrong)] per pixel."""
    out = []
    for m in np.flatnonzero(h.sum(1)):
        out += [(int(m), 0)] * int(h[m, 0]) + [(int(m), 1)] * int(h[m, 1])
    return out


@pytest.mark.parametrize("seed", range(4))
def test_auroc_is_the_mann_whitney_statistic_with_ties_at_one_half(seed):
    rng = np.random.default_rng(seed)
    h = random_hist(rng, 12, 4)
    s = samples_of(h)
    pos = [m for m, w in s if w]; neg = [m for m, w in s if not w]
    u = sum(Fraction(1) if a > b else (Fraction(1, 2) if a == b else Fraction(0)) for a in pos for b in neg)
    want = u / (len(pos) * len(neg))
    assert rel.detection_measures(h)["auroc"] == pytest.approx(float(want), rel=1e-13, abs=0)


@pytest.mark.parametrize("seed", range(4))
def test_aupr_and_aurc_are_the_per_sample_definitions_when_a_bin_holds_one_pixel(seed):
    rng = np.random.default_rng(10 + seed)
    h = np.zeros((M, 2), np.int64)
    at = rng.choice(M, 40, replace=False)
    h[at, rng.integers(0, 2, 40)] = 1
    s = sorted(samples_of(h))                                         # ascending uncertainty
    n = len(s); W = sum(w for _, w in s)
    # average precision: for every wrong pixel, the share of wrong pixels among those at least as uncertain
    ap = sum(Fraction(sum(w for _, w in s[i:]), n - i) for i, (_, w) in enumerate(s) if w) / W
    # AURC: the mean over coverages i / n of the risk of the i most confident pixels
    aurc = sum(Fraction(sum(w for _, w in s[:i]), i) for i in range(1, n + 1)) / n
    got = rel.detection_measures(h)
    assert got["aupr"] == pytest.approx(float(ap), rel=1e-13, abs=0)
    assert got["aurc"] == pytest.approx(float(aurc), rel=1e-13, abs=0)
    r = W / n
    assert got["eaurc"] == pytest.approx(float(aurc) - (r + (1 - r) * math.log(1 - r)), rel=1e-12, abs=1e-15)
    rc = got["riskCoverage"]
    assert rc["bin"] == [m for m, _ in s] and rc["coverage"][-1] == 1.0 and rc["risk"][-1] == pytest.approx(r, rel=1e-15)


def test_a_perfect_ranking_has_auroc_one_and_no_excess_aurc():
    h = np.zeros((M, 2), np.int64)
    h[:600, 0] = 1; h[600:, 1] = 1                                     # every wrong pixel more uncertain than every correct one
    got = rel.detection_measures(h)
    assert got["auroc"] == 1.0 and got["aupr"] == pytest.approx(1.0, rel=1e-15)
    # the discrete optimum is sum_{i > K} (i - K) / i / n; E-AURC's closed form is its large-n limit
    n, K = M, 600
    assert got["aurc"] == pytest.approx(sum((i - K) / i for i in range(K + 1, n + 1)) / n, rel=1e-13)
    assert abs(got["eaurc"]) < 2e-3


def test_ece_and_mce_against_a_direct_loop():
    rng = np.random.default_rng(3)
    B = 15
    calib = np.zeros((B, 3), np.int64)
    for b in (0, 3, 7, 14):
        n = int(rng.integers(1, 1000))
        calib[b] = (n, int(rng.integers(0, n + 1)), int(rng.integers(int(b / B * n * 2 ** 24), int((b + 1) / B * n * 2 ** 24))))
    n = int(calib[:, 0].sum())
    sums = np.array([n, calib[:, 1].sum(), 123456789, 987654321], np.int64)
    ece = Fraction(0); mce = Fraction(0)
    for b in range(B):
        if calib[b, 0]:
            gap = abs(Fraction(int(calib[b, 1]), int(calib[b, 0])) - Fraction(int(calib[b, 2]), int(calib[b, 0]) * 2 ** 24))
            ece += Fraction(int(calib[b, 0]), n) * gap
            mce = max(mce, gap)
    got = rel.calibration_measures(calib, sums)
    assert got["ece"] == pytest.approx(float(ece), rel=1e-13) and got["mce"] == pytest.approx(float(mce), rel=1e-13)
    assert got["accuracy"] == int(sums[1]) / n and got["nll"] == 123456789 / (n * 65536.0) and got["brier"] == 987654321 / (n * 8388608.0)
    assert got["meanConfidence"] == pytest.approx(float(Fraction(int(calib[:, 2].sum()), n * 2 ** 24)), rel=1e-15)
    d = got["reliabilityDiagram"]
    assert d["count"] == calib[:, 0].tolist() and math.isnan(d["accuracy"][1]) and d["accuracy"][3] == calib[3, 1] / calib[3, 0]


def test_all_correct_all_wrong_and_empty_give_nan_where_a_denominator_is_zero():
    h = np.zeros((M, 2), np.int64)
    h[5, 0] = 3; h[9, 0] = 2
    g = rel.detection_measures(h)                                       # all correct: no positive
    assert math.isnan(g["auroc"]) and math.isnan(g["aupr"]) and g["aurc"] == 0.0 and g["eaurc"] == 0.0
    g = rel.detection_measures(h[:, ::-1])                              # all wrong: no negative
    assert math.isnan(g["auroc"]) and g["aupr"] == 1.0 and g["aurc"] == 1.0 and g["eaurc"] == 0.0
    g = rel.detection_measures(np.zeros((M, 2), np.int64))
    assert all(math.isnan(g[k]) for k in ("auroc", "aupr", "aurc", "eaurc")) and g["riskCoverage"]["bin"] == []
    c = rel.calibration_measures(np.zeros((15, 3), np.int64), np.zeros(4, np.int64))
    assert all(math.isnan(c[k]) for k in ("accuracy", "meanConfidence", "nll", "brier", "ece", "mce"))


def test_cityscapes_lut_against_the_labels_table():
    lut = rel.cityscapes_lut()
    assert lut.dtype == np.uint8 and lut.shape == (256,)
    seen = set()
    for name, id_, train_id, *_ in ce.LABELS:
        if id_ < 0:
            continue
        assert lut[id_] == (255 if train_id == 0 else train_id), name
        seen.add(id_)
    assert seen == set(range(34)) and (lut[34:] == 255).all()
    assert sorted(set(lut[:34].tolist()) - {255}) == list(range(1, 20))


def test_validation_errors():
    p = np.full((4, 3), 1 / 3, f32); gt = np.zeros(4, np.uint8); lut = rel.identity_lut(); s = np.zeros(4, f32)
    for kw in (dict(bins=0), dict(bins=65), dict(bins=1.5), dict(scores=[s] * 4, scales=[1.0] * 4), dict(scores=[s], scales=[]),
               dict(scores=[s], scales=[0.0]), dict(scores=[s], scales=[-1.0]), dict(scores=[s], scales=[float('nan')]),
               dict(scores=[s], scales=[float('inf')]), dict(scores=[s.astype(np.float64)], scales=[1.0]), dict(scores=[s[:3]], scales=[1.0])):
        with pytest.raises(ValueError):
            rel.counts_numpy(p, gt, lut, **kw)
    for args in ((p.astype(np.float64), gt, lut), (p, gt.astype(np.int64), lut), (p, gt[:3], lut), (p, gt, lut[:255]), (p, gt, lut.astype(np.int32)),
                 (p[:, :1], gt, lut)):
        with pytest.raises(ValueError):
            rel.counts_numpy(*args)
    with pytest.raises(ValueError):
        rel.Evaluator(score_names=("entropy",), score_max=0.0)
    with pytest.raises(ValueError):
        rel.Evaluator(score_names=("a", "b"), score_max=(1.0,))
    with pytest.raises(ValueError):
        rel.Evaluator(bins=100)
    ev = rel.Evaluator(num_classes=3, score_names=("entropy",))
    with pytest.raises(ValueError):
        ev.add(p, gt, [])                                             # the score is missing
    with pytest.raises(ValueError):
        rel.Evaluator(num_classes=5).add(p, gt)                       # 3 classes for an evaluator of 5
    with pytest.raises(ValueError):
        rel.measures(*rel.new_tables(15, 1), score_names=())


def nan_equal(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(nan_equal(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(nan_equal(x, y) for x, y in zip(a, b))
    if isinstance(a, float) and math.isnan(a):
        return isinstance(b, float) and math.isnan(b)
    return a == b


def test_evaluator_accumulates_and_the_json_round_trip(tmp_path):
    rng = np.random.default_rng(8)
    x = rng.normal(0, 3, (3, 200, 20)).astype(f32)
    p = np.exp(x - x.max(-1, keepdims=True)); p = (p / p.sum(-1, keepdims=True)).astype(f32)
    gt = rng.integers(0, 34, (3, 200), dtype=np.uint8)
    ent = (-(p * np.log(np.maximum(p, 1e-38))).sum(-1)).astype(f32)
    ev = rel.Evaluator(bins=10, num_classes=20, lut=rel.cityscapes_lut(), score_names=("entropy",))
    for n in range(3):
        ev.add(p[n], gt[n], [ent[n]])
    whole = rel.counts_numpy(p, gt, rel.cityscapes_lut(), [ent], [f32(M) / f32(math.log(20))], 10)
    assert all((a == b).all() for a, b in zip(ev.tables(), whole))
    res = ev.results()
    assert list(res["scores"]) == ["maxProb", "entropy"] and res["bins"] == 10 and res["scoreMax"]["entropy"] == math.log(20)
    assert res["pixels"] == int((rel.cityscapes_lut()[gt] != 255).sum()) and res["errorRate"] == pytest.approx(1 - res["accuracy"], rel=1e-14)
    path = str(tmp_path / "sub" / "reliability.json")
    rel.write_result_json(res, path)
    back = json.load(open(path))
    assert nan_equal(json.loads(json.dumps(rel.result_dict(res))), back)
    assert back["tables"]["calib"] == res["tables"]["calib"].tolist() and back["ece"] == res["ece"]
    assert back["scores"]["entropy"]["auroc"] == res["scores"]["entropy"]["auroc"]
