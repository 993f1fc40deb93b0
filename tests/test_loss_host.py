"""The float64 restatement of the weighted and OHEM training losses (fcn8s_tensorflow_amd/loss.py) against torch's cross_entropy and a
brute-force sort-based definition, the class-weight recipes and the argument checks.  No GPU."""
import math

import numpy as np
import pytest
import torch

from fcn8s_tensorflow_amd import loss as L


def batch(P, C, seed, ignore=0.1):
    rng = np.random.default_rng(seed)
    x = rng.normal(0, 2, (P, C))
    lab = rng.integers(0, C, P)
    lab[rng.random(P) < ignore] = 255
    return x, lab


def brute_ohem(x, lab, w, thresh, min_kept):
    """OHEM straight from its definition: sort the valid losses, take the k-th, keep everything at or above t."""
    P, C = x.shape
    valid = [p for p in range(P) if lab[p] < C]
    l = {}
    for p in valid:
        m = max(x[p])
        l[p] = m + math.log(sum(math.exp(v - m) for v in x[p])) - x[p][lab[p]]
    tau = float(np.float32(-math.log(float(np.float32(thresh)))))
    k = min(min_kept, len(valid))
    srt = sorted((l[p] for p in valid), reverse=True)
    t = min(tau, srt[k - 1]) if k > 0 else tau
    kept = [p for p in valid if l[p] >= t]
    loss = sum(w[lab[p]] * l[p] for p in kept) / len(kept) if kept else 0.0
    d = np.zeros((P, C))
    for p in kept:
        e = np.exp(x[p] - x[p].max()); sm = e / e.sum()
        sm[lab[p]] -= 1.0
        d[p] = w[lab[p]] / len(kept) * sm
    mask = np.zeros(P, bool); mask[kept] = True
    return loss, d, mask, t


@pytest.mark.parametrize("C", [20, 4, 12])
def test_weighted_matches_torch_cross_entropy(C):
    x, lab = batch(3000, C, C)
    w = np.random.default_rng(1).uniform(0.0, 3.0, C)
    r = L.restate(x, lab, class_weights=w)
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    ref = torch.nn.functional.cross_entropy(xt, torch.tensor(lab), weight=torch.tensor(w), reduction='sum', ignore_index=255) / x.shape[0]
    ref.backward()
    assert abs(r["loss"] - ref.item()) <= 1e-12 * abs(ref.item())
    np.testing.assert_allclose(r["dlogits"], xt.grad.numpy(), rtol=0, atol=1e-15)
    assert r["valid"] == int((lab < C).sum()) == r["num_kept"] and r["threshold"] == 0.0


def check_ohem(x, lab, w, thresh, min_kept):
    r = L.restate(x, lab, class_weights=w, ohem_thresh=thresh, ohem_min_kept=min_kept)
    loss, d, mask, t = brute_ohem(x, lab, np.ones(x.shape[1]) if w is None else w, thresh, min_kept)
    assert (r["kept"] == mask).all()
    assert r["num_kept"] == int(mask.sum()) and r["threshold"] == t
    assert abs(r["loss"] - loss) <= 1e-12 * max(1.0, abs(loss))
    np.testing.assert_allclose(r["dlogits"], d, rtol=0, atol=1e-15)
    return r


@pytest.mark.parametrize("thresh,min_kept", [(0.7, 500), (0.7, 10), (0.2, 2000), (0.9, 0), (0.5, 10 ** 9), (1.0, 100)])
def test_ohem_matches_sort_definition(thresh, min_kept):
    x, lab = batch(2000, 20, 3)
    w = np.random.default_rng(4).uniform(0.5, 2.0, 20)
    r = check_ohem(x, lab, w, thresh, min_kept)
    V = int((lab < 20).sum())
    if min_kept > V:
        assert r["num_kept"] == V                  # every valid pixel is kept
    if thresh == 1.0:
        assert r["num_kept"] == V and r["threshold"] == 0.0
    if min_kept == 0:
        assert r["threshold"] == L.tau(thresh)


def test_ohem_ties_straddling_k():
    x, lab = batch(400, 20, 5, ignore=0.0)
    x[100:160] = x[7]; lab[100:160] = lab[7]       # 61 pixels share one loss
    l = L.pixel_losses(x, lab)
    order = np.argsort(-l, kind="stable")
    rank = int(np.nonzero(order == 7)[0].min())    # the tied group starts at this rank; k lands inside it
    r = check_ohem(x, lab, None, 1e-6, rank + 5)
    assert r["kept"][100:160].all() and r["kept"][7]
    assert r["num_kept"] >= rank + 61


def test_ohem_precomputed_losses_drive_the_selection():
    x, lab = batch(500, 12, 6)
    l = L.pixel_losses(x, lab).astype(np.float32)
    r = L.restate(x, lab, ohem_thresh=0.6, ohem_min_kept=300, pixel_loss=l)
    valid = lab < 12
    assert r["threshold"] == float(np.float32(r["threshold"]))
    assert (r["kept"] == (valid & (np.where(valid, l, -1) >= r["threshold"]))).all()


def test_all_ignored():
    x, _ = batch(100, 20, 7)
    lab = np.full(100, 255)
    for thresh in (None, 0.7):
        r = L.restate(x, lab, ohem_thresh=thresh, ohem_min_kept=10)
        assert r["loss"] == 0.0 and not r["dlogits"].any() and r["valid"] == 0 and r["num_kept"] == 0
    assert brute_ohem(x, lab, np.ones(20), 0.7, 10)[0] == 0.0


def test_class_weight_recipes():
    lab1 = np.array([[0, 0, 0, 1], [0, 0, 255, 1]])          # image 1: 7 labelled pixels, classes 0 (5) and 1 (2)
    lab2 = np.array([[2, 2], [1, 7]])                          # image 2: id 7 >= C is ignored; 3 labelled pixels, classes 1 (1) and 2 (2)
    counts, img = L.class_pixel_counts([lab1[None], lab2], 3)
    assert counts.tolist() == [5, 3, 2] and img.tolist() == [7, 10, 3]
    # freq = [5/7, 3/10, 2/3] -> median 2/3 -> w = [14/15, 20/9, 1]
    np.testing.assert_allclose(L.median_frequency_weights(counts, img), [14 / 15, 20 / 9, 1.0], rtol=1e-6)
    np.testing.assert_allclose(L.median_frequency_weights([4, 0, 2], [6, 0, 3]), [1.0, 0.0, 1.0], rtol=1e-6)
    # p = [0.5, 0.3, 0.2]
    np.testing.assert_allclose(L.enet_weights(counts), [1 / math.log(1.52), 1 / math.log(1.32), 1 / math.log(1.22)], rtol=1e-6)
    np.testing.assert_allclose(L.enet_weights([1, 1], c=1.5), [1 / math.log(2.0)] * 2, rtol=1e-6)


def test_argument_checks():
    assert L.validate(None, None, 100000, 20) == (None, 0.0, 100000)
    w, t, k = L.validate([1.0] * 19 + [0.0], 0.7, 5, 20)
    assert w.dtype == np.float32 and t == float(np.float32(0.7)) and k == 5
    assert L.validate(None, 1.0, 0, 3)[1] == 1.0
    for bad in ([1.0] * 19, [1.0] * 19 + [-1.0], [1.0] * 19 + [float("nan")], [1.0] * 19 + [float("inf")], [0.0] * 20):
        with pytest.raises(ValueError):
            L.validate(bad, None, 0, 20)
    for bad in (-0.1, 1.5, float("nan"), float("inf"), "x"):
        with pytest.raises(ValueError):
            L.validate(None, bad, 0, 20)
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError):
            L.validate(None, 0.7, bad, 20)
