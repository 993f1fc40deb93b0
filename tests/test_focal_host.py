"""The focal loss on the CPU (fcn8s_set_focal, fcn8s_op_focal_xent; the definition is in include/fcn8s_hip.h, restated in
fcn8s_tensorflow_amd/loss.py): `focal_restate` in float64 against the golden fixture's plain-Python doubles and against torch's float64
autograd of sum w u^gamma (-log p_y) / P at 1e-12, its identities, the float32 restatement's distance, the validation, and the declarations of
the C ABI.

The per-pixel scalar `a` is compared on the rows with u > 1e-4 only: on a confident row l = (m + log S) - z_y is a difference of numbers
near 45 and carries an absolute error of an ulp of 45 (7e-15), which u^(gamma - 1) magnifies in `a` -- but there a multiplies a gradient row
of size u, and the gradient, the loss and f are held to 1e-12 everywhere."""
import os
import re

import numpy as np
import pytest
import torch

from fcn8s_tensorflow_amd import loss as LM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "focal_cases.npz")
GAMMAS = (0.5, 1.0, 2.0, 5.0)
NCASES = 19


def golden():
    """The fixture's cases as dicts (tests/golden/make_focal_cases.py)."""
    f = np.load(GOLDEN)
    out = []
    for i, (N, HW, C, K, gamma, has_cw, has_pw) in enumerate(f["params"]):
        c = dict(N=int(N), HW=int(HW), C=int(C), K=int(K), gamma=float(gamma))
        z = (f["z_%d" % i].astype(np.float64) / 128.0).astype(np.float32)
        z[:, c["K"]:] = -1e30
        c.update(logits=z, labels=f["lab_%d" % i], cw=f["cw_%d" % i] if has_cw else None, codes=f["codes_%d" % i] if has_pw else None,
                 table=f["table_%d" % i] if has_pw else None)
        c["pw"] = c["table"][c["codes"]] if has_pw else None
        c.update({k: f["%s_%d" % (k, i)] for k in ("f", "a", "dlogits", "bias")}, loss=float(f["loss_%d" % i]))
        out.append(c)
    return out


def case_id(c):
    return "%dx%d_C%d_K%d_g%g%s%s" % (c["N"], c["HW"], c["C"], c["K"], c["gamma"], "_cw" if c["cw"] is not None else "", "_pw" if c["pw"] is not None else "")


def make_case(P, C, K, seed, ignore=0.2, confident=True):
    """Inputs of the fixture's kind: 3 N(0, 1), every 7th row (from row 6) + 40 on one class (every 28th + 160) and half of those labelled with it, some rows + 12, every 11th row
    flat, padding columns at -1e30, 20 % of the labels 255.  `confident` False leaves the + 40 and + 160 rows out: then no product on the way to a
    gradient entry falls below FLT_MIN, where doubling a factor no longer doubles the rounded product.  The confident rows start at row 6, so
    that P = 1 is an ordinary pixel: a batch that is one saturated pixel has a gradient row of size u^gamma whose every digit is the rounding of
    logf(u) magnified by gamma - 1 (the float32 restatement's own distance to float64 reaches 1.0 of the largest entry there), so a distance
    relative to the largest entry says nothing on it."""
    rng = np.random.default_rng(seed)
    z = (3.0 * rng.standard_normal((P, C))).astype(np.float32)
    lab = rng.integers(0, K, P).astype(np.uint8)
    lab[rng.random(P) < ignore] = 255
    z[2::5, rng.integers(0, K)] += 12.0
    z[3::11] = z[3::11, :1]
    k = int(rng.integers(0, K))
    if confident:
        z[6::7, k] += 40.0
        z[13::28, k] += 120.0                                                 # ... and so far ahead that the others' expf is 0 in fp32: u = 0
        hit = np.zeros(P, bool); hit[13::14] = True
        lab[hit & (lab != 255)] = k
    if K < C:
        z[:, K:] = -1e30
    return z, lab


def weights(C, K, seed):
    rng = np.random.default_rng(seed)
    cw = (rng.integers(2, 17, C) / 8.0).astype(np.float32)
    cw[1 % K] = 0.0
    cw[K:] = 0.0
    return cw


def autograd(z, lab, gamma, cw=None, pw=None):
    """torch float64: sum_p w_p u_p^gamma (-log p_y) / P with u the sum of the OTHER classes' softmax (written as 1 - p_y, torch gives NaN for
    gamma < 1 on rows whose p_y rounds to 1) and rows with u = 0 masked."""
    P, C = z.shape
    valid = lab < C
    y = torch.tensor(np.where(valid, lab, 0).astype(np.int64))
    zt = torch.tensor(z.astype(np.float64), requires_grad=True)
    sm = torch.softmax(zt, -1)
    others = torch.ones(P, C, dtype=torch.bool)
    others[torch.arange(P), y] = False
    u = (sm * others).sum(-1)
    nll = -torch.log_softmax(zt, -1)[torch.arange(P), y]
    pos = u > 0
    mod = torch.where(pos, torch.where(pos, u, torch.ones_like(u)) ** gamma, torch.zeros_like(u))
    w = np.ones(P) if cw is None else np.asarray(cw, np.float64)[np.where(valid, lab, 0)]
    if pw is not None:
        w = (w.astype(np.float32) * np.asarray(pw, np.float32)).astype(np.float64)
    w = torch.tensor(np.where(valid, w, 0.0))
    loss = (w * mod * nll).sum() / P
    loss.backward()
    return float(loss.detach()), zt.grad.numpy(), mod.detach().numpy() * valid


@pytest.mark.parametrize("i", range(NCASES))
def test_float64_restatement_matches_the_golden_fixture(i):
    """The fixture comes from plain Python loops with math.exp / math.log and u ** gamma and shares nothing with loss.py."""
    cases = golden()
    assert len(cases) == NCASES
    c = cases[i]
    r = LM.focal_restate(c["logits"], c["labels"], c["gamma"], c["cw"], c["pw"])
    valid = c["labels"] < c["C"]
    assert np.array_equal(r["valid"], valid)
    dmax = np.abs(c["dlogits"]).max()
    if dmax == 0.0:                                                           # (P = 1 and an ignored or zero-weight pixel)
        assert not r["dlogits"].any() and r["loss"] == c["loss"]
        return
    assert abs(r["loss"] - c["loss"]) <= 1e-12 * abs(c["loss"]), case_id(c)
    assert np.abs(r["dlogits"] - c["dlogits"]).max() <= 1e-12 * dmax
    assert np.abs(r["bias"] - c["bias"]).max() <= 1e-12 * np.abs(c["dlogits"]).sum(0).max()
    assert np.abs(r["f"] - c["f"]).max() <= 1e-12 * max(np.abs(c["f"]).max(), 1e-300)
    with np.errstate(divide='ignore', invalid='ignore'):
        u = np.where(c["f"] > 0, c["f"] ** (1.0 / c["gamma"]), 0.0)
    big = u > 1e-4
    assert np.abs(r["a"] - c["a"])[big].max(initial=0.0) <= 1e-9 * max(np.abs(c["a"]).max(), 1e-300)
    assert not r["dlogits"][~valid].any() and not r["dlogits"][:, c["K"]:].any()


def test_the_fixture_covers_what_it_says():
    cases = golden()
    assert {c["N"] * c["HW"] for c in cases} == {1, 15, 255, 256, 257, 513, 600} and {c["C"] for c in cases} == {2, 4, 19, 20, 21, 64}
    assert {c["gamma"] for c in cases} == set(GAMMAS) and any(c["K"] < c["C"] for c in cases)
    assert any(c["cw"] is not None and c["pw"] is None for c in cases) and any(c["cw"] is None and c["pw"] is not None for c in cases)
    assert all((c["cw"] == 0).any() for c in cases if c["cw"] is not None)
    assert os.path.getsize(GOLDEN) < 600 * 1024
    big = [c for c in cases if c["N"] * c["HW"] >= 255]
    for c in big:
        valid = c["labels"] < c["C"]
        assert 0.1 < (~valid).mean() < 0.3
        assert ((c["f"] == 0) & valid).any() or c["gamma"] < 1 or (c["f"][valid] < 1e-12).any()     # rows with u = 0 or tiny


@pytest.mark.parametrize("gamma", GAMMAS + (0.25, 8.0))
@pytest.mark.parametrize("C,K", [(20, 20), (20, 19), (4, 4), (2, 2), (21, 21)])
@pytest.mark.parametrize("wts", ["none", "cw", "cw_pw"])
def test_float64_restatement_matches_autograd(gamma, C, K, wts):
    P = 150
    z, lab = make_case(P, C, K, 5 + C + K)
    cw = weights(C, K, 3) if wts != "none" else None
    pw = (np.random.default_rng(4).integers(0, 49, P) / 16.0).astype(np.float32) if wts == "cw_pw" else None
    r = LM.focal_restate(z, lab, gamma, cw, pw)
    loss, g, mod = autograd(z, lab, gamma, cw, pw)
    assert np.isfinite(g).all() and np.isfinite(r["dlogits"]).all()
    assert abs(r["loss"] - loss) <= 1e-12 * abs(loss)
    assert np.abs(r["dlogits"] - g).max() <= 1e-12 * np.abs(g).max()
    assert np.abs(r["f"] - mod).max() <= 1e-12 * np.abs(mod).max()
    assert np.abs(r["bias"] - r["dlogits"].sum(0)).max() <= 1e-15
    valid = lab < C
    assert not r["dlogits"][~valid].any() and not r["dlogits"][:, K:].any() and not r["a"][~valid].any()
    assert r["a"].max() <= 1.0 + gamma / np.e + 1e-9              # a = u^(gamma-1) (u + gamma l s_y), u <= 1 and l s_y = -(1 - u) log(1 - u) <= 1 / e


def test_identities_of_the_restatement():
    z, lab = make_case(257, 20, 19, 11)
    cw = weights(20, 19, 1)
    for dtype in (np.float64, np.float32):
        r = LM.focal_restate(z, lab, 2.0, cw, dtype=dtype)
        # gamma = 1: t = 1 exactly, so f = u (<= 1) and f l = u l
        r1 = LM.focal_restate(z, lab, 1.0, dtype=dtype)
        assert r1["f"].dtype == dtype and (r1["f"] <= 1).all() and (r1["f"][r1["valid"]] >= 0).all()
        # all weights x 2: the loss and every entry double exactly (on inputs that keep every product above FLT_MIN: see make_case)
        zm, lm = make_case(257, 20, 19, 11, confident=False)
        rm, r2 = LM.focal_restate(zm, lm, 2.0, cw, dtype=dtype), LM.focal_restate(zm, lm, 2.0, 2 * cw, dtype=dtype)
        assert r2["loss"] == 2 * rm["loss"] and np.array_equal(r2["dlogits"], 2 * rm["dlogits"]) and rm["dlogits"].any()
        # a class weight 0 = relabelling that class to 255
        rel = np.where(lab == 1, 255, lab).astype(np.uint8)
        r3 = LM.focal_restate(z, rel, 2.0, cw, dtype=dtype)
        assert r3["loss"] == r["loss"] and np.array_equal(r3["dlogits"], r["dlogits"])
        # pixel weights of 1 = none
        r4 = LM.focal_restate(z, lab, 2.0, cw, np.ones(257, np.float32), dtype=dtype)
        assert r4["loss"] == r["loss"] and np.array_equal(r4["dlogits"], r["dlogits"])


@pytest.mark.parametrize("gamma", (0.25,) + GAMMAS + (8.0,))
@pytest.mark.parametrize("C", [4, 20, 64])
def test_float32_restatement_stays_inside_the_bars(gamma, C):
    """The distances E that tests/test_focal_ops_gpu.py prints next to the device's: the float32 form alone stays inside the project's bars."""
    z, lab = make_case(600, C, C, 17 + C)
    cw = weights(C, C, 2)
    r, r32 = LM.focal_restate(z, lab, gamma, cw), LM.focal_restate(z, lab, gamma, cw, dtype=np.float32)
    dmax, col = np.abs(r["dlogits"]).max(), np.abs(r["dlogits"]).sum(0).max()
    E = (abs(r32["loss"] - r["loss"]) / abs(r["loss"]), np.abs(r32["bias"] - r["bias"]).max() / col, np.abs(r32["dlogits"] - r["dlogits"]).max() / dmax)
    print("gamma %g C %d: E loss %.2e bias %.2e dlogits %.2e" % ((gamma, C) + E))
    assert E[0] <= 1e-5 and E[1] <= 1e-5 and E[2] <= 2e-6
    u0 = (r32["f"] == 0) & r32["valid"]
    assert not r32["dlogits"][u0].any()                                       # a row with u = 0 is a row of zeros
    assert np.isfinite(r32["dlogits"]).all() and r32["a"].max() <= (1.0 + gamma / np.e) * (1 + 1e-5)     # (the bound of the float64 test)


def test_validate_focal_refusals():
    assert LM.validate_focal(None) == 0.0 and LM.validate_focal(0) == 0.0 and LM.validate_focal(2) == 2.0 and LM.validate_focal(8.0) == 8.0
    assert LM.validate_focal(0.1) == float(np.float32(0.1))
    assert LM.validate_focal(2.0, None) == 2.0 and LM.validate_focal(2.0, 0) == 2.0 and LM.validate_focal(0.0, 0.7) == 0.0
    for bad in (-1, -1e-9, 8.5, float("nan"), float("inf"), "x", True, [1.0, 2.0], 1e40):
        with pytest.raises(ValueError):
            LM.validate_focal(bad)
    with pytest.raises(ValueError):
        LM.validate_focal(2.0, 0.7)
    with pytest.raises(ValueError):
        LM.focal_restate(np.zeros((3, 4)), np.zeros(3), 0.0)
    with pytest.raises(ValueError):
        LM.focal_restate(np.zeros((3, 4)), np.zeros(2), 1.0)
    with pytest.raises(ValueError):
        LM.focal_restate(np.zeros((3, 4)), np.zeros(3), 1.0, pixel_weights=np.ones(2))
    with pytest.raises(ValueError):
        LM.focal_restate(np.zeros((3, 4)), np.zeros(3), 1.0, dtype=np.float16)


def test_the_abi_declares_and_binds_the_new_symbols():
    from fcn8s_tensorflow_amd import _lib as L
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "fcn8s_hip.h")).read(), flags=re.S)
    for name in ("fcn8s_set_focal", "fcn8s_op_focal_xent_work_bytes", "fcn8s_op_focal_xent"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in L.SIGNATURES and hasattr(L.lib, name)
    assert len(L.SIGNATURES["fcn8s_op_focal_xent"][1]) == 14
    assert int(L.lib.fcn8s_op_focal_xent_work_bytes()) >= 1024 * (16 + 64 * 4)
