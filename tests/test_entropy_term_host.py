"""The entropy term on the CPU (fcn8s_set_entropy_term, fcn8s_op_entropy_term; the definition is in include/fcn8s_hip.h, restated in
fcn8s_tensorflow_amd/loss.py): `entropy_restate` in float64 against torch's float64 autograd of the textbook expression at 1e-12 (the bar of
tests/test_soft_targets_host.py), against the golden fixture's plain-Python doubles, its identities, the float32 restatement's distance, the
validation, and the declarations of the C ABI."""
import math
import os
import re

import numpy as np
import pytest
import torch

from fcn8s_tensorflow_amd import loss as LM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "entropy_term_cases.npz")


def golden():
    """The fixture's cases as dicts (tests/golden/make_entropy_term_cases.py)."""
    f = np.load(GOLDEN)
    out = []
    for i, (N, HW, C, K, pset, first, weight) in enumerate(f["params"]):
        c = dict(N=int(N), HW=int(HW), C=int(C), K=int(K), pixels=LM.ENTROPY_PIXEL_SETS[int(pset)], first_image=int(first), weight=float(weight))
        c.update(logits=(f["z_%d" % i].astype(np.float64) / 128.0).astype(np.float32), labels=f["lab_%d" % i])
        c.update({k: f["%s_%d" % (k, i)] for k in ("h", "dlogits", "bias")}, term=float(f["term_%d" % i]))
        out.append(c)
    return out


def case(N, HW, C, K, seed, ignore=0.1):
    rng = np.random.default_rng(seed)
    z = (3.0 * rng.standard_normal((N * HW, C))).astype(np.float32)
    if K < C:
        z[:, K:] = -1e30                                                   # the padding columns of a model with K logical classes
    lab = rng.integers(0, K, N * HW).astype(np.uint8)
    lab[rng.random(N * HW) < ignore] = 255
    return z, lab


def autograd(z, lab, pixels, K, first, HW):
    P, C = z.shape
    zt = torch.tensor(z[:, :K].astype(np.float64), requires_grad=True)
    used = np.arange(P) >= first * HW
    if pixels == 'unlabeled':
        used &= lab >= C
    elif pixels == 'valid':
        used &= lab < C
    h = (-torch.softmax(zt, -1) * torch.log_softmax(zt, -1)).sum(-1)
    term = h[torch.tensor(used)].sum() / (P * math.log(K))
    g = np.zeros((P, K))
    if used.any():
        term.backward()
        g = zt.grad.numpy()
    return float(term.detach()), h.detach().numpy() * used, g, used


@pytest.mark.parametrize("pixels", LM.ENTROPY_PIXEL_SETS)
@pytest.mark.parametrize("first", [0, 1, 3])
@pytest.mark.parametrize("C,K", [(20, 20), (20, 19), (4, 2)])
def test_float64_restatement_matches_autograd(pixels, first, C, K):
    N, HW = 3, 50
    z, lab = case(N, HW, C, K, 5 + C + K)
    r = LM.entropy_restate(z, lab, weight=1.0, pixels=pixels, ncols=K, first_image=first, pixels_per_image=HW)
    term, h, g, used = autograd(z, lab, pixels, K, first, HW)
    assert np.array_equal(r["used"], used)
    if first == N:
        assert not used.any() and r["term"] == 0.0 and not r["dlogits"].any() and not r["h"].any() and not r["bias"].any()
        return
    assert used.any() and (pixels == 'all' or not used[first * HW:].all())
    assert abs(r["term"] - term) <= 1e-12 * max(abs(term), 1e-300) and r["loss"] == r["term"]
    assert np.abs(r["h"] - h).max() <= 1e-12 * np.abs(h).max()
    assert np.abs(r["dlogits"][:, :K] - g).max() <= 1e-12 * np.abs(g).max()
    assert not r["dlogits"][:, K:].any() and not r["dlogits"][~used].any()
    assert np.abs(r["bias"] - r["dlogits"].sum(0)).max() <= 1e-15
    assert np.isfinite(r["dlogits"]).all()


def test_float64_restatement_matches_the_golden_fixture():
    """The fixture comes from plain Python loops with math.exp / math.log and shares nothing with loss.py."""
    cases = golden()
    assert len(cases) >= 20 and os.path.getsize(GOLDEN) < 1 << 20
    assert {c["N"] * c["HW"] for c in cases} == {1, 15, 255, 256, 257, 513, 600}
    assert {(c["C"], c["K"]) for c in cases} == {(4, 2), (20, 19), (20, 20), (21, 21), (64, 64)}
    for c in cases:
        r = LM.entropy_restate(c["logits"], c["labels"], c["weight"], c["pixels"], c["K"], c["first_image"], c["HW"])
        assert abs(r["term"] - c["term"]) <= 1e-12 * max(abs(c["term"]), 1e-300), c
        assert np.abs(r["h"] - c["h"]).max() <= 1e-12 * max(np.abs(c["h"]).max(), 1e-300)
        assert np.abs(r["dlogits"] - c["dlogits"]).max() <= 1e-12 * max(np.abs(c["dlogits"]).max(), 1e-300)
        assert np.abs(r["bias"] - c["bias"]).max() <= 1e-12 * max(np.abs(c["dlogits"]).sum(0).max(), 1e-300)


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("K", [2, 19, 20, 64])
def test_equal_logits_give_log_K_and_no_gradient(dt, K):
    P = 12
    z = np.repeat(np.linspace(-5, 5, P)[:, None], K, 1).astype(np.float32)
    lab = np.full(P, 255, np.uint8)
    lab[::3] = 0
    r = LM.entropy_restate(z, lab, 1.0, 'unlabeled', dtype=dt)
    eps = np.finfo(dt).eps
    n = int(r["used"].sum())
    assert n == 8 and np.abs(r["h"][r["used"]] - math.log(K)).max() <= 4 * K * eps * math.log(K)
    assert abs(r["term"] - n / P) <= 4 * K * eps
    # the row's gradient is coef s (b - sum s b) with every b = 0: exactly 0 (the header says why ls + h is taken in that form)
    assert not r["dlogits"].any()


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_identities(dt):
    z, lab = case(2, 40, 20, 20, 3)
    z[5] = 0.0
    z[5, 7] = 200.0                                                            # a 200-logit margin: in float32 the other classes' expf underflows to 0
    z[6] = 0.0
    z[6, 3] = 800.0                                                            # ... and an 800-logit margin does the same to float64's exp
    r = LM.entropy_restate(z, lab, 0.5, 'all', dtype=dt)
    assert r["h"][6] == 0.0 and (r["h"][5] == 0.0 if dt is np.float32 else 0.0 < r["h"][5] < 1e-80)
    assert not r["dlogits"][6].any() and np.isfinite(r["dlogits"]).all() and np.isfinite(r["term"])
    assert (r["h"] >= 0).all() and r["h"].max() <= math.log(20) * (1 + 1e-6)
    eps = np.finfo(dt).eps
    # every gradient row sums to 0 within rounding
    assert np.abs(r["dlogits"].astype(np.float64).sum(1)).max() <= 64 * eps * np.abs(r["dlogits"]).max()
    # a constant added to a row changes nothing (exact shifts in float32: multiples of 8 on logits of a few units keep 20 bits)
    zq = np.round(z * 1024) / 1024
    a = LM.entropy_restate(zq, lab, 0.5, 'all', dtype=dt)
    shift = np.where(np.arange(80) % 2 == 0, 8.0, -16.0)[:, None]
    shift[5:7] = 0.0
    b = LM.entropy_restate((zq + shift).astype(np.float32), lab, 0.5, 'all', dtype=dt)
    assert np.array_equal(a["dlogits"], b["dlogits"]) and a["term"] == b["term"]
    # weight -w: the negated gradient and loss, the same term
    n = LM.entropy_restate(z, lab, -0.5, 'all', dtype=dt)
    assert np.array_equal(n["dlogits"], -r["dlogits"]) and n["term"] == r["term"] and n["loss"] == -r["loss"]
    # the weight is linear, the term does not see it
    d = LM.entropy_restate(z, lab, 1.0, 'all', dtype=dt)
    assert d["term"] == r["term"] and np.abs(d["dlogits"] - 2 * r["dlogits"]).max() <= 2 * eps * np.abs(d["dlogits"]).max()


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_a_non_finite_logit_poisons_its_own_row_and_the_term(dt, bad):
    z, lab = case(1, 30, 20, 20, 4)
    clean = LM.entropy_restate(z, lab, 1.0, 'all', dtype=dt)
    z[11, 3] = bad
    r = LM.entropy_restate(z, lab, 1.0, 'all', dtype=dt)
    assert np.isnan(r["dlogits"][11]).all() and np.isnan(r["h"][11]) and np.isnan(r["term"])
    rest = np.arange(30) != 11
    assert np.array_equal(r["dlogits"][rest], clean["dlogits"][rest]) and np.array_equal(r["h"][rest], clean["h"][rest])
    # ... but not when its pixel is outside U
    lab[11] = 3
    r = LM.entropy_restate(z, lab, 1.0, 'unlabeled', dtype=dt)
    assert np.isfinite(r["term"]) and np.isfinite(r["dlogits"]).all()


def test_padding_columns_never_take_part():
    z, lab = case(1, 64, 20, 19, 8)
    assert (z[:, 19] == -1e30).all()
    for dt in (np.float64, np.float32):
        r = LM.entropy_restate(z, lab, 1.0, 'valid', ncols=19, dtype=dt)
        assert not r["dlogits"][:, 19].any() and np.isfinite(r["dlogits"]).all() and np.isfinite(r["term"])
        same = LM.entropy_restate(z[:, :19], lab, 1.0, 'all', dtype=dt)           # (labels < 19 < 20 or 255: 'valid' of C = 20 is a subset)
        v = r["used"]
        assert np.array_equal(r["dlogits"][v, :19], same["dlogits"][v])           # the same arithmetic: the 20th column is never read


def test_float32_restatement_is_close_to_the_definition():
    z, lab = case(2, 500, 20, 20, 9)
    a = LM.entropy_restate(z, lab, 1.0, 'all')
    b = LM.entropy_restate(z, lab, 1.0, 'all', dtype=np.float32)
    assert b["dlogits"].dtype == np.float32 and b["h"].dtype == np.float32
    assert abs(a["term"] - b["term"]) <= 1e-6 * a["term"]
    assert np.abs(a["dlogits"] - b["dlogits"]).max() <= 2e-6 * np.abs(a["dlogits"]).max()
    assert 0 < np.abs(a["dlogits"] - b["dlogits"]).max()


def test_validation():
    assert LM.validate_entropy_term() == (0.0, 0, 0)
    assert LM.validate_entropy_term(0) == (0.0, 0, 0)
    assert LM.validate_entropy_term(-0.5, 'valid', 2) == (-0.5, 1, 2)
    assert LM.validate_entropy_term(0.1, 'all')[1] == 2 and LM.validate_entropy_term(0.1)[0] == float(np.float32(0.1))
    for kw in (dict(weight=float("nan")), dict(weight=float("inf")), dict(weight=1e39), dict(weight="x"), dict(weight=True),
               dict(weight=1.0, pixels="none"), dict(weight=1.0, pixels=1), dict(weight=1.0, first_image=-1), dict(weight=1.0, first_image=0.5),
               dict(weight=1.0, first_image=True), dict(weight=1.0, first_image=1 << 31)):
        with pytest.raises(ValueError):
            LM.validate_entropy_term(**kw)
    z, lab = case(1, 8, 20, 20, 1)
    for kw in (dict(ncols=1), dict(ncols=21), dict(dtype=np.float16), dict(pixels_per_image=3), dict(pixels='labeled'), dict(weight=float("nan"))):
        with pytest.raises(ValueError):
            LM.entropy_restate(z, lab, **kw)
    with pytest.raises(ValueError):
        LM.entropy_restate(z, lab[:5])


def test_the_c_abi_declares_the_term_and_its_op():
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "fcn8s_hip.h")).read(), flags=re.S)
    from fcn8s_tensorflow_amd import _lib as L
    for name in ("fcn8s_set_entropy_term", "fcn8s_get_entropy_term", "fcn8s_op_entropy_term", "fcn8s_op_entropy_term_work_bytes"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in L.SIGNATURES and hasattr(L.lib, name), name
    assert len(L.SIGNATURES["fcn8s_op_entropy_term"][1]) == 15 and len(L.SIGNATURES["fcn8s_set_entropy_term"][1]) == 5
    mk = open(os.path.join(ROOT, "fcn8s_tensorflow_amd", "csrc", "Makefile")).read()
    assert "entropy_min.o" in mk
