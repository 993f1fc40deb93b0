"""The soft-target (distillation) term on the CPU (fcn8s_set_soft_targets; the definition is in include/fcn8s_hip.h, restated in
fcn8s_tensorflow_amd/loss.py): the float64 restatement against torch's float64 autograd of kl_div(log_softmax(z / T), q, 'sum') T^2 / P, the
float32 restatement's distance to it, the padding column, all-ignored batches, the validation's refusals, and the C ABI's bindings."""
import numpy as np
import pytest
import torch

from fcn8s_tensorflow_amd import loss as LM


def case(P=700, C=20, K=20, seed=0, ignore=0.1, sharp=3.0):
    rng = np.random.default_rng(seed)
    z = (rng.standard_normal((P, C)) * 3).astype(np.float32)
    if K < C:
        z[:, K:] = -1e30                                            # the padding classes' logits
    t = np.exp(sharp * rng.standard_normal((P, K)))
    t /= t.sum(1, keepdims=True)
    lab = rng.integers(0, K, P).astype(np.uint8)
    lab[rng.random(P) < ignore] = 255
    return z, t.astype(np.float32), lab


def torch_reference(z, t, lab, T, pixels, K):
    """loss and d loss / d z by autograd, float64, from torch's own tempered teacher."""
    P, C = z.shape
    zt = torch.tensor(z.astype(np.float64), requires_grad=True)
    tt = torch.tensor(t[:, :K].astype(np.float64))
    q = torch.softmax(torch.log(torch.clamp(tt, min=float(np.finfo(np.float32).tiny))) / T, 1)
    used = torch.ones(P, dtype=torch.bool) if pixels == 'all' else torch.tensor(lab < C)
    ls = torch.log_softmax(zt[:, :K] / T, 1)
    loss = torch.nn.functional.kl_div(ls[used], q[used], reduction='sum') * T * T / P
    loss.backward()
    return float(loss.detach()), zt.grad.numpy()


@pytest.mark.parametrize("T", [1.0, 2.0, 4.0])
@pytest.mark.parametrize("pixels", ["valid", "all"])
@pytest.mark.parametrize("K", [20, 19])
def test_float64_restatement_against_autograd(T, pixels, K):
    z, t, lab = case(K=K, seed=int(T) * 10 + K)
    r = LM.soft_target_restate(z, t, lab, weight=1.0, temperature=T, pixels=pixels, ncols=K)
    loss, grad = torch_reference(z, t, lab, T, pixels, K)
    assert abs(r["term"] - loss) <= 1e-12, (r["term"], loss)
    assert np.abs(r["dlogits"] - grad).max() <= 1e-12
    assert np.isfinite(r["term"]) and np.isfinite(r["loss"]) and np.isfinite(r["dlogits"]).all() and np.isfinite(r["kd"]).all()
    if K < 20:
        assert (r["dlogits"][:, K:] == 0).all()                     # exactly 0: the padding column never takes part
    assert (r["dlogits"][~r["used"]] == 0).all() and (r["kd"][~r["used"]] == 0).all()
    assert r["term"] > 0 and (r["kd"] >= -1e-12).all()
    np.testing.assert_allclose(r["bias"], grad.sum(0), atol=1e-12)


def test_weight_scales_loss_and_gradient_and_leaves_the_term():
    z, t, lab = case(seed=3)
    a = LM.soft_target_restate(z, t, lab, weight=1.0, temperature=2.0)
    b = LM.soft_target_restate(z, t, lab, weight=0.25, temperature=2.0)
    assert a["term"] == b["term"] and b["loss"] == 0.25 * a["term"]
    np.testing.assert_allclose(b["dlogits"], 0.25 * a["dlogits"], rtol=0, atol=1e-18)


@pytest.mark.parametrize("T", [1.0, 2.0])
@pytest.mark.parametrize("K", [20, 19])
def test_float32_restatement_is_close_and_finite(T, K):
    z, t, lab = case(K=K, seed=5)
    r64 = LM.soft_target_restate(z, t, lab, temperature=T, ncols=K)
    r32 = LM.soft_target_restate(z, t, lab, temperature=T, ncols=K, dtype=np.float32)
    assert r32["dlogits"].dtype == np.float32 and np.isfinite(r32["dlogits"]).all() and np.isfinite(r32["term"])
    assert abs(r32["term"] - r64["term"]) <= 1e-5 * r64["term"]
    assert np.abs(r32["dlogits"] - r64["dlogits"]).max() <= 2e-6 * np.abs(r64["dlogits"]).max()
    if K < 20:
        assert (r32["dlogits"][:, K:] == 0).all()


def test_all_ignored_labels():
    z, t, lab = case(seed=7)
    lab[:] = 255
    v = LM.soft_target_restate(z, t, lab, pixels='valid')
    a = LM.soft_target_restate(z, t, lab, pixels='all')
    assert v["term"] == 0.0 and (v["dlogits"] == 0).all()
    assert a["term"] > 0.0 and np.abs(a["dlogits"]).max() > 0


def test_targets_equal_to_the_student_give_zero_and_one_hot_gives_the_cross_entropy():
    z, _, lab = case(seed=9, ignore=0.1)
    sm = np.exp(z.astype(np.float64) - z.max(1, keepdims=True)); sm /= sm.sum(1, keepdims=True)
    r = LM.soft_target_restate(z, sm, lab, temperature=1.0)
    assert abs(r["term"]) <= 1e-12 and np.abs(r["dlogits"]).max() <= 1e-15
    onehot = np.zeros_like(sm)
    v = lab < 20
    onehot[np.nonzero(v)[0], lab[v]] = 1.0
    onehot[~v, 0] = 1.0                                             # (rows outside U: anything)
    r = LM.soft_target_restate(z, onehot, lab, temperature=1.0, pixels='valid')
    ce = LM.restate(z, lab)
    assert abs(r["term"] - ce["loss"]) <= 1e-9 * ce["loss"]
    assert np.abs(r["dlogits"] - ce["dlogits"]).max() <= 1e-9 * np.abs(ce["dlogits"]).max()


def test_a_non_finite_target_row_turns_its_pixel_into_nan():
    z, t, lab = case(P=50, seed=11, ignore=0.0)
    t[7, 3] = np.nan; t[9, 0] = np.inf
    for dt in (np.float64, np.float32):
        r = LM.soft_target_restate(z, t, lab, dtype=dt)
        assert np.isnan(r["term"]) and np.isnan(r["kd"][[7, 9]]).all() and np.isnan(r["dlogits"][[7, 9]]).all()
        ok = np.ones(50, bool); ok[[7, 9]] = False
        assert np.isfinite(r["kd"][ok]).all() and np.isfinite(r["dlogits"][ok]).all()


def test_validation_refusals():
    assert LM.validate_soft_targets() == (0.0, 1.0, 0)
    assert LM.validate_soft_targets(0) == (0.0, 1.0, 0)
    assert LM.validate_soft_targets(0.5, 2, 'all') == (0.5, 2.0, 1)
    for kw in (dict(weight=-1.0), dict(weight=float("nan")), dict(weight=float("inf")), dict(weight="x"), dict(weight=True), dict(weight=1e39),
               dict(weight=1.0, temperature=0.0), dict(weight=1.0, temperature=-2.0), dict(weight=1.0, temperature=float("nan")),
               dict(weight=1.0, temperature=float("inf")), dict(weight=1.0, temperature=None), dict(weight=1.0, pixels="some"),
               dict(weight=1.0, pixels=1)):
        with pytest.raises(ValueError):
            LM.validate_soft_targets(**kw)
    z, t, lab = case(P=10)
    for kw in (dict(ncols=0), dict(ncols=21), dict(dtype=np.float16)):
        with pytest.raises(ValueError):
            LM.soft_target_restate(z, t, lab, **kw)
    with pytest.raises(ValueError):
        LM.soft_target_restate(z, t[:, :10], lab)


def test_the_abi_has_the_three_entries_and_none_of_them_takes_a_stream():
    import os
    import re
    from fcn8s_tensorflow_amd import _lib
    names = ("fcn8s_set_soft_targets", "fcn8s_bind_soft_targets", "fcn8s_get_soft_target_term")
    for n in names:
        assert n in _lib.SIGNATURES and hasattr(_lib.lib, n)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fcn8s_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    for n in names:
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % n, text).group(1)
        assert "stream" not in decl and decl.split(",")[0].strip() == "fcn8s_model* m", decl
    assert not [n for n in re.findall(r"\b(fcn8s_op_\w+)\s*\(", text) if "soft_target" in n]
