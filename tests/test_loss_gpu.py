"""Class-weighted and OHEM training losses on the GPU (fcn8s_set_loss, fcn8s_op_softmax_xent_ex; definitions in include/fcn8s_hip.h and
fcn8s_tensorflow_amd/loss.py): the kernels against the float64 restatement, the OHEM selection exactly against the restatement applied
to the device's own per-pixel losses, the unchanged default, exact identities of a whole training step, the model-level selection in
fp32 and bf16_train, allocation and determinism, and the facade."""
import ctypes as C

import numpy as np
import pytest
import torch

from fcn8s_tensorflow_amd import loss as LM
from oracle import fcn8s_oracle as orc

pytestmark = pytest.mark.gpu
SMALL = (8, 16, 32, 64, 64, 128, 128)
W64 = (64, 64, 128, 256, 256, 256, 128)          # bf16_train needs channel widths % 64 == 0
LAST_BIAS = "fc7_pool4_pool3_conv2d_trans/bias"


def _lib():
    from fcn8s_tensorflow_amd import _lib
    return _lib


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def op_batch(npix, Cc, seed, ignore=0.1):
    rng = np.random.default_rng(seed)
    logits = (rng.standard_normal((npix, Cc)) * 3).astype(np.float32)
    lab = rng.integers(0, Cc, npix).astype(np.uint8)
    lab[rng.random(npix) < ignore] = 255
    return logits, lab


def run_ex(logits, lab, w=None, thresh=0.0, min_kept=0):
    """fcn8s_op_softmax_xent_ex -> (loss, dlogits, pixel_loss, stats)."""
    L = _lib()
    npix, Cc = logits.shape
    ld, lb = torch.tensor(logits).cuda(), torch.tensor(lab).cuda()
    wd = torch.tensor(np.asarray(w, np.float32)).cuda() if w is not None else None
    dl = torch.full((npix, Cc), 7.0).cuda(); lo = torch.zeros(1).cuda()
    pl = torch.zeros(npix).cuda(); st = torch.zeros(3, dtype=torch.int64).cuda()
    L.check(L.lib.fcn8s_op_softmax_xent_ex(None, ptr(ld), ptr(lb), ptr(wd), float(thresh), int(min_kept), ptr(dl), ptr(lo), ptr(pl), ptr(st), npix, Cc))
    torch.cuda.synchronize()
    return float(lo.cpu()), dl.cpu().numpy(), pl.cpu().numpy(), st.cpu().numpy()


def f32_bits(x):
    return int(np.float32(x).view(np.uint32))


@pytest.mark.parametrize("Cc", [20, 4, 12])
def test_op_weighted_matches_restatement(Cc):
    logits, lab = op_batch(5000, Cc, Cc)
    w = np.random.default_rng(1).uniform(0.2, 3.0, Cc).astype(np.float32)
    loss, dl, _, st = run_ex(logits, lab, w=w)
    r = LM.restate(logits, lab, class_weights=w)
    assert abs(loss - r["loss"]) <= 2e-6 * abs(r["loss"])
    assert np.abs(dl - r["dlogits"]).max() <= 2e-6 * np.abs(r["dlogits"]).max()
    assert st.tolist() == [r["valid"], r["valid"], 0]


@pytest.mark.parametrize("Cc", [20, 4, 12])
@pytest.mark.parametrize("thresh,min_kept", [(0.7, 1500), (0.7, 10), (1.0, 50), (0.05, 10 ** 9), (0.3, 0)])
def test_op_ohem_selection_is_exact(Cc, thresh, min_kept):
    logits, lab = op_batch(6000, Cc, 100 + Cc)
    w = np.random.default_rng(2).uniform(0.5, 2.0, Cc).astype(np.float32)
    loss, dl, pl, st = run_ex(logits, lab, w=w, thresh=thresh, min_kept=min_kept)
    valid = lab < Cc
    assert (pl[~valid] == -1.0).all()
    l64 = LM.pixel_losses(logits, lab)
    assert np.abs(pl[valid] - l64[valid]).max() <= 1e-5 * max(1.0, np.abs(l64[valid]).max())
    r = LM.restate(logits, lab, class_weights=w, ohem_thresh=thresh, ohem_min_kept=min_kept, pixel_loss=pl)
    kept = (dl != 0).any(1)
    np.testing.assert_array_equal(kept, r["kept"])
    assert st.tolist() == [r["valid"], r["num_kept"], f32_bits(r["threshold"])]
    assert abs(loss - r["loss"]) <= 2e-6 * max(1e-30, abs(r["loss"]))
    assert np.abs(dl - r["dlogits"]).max() <= 2e-6 * np.abs(r["dlogits"]).max()


@pytest.mark.parametrize("Cc", [20, 4, 12])
def test_op_ohem_ties_at_the_kth_loss(Cc):
    logits, lab = op_batch(4000, Cc, 200 + Cc)
    _, _, pl, _ = run_ex(logits, lab, thresh=1e-6, min_kept=1)
    valid = np.nonzero(lab < Cc)[0]
    src = valid[np.argsort(pl[valid])[len(valid) // 2]]           # a pixel of median loss, copied into 80 others
    dup = valid[valid != src][-80:]
    logits[dup] = logits[src]; lab[dup] = lab[src]
    _, _, pl, _ = run_ex(logits, lab, thresh=1e-6, min_kept=1)
    assert (pl[dup] == pl[src]).all()
    above, tied = int((pl[valid] > pl[src]).sum()), int((pl[valid] == pl[src]).sum())
    assert tied >= 81
    k = above + 30                                                  # inside the tied group
    loss, dl, pl, st = run_ex(logits, lab, thresh=1e-6, min_kept=k)
    r = LM.restate(logits, lab, ohem_thresh=1e-6, ohem_min_kept=k, pixel_loss=pl)
    assert r["threshold"] == float(pl[src]) and r["num_kept"] == above + tied
    np.testing.assert_array_equal((dl != 0).any(1), r["kept"])
    assert st.tolist() == [r["valid"], above + tied, f32_bits(pl[src])]
    assert abs(loss - r["loss"]) <= 2e-6 * r["loss"]


@pytest.mark.parametrize("Cc", [20, 4, 12])
def test_op_default_and_unit_weights_are_bit_identical(Cc):
    L = _lib()
    logits, lab = op_batch(3000, Cc, 300 + Cc)
    ld, lb = torch.tensor(logits).cuda(), torch.tensor(lab).cuda()
    dl0 = torch.empty(3000, Cc).cuda(); lo0 = torch.zeros(1).cuda()
    L.check(L.lib.fcn8s_op_softmax_xent(None, ptr(ld), ptr(lb), ptr(dl0), ptr(lo0), 3000, Cc))
    torch.cuda.synchronize()
    for w in (None, np.ones(Cc, np.float32)):
        loss, dl, _, _ = run_ex(logits, lab, w=w)
        assert f32_bits(loss) == f32_bits(float(lo0.cpu()))
        np.testing.assert_array_equal(dl.view(np.uint32), dl0.cpu().numpy().view(np.uint32))


# ---- the model -------------------------------------------------------------------------------------------------------------------
def engine(widths=SMALL, precision="fp32", **opts):
    from fcn8s_tensorflow_amd.engine import Engine
    return Engine(20, widths=widths, device_id=0, seed=0, precision=precision, options=opts)


def model_case(widths, n=2, h=64, w=96, seed=3, ignore=0.1, decoder_std_scale=30.0):
    P = orc.init_params(20, widths, seed=seed, decoder_std_scale=decoder_std_scale, bias_std=0.05)
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    lab = rng.integers(0, 20, (n, h, w), dtype=np.uint8)
    lab[rng.random((n, h, w)) < ignore] = 255
    return P, img, lab


def step_grads(e, P, img, lab, **loss_cfg):
    e.set_params(P)
    if loss_cfg:
        e.set_loss(**loss_cfg)
    loss = e.forward_backward(img, lab, keep_prob=1.0, l2_rate=0.0)
    return loss, {k: v.copy() for k, v in e.get_grads().items()}


def assert_bits(a, b, scale=1.0):
    assert np.float32(a[0]) * np.float32(scale) == np.float32(b[0]), (a[0], b[0])
    assert len(a[1]) == len(b[1]) == 42
    for k in a[1]:
        np.testing.assert_array_equal((a[1][k] * np.float32(scale)).view(np.uint32), b[1][k].view(np.uint32), err_msg=k)


@pytest.mark.parametrize("tconv_gemm", [0, 1])
def test_unit_weights_leave_every_gradient_bit_identical(tconv_gemm):
    P, img, lab = model_case(SMALL)
    ref = step_grads(engine(deterministic=1, tconv_gemm=tconv_gemm), P, img, lab)
    got = step_grads(engine(deterministic=1, tconv_gemm=tconv_gemm), P, img, lab, class_weights=np.ones(20))
    assert_bits(ref, got)


def test_doubled_weights_double_loss_and_gradients_exactly():
    P, img, lab = model_case(SMALL, seed=4)
    ref = step_grads(engine(deterministic=1), P, img, lab)
    got = step_grads(engine(deterministic=1), P, img, lab, class_weights=np.full(20, 2.0))
    assert_bits(ref, got, scale=2.0)


def test_one_hot_weights_equal_relabelling_to_ignore():
    P, img, lab = model_case(SMALL, seed=5)
    w = np.zeros(20); w[[0, 3, 7, 8, 15, 19]] = 1.0
    got = step_grads(engine(deterministic=1), P, img, lab, class_weights=w)
    relab = lab.copy(); relab[(lab < 20) & (w[np.minimum(lab, 19)] == 0)] = 255
    ref = step_grads(engine(deterministic=1), P, img, relab)
    assert_bits(ref, got)


def _gap_configs(l, valid, tol):
    """(tau binding, min_kept binding) configurations whose threshold sits in the widest gap of the sorted float64 losses (10th to 90th
    percentile from the top, losses below 80 so that a float32 threshold can put tau above them), a gap far wider than the fp32 round-off
    `tol` of a device loss."""
    s = np.sort(l[valid])[::-1]
    idx = np.arange(len(s) // 10, len(s) * 9 // 10)
    idx = idx[s[idx] < 80.0]
    i = int(idx[np.argmax(s[idx] - s[idx + 1])])
    assert s[i] - s[i + 1] > 20 * tol
    by_tau = dict(ohem_thresh=float(np.exp(-0.5 * (s[i] + s[i + 1]))), ohem_min_kept=10)
    by_k = dict(ohem_thresh=1e-37, ohem_min_kept=int(i + 1))          # tau = 85.2: the k-th largest loss decides
    return by_tau, by_k


@pytest.mark.parametrize("precision,widths", [("fp32", SMALL), ("bf16_train", W64)])
@pytest.mark.parametrize("tconv_gemm", [0, 1])
def test_model_ohem_matches_restatement(precision, widths, tconv_gemm):
    P, img, lab = model_case(widths, seed=6, decoder_std_scale=3.0)
    n, h, w = lab.shape
    e = engine(widths, precision, tconv_gemm=tconv_gemm)
    e.set_params(P)
    e.forward_backward(img, lab, keep_prob=1.0)
    logits = e.activation("logits", (n, h, w, 20)).reshape(-1, 20)
    valid = lab.reshape(-1) < 20
    tol = 4e-6 * max(1.0, float(np.abs(logits).max()))                # round-off of an fp32 l_p = m + log(s) - v
    by_tau, by_k = _gap_configs(LM.pixel_losses(logits, lab), valid, tol)
    cw = np.random.default_rng(7).uniform(0.5, 2.0, 20).astype(np.float32)
    for cfg in (by_tau, by_k):
        e.set_loss(class_weights=cw, **cfg)
        loss = e.forward_backward(img, lab, keep_prob=1.0)
        logits = e.activation("logits", (n, h, w, 20)).reshape(-1, 20)
        r = LM.restate(logits, lab, class_weights=cw, **cfg)
        st = e.loss_stats()
        assert (st["valid"], st["kept"]) == (r["valid"], r["num_kept"]), (cfg, st, r["num_kept"])
        assert abs(st["threshold"] - r["threshold"]) <= tol
        if cfg is by_tau:
            assert st["threshold"] == LM.tau(cfg["ohem_thresh"])
        assert abs(loss - r["loss"]) <= 1e-5 * r["loss"] + tol
        db = e.get_grads()[LAST_BIAS]
        ref = r["dlogits"].sum(0)
        assert np.abs(db - ref).max() <= 1e-5 * np.abs(r["dlogits"]).sum(0).max(), (cfg, db, ref)
    e.set_loss()
    e.forward_backward(img, lab, keep_prob=1.0)
    with pytest.raises(Exception, match="without a loss configuration"):
        e.loss_stats()
    e.close()


def test_repeated_ohem_steps_allocate_nothing_and_deterministic_mode_reproduces():
    P, img, lab = model_case(SMALL, seed=8)
    cw = np.random.default_rng(9).uniform(0.5, 2.0, 20)
    params = []
    for _ in range(2):
        e = engine(deterministic=1)
        e.set_params(P)
        e.set_loss(class_weights=cw, ohem_thresh=0.7, ohem_min_kept=3000)
        e.train_step(img, lab, 1e-3, keep_prob=1.0)
        a = e.get_option("workspace_allocations")
        l2, _ = e.train_step(img, lab, 1e-3, keep_prob=1.0)
        e.train_step(img, lab, 1e-3, keep_prob=1.0)
        assert e.get_option("workspace_allocations") == a and np.isfinite(l2)
        params.append({k: v.copy() for k, v in e.get_params().items()})
        e.close()
    for k in params[0]:
        np.testing.assert_array_equal(params[0][k].view(np.uint32), params[1][k].view(np.uint32), err_msg=k)


def test_bad_arguments_raise():
    from fcn8s_tensorflow_amd import _lib as L
    e = engine()
    for kw in (dict(class_weights=np.ones(19)), dict(class_weights=-np.ones(20)), dict(class_weights=np.zeros(20)),
               dict(class_weights=np.full(20, np.nan)), dict(ohem_thresh=1.5), dict(ohem_thresh=-0.2), dict(ohem_thresh=0.7, ohem_min_kept=-1)):
        with pytest.raises(ValueError):
            e.set_loss(**kw)
    ones = (C.c_float * 20)(*([1.0] * 20))
    assert L.lib.fcn8s_set_loss(e.h, ones, 19, 0.0, 0) == L.ERR_BAD_ARG
    assert L.lib.fcn8s_set_loss(e.h, None, 0, 1.5, 0) == L.ERR_BAD_ARG
    assert L.lib.fcn8s_set_loss(e.h, None, 0, 0.5, -1) == L.ERR_BAD_ARG
    assert L.lib.fcn8s_set_loss(e.h, None, 0, float("nan"), 0) == L.ERR_BAD_ARG
    e.close()


def gen(n, h, w, seed):
    rng = np.random.default_rng(seed)
    while True:
        img = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
        lab = rng.integers(0, 19, (n, h, w), dtype=np.uint8)
        yield img, orc.one_hot(lab, 19)


def test_facade_train_with_loss_configuration():
    from fcn8s_tensorflow_amd.fcn8s import FCN8s
    m = FCN8s(vgg16_dir='synthetic:3', num_classes=19, widths=SMALL)      # 19 classes: the weights are padded to the library's 20
    cw = np.linspace(0.5, 2.0, 19)
    with pytest.raises(ValueError):
        m.train(gen(2, 32, 64, 0), 1, 1, lambda s: 1e-3, ohem_thresh=2.0)
    with pytest.raises(ValueError):
        m.train(gen(2, 32, 64, 0), 1, 1, lambda s: 1e-3, class_weights=np.ones(20))
    m.train(gen(2, 32, 64, 0), epochs=1, steps_per_epoch=2, learning_rate_schedule=lambda s: 1e-3, class_weights=cw, ohem_thresh=0.7,
            ohem_min_kept=1000, metrics={'loss'}, eval_frequency=1, record_summaries=False)
    assert m.g_step == 2 and np.isfinite(m.training_loss)
    assert m.engine.loss_config is None                                  # restored
    m.evaluate(gen(2, 32, 64, 1), 1, metrics={'loss'})
    a = m.metric_values[0]
    m2 = FCN8s(vgg16_dir='synthetic:3', num_classes=19, widths=SMALL)
    m2.engine.set_params(m.engine.get_params())
    m2.evaluate(gen(2, 32, 64, 1), 1, metrics={'loss'})
    assert np.isfinite(a) and abs(a - m2.metric_values[0]) <= 1e-6 * abs(a)
