"""Whole-path parity: the HIP library (through the C ABI) against the CPU oracle on
the same seeded inputs.  Tolerances: logits within 1e-3 absolute (BASELINE.json
north_star), argmax identical wherever the oracle's top-2 softmax margin exceeds
1e-4, gradients within 3e-4 of each tensor's max magnitude along the device's ReLU / max-pool
decisions (device_decisions: fixed seeds, no search for tie-free cases)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import fcn8s_oracle as orc  # noqa: E402  (checker only)

SMALL = (8, 16, 32, 64, 64, 128, 128)


def make_engine(widths=None, C=20, seed=0, options=None):
    from fcn8s_tensorflow_amd.engine import Engine
    return Engine(C, widths=widths, device_id=0, seed=seed, options=options or {})


def batch(n, h, w, C=20, seed=0):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8), rng.integers(0, C, (n, h, w), dtype=np.uint8))


def case(widths, n, h, w, seed, decoder_std_scale=30.0):
    """(params, images, labels) of ONE fixed seed -- no search for a convenient one."""
    P = orc.init_params(20, widths or orc.DEFAULT_WIDTHS, seed=seed, decoder_std_scale=decoder_std_scale, bias_std=0.05)
    img, lab = batch(n, h, w, seed=seed + 100)
    return P, img, lab


def device_decisions(e, P, img, nhw, relu_tol=1e-5, tie_tol=2e-5, max_frac=1e-4, **fwd_kw):
    """The discrete decisions the device's last training pass took -- which ReLU units are on (Engine.relu_branches) and where each
    max-pool window routes its gradient (Engine.pool_routes) -- after checking that they differ from the oracle's own decisions only
    where the decision is a coin flip in fp32: a ReLU unit may differ only if its activation is within `relu_tol` of zero (relative to
    the layer's largest), a pool route only if the oracle's two largest window entries agree to `tie_tol` of the layer's largest
    activation (Winograd F(6x6) carries a round-off of 2e-5 of the output range, tools/winograd_matrices.py; measured worst gap at a
    differing route at 1024x512: 4.4e-6) -- or the window's maximum is within relu_tol of zero, for routes that differ in on/off.  Gradient parity is
    then taken along these decisions
    (oracle `branches=` / `routes=`): both sides differentiate the same piecewise-linear function, on any seed."""
    br = e.relu_branches(nhw)
    rt = e.pool_routes(nhw)
    _, acts = orc.forward(P, img, keep=True, **fwd_kw)
    stats = {"relu_units": 0, "relu_differ": 0, "relu_worst": 0.0, "windows": 0, "routes_differ": 0, "route_worst_gap": 0.0}
    for k, on in br.items():
        ref = acts[k]
        stats["relu_units"] += on.size
        d = on != (ref > 0)
        if d.any():
            stats["relu_differ"] += int(d.sum())
            gpu = e.activation(k, ref.shape, missing_ok=True)          # (None: fused with the next conv's input transform, no tensor to look at)
            big = np.abs(ref[d]) if gpu is None else np.maximum(np.abs(gpu[d]), np.abs(ref[d]))
            stats["relu_worst"] = max(stats["relu_worst"], float(big.max() / (np.abs(ref).max() + 1e-30)))
    own, gaps = orc.pool_routes(acts)
    for b, nconv in enumerate(orc.CONVS_PER_BLOCK, start=1):
        k = "pool%d" % b
        stats["windows"] += own[k].size
        d = rt[k] != own[k]
        if d.any():
            stats["routes_differ"] += int(d.sum())
            onoff = d & ((rt[k] == 4) != (own[k] == 4))                 # differ in whether the window is on at all: a ReLU coin flip
            tie = d & ~onoff
            if tie.any():
                stats["route_worst_gap"] = max(stats["route_worst_gap"], float(gaps[k][tie].max()))
            if onoff.any():
                top = acts[k][onoff]
                stats["relu_worst"] = max(stats["relu_worst"], float(np.abs(top).max() / (np.abs(acts[k]).max() + 1e-30)))
    assert stats["relu_differ"] <= max_frac * stats["relu_units"] and stats["relu_worst"] < relu_tol, stats
    assert stats["routes_differ"] <= 10 * max_frac * stats["windows"] and stats["route_worst_gap"] <= tie_tol, stats
    return br, rt, stats


def rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() / (np.abs(b).max() + 1e-30))


def argmax_agree(pred, sm_ref, margin=1e-4):
    ref = np.argmax(sm_ref, -1)
    srt = np.sort(sm_ref, -1)
    safe = (srt[..., -1] - srt[..., -2]) > margin
    return (pred[safe] == ref[safe]).all(), float((~safe).mean())


@pytest.mark.parametrize("widths,n,h,w", [(SMALL, 2, 64, 96), (None, 1, 32, 64)])
def test_forward_logits_and_argmax(widths, n, h, w):
    P = orc.init_params(20, widths or orc.DEFAULT_WIDTHS, seed=1, decoder_std_scale=30.0, bias_std=0.05)
    img, _ = batch(n, h, w)
    e = make_engine(widths)
    e.set_params(P)
    pred = e.predict(img, argmax=True)
    assert pred.dtype == np.int64 and pred.shape == (n, h, w)
    logits = e.activation("logits", (n, h, w, 20))
    ref, acts = orc.forward(P, img, keep=True)
    assert np.abs(logits - ref).max() < 1e-3 * max(1.0, np.abs(ref).max())
    for name in ("pool3", "pool4", "fc7"):
        a = e.activation(name, acts[name].shape)
        assert rel(a, acts[name]) < 1e-4, name
    sm_ref = orc.softmax(ref)
    ok, frac_close = argmax_agree(pred, sm_ref)
    assert ok and frac_close < 0.05
    sm = e.predict(img, argmax=False)
    assert sm.dtype == np.float32 and np.abs(sm - orc.softmax(logits)).max() < 1e-6   # kernel vs softmax of its own logits
    assert np.abs(sm - sm_ref).max() < 1e-3                                          # end to end vs the oracle
    # float32 images take the same path as uint8 (the reference feeds either)
    pred_f = e.predict(img.astype(np.float32), argmax=True)
    np.testing.assert_array_equal(pred_f, pred)
    e.close()


@pytest.mark.parametrize("widths,n,h,w,l2", [(SMALL, 2, 64, 64, 0.0), (SMALL, 1, 32, 96, 1e-2), (None, 1, 32, 32, 0.0),
                                                (None, 2, 32, 64, 0.0),    # full width, W % 64 == 0: the specialised conv1_1 / 3x3 wgrad kernels
                                                (SMALL, 1, 128, 128, 1e-3),   # 4x4 fc6 map: fc6 through the Winograd sub-filter decomposition
                                                (SMALL, 1, 96, 160, 1e-3), (SMALL, 2, 64, 224, 0.0),    # sizes that are not multiples of the 6x6 tile in any block
                                                ((64, 192, 192, 64, 64, 128, 192), 1, 96, 160, 0.0)])   # widths (192) the transposed-B GEMM of the adjoint data gradients does not take
def test_gradients(widths, n, h, w, l2):
    """All 42 gradient tensors on a fixed seed per shape, the oracle differentiating along the device's ReLU / max-pool decisions
    (device_decisions: those may differ from the oracle's own only at fp32 coin flips)."""
    P, img, lab = case(widths, n, h, w, seed=2)
    e = make_engine(widths)
    e.set_params(P)
    loss = e.forward_backward(img, orc.one_hot(lab, 20), keep_prob=1.0, l2_rate=l2)   # one-hot like the reference feeds
    g = e.get_grads()
    br, rt, stats = device_decisions(e, P, img, (n, h, w))
    e.close()
    loss_ref, g_ref, _ = orc.loss_and_grads(P, img, orc.one_hot(lab, 20).astype(np.float32), l2_rate=l2, branches=br, routes=rt)
    assert abs(loss - loss_ref) < 1e-4 * max(1.0, abs(loss_ref))
    errs = {k: rel(g[k], g_ref[k]) for k in g_ref}
    worst = max(errs, key=errs.get)
    print("%s: %s; worst gradient error %s %.2e" % ((widths, n, h, w), stats, worst, errs[worst]))
    assert errs[worst] < 3e-4, (worst, errs[worst])        # measured: at most 1e-4 (the last transposed conv's kernel), 4e-5 elsewhere


@pytest.mark.parametrize("n,hw", [(2, 64), (1, 128)])      # 128: fc6 runs through the Winograd path (dropout fused in its output transform)
def test_dropout_statistics_and_parity(n, hw):
    widths = SMALL
    P, img, lab = case(widths, n, hw, hw, seed=4)
    e = make_engine(widths, seed=1234)
    e.set_params(P)
    loss = e.forward_backward(img, lab, keep_prob=0.5)
    m6, m7 = e.dropout_masks((n, hw // 32, hw // 32, widths[5]), (n, hw // 32, hw // 32, widths[6]))
    assert set(np.unique(m6)) <= {0.0, 1.0} and 0.3 < m6.mean() < 0.7 and 0.3 < m7.mean() < 0.7
    assert not np.array_equal(m6, m7)
    g = e.get_grads()
    rt = e.pool_routes((n, hw, hw))           # (the fc6 / fc7 records carry the dropout mask here, so only the pool routes are aligned)
    e.close()
    loss_ref, g_ref, _ = orc.loss_and_grads(P, img, orc.one_hot(lab, 20).astype(np.float32), keep_prob=0.5, masks=(m6, m7), routes=rt)
    assert abs(loss - loss_ref) < 1e-4 * max(1.0, abs(loss_ref))
    for k in g_ref:
        assert rel(g[k], g_ref[k]) < 2e-3, k


@pytest.mark.parametrize("widths,n,h,w", [(SMALL, 2, 64, 96), (SMALL, 1, 128, 128), (None, 1, 32, 64)])
def test_bf16_fc_mode_config5(widths, n, h, w):
    """BASELINE config 5's arithmetic: forward fc6 / fc7 on the bf16 MFMA (operands rounded to bfloat16, fp32
    accumulate), everything else fp32.  Parity is against the oracle running the SAME rounding (logits 1e-3, gradients
    1e-2 in L2); the distance to the pure-fp32 oracle is what the mode costs and is only reported."""
    # full width: a milder decoder than the fp32 tests use, so that the logits are O(1-10) -- with logits in the
    # hundreds the softmax saturates and turns the 2e-4 bf16-boundary effect (below) into percent-level gradient changes
    P, img, lab = case(widths, n, h, w, seed=6, decoder_std_scale=30.0 if widths else 6.0)
    e = make_engine(widths)
    with pytest.raises(ValueError):
        e.set_precision('fp16')
    e.set_precision('bf16_fc')
    e.set_params(P)
    pred = e.predict(img, argmax=True)
    logits = e.activation("logits", (n, h, w, 20))
    ref, acts = orc.forward(P, img, keep=True, bf16_fc=True)
    scale = max(1.0, float(np.abs(ref).max()))
    assert np.abs(logits - ref).max() < 1e-3 * scale
    # (an input that differs from the oracle's by fp32 round-off can land on the other side of a bf16 rounding
    #  boundary, a 2^-9 step for that operand -- hence 1e-3 here where the fp32 mode holds 1e-4)
    assert rel(e.activation("fc7", acts["fc7"].shape), acts["fc7"]) < 1e-3
    # argmax: identical wherever the oracle's top-2 LOGIT margin exceeds twice the logit tolerance of this mode
    srt = np.sort(ref, -1)
    safe = (srt[..., -1] - srt[..., -2]) > 2e-3 * scale
    assert safe.mean() > 0.9 and (pred[safe] == np.argmax(ref, -1)[safe]).all()
    ref32 = orc.forward(P, img)
    cost = float(np.abs(ref - ref32).max()) / scale
    assert 1e-6 < cost < 5e-2, cost                      # bf16 rounding is visible, and small
    assert np.abs(logits - ref32).max() > 0.2 * np.abs(ref - ref32).max()      # the GPU really took the bf16 path

    onehot = orc.one_hot(lab, 20)
    loss = e.forward_backward(img, onehot, keep_prob=1.0, l2_rate=1e-3)
    # along the device's decisions; a bf16 rounding-boundary flip moves fc6 / fc7 pre-activations by ~2e-4 of their scale, so ReLU units
    # up to 1e-3 of the layer's largest may legitimately sit on the other side
    br, rt, _ = device_decisions(e, P, img, (n, h, w), relu_tol=1e-3, tie_tol=1e-3, bf16_fc=True)
    loss_ref, g_ref, _ = orc.loss_and_grads(P, img, onehot.astype(np.float32), l2_rate=1e-3, bf16_fc=True, branches=br, routes=rt)
    assert abs(loss - loss_ref) < 1e-4 * max(1.0, abs(loss_ref))
    g = e.get_grads()
    for k in g_ref:
        # L2-relative, 1e-2, where the fp32 mode holds 2e-3 element-wise (and measures 1e-4): the bf16 boundary effect above
        # perturbs fc6 / fc7 pre-activations by ~2e-4 of their scale, enough to switch an occasional ReLU unit that sits at
        # zero on or off -- a whole row / column of a weight gradient then differs (a discrete, legitimate difference that an
        # element-wise max would report as several percent), while everything else agrees to round-off
        gk, rk = np.asarray(g[k], np.float64), np.asarray(g_ref[k], np.float64)
        l2 = float(np.linalg.norm(gk - rk) / (np.linalg.norm(rk) + 1e-30))
        assert l2 < 1e-2, (k, l2)
        assert rel(gk, rk) < 1e-1, (k, rel(gk, rk))                 # no element is grossly off

    # dropout uses the same Philox stream in both precisions: the masks the library reports reproduce its loss
    loss_d = e.forward_backward(img, lab, keep_prob=0.5)
    m6, m7 = e.dropout_masks((n, h // 32, w // 32, e.widths[5]), (n, h // 32, w // 32, e.widths[6]))
    loss_dref, _, _ = orc.loss_and_grads(P, img, onehot.astype(np.float32), keep_prob=0.5, masks=(m6, m7), bf16_fc=True)
    assert abs(loss_d - loss_dref) < 1e-4 * max(1.0, abs(loss_dref))
    # back to fp32: bit-identical to an engine that never left it
    e.set_precision('fp32')
    a = e.predict(img, argmax=False)
    e2 = make_engine(widths); e2.set_params(P)
    np.testing.assert_array_equal(a, e2.predict(img, argmax=False))
    e.close(); e2.close()


@pytest.mark.parametrize("precision", ["fp32", "f32x3"])
@pytest.mark.parametrize("widths,n,h,w,l2", [(None, 2, 32, 64, 0.0), (SMALL, 1, 128, 128, 1e-3), (SMALL, 1, 96, 160, 1e-3)])
def test_gradients_along_the_device_branches(precision, widths, n, h, w, l2):
    """Gradient parity on a FIXED seed in both arithmetic modes, made independent of ReLU coin flips: a pre-activation the oracle computes as
    -1e-7 of the layer's range and the GPU as +1e-7 (both inside fp32 round-off) switches one element of dZ on, which moves a whole
    row of a weight gradient by far more than any tolerance (on random full-width cases at 2 x 32 x 64 that happens in 5 of 14 seeds).
    So the oracle differentiates along the branches the device took (Engine.relu_branches -> oracle `branches=`), and the test checks
    separately that those differ from the oracle's own only at units within round-off of zero.  FCN8S_PREC_F32X3 (every large GEMM on
    the bf16 MFMA, fp32 operands split exactly into three bf16 pieces) must hold the same bounds as fp32 and must have run the split kernels."""
    e = make_engine(widths)
    e.set_precision(precision)
    seed = 2
    P = orc.init_params(20, widths or orc.DEFAULT_WIDTHS, seed=seed, decoder_std_scale=30.0, bias_std=0.05)
    img, lab = batch(n, h, w, seed=seed + 100)
    e.set_params(P)
    e.profile(2); e.profile_reset()
    loss = e.forward_backward(img, orc.one_hot(lab, 20), keep_prob=1.0, l2_rate=l2)
    kernels = [k for k in e.profile_results() if k.startswith("kernel:")]
    e.profile(0)
    if precision == "f32x3":
        assert any("gemm_glds_x3_kernel" in k for k in kernels) and any("wgrad_glds_x3_kernel" in k for k in kernels), kernels
        assert not any("gemm_glds_kernel" in k or "wgrad_glds_kernel" in k for k in kernels), kernels
    else:
        assert not any("_x3_kernel" in k for k in kernels), kernels
    g = e.get_grads()
    logits = e.activation("logits", (n, h, w, 20))
    br, rt, stats = device_decisions(e, P, img, (n, h, w))       # only decisions within round-off of a tie may differ
    n_diff, n_units, worst = stats["relu_differ"], stats["relu_units"], stats["relu_worst"]
    loss_ref, g_ref, logits_ref = orc.loss_and_grads(P, img, orc.one_hot(lab, 20).astype(np.float32), l2_rate=l2, branches=br, routes=rt)
    assert abs(loss - loss_ref) < 1e-4 * max(1.0, abs(loss_ref))
    assert np.abs(logits - logits_ref).max() < 1e-3 * max(1.0, np.abs(logits_ref).max())
    errs = {k: rel(g[k], g_ref[k]) for k in g_ref}
    worst_k = max(errs, key=errs.get)
    print("%s %s: %d of %d ReLU units differ from the oracle's (largest such activation %.1e of its layer's max); worst gradient error %s %.2e"
          % (precision, (widths, n, h, w), n_diff, n_units, worst, worst_k, errs[worst_k]))
    assert errs[worst_k] < 3e-4, (worst_k, errs[worst_k])
    e.close()


def test_f32x2_mode_gradients():
    """FCN8S_PREC_F32X2 ('f32x2'): every LDS-DMA GEMM of the step with two bf16 pieces per operand (16 significand bits enter each
    product, fp32 accumulation) -- a reduced-precision mode, so its bound is its own: logits to 1e-3 (the fp32 bound still holds) and
    gradients along the device's decisions to 3e-3 of each tensor's largest entry (fp32 / f32x3: 3e-4; measured here 1.05e-3, on the last
    transposed conv's kernel, whose entries are sums over every pixel of products that nearly cancel), on the full-width case of
    test_gradients_along_the_device_branches.  The split kernels must have run, the f32 and x3 ones must not."""
    e = make_engine(None)
    e.set_precision("f32x2")
    n, h, w, seed = 2, 32, 64, 2
    P = orc.init_params(20, orc.DEFAULT_WIDTHS, seed=seed, decoder_std_scale=30.0, bias_std=0.05)
    img, lab = batch(n, h, w, seed=seed + 100)
    e.set_params(P)
    e.profile(2); e.profile_reset()
    loss = e.forward_backward(img, orc.one_hot(lab, 20), keep_prob=1.0, l2_rate=0.0)
    kernels = [k for k in e.profile_results() if k.startswith("kernel:")]
    e.profile(0)
    assert any("gemm_glds_x2_kernel" in k for k in kernels) and any("wgrad_glds_x2_kernel" in k for k in kernels) and any("gemm_glds_nt_x2_kernel" in k for k in kernels), kernels
    assert not any("gemm_glds_kernel" in k or "wgrad_glds_kernel" in k or "_x3_kernel" in k for k in kernels), kernels
    g = e.get_grads()
    logits = e.activation("logits", (n, h, w, 20))
    br, rt, stats = device_decisions(e, P, img, (n, h, w), relu_tol=1e-4, tie_tol=1e-4)
    loss_ref, g_ref, logits_ref = orc.loss_and_grads(P, img, orc.one_hot(lab, 20).astype(np.float32), l2_rate=0.0, branches=br, routes=rt)
    assert abs(loss - loss_ref) < 1e-4 * max(1.0, abs(loss_ref))
    lerr = float(np.abs(logits - logits_ref).max() / max(1.0, np.abs(logits_ref).max()))
    errs = {k: rel(g[k], g_ref[k]) for k in g_ref}
    worst_k = max(errs, key=errs.get)
    print("f32x2: logits %.2e of their scale; worst gradient error %s %.2e; %d of %d ReLU units on the other side (largest %.1e)"
          % (lerr, worst_k, errs[worst_k], stats["relu_differ"], stats["relu_units"], stats["relu_worst"]))
    assert lerr < 1e-3
    assert errs[worst_k] < 3e-3, (worst_k, errs[worst_k])
    e.close()


@pytest.mark.parametrize("precision", ["fp32", "f32x3"])
def test_training_overfits_one_batch(precision):
    """The step is usable, not just locally correct: 40 TF-Adam steps on one fixed batch (small widths, dropout off) drive the loss
    from ln(20)-ish well down, monotonically on a 5-step average, in either arithmetic mode; both modes end within a few percent of
    each other (their steps differ by fp32 round-off only, which the optimisation does not amplify on this scale)."""
    P = orc.init_params(20, SMALL, seed=3, decoder_std_scale=30.0, bias_std=0.05)
    img, lab = batch(2, 64, 96, seed=5)
    e = make_engine(SMALL)
    e.set_params(P)
    e.set_precision(precision)
    losses = [e.train_step(img, lab, 2e-4, keep_prob=1.0)[0] for _ in range(40)]
    e.close()
    assert all(np.isfinite(losses))
    avg = [float(np.mean(losses[i:i + 5])) for i in range(0, 40, 5)]
    assert all(b < a for a, b in zip(avg, avg[1:])), avg
    assert losses[-1] < 0.6 * losses[0], (losses[0], losses[-1])
    test_training_overfits_one_batch.final = getattr(test_training_overfits_one_batch, "final", {})
    test_training_overfits_one_batch.final[precision] = losses[-1]
    f = test_training_overfits_one_batch.final
    if len(f) == 2:
        assert abs(f["fp32"] - f["f32x3"]) < 0.05 * f["fp32"], f


def test_tf_adam_training_steps():
    """Three fused train steps (sess.run(train_op)): each step is checked against the oracle's
    gradient + TF-Adam update started from the library's own pre-step state, so that Adam's
    sign-like first steps (update ~ lr*g/|g|) cannot amplify round-off in near-zero gradients
    into a chaotic divergence between the two trajectories."""
    widths = SMALL
    P = orc.init_params(20, widths, seed=6, decoder_std_scale=30.0, bias_std=0.05)
    # (reductions in a fixed order: the parameters steps 2 and 3 start from are then the same in every run -- with float atomics they differ in the last
    #  bit from run to run, and once in a few hundred runs of this small network a ReLU unit sits within that bit of zero: one full-suite run of round 5 saw
    #  conv1_1/filter 3.7 % off at step 3 and three reruns did not)
    e = make_engine(widths, options={"deterministic": 1})
    e.set_params(P)
    lr = 1e-3

    def unflat(flat):
        return {k: flat[off:off + int(np.prod(shp))].reshape(shp).copy() for k, (shp, off) in e.specs.items()}

    for t in range(1, 4):
        before = e.get_params()
        mflat, vflat = e.get_opt_state()
        m, v_ = unflat(mflat), unflat(vflat)
        img, lab = batch(2, 32, 64, seed=10 * t)
        loss, step = e.train_step(img, lab, learning_rate=lr, keep_prob=1.0, l2_rate=1e-3)
        assert step == t
        rt = e.pool_routes((2, 32, 64))                # the oracle routes its max-pool gradients like the step did
        loss_ref, g_ref, _ = orc.loss_and_grads(before, img, orc.one_hot(lab, 20).astype(np.float32), l2_rate=1e-3, routes=rt)
        assert abs(loss - loss_ref) < 2e-4 * max(1.0, abs(loss_ref))
        got = e.get_params()
        g_gpu = e.get_grads()                     # the gradients the fused update consumed
        for k in before:
            assert rel(g_gpu[k], g_ref[k]) < 2e-3, (k, t)
            want, _, _ = orc.tf_adam_step(before[k], g_gpu[k], m[k], v_[k], t, lr)
            assert np.abs(got[k] - want).max() < 2e-6, (k, t, np.abs(got[k] - want).max())
    assert e.global_step == 3
    e.close()


def test_eval_metrics():
    """Streaming metrics (fcn8s_tensorflow.py:273-322).  Integer work is exact: the confusion matrix the library accumulates equals
    the one built from its own per-pixel predictions; those predictions equal the oracle's wherever the oracle's top-2 softmax
    margin exceeds 1e-4 and are one of the oracle's two best classes elsewhere; mean IoU / accuracy follow the reference's
    formulas exactly on that matrix and differ from the oracle's values by no more than the near-tie pixels can move them."""
    widths = SMALL
    P = orc.init_params(20, widths, seed=7, decoder_std_scale=30.0, bias_std=0.05)
    e = make_engine(widths)
    e.set_params(P)
    sm = orc.StreamingMetrics(20)
    e.metrics_reset()
    cm_own = np.zeros((20, 20), np.int64)
    n_unsafe = 0
    for i, n in enumerate((2, 1, 2)):            # ragged batches: the per-batch loss mean weighs them equally
        img, lab = batch(n, 32, 64, seed=20 + i)
        lab[:, :, :16] = 3                        # leave some classes absent from the ground truth
        e.eval_step(img, orc.one_hot(lab, 20))
        loss, l, p = orc.eval_step(P, img, orc.one_hot(lab, 20).astype(np.float32))
        sm.update(loss, l, p)
        pred = e.predict(img, argmax=True)        # the same forward pass, per pixel
        soft = orc.softmax(orc.forward(P, img))
        order = np.argsort(soft, -1)
        safe = (np.take_along_axis(soft, order[..., -1:], -1) - np.take_along_axis(soft, order[..., -2:-1], -1))[..., 0] > 1e-4
        assert (pred[safe] == p[safe]).all()
        assert ((pred == order[..., -1]) | (pred == order[..., -2]))[~safe].all()
        n_unsafe += int((~safe).sum())
        cm_own += orc.confusion_matrix(lab, pred, 20)
    loss, miou, acc = e.metrics_get()
    rl, rm, ra = sm.values()
    cm, _, cnt = e.metrics_raw()
    total = 5 * 32 * 64
    assert cnt == 3 and cm.sum() == total
    assert abs(loss - rl) < 1e-4 * max(1, abs(rl))
    np.testing.assert_array_equal(cm, cm_own)                                       # bit-exact counting
    assert abs(miou - orc.mean_iou_from_confusion(cm)) < 1e-12                      # the reference's formulas on that matrix
    assert abs(acc - orc.accuracy_from_confusion(cm)) < 1e-12
    assert n_unsafe <= 0.002 * total
    assert abs(acc - ra) <= n_unsafe / total + 1e-12                                # a near-tie pixel moves accuracy by at most 1/total
    assert abs(miou - rm) <= 1e-12 if n_unsafe == 0 else abs(miou - rm) < 5e-3
    # TF 1.3.0's variant: absent classes count as IoU 0 in the mean
    _, miou_all, _ = e.metrics_get(all_classes=True)
    assert abs(miou_all - orc.mean_iou_from_confusion(cm, valid_only=False)) < 1e-12
    # ... which differs from the valid-class mean as soon as a class occurs neither in the labels nor in the predictions
    import ctypes as C
    from fcn8s_tensorflow_amd import _lib as L
    cm2 = cm.copy(); cm2[7, :] = 0; cm2[:, 7] = 0; cm2[12, :] = 0; cm2[:, 12] = 0
    L.check(L.lib.fcn8s_metrics_set_raw(e.h, np.ascontiguousarray(cm2).ctypes.data_as(C.c_void_p), 1.5, 3), e.h)
    l2, miou_valid, acc2 = e.metrics_get()
    _, miou_all, _ = e.metrics_get(all_classes=True)
    assert l2 == 0.5
    assert abs(miou_valid - orc.mean_iou_from_confusion(cm2, valid_only=True)) < 1e-12
    assert abs(miou_all - orc.mean_iou_from_confusion(cm2, valid_only=False)) < 1e-12
    assert abs(miou_all - miou_valid * 18 / 20) < 1e-12
    e.metrics_reset()
    assert e.metrics_raw()[0].sum() == 0
    e.close()


def test_out_of_range_label_ids_are_ignored():
    """Ids outside [0, C) -- a 255 'ignore' id, or the id an all-zero one-hot row is given -- contribute neither loss nor
    gradient (TF's softmax_cross_entropy_with_logits of an all-zero row is 0, fcn8s_tensorflow.py:253)."""
    widths = SMALL
    P = orc.init_params(20, widths, seed=2, decoder_std_scale=30.0, bias_std=0.05)
    img, lab = batch(2, 32, 64, seed=9)
    onehot = orc.one_hot(lab, 20).astype(np.float32)
    hole = np.zeros(lab.shape, bool); hole[:, 5:20, 10:40] = True
    onehot[hole] = 0.0                            # all-zero rows
    lab_ign = lab.copy(); lab_ign[hole] = 255
    e = make_engine(widths)
    e.set_params(P)
    loss_ids = e.forward_backward(img, lab_ign, keep_prob=1.0)
    g_ids = e.get_grads()
    loss_ref, g_ref, _ = orc.loss_and_grads(P, img, onehot)
    assert abs(loss_ids - loss_ref) < 1e-4 * max(1.0, abs(loss_ref))
    # TF's fused kernel returns softmax - labels as the gradient even for an all-zero row (it assumes rows sum to 1); the true
    # derivative of -sum(labels * log_softmax) is zero there, which is what autograd (the oracle) and the library compute
    for k in g_ref:
        assert rel(g_ids[k], g_ref[k]) < 2e-3, k
    e.close()


def test_algorithm_options():
    """fcn8s_set_option: the maintained variants of the 3x3 stack (F(6x6) / F(4x4) / direct) and of the last transposed conv agree
    with each other to fp32 round-off, options round-trip, unknown keys are errors."""
    P = orc.init_params(20, SMALL, seed=5, decoder_std_scale=30.0, bias_std=0.05)
    img, lab = batch(2, 96, 160, seed=3)       # (two images: a single image gets its tiles chosen with GEMM-row padding in mind, model.hip wino_tile_for)
    outs = {}
    for name, opts in (("default", {}), ("f4", {"winograd_tile": 4}), ("direct", {"winograd_min_cin": 0, "winograd_fc6": 0}), ("phases", {"tconv_gemm": 0})):
        e = make_engine(SMALL)
        for k, v in opts.items():
            e.set_option(k, v)
            assert e.get_option(k) == v
        e.set_params(P)
        e.forward_backward(img, lab, keep_prob=1.0)
        outs[name] = (e.activation("logits", (2, 96, 160, 20)), e.get_grads())
        if name == "default":
            assert e.get_option("winograd_tile") == 6 and e.get_option("winograd_min_cin") == 64
            with pytest.raises(ValueError):
                e.set_option("no_such_option", 1)
            with pytest.raises(ValueError):
                e.set_option("winograd_tile", 5)
            e.set_option("winograd_tile", 4)                   # switching after a pass: the workspace is rebuilt
            e.forward_backward(img, lab, keep_prob=1.0)
            np.testing.assert_allclose(e.activation("logits", (2, 96, 160, 20)), outs["default"][0], rtol=0, atol=1e-3 * np.abs(outs["default"][0]).max())
        e.close()
    ref_l, ref_g = outs["direct"]
    for name in ("default", "f4", "phases"):
        l, g = outs[name]
        assert np.abs(l - ref_l).max() < 1e-3 * np.abs(ref_l).max(), name
        if name != "direct":
            assert not np.array_equal(l, ref_l) or name == "phases"
    assert not np.array_equal(outs["default"][0], outs["f4"][0])          # the options really select different arithmetic


def test_errors_are_python_exceptions():
    e = make_engine(SMALL)
    img, lab = batch(1, 48, 64)
    with pytest.raises(ValueError):
        e.predict(img)                            # 48 is not a multiple of 32
    with pytest.raises(ValueError):
        e.set_params({"nope/filter": np.zeros(3, np.float32)})
    with pytest.raises(ValueError):
        e.train_step(batch(1, 32, 32)[0], np.zeros((1, 32, 16), np.uint8), 1e-3)
    # parity instrumentation: only after a TRAINING forward pass, and only with the exact size
    import ctypes as C
    from fcn8s_tensorflow_amd import _lib as L
    buf = np.empty(8, np.uint8)
    assert L.lib.fcn8s_get_pool_routing(e.h, 1, buf.ctypes.data_as(C.c_void_p), buf.size) == L.ERR_STATE
    e.predict(batch(1, 32, 32)[0])
    assert L.lib.fcn8s_get_pool_routing(e.h, 1, buf.ctypes.data_as(C.c_void_p), buf.size) == L.ERR_STATE      # a prediction keeps no routes
    img32, lab32 = batch(1, 32, 32)
    e.forward_backward(img32, lab32)
    assert L.lib.fcn8s_get_pool_routing(e.h, 1, buf.ctypes.data_as(C.c_void_p), buf.size) == L.ERR_SHAPE
    assert L.lib.fcn8s_get_pool_routing(e.h, 6, buf.ctypes.data_as(C.c_void_p), buf.size) == L.ERR_BAD_ARG
    routes = e.pool_routes((1, 32, 32))
    assert [routes["pool%d" % b].shape for b in range(1, 6)] == [(1, 32 >> b, 32 >> b, SMALL[b - 1]) for b in range(1, 6)]
    assert all(r.max() <= 4 for r in routes.values())
    # the routes say where pool_b's gradient goes: a route of 4 (off) exactly where the pooled activation is not > 0
    p1 = e.activation("pool1", (1, 16, 16, SMALL[0]))
    np.testing.assert_array_equal(routes["pool1"] == 4, ~(p1 > 0))
    assert e.check_replicas() is True                  # one rank: nothing to compare
    e.close()


def test_frozen_parameters_cache_and_invalidation():
    """fcn8s_freeze_params: identical predictions with the cached transformed filters, across image sizes (the Winograd tile
    and with it the bank's shape depends on the size), and every parameter change leaves the frozen state."""
    widths = SMALL
    P = orc.init_params(20, widths, seed=3, decoder_std_scale=30.0, bias_std=0.05)
    img, _ = batch(2, 128, 160)
    small, _ = batch(1, 32, 64, seed=5)
    e = make_engine(widths); e.set_params(P)
    ref = e.predict(img, argmax=False); ref_small = e.predict(small, argmax=False)
    e.freeze(True)
    for _ in range(2):                                   # first call fills the cache, second uses it
        np.testing.assert_array_equal(e.predict(img, argmax=False), ref)
        np.testing.assert_array_equal(e.predict(small, argmax=False), ref_small)
    P2 = orc.init_params(20, widths, seed=4, decoder_std_scale=30.0, bias_std=0.05)
    e.set_params(P2)                                     # unfreezes: no stale filters
    e2 = make_engine(widths); e2.set_params(P2)
    np.testing.assert_array_equal(e.predict(img, argmax=False), e2.predict(img, argmax=False))
    e.freeze(True); e.predict(img)
    e.train_step(img, batch(2, 128, 160)[1], 1e-3, keep_prob=1.0)      # a training step unfreezes as well ...
    after = e.predict(img, argmax=False)                               # ... so this must not see the filters cached before it
    e.freeze(False)
    np.testing.assert_array_equal(after, e.predict(img, argmax=False))
    assert np.abs(after - e2.predict(img, argmax=False)).max() > 0     # and the step did change the weights
    e.close(); e2.close()


def test_bucket_api_and_fused_step_give_the_same_gradients():
    """A full-width split-phase step (fcn8s_forward_loss + fcn8s_backward_bucket) and the fused fcn8s_train_step run one schedule and
    produce the same loss and gradients.  The retired schedule options are unknown keys now."""
    import ctypes as C
    from fcn8s_tensorflow_amd import _lib as L
    from fcn8s_tensorflow_amd.engine import Engine
    P = orc.init_params(20, seed=3, decoder_std_scale=30.0, bias_std=0.05)
    img, lab = batch(1, 192, 192, seed=9)
    e = Engine(20)
    for key in (b"defer_wgrad", b"defer_start_block", b"defer_tail_cus", b"bf16_fuse_convert"):
        assert L.lib.fcn8s_set_option(e.h, key, 1) == L.ERR_NOT_FOUND, key
        v = C.c_int64(-1)
        assert L.lib.fcn8s_get_option(e.h, key, C.byref(v)) == L.ERR_NOT_FOUND, key
    e.set_params(P)
    loss2 = e.forward_backward(img, lab, keep_prob=1.0, l2_rate=1e-3)               # bucket API
    g2 = e.get_grads()
    loss, step = e.train_step(img, lab, 1e-6, keep_prob=1.0, l2_rate=1e-3)         # fused step, same parameters
    g1 = e.get_grads()                                                               # the gradients the update consumed
    e.close()
    assert loss == loss2
    for k in g2:
        # (split-K sums use float atomics: their order is not reproducible between two runs of the SAME schedule either)
        assert rel(g1[k], g2[k]) < 1e-4, k


def test_bf16_fc_256_tile_kernel():
    """The 256 x 256 LDS-DMA kernel of the bf16_fc mode (gemm_bf16.hip: zero-padded bf16 activations, transposed bf16 kernel, staggered
    wave groups) at a shape it takes -- full width, 4 x 256x256, i.e. 256 GEMM rows -- against the oracle applying the same operand
    rounding, and against the 128 x 128 kernel of the same mode (same products, another summation order); dropout uses the same Philox
    stream in both.  `bf16_gemm256` = 2 forces the kernel where option 1 (the default) would find too few tiles to fill the chip."""
    from fcn8s_tensorflow_amd.engine import Engine
    n, h, w = 4, 256, 256
    P = orc.init_params(20, seed=8, decoder_std_scale=6.0, bias_std=0.05)
    img, lab = batch(n, h, w, seed=21)
    outs = {}
    for mode in (2, 0):
        e = Engine(20, precision='bf16_fc', options={"bf16_gemm256": mode})
        e.set_params(P)
        e.profile(2); e.profile_reset()
        loss = e.forward_backward(img, lab, keep_prob=1.0, l2_rate=0.0)
        kernels = [k for k in e.profile_results() if k.startswith("kernel:")]
        e.profile(0)
        assert any("conv_bf16_256_kernel" in k for k in kernels) == (mode == 2), kernels
        fc6 = e.activation("fc6", (n, h // 32, w // 32, 4096)); fc7 = e.activation("fc7", (n, h // 32, w // 32, 4096))
        logits = e.activation("logits", (n, h, w, 20))
        loss_d = e.forward_backward(img, lab, keep_prob=0.5)
        m6, m7 = e.dropout_masks((n, h // 32, w // 32, 4096), (n, h // 32, w // 32, 4096))
        if mode == 2:        # frozen parameters: the transposed bf16 kernels are made once and reused, predictions unchanged
            e.freeze(True)
            p1 = e.predict(img, argmax=False); p2 = e.predict(img, argmax=False)
            np.testing.assert_array_equal(p1, p2)
            e.freeze(False)
            np.testing.assert_array_equal(p1, e.predict(img, argmax=False))
        outs[mode] = (loss, fc6, fc7, logits, loss_d, m6, m7)
        e.close()
    ref, acts = orc.forward(P, img, keep=True, bf16_fc=True)
    scale = max(1.0, float(np.abs(ref).max()))
    loss, fc6, fc7, logits = outs[2][:4]
    assert rel(fc6, acts["fc6"]) < 1e-3 and rel(fc7, acts["fc7"]) < 1e-3
    assert np.abs(logits - ref).max() < 1e-3 * scale
    # the two kernels of the mode agree to summation order
    assert rel(outs[2][1], outs[0][1]) < 1e-4 and rel(outs[2][2], outs[0][2]) < 1e-3 and abs(outs[2][0] - outs[0][0]) < 1e-4 * max(1.0, abs(outs[0][0]))
    np.testing.assert_array_equal(outs[2][5], outs[0][5]); np.testing.assert_array_equal(outs[2][6], outs[0][6])
    loss_dref, _, _ = orc.loss_and_grads(P, img, orc.one_hot(lab, 20).astype(np.float32), keep_prob=0.5, masks=(outs[2][5], outs[2][6]), bf16_fc=True)
    assert abs(outs[2][4] - loss_dref) < 1e-3 * max(1.0, abs(loss_dref))


def test_bf16_train_mode():
    """FCN8S_PREC_BF16_TRAIN ('bf16_train'): conv1_2 .. conv5_3, fc6 and fc7 as direct convolutions with bf16-rounded operands in
    the forward pass, the data gradient and the weight gradient (fp32 accumulate; conv1_1, pools, decoder, loss exact fp32; no Winograd transform
    anywhere) -- against the oracle in the same arithmetic (`bf16_train=True`: _ConvBf16Train).  A network whose widths are multiples of 64, two
    64 x 96 images (row counts 12 288 .. 12 per layer: whole and partial row tiles of the convolution kernel, split and unsplit weight gradients):
      (1) each layer's forward arithmetic exactly: the device's output against the same-rounding convolution of the DEVICE's own input (1e-4);
      (2) end to end: activations and logits against the oracle to 2e-2 of their range (inputs that differ by fp32 round-off cross bf16
          rounding boundaries: a 2^-8 step per crossing);
      (3) all gradients against the oracle's along the device's ReLU / pool decisions to 2e-2 in L2 (measured 7.3e-3) (the kernels' own arithmetic is held to 1e-5 by
          tests/test_ops_gpu.py::test_conv_bf16_train_kernels; what is left here is those boundary crossings, now also in dY);
      (4) the kernels that ran: conv_bf16_256_kernel<64|128|256> and wgrad_bf16_kernel, no Winograd kernel, no fp32 position GEMM;
      (5) a training step runs, and leaving the mode gives back the fp32 predictions of an engine that never entered it."""
    import torch
    from fcn8s_tensorflow_amd.engine import Engine
    widths = (64, 64, 128, 256, 256, 256, 128)
    n, h, w = 2, 64, 96
    P = orc.init_params(20, widths, seed=9, decoder_std_scale=6.0, bias_std=0.05)
    img, lab = batch(n, h, w, seed=31)
    # (option bf16_acts = 0: every activation also as an fp32 tensor, for (1)-(3) to look at; the default keeps a conv -> conv activation only as the
    #  consumer's bf16 copy -- same values into every product: test_bf16_train_without_fp32_inner_activations holds it to this engine's gradients bit for bit)
    e = Engine(20, widths=widths, precision="bf16_train", options={"bf16_acts": 0})
    e.set_params(P)
    e.profile(2); e.profile_reset()
    onehot = orc.one_hot(lab, 20)
    loss = e.forward_backward(img, onehot, keep_prob=1.0, l2_rate=1e-3)
    prof = e.profile_results()
    e.profile(0)
    kernels = {k[7:]: int(v["launches"]) for k, v in prof.items() if k.startswith("kernel:")}
    assert sum(v for k, v in kernels.items() if "conv_bf16_" in k) == 14 + 14, kernels          # 14 forward convolutions + 14 data gradients (none of either for conv1_1)
    assert sum(v for k, v in kernels.items() if "wgrad_bf16" in k) == 14, kernels
    # (which column tile a launch takes -- 64, 128 or 256 -- follows from its block count: at this size all take the 64-column tile; the three are
    #  held to the same arithmetic one by one in tests/test_ops_gpu.py::test_conv_bf16_train_kernels)
    assert not any("wino" in k or "gemm_glds_nt" in k or "_x2_" in k or "_x3_" in k for k in kernels), kernels      # (gemm_glds / wgrad_glds: the last transposed conv, exact fp32)
    logits = e.activation("logits", (n, h, w, 20))
    # (1) per layer, the device's own input
    rb = lambda t: t.to(torch.bfloat16).to(torch.float32)
    wd = widths
    shp = lambda name, d, c: (n, h >> d, w >> d, c)
    layers = [("conv1_1", "conv1_2", shp("", 0, wd[0]), shp("", 0, wd[0]), "conv1_2/filter", "conv1_2/biases"),
              ("pool1", "conv2_1", shp("", 1, wd[0]), shp("", 1, wd[1]), "conv2_1/filter", "conv2_1/biases"),
              ("conv3_1", "conv3_2", shp("", 2, wd[2]), shp("", 2, wd[2]), "conv3_2/filter", "conv3_2/biases"),
              ("conv5_2", "conv5_3", shp("", 4, wd[4]), shp("", 4, wd[4]), "conv5_3/filter", "conv5_3/biases"),
              ("pool5", "fc6", shp("", 5, wd[4]), shp("", 5, wd[5]), "fc6/weights", "fc6/biases"),
              ("fc6", "fc7", shp("", 5, wd[5]), shp("", 5, wd[6]), "fc7/weights", "fc7/biases")]
    for src, dst, sshape, dshape, wname, bname in layers:
        x = torch.from_numpy(e.activation(src, sshape)).permute(0, 3, 1, 2)
        wk = torch.from_numpy(P[wname]); k = wk.shape[0]
        want = torch.relu(torch.nn.functional.conv2d(rb(x), rb(wk).permute(3, 2, 0, 1), torch.from_numpy(P[bname]), padding=(k - 1) // 2)).permute(0, 2, 3, 1).numpy()
        got = e.activation(dst, dshape)
        assert rel(got, want) < 1e-4, (dst, rel(got, want))
    # (2) end to end
    ref, acts = orc.forward(P, img, keep=True, bf16_train=True)
    scale = max(1.0, float(np.abs(ref).max()))
    for k in ("conv1_2", "conv3_1", "conv4_2", "pool5", "fc7"):
        assert rel(e.activation(k, acts[k].shape), acts[k]) < 2e-2, (k, rel(e.activation(k, acts[k].shape), acts[k]))
    assert np.abs(logits - ref).max() < 2e-2 * scale
    ref32 = orc.forward(P, img)
    cost = float(np.abs(ref - ref32).max()) / scale
    assert 1e-5 < cost < 1e-1, cost
    assert np.abs(logits - ref32).max() > 0.2 * np.abs(ref - ref32).max()
    # (3) gradients along the device's decisions
    g = e.get_grads()
    br, rt, stats = device_decisions(e, P, img, (n, h, w), relu_tol=3e-2, tie_tol=3e-2, max_frac=5e-3, bf16_train=True)
    loss_ref, g_ref, _ = orc.loss_and_grads(P, img, onehot.astype(np.float32), l2_rate=1e-3, bf16_train=True, branches=br, routes=rt)
    _, g_32, _ = orc.loss_and_grads(P, img, onehot.astype(np.float32), l2_rate=1e-3, branches=br, routes=rt)
    assert abs(loss - loss_ref) < 2e-2 * max(1.0, abs(loss_ref))
    worst = ("", 0.0)
    for k in g_ref:
        gk, rk = np.asarray(g[k], np.float64), np.asarray(g_ref[k], np.float64)
        l2 = float(np.linalg.norm(gk - rk) / (np.linalg.norm(rk) + 1e-30))
        if l2 > worst[1]:
            worst = (k, l2)
        assert l2 < 2e-2, (k, l2)
    d32 = max(float(np.linalg.norm(np.asarray(g_ref[k], np.float64) - g_32[k]) / (np.linalg.norm(g_32[k]) + 1e-30)) for k in g_ref)
    print("bf16_train: worst gradient tensor %s %.2e in L2 against the same-arithmetic oracle (that oracle is %.2e from the fp32 graph's gradients); %s" % (worst[0], worst[1], d32, stats))
    # the mode's arithmetic is the same on every backward pass (round 5's held-back fc7 weight gradient ran the fp32 kernel: ADVICE round 5): the same fc6 / fc7
    # weight gradients on each repeat, to the round-off of their atomically joined split sums
    for rep in range(2):
        e.forward_backward(img, onehot, keep_prob=1.0, l2_rate=1e-3)
        g2 = e.get_grads()
        for k in ("fc7/weights", "fc6/weights", "conv4_2/filter", "fc7/biases"):
            assert rel(g2[k], g[k]) < 1e-5, (rep, k, rel(g2[k], g[k]))
    # (5)
    loss2, step = e.train_step(img, lab, 1e-6, keep_prob=0.5)
    assert step == 1 and np.isfinite(loss2)
    # the two options the mode overrides keep the CALLER's values: reported while the mode is on, and a change made meanwhile takes effect on leaving
    assert e.get_option("winograd_min_cin") == 64 and e.get_option("winograd_fc6") == 1
    e.set_option("winograd_min_cin", 128)
    assert e.get_option("winograd_min_cin") == 128
    e.set_precision('fp32')
    assert e.get_option("winograd_min_cin") == 128 and e.get_option("winograd_fc6") == 1
    e.set_option("winograd_min_cin", 64)
    e.set_params(P)
    a = e.predict(img, argmax=False)
    e2 = Engine(20, widths=widths); e2.set_params(P)
    np.testing.assert_array_equal(a, e2.predict(img, argmax=False))
    e.close(); e2.close()
    with pytest.raises(Exception):
        Engine(20, widths=SMALL, precision="bf16_train")            # widths that are not multiples of 64


def test_bf16_train_prediction_takes_the_training_data_flow():
    """Option `bf16_infer_copies` (default 1; round 6): an evaluation / prediction pass of FCN8S_PREC_BF16_TRAIN runs the training pass's kernels and data flow (padded
    bf16 copies from the producers' epilogues, flat-position kernel, pools on the copies), so its logits are the training pass's BIT FOR BIT at keep_prob 1; the
    round-5 flow (0: fp32 tensors converted layer by layer, tile kernel) adds a dot product's taps in another order: outputs that differ in their last fp32 bit
    round to the other bf16 neighbour in the next layer (a 2^-8 step per crossing), so the two flows agree to 2e-2 of the logit scale (measured 7.5e-3; the
    bound test_bf16_train_mode holds the mode to against its oracle) and give the same argmax wherever the top-2 margin exceeds 4e-2; metrics agree accordingly."""
    import torch
    from fcn8s_tensorflow_amd.engine import Engine
    widths = (64, 64, 128, 256, 256, 256, 128)
    n, h, w = 2, 64, 96
    P = orc.init_params(20, widths, seed=9, decoder_std_scale=6.0, bias_std=0.05)
    img, lab = batch(n, h, w, seed=31)
    e = Engine(20, widths=widths, precision="bf16_train")
    e.set_params(P)
    e.forward_backward(img, lab, keep_prob=1.0)
    lg_train = e.activation("logits", (n, h, w, 20)).copy()
    pred = e.predict(img, argmax=True)
    lg_pred = e.activation("logits", (n, h, w, 20)).copy()
    np.testing.assert_array_equal(lg_pred, lg_train)
    e.metrics_reset(); e.eval_step(img, lab); cm_new = e.metrics_raw()[0].copy()
    e.set_option("bf16_infer_copies", 0)
    pred0 = e.predict(img, argmax=True)
    lg0 = e.activation("logits", (n, h, w, 20))
    scale = max(1.0, float(np.abs(lg_train).max()))
    assert np.abs(lg0 - lg_train).max() < 2e-2 * scale, np.abs(lg0 - lg_train).max() / scale
    srt = np.sort(lg_train, -1)
    safe = (srt[..., -1] - srt[..., -2]) > 4e-2 * scale
    assert safe.mean() > 0.1 and (np.asarray(pred)[safe] == np.asarray(pred0)[safe]).all()
    e.metrics_reset(); e.eval_step(img, lab); cm_old = e.metrics_raw()[0]
    assert np.abs(cm_new.astype(np.int64) - cm_old.astype(np.int64)).sum() <= 2 * int((~safe).sum())
    e.close()


def test_bf16_train_without_fp32_inner_activations():
    """Option `bf16_acts` (default 1) of FCN8S_PREC_BF16_TRAIN: in a training pass the output of a conv that feeds another conv (conv1_1, conv2_1,
    conv3_1, conv3_2, ...) is written ONLY as the consumer's padded bf16 copy -- by the producer's epilogue (conv1_tile_kernel, conv_bf16_rows_kernel) --
    and the ReLU mask of the consumer's data gradient is the sign of that copy; the data gradient of such a consumer writes ONLY the padded bf16 copy of
    its output (the producer's dY) and that layer's bias gradient.  Every product sees the values it saw with the fp32 tensors kept
    (bf16(y) either way), so with reductions in a fixed order (option `deterministic`) loss, logits and all 42 gradient tensors are BIT-identical
    between `bf16_acts` 1 and 0; test_bf16_train_mode holds the 0 side to the oracle.  The activations that no longer exist say so."""
    from fcn8s_tensorflow_amd.engine import Engine
    from fcn8s_tensorflow_amd._lib import Fcn8sError
    widths = (64, 64, 128, 256, 256, 256, 128)
    n, h, w = 2, 64, 96
    P = orc.init_params(20, widths, seed=9, decoder_std_scale=6.0, bias_std=0.05)
    img, lab = batch(n, h, w, seed=31)
    out = {}
    for acts in (1, 0):
        e = Engine(20, widths=widths, precision="bf16_train", options={"bf16_acts": acts, "deterministic": 1})
        assert e.get_option("bf16_acts") == acts
        e.set_params(P)
        e.profile(2); e.profile_reset()
        loss = e.forward_backward(img, lab, keep_prob=0.5, l2_rate=1e-3)
        groups = {k: int(v["launches"]) for k, v in e.profile_results().items() if ":" not in k}
        e.profile(0)
        out[acts] = (loss, e.activation("logits", (n, h, w, 20)), e.activation("conv3_3", (n, h // 4, w // 4, 128)), e.activation("pool3", (n, h // 8, w // 8, 128)), e.get_grads(), groups)
        for name, shape in (("conv1_1", (n, h, w, 64)), ("conv3_2", (n, h // 4, w // 4, 128)), ("conv5_1", (n, h // 16, w // 16, 256)), ("pool1", (n, h // 2, w // 2, 64)),
                            ("pool5", (n, h // 32, w // 32, 256)), ("conv1_2", (n, h, w, 64)), ("conv5_3", (n, h // 16, w // 16, 256))):
            if acts:
                with pytest.raises(Fcn8sError, match="bf16_acts"):
                    e.activation(name, shape)
            else:
                assert np.isfinite(e.activation(name, shape)).all()
        # an inference pass takes the training pass's data flow (option bf16_infer_copies, default 1: the same tensors exist or do not); with that option off
        # it writes every fp32 tensor again
        e.predict(img, argmax=False)
        if acts:
            with pytest.raises(Fcn8sError, match="bf16_acts"):
                e.activation("conv3_2", (n, h // 4, w // 4, 128))
        else:
            assert np.isfinite(e.activation("conv3_2", (n, h // 4, w // 4, 128))).all()
        e.set_option("bf16_infer_copies", 0)
        e.predict(img, argmax=False)
        assert np.isfinite(e.activation("conv3_2", (n, h // 4, w // 4, 128))).all()
        e.close()
    assert out[1][0] == out[0][0]
    for i in (1, 2, 3):
        np.testing.assert_array_equal(out[1][i], out[0][i])
    # ... and the same in the backward pass: the output gradient of a conv that FOLLOWS a bf16 conv (conv2_1, conv3_1, conv3_2, ... -- not conv1_1, whose
    # weight gradient is exact fp32) is written only as its padded bf16 copy, and its bias gradient is summed from the fp32 values in the producing
    # kernel's epilogue: another summation order for those seven bias gradients (1e-5), everything else bit for bit
    inner = {"conv%d_%d/biases" % (b, i) for b, n_ in ((2, 2), (3, 3), (4, 3), (5, 3)) for i in range(1, n_)}
    for k in out[0][4]:
        if k in inner:
            assert rel(out[1][4][k], out[0][4][k]) < 1e-5, k
            assert np.abs(out[0][4][k]).max() > 0
        else:
            np.testing.assert_array_equal(out[1][4][k], out[0][4][k], err_msg=k)
    # the conversion passes that went away: 8 forward copies (13 convs - 5 block heads; conv1_2's comes from conv1_1's kernel), those 7 gradients, and the
    # 5 copies of the pooled maps (conv2_1 .. conv5_1, fc6), which the pools write themselves (pool1, pool2 and pool5 as nothing else), and fc7's input copy,
    # which comes out of fc6's epilogue
    assert out[0][5]["bf16_convert"] - out[1][5]["bf16_convert"] == 8 + 7 + 5 + 1, (out[0][5], out[1][5])


@pytest.mark.parametrize("mode", ["bf16_fwd", "bf16_fwd_x2"])
def test_bf16_fwd_mode(mode):
    """FCN8S_PREC_BF16_FWD_X2 ('bf16_fwd_x2') is the same mode with two bf16 pieces per operand instead of three in the non-bf16 GEMMs (16
    significand bits: far inside this test's bounds, which the 8-bit forward rounding sets).
    FCN8S_PREC_BF16_FWD ('bf16_fwd'): conv3_1 .. conv5_3, fc6 and fc7 forward with bf16-rounded operands on the bf16 MFMA (fp32
    accumulate), every other GEMM in the f32x3 arithmetic -- against the oracle applying the same rounding to the same layers
    (`bf16_fc=True, bf16_convs=True`): logits to 1e-3 of their scale, gradients along the device's decisions to 1e-2 in L2 (a bf16
    rounding-boundary flip moves pre-activations by ~2e-4 of their scale, so units up to 1e-3 of a layer's largest may sit on the other
    side of zero).  Full width, one 256x256 image: 4096 / 1024 / 256 GEMM rows in blocks 3 / 4 / 5, all on the 256 x 256 kernel."""
    from fcn8s_tensorflow_amd.engine import Engine
    n, h, w = 1, 256, 256
    P = orc.init_params(20, seed=9, decoder_std_scale=6.0, bias_std=0.05)
    img, lab = batch(n, h, w, seed=31)
    e = Engine(20, precision=mode, options={"bf16_gemm256": 2})
    e.set_params(P)
    e.profile(2); e.profile_reset()
    onehot = orc.one_hot(lab, 20)
    loss = e.forward_backward(img, onehot, keep_prob=1.0, l2_rate=1e-3)
    prof = e.profile_results()
    e.profile(0)
    k256 = [v for k, v in prof.items() if k.startswith("kernel:") and "conv_bf16_256_kernel" in k]
    assert k256 and sum(int(v["launches"]) for v in k256) >= 9, {k: v["launches"] for k, v in prof.items() if k.startswith("kernel:")}
    mine, other = ("_x3_kernel", "_x2_kernel") if mode == "bf16_fwd" else ("_x2_kernel", "_x3_kernel")
    assert any(mine in k for k in prof) and not any(k.startswith("kernel:") and ("gemm_glds_kernel" in k or "wgrad_glds_kernel<" in k or other in k) for k in prof)
    logits = e.activation("logits", (n, h, w, 20))
    # (1) the arithmetic of each bf16 layer, exactly: the layer's output on the device against the oracle's convolution of the bf16-rounded
    #     operands applied to the DEVICE's own input of that layer -- identical rounding, only the fp32 summation order differs
    import torch
    rb = lambda t: t.to(torch.bfloat16).to(torch.float32)
    wd = e.widths
    shapes = {"pool2": (n, h // 4, w // 4, wd[1]), "conv3_1": (n, h // 4, w // 4, wd[2]), "conv4_1": (n, h // 8, w // 8, wd[3]), "conv4_2": (n, h // 8, w // 8, wd[3]),
              "conv5_2": (n, h // 16, w // 16, wd[4]), "conv5_3": (n, h // 16, w // 16, wd[4]), "fc6": (n, h // 32, w // 32, wd[5]), "fc7": (n, h // 32, w // 32, wd[6])}
    for src, dst, wname, bname in (("pool2", "conv3_1", "conv3_1/filter", "conv3_1/biases"), ("conv4_1", "conv4_2", "conv4_2/filter", "conv4_2/biases"),
                                   ("conv5_2", "conv5_3", "conv5_3/filter", "conv5_3/biases"), ("fc6", "fc7", "fc7/weights", "fc7/biases")):
        x = torch.from_numpy(e.activation(src, shapes[src])).permute(0, 3, 1, 2)
        wk = torch.from_numpy(P[wname]); k = wk.shape[0]
        want = torch.relu(torch.nn.functional.conv2d(rb(x), rb(wk).permute(3, 2, 0, 1), torch.from_numpy(P[bname]), padding=(k - 1) // 2)).permute(0, 2, 3, 1).numpy()
        got = e.activation(dst, shapes[dst])
        assert rel(got, want) < 1e-4, (dst, rel(got, want))
    # (2) end to end against the oracle rounding the same layers.  Looser: the inputs of a bf16 layer differ from the oracle's by fp32
    #     round-off, which moves a fraction of them across a bf16 rounding boundary (a 2^-8 step for that element); over eleven rounded
    #     layers that adds up to a few 1e-3 of an activation's range
    ref, acts = orc.forward(P, img, keep=True, bf16_fc=True, bf16_convs=True)
    scale = max(1.0, float(np.abs(ref).max()))
    for k in ("conv3_1", "conv4_2", "pool5", "fc7"):
        assert rel(e.activation(k, acts[k].shape), acts[k]) < 2e-2, (k, rel(e.activation(k, acts[k].shape), acts[k]))
    assert np.abs(logits - ref).max() < 2e-2 * scale
    ref32 = orc.forward(P, img)
    cost = float(np.abs(ref - ref32).max()) / scale
    assert 1e-5 < cost < 1e-1, cost                                 # the rounding is visible ...
    assert np.abs(logits - ref32).max() > 0.2 * np.abs(ref - ref32).max()      # ... and the GPU really rounded
    # (3) gradients: those of the fp32 graph at the bf16-forward activations (straight-through), along the device's decisions
    g = e.get_grads()
    br, rt, stats = device_decisions(e, P, img, (n, h, w), relu_tol=3e-2, tie_tol=3e-2, max_frac=2e-3, bf16_fc=True, bf16_convs=True)
    loss_ref, g_ref, _ = orc.loss_and_grads(P, img, onehot.astype(np.float32), l2_rate=1e-3, bf16_fc=True, bf16_convs=True, branches=br, routes=rt)
    assert abs(loss - loss_ref) < 2e-2 * max(1.0, abs(loss_ref))
    for k in g_ref:
        gk, rk = np.asarray(g[k], np.float64), np.asarray(g_ref[k], np.float64)
        l2 = float(np.linalg.norm(gk - rk) / (np.linalg.norm(rk) + 1e-30))
        assert l2 < 5e-2, (k, l2)
    # a training step runs and the mode can be left again: back in fp32 the predictions are those of an engine that never left it
    loss2, step = e.train_step(img, lab, 1e-6, keep_prob=0.5)
    assert step == 1 and np.isfinite(loss2)
    e.set_precision('fp32')
    e.set_params(P)
    a = e.predict(img, argmax=False)
    e2 = Engine(20); e2.set_params(P)
    np.testing.assert_array_equal(a, e2.predict(img, argmax=False))
    e.close(); e2.close()


@pytest.mark.parametrize("mode", ["bf16_fwd", "bf16_fwd_x2"])
def test_bf16_copy_written_by_the_input_transform_is_bit_identical(mode):
    """bf16 forward modes, training: the padded bf16 copy of a layer's input that its direct bf16 convolution reads is written by the layer's
    Winograd input transform (option bf16_copy_by_transform, default 1) instead of a conversion pass of its own.  Same conversion (RNE) of the
    same values into the same zero-bordered layout: the loss, the logits and the bf16 layers' activations carry identical bits (the gradients
    agree to the run-to-run summation order of the atomically reduced split GEMMs, measured in the same test),
    the conversion kernel disappears from the training pass for the F(6x6,3x3) layers among conv3_1 .. conv5_3 (layers on smaller tiles, fc6
    and fc7 keep it), and inference -- which has no transform to ride on -- still converts.  Sizes with partial F(6x6) edge tiles in both directions (256 = 42 * 6 + 4, 64 = 10 * 6 + 4, ...)
    and a batch of two (the per-image border of the copy)."""
    from fcn8s_tensorflow_amd.engine import Engine
    P = orc.init_params(20, seed=19, decoder_std_scale=6.0, bias_std=0.05)
    for n, h, w in ((1, 256, 256), (2, 256, 512)):
        img, lab = batch(n, h, w, seed=51)
        outs, counts = [], []
        for by_transform in (1, 0):
            e = Engine(20, precision=mode, options={"bf16_gemm256": 2, "bf16_copy_by_transform": by_transform})
            assert e.get_option("bf16_copy_by_transform") == by_transform
            e.set_params(P)
            e.profile(2); e.profile_reset()
            loss = e.forward_backward(img, orc.one_hot(lab, 20), keep_prob=1.0, l2_rate=1e-3)
            prof = e.profile_results(); e.profile(0)
            conv = sum(int(v["launches"]) for k, v in prof.items() if k.startswith("kernel:") and "f32_to_bf16_padded_kernel" in k)
            riding = sum(int(v["launches"]) for k, v in prof.items() if k.startswith("kernel:") and "wino_input_kernel<6, 2, 3, true>" in k)
            counts.append((conv, riding))
            g = e.get_grads()
            acts = {k: e.activation(k, s) for k, s in (("conv3_2", (n, h // 4, w // 4, 256)), ("conv4_3", (n, h // 8, w // 8, 512)), ("logits", (n, h, w, 20)))}
            # a second step on the same engine: the borders of the kept copies are still zero after the interiors were rewritten
            loss_b = e.forward_backward(img, orc.one_hot(lab, 20), keep_prob=1.0, l2_rate=1e-3)
            assert loss_b == loss
            g_again = e.get_grads()                              # the same pass repeated: what the atomically reduced (split) GEMMs of the backward chain differ by, run to run
            pred = e.predict(img, argmax=False)                  # inference on the same workspace: converts for itself
            outs.append((loss, g, acts, pred, g_again))
            e.close()
        # every F(6x6) layer of blocks 3 - 5 lost its conversion pass to the transform (layers on smaller tiles, fc6 and fc7 keep theirs)
        assert counts[1][1] == 0 and counts[0][1] >= 3 and counts[0][0] + counts[0][1] == counts[1][0], counts
        assert outs[0][0] == outs[1][0]
        for k in outs[0][1]:
            # (small launches split their reductions over blocks and add the parts with atomics: the gradients of one engine differ between two
            #  identical passes by that summation order, and the two forms may differ by no more than that)
            noise = max(rel(outs[0][1][k], outs[0][4][k]), rel(outs[1][1][k], outs[1][4][k]))
            assert rel(outs[0][1][k], outs[1][1][k]) <= max(2e-6, 4 * noise), (k, noise)
        for k in outs[0][2]:
            np.testing.assert_array_equal(outs[0][2][k], outs[1][2][k], err_msg=k)
        np.testing.assert_array_equal(outs[0][3], outs[1][3])


def test_conv1_1_inside_conv1_2_input_transform():
    """Option conv1_in_transform (default 1): conv1_2's F(6x6,3x3) input transform evaluates conv1_1 on its own 8 x 8 patches, straight from the
    preprocessed image; conv1_1's activation tensor is never written.  Same arithmetic in another summation order (VALU fma chain instead of the MFMA
    kernel's), so everything downstream agrees to round-off: loss, logits, the softmax; the 42 gradients up to the odd tie flip; the ReLU record the transform keeps
    is the sign of the two-kernel form's activation wherever that is not within round-off of zero.  Sizes with partial F(6x6) edge tiles in both
    directions (32 = 5 * 6 + 2, 64 = 10 * 6 + 4, 160 = 26 * 6 + 4), image borders inside the staged window, a batch of two, inference and
    training, and a block whose eighth tile column lies outside the image (tw = 6, 11, 27: not multiples of the 8 tiles a block owns)."""
    from fcn8s_tensorflow_amd.engine import Engine
    from fcn8s_tensorflow_amd import _lib as L
    P = orc.init_params(20, seed=23, decoder_std_scale=6.0, bias_std=0.05)
    for n, h, w in ((2, 32, 64), (1, 96, 160)):
        img, lab = batch(n, h, w, seed=57)
        outs = []
        for fused in (1, 0):
            e = Engine(20, options={"conv1_in_transform": fused})
            assert e.get_option("conv1_in_transform") == fused
            e.set_params(P)
            e.profile(2); e.profile_reset()
            loss = e.forward_backward(img, orc.one_hot(lab, 20), keep_prob=1.0, l2_rate=1e-3)
            ks = [k for k in e.profile_results() if k.startswith("kernel:")]
            e.profile(0)
            assert any("wino_input_conv1_kernel" in k for k in ks) == bool(fused), ks
            assert any("conv1_tile_kernel" in k or "conv1_glds_kernel" in k for k in ks) == (not fused), ks
            g = e.get_grads()
            loss2 = e.forward_backward(img, orc.one_hot(lab, 20), keep_prob=1.0, l2_rate=1e-3)
            g2 = e.get_grads()
            logits = e.activation("logits", (n, h, w, 20))
            br = e.relu_branches((n, h, w))["conv1_1"]
            if fused:
                with pytest.raises(L.Fcn8sError):
                    e.activation("conv1_1", (n, h, w, 64))
                act = None
            else:
                act = e.activation("conv1_1", (n, h, w, 64))
            pred = e.predict(img, argmax=False)
            ks = [k for k in e.profile_results() if k.startswith("kernel:")]
            outs.append((loss, g, logits, br, act, pred, g2, loss2))
            e.close()
        f, u = outs
        assert abs(f[0] - u[0]) <= 2e-6 * abs(u[0]) and f[0] == f[7]
        assert np.abs(f[2] - u[2]).max() <= 2e-5 * max(1.0, np.abs(u[2]).max())
        assert np.abs(f[5] - u[5]).max() <= 2e-5
        # gradients: the two forms' activations differ by round-off (1e-7 at conv1_1, 1e-5 after the Winograd layers), which flips the odd ReLU unit or
        # pool route that sits within round-off of a tie -- on these small maps (conv5_x: 6 x 10 pixels) one flipped unit moves a weight gradient by
        # a percent.  The strict gate for this path is every oracle test of this suite (they run with the option's default, along the device's own
        # decisions, to 1e-4); here: the same gradients up to a few such flips.
        for k in f[1]:
            a, b = np.asarray(f[1][k], np.float64), np.asarray(u[1][k], np.float64)
            assert np.linalg.norm(a - b) <= 3e-2 * np.linalg.norm(b) + 1e-12, (k, np.linalg.norm(a - b) / np.linalg.norm(b))
        differ = f[3] != u[3]
        assert differ.mean() < 1e-4 and (not differ.any() or np.abs(u[4][differ]).max() < 1e-5 * np.abs(u[4]).max())
        # and against the checker
        ref, acts = orc.forward(P, img, keep=True)
        assert np.abs(f[2] - ref).max() < 1e-3 * max(1.0, np.abs(ref).max())


def test_conv1_1_tile_kernel_is_bit_identical_to_the_gather_kernel():
    """conv1_1 forward: the spatial-tile kernel (halo tile in LDS, MFMA fragments read straight from it) performs the same products in the
    same order as the LDS-DMA gather kernel -- identical bits -- on image sizes with partial edge handling in every direction."""
    from fcn8s_tensorflow_amd.engine import Engine
    P = orc.init_params(20, seed=11, decoder_std_scale=6.0, bias_std=0.05)
    for n, h, w in ((2, 32, 64), (1, 96, 160)):
        img, _ = batch(n, h, w, seed=41)
        outs = []
        for tiled in (1, 0):
            e = Engine(20, options={"conv1_tiled": tiled, "conv1_in_transform": 0})
            assert e.get_option("conv1_tiled") == tiled
            e.set_params(P)
            e.profile(2); e.profile_reset()
            e.predict(img)
            ks = [k for k in e.profile_results() if k.startswith("kernel:")]
            e.profile(0)
            assert any("conv1_tile_kernel" in k for k in ks) == bool(tiled) and any("conv1_glds_kernel" in k for k in ks) == (not tiled), ks
            outs.append(e.activation("conv1_1", (n, h, w, 64)))
            e.close()
        np.testing.assert_array_equal(outs[0], outs[1])
        ref = orc.forward(P, img, keep=True)[1]["conv1_1"]
        assert rel(outs[0], ref) < 1e-5


def test_conv1_1_weight_gradient_mfma_kernel():
    """conv1_1's weight and bias gradients: the MFMA kernel ((27 taps x channels + a row of ones) x 64 product over the pixels, halo tile in
    LDS) against the previous kernels on the same engine state -- same sums in another order, so 2e-5 of the tensor's largest entry --
    on a size only the generic kernel took before (W % 64 != 0) and on one the VALU kernel took."""
    from fcn8s_tensorflow_amd.engine import Engine
    P = orc.init_params(20, seed=12, decoder_std_scale=6.0, bias_std=0.05)
    for n, h, w in ((2, 32, 64), (1, 96, 160), (3, 32, 96)):
        img, lab = batch(n, h, w, seed=43)
        got = []
        for mfma in (1, 0):
            e = Engine(20, options={"conv1_wgrad_mfma": mfma})
            assert e.get_option("conv1_wgrad_mfma") == mfma
            e.set_params(P)
            e.profile(2); e.profile_reset()
            e.forward_backward(img, orc.one_hot(lab, 20), keep_prob=1.0, l2_rate=0.0)
            ks = [k for k in e.profile_results() if k.startswith("kernel:")]
            e.profile(0)
            assert any("conv1_wgrad_mfma_kernel" in k for k in ks) == bool(mfma), ks
            got.append((e.grad_view("conv1_1/filter").cpu().numpy().copy(), e.grad_view("conv1_1/biases").cpu().numpy().copy()))
            e.close()
        for a, b in zip(got[0], got[1]):
            assert np.abs(b).max() > 0 and rel(a, b) < 2e-5, (n, h, w, rel(a, b))


@pytest.mark.parametrize("widths,n,h,w,expect", [(None, 2, 32, 64, None), (None, 1, 96, 160, True), ((64, 192, 192, 64, 64, 128, 192), 1, 96, 160, True),
                                                   (SMALL, 2, 64, 224, None), (SMALL, 1, 192, 192, None)])
def test_fused_dgrad_output_and_next_dout_transform(widths, n, h, w, expect):
    """Inside a block the gather kernel of a conv's data gradient hands the previous conv dM = A dZ A^T directly (dZ is never written).
    Same gradients as the two-kernel form (another summation order inside the tile transform: 2e-5 of each tensor's largest entry), and the
    fused kernel really runs where the conditions hold (channels % 64 == 0 on both sides, F(6x6)) -- 96x160 has partial edge tiles."""
    from fcn8s_tensorflow_amd.engine import Engine
    P, img, lab = case(widths, n, h, w, seed=5)
    got, ran = [], []
    for fuse in (1, 0):
        e = Engine(20, widths=widths, options={"fuse_dgrad_dout": fuse})
        e.set_params(P)
        e.profile(2); e.profile_reset()
        loss = e.forward_backward(img, orc.one_hot(lab, 20), keep_prob=1.0, l2_rate=1e-3)
        ks = [k for k in e.profile_results() if k.startswith("kernel:")]
        e.profile(0)
        ran.append(any("wino_dgrad_output_dout_kernel" in k for k in ks))
        got.append((loss, e.get_grads()))
        e.close()
    assert not ran[1]
    if expect is not None:              # (small maps pick F(4x4) / F(2x2) tiles, narrow layers the direct kernels: nothing to fuse there)
        assert ran[0] == expect, ran
    assert got[0][0] == got[1][0]
    for k in got[1][1]:
        assert rel(got[0][1][k], got[1][1][k]) < 2e-5, (k, rel(got[0][1][k], got[1][1][k]))


def test_two_engines_with_different_options_do_not_touch_each_other():
    """Every algorithm option lives in the model it was set on (round 3 still had three process-wide switches): two engines alive in one
    process with opposite settings each keep running their own kernels, in either order of use, and a third engine made afterwards has
    the defaults.  The op-level context (fcn8s_set_option(NULL, ...)) is per thread and never reaches a model."""
    from fcn8s_tensorflow_amd.engine import Engine
    from fcn8s_tensorflow_amd import _lib as L
    import ctypes as C
    P = orc.init_params(20, seed=12, decoder_std_scale=6.0, bias_std=0.05)
    img, lab = batch(2, 32, 64, seed=43)
    a = Engine(20, options={"conv1_tiled": 0, "conv1_wgrad_mfma": 0, "conv1_in_transform": 0})
    b = Engine(20, options={"conv1_tiled": 1, "conv1_wgrad_mfma": 1, "conv1_in_transform": 0}, precision="f32x2")
    L.check(L.lib.fcn8s_set_option(None, b"op_split_pieces", 3))          # this thread's op context: must not leak into either model
    try:
        def kernels(e):
            e.set_params(P)
            e.profile(2); e.profile_reset()
            e.forward_backward(img, lab, keep_prob=1.0)
            ks = [k for k in e.profile_results() if k.startswith("kernel:")]
            e.profile(0)
            return ks
        for order in ((a, b), (b, a), (a, b)):
            for e in order:
                ks = kernels(e)
                if e is a:
                    assert any("conv1_glds_kernel" in k for k in ks) and not any("conv1_tile_kernel" in k for k in ks), ks
                    assert not any("conv1_wgrad_mfma_kernel" in k for k in ks), ks
                    assert any("gemm_glds_kernel<" in k for k in ks) and not any("_x2_kernel" in k or "_x3_kernel" in k for k in ks), ks
                else:
                    assert any("conv1_tile_kernel" in k for k in ks) and any("conv1_wgrad_mfma_kernel" in k for k in ks), ks
                    assert any("_x2_kernel" in k for k in ks) and not any("gemm_glds_kernel<" in k or "_x3_kernel" in k for k in ks), ks
        assert (a.get_option("conv1_tiled"), a.get_option("conv1_wgrad_mfma")) == (0, 0) and (b.get_option("conv1_tiled"), b.get_option("conv1_wgrad_mfma")) == (1, 1)
        c = Engine(20)
        assert (c.get_option("conv1_tiled"), c.get_option("conv1_wgrad_mfma")) == (1, 1)
        ks = kernels(c)
        # (default: conv1_1 inside conv1_2's input transform, neither of the two conv1_1 kernels)
        assert c.get_option("conv1_in_transform") == 1 and any("wino_input_conv1_kernel" in k for k in ks) and not any("conv1_tile_kernel" in k or "conv1_glds_kernel" in k for k in ks), ks
        assert any("gemm_glds_kernel<" in k for k in ks) and not any("_x3_kernel" in k for k in ks), ks
        c.close()
        # the op context belongs to the thread that set it
        import threading
        seen = []
        def other():
            v = C.c_int64(-1); L.check(L.lib.fcn8s_get_option(None, b"op_split_pieces", C.byref(v))); seen.append(int(v.value))
        t = threading.Thread(target=other); t.start(); t.join()
        v = C.c_int64(-1); L.check(L.lib.fcn8s_get_option(None, b"op_split_pieces", C.byref(v)))
        assert seen == [0] and v.value == 3
        assert L.lib.fcn8s_set_option(None, b"conv1_tiled", 0) == L.ERR_NOT_FOUND           # a model option needs a model
    finally:
        L.check(L.lib.fcn8s_set_option(None, b"op_split_pieces", 0))
        a.close(); b.close()


@pytest.mark.parametrize("widths,n,h,w", [(None, 1, 96, 160), (None, 2, 64, 224), ((64, 64, 128, 128, 128, 128, 128), 1, 192, 192), ((64, 128, 192, 64, 64, 128, 128), 1, 96, 96)])
def test_fused_output_and_next_input_transform_is_bit_identical(widths, n, h, w):
    """Forward, inside a block: conv L's output transform and conv L+1's input transform as ONE kernel (wino_out_in_kernel: the tile
    stays in registers, neighbours' borders go through LDS, a block walks down the tile rows) against the two-kernel form.  The fused
    kernel runs the same fma chains in the same order, so everything downstream -- pooled activations, softmax, loss -- has the same bits,
    and the gradients differ by the weight-gradient atomics' summation order only; the ReLU record it writes is the one the backward pass
    masks with.  Sizes with partial edge tiles in both directions, strips narrower and wider than a block, widths (192) that leave the
    kernel's channel groups ragged (C % 64 == 0 is all it needs).  The activation a fused launch no longer writes is reported as such."""
    from fcn8s_tensorflow_amd.engine import Engine
    P, img, lab = case(widths, n, h, w, seed=5)
    got = []
    for fuse in (2, 0):             # (2 = wherever the shapes allow; the default, 1, leaves launches with very short row ranges -- these small cases -- on two kernels)
        e = Engine(20, widths=widths, options={"fuse_out_in": fuse, "conv1_in_transform": 0})      # (conv1_1 materialised in both forms: this test counts what the fusion leaves out)
        assert e.get_option("fuse_out_in") == fuse
        e.set_params(P)
        e.profile(2); e.profile_reset()
        loss = e.forward_backward(img, orc.one_hot(lab, 20), keep_prob=1.0, l2_rate=1e-3)
        ks = [k for k in e.profile_results() if k.startswith("kernel:")]
        e.profile(0)
        ran = any("wino_out_in_kernel" in k for k in ks)
        assert ran == (fuse == 2), ks
        g = e.get_grads()
        br = e.relu_branches((n, h, w))
        wd = e.widths
        pools = [e.activation("pool%d" % b, (n, h >> b, w >> b, wd[b - 1])) for b in (2, 3, 4)]
        # the ReLU record, decoded by the library, = (activation > 0) wherever the activation exists; a fused launch's activation does not
        from fcn8s_tensorflow_amd import _lib as L
        import ctypes as C
        missing = []
        for blk, nconv in enumerate((2, 2, 3, 3, 3), start=1):
            for i in range(1, nconv):
                name = "conv%d_%d" % (blk, i)
                shp = (n, h >> (blk - 1), w >> (blk - 1), wd[blk - 1])
                rec = np.empty(shp, np.uint8)
                has_rec = L.lib.fcn8s_get_relu_record(e.h, name.encode(), rec.ctypes.data_as(C.c_void_p), rec.size) == 0
                if has_rec:
                    np.testing.assert_array_equal(rec.astype(bool), br[name])
                try:
                    act = e.activation(name, shp)
                    if has_rec:
                        np.testing.assert_array_equal(act > 0, rec.astype(bool))
                except L.Fcn8sError as ex:
                    assert "not materialised" in str(ex) and has_rec
                    missing.append(name)
        assert bool(missing) == (fuse == 2), missing
        sm = e.predict(img, argmax=False)           # (inference pass: V' goes to the shared scratch instead of the kept buffer)
        got.append((loss, g, br, pools, sm))
        e.close()
    assert got[0][0] == got[1][0]
    for a, b in zip(got[0][3], got[1][3]):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(got[0][4], got[1][4])
    for k in got[1][2]:
        np.testing.assert_array_equal(got[0][2][k], got[1][2][k])
    for k in got[1][1]:
        assert rel(got[0][1][k], got[1][1][k]) < 2e-5, (k, rel(got[0][1][k], got[1][1][k]))
    # inference on engines that never trained, on another image (a pass that merely found the previous pass's V lying in the right buffer
    # once went unnoticed): the fused kernel must hand its V to the buffer the next conv really reads
    img2, _ = batch(n, h, w, seed=77)
    fresh = []
    for fuse in (2, 0):
        e = Engine(20, widths=widths, options={"fuse_out_in": fuse}); e.set_params(P)
        fresh.append(e.predict(img2, argmax=False))
        e.freeze(True); again = e.predict(img2, argmax=False); e.freeze(False)
        np.testing.assert_array_equal(again, fresh[-1])
        e.close()
    np.testing.assert_array_equal(fresh[0], fresh[1])
    with pytest.raises(ValueError):
        Engine(20, options={"fuse_out_in": 3})


@pytest.mark.parametrize("optimizer", ["sgd", "adam_deterministic"])
def test_free_running_training_trajectory_follows_the_oracle(optimizer):
    """The closest thing to the reference's "train it and look at the curve" that can be checked offline: the library and the CPU oracle
    each train the SAME small-width FCN-8s from the same initial variables on the same four batches of a learnable task (label = a function
    of the pixel colour), free-running for 32 (SGD) / 16 (Adam) steps -- no per-step re-synchronisation as in test_tf_adam_training_steps -- with SGD+momentum and
    with the reference's TF-Adam (fcn8s_tensorflow.py:256).  The two loss curves must stay together (fp32 round-off grows along a trajectory;
    the bound below is 10x the largest gap seen) and both must actually learn.  Only SGD + momentum runs free here: TF-Adam's update is sign-like
    wherever a gradient is at round-off level, and the library's own weight-gradient atomics (summation order differs from run to run) are enough
    to send two Adam trajectories apart after a dozen steps -- measured loss gaps between 1e-6 and 2e-2 for the same 16 steps on different runs.
    Adam is checked step by step instead (test_tf_adam_training_steps), each step restarted from the library's own state.
    Round 5: with the library in DETERMINISTIC mode (option `deterministic`: the split reductions are joined in a fixed order, no atomics) its
    trajectory is the same on every run, so the TF-Adam arm runs free again ("adam_deterministic"): two fresh engines must end in bit-identical
    parameters, and the loss curve is held against the oracle's with a bound that no longer has to cover run-to-run scatter."""
    from fcn8s_tensorflow_amd import _lib as L
    import torch
    det = optimizer.endswith("_deterministic")
    optimizer = optimizer.split("_")[0]
    torch.set_num_threads(min(int(os.environ.get("FCN8S_TEST_THREADS", "8")), torch.get_num_threads()))            # (tiny CPU convolutions: hundreds of threads only get in each other's way)
    widths = SMALL
    P = orc.init_params(20, widths, seed=21, decoder_std_scale=5.0, bias_std=0.05)
    rng = np.random.default_rng(5)
    batches = []
    for _ in range(4):
        base = rng.integers(0, 256, (2, 8, 8, 3), dtype=np.uint8)
        img = np.clip(np.kron(base, np.ones((1, 8, 8, 1), np.uint8)).astype(np.int32) + rng.integers(-6, 7, (2, 64, 64, 3)), 0, 255).astype(np.uint8)
        lab = ((img[..., 0].astype(np.int32) // 32) * 2 + (img[..., 1] > 127)).astype(np.uint8) % 20        # 16 classes, decided by two channels
        batches.append((img, lab))
    lr = 0.2 if optimizer == "sgd" else 2e-3
    STEPS = 32 if optimizer == "sgd" else 16          # (Adam's sign-like steps make two fp32 trajectories part company eventually: keep it short)
    opt = L.OPT_SGD_MOMENTUM if optimizer == "sgd" else L.OPT_TF_ADAM
    runs = []
    for _ in range(2 if det else 1):
        e = make_engine(widths, options={"deterministic": 1} if det else None)
        e.set_params(P)
        dev = []
        for t in range(STEPS):
            img, lab = batches[t % 4]
            loss, step = e.train_step(img, lab, lr, keep_prob=1.0, l2_rate=1e-4, optimizer=opt)
            dev.append(loss)
        runs.append((dev, e.get_params()))
        e.close()
    dev, final_dev = runs[0]
    if det:                                            # the whole trajectory, bit for bit, on a second engine
        assert runs[1][0] == dev
        for k in final_dev:
            np.testing.assert_array_equal(runs[1][1][k], final_dev[k], err_msg=k)
    Pc = {k: v.copy() for k, v in P.items()}
    m = {k: np.zeros_like(v) for k, v in P.items()}; v2 = {k: np.zeros_like(v) for k, v in P.items()}
    ref = []
    for t in range(STEPS):
        img, lab = batches[t % 4]
        loss, g, _ = orc.loss_and_grads(Pc, img, orc.one_hot(lab, 20).astype(np.float32), l2_rate=1e-4)
        ref.append(loss)
        for k in Pc:
            if optimizer == "sgd":
                Pc[k], m[k] = orc.sgd_momentum_step(Pc[k], g[k], m[k], lr)
            else:
                Pc[k], m[k], v2[k] = orc.tf_adam_step(Pc[k], g[k], m[k], v2[k], t + 1, lr)
    dev, ref = np.asarray(dev), np.asarray(ref)
    gap = np.abs(dev - ref) / np.maximum(1.0, np.abs(ref))
    drift = max(rel(final_dev[k], Pc[k]) for k in Pc)
    print("free-running %s: loss %.4f -> %.4f (oracle %.4f -> %.4f), largest loss gap %.2e, largest parameter drift %.2e of the tensor's largest entry"
          % (optimizer, dev[0], dev[-1], ref[0], ref[-1], float(gap.max()), drift))
    need = 0.1 if optimizer == "sgd" else 0.03
    assert dev[-4:].mean() < dev[:4].mean() - need and ref[-4:].mean() < ref[:4].mean() - need, (dev, ref)      # both learn (ln 20 = 3.0 -> ~2.8 after 32 steps)
    # SGD + momentum is a linear recurrence in the gradients: measured loss gap 1.6e-7, parameter drift 4e-6.  TF-Adam's update is
    # lr * m / (sqrt(v) + eps), i.e. sign-like wherever a gradient is at round-off level (+-lr per step whatever its size), so single
    # parameters of near-dead units walk apart while the loss curves stay together: only the curves are compared for it.
    # (measured over several oracle thread counts: loss gap 1.6e-7 .. 7.6e-7 for SGD, 3e-7 .. 1.1e-6 for Adam; parameter drift 3e-6 .. 2.4e-3 for SGD --
    #  one max-pool tie routed the other way moves a handful of weights by that much -- and 6e-4 .. 4.7e-3 for Adam)
    #  (a later run, inside the whole suite: loss gap 2.1e-5, drift 1.1e-2 -- the library's own weight-gradient atomics make its trajectory differ
    #  from run to run by as much; the bounds leave an order of magnitude over the largest values seen)
    assert gap.max() < (2e-4 if optimizer == "sgd" else 2e-3), gap
    assert drift < 1e-1, drift
