"""The exponential moving average of the parameters at the model level (fcn8s_set_ema / fcn8s_ema_swap, Engine.set_ema /
averaged_weights, FCN8s.train(ema_decay=...) / FCN8s.averaged_weights; definitions in include/fcn8s_hip.h, "the average").

References: a second engine without the average (training must not notice it: bits), optim.py's float64 recursion over the parameter
snapshots (the shadow: to 4 K 2^-23 M), and -- for the swap -- a fresh engine given the shadow as its parameters (bits: the fresh-model
rule of tests/test_state_coherence_gpu.py)."""
import itertools
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import fcn8s_oracle as orc  # noqa: E402  (checker only: the synthetic parameters of the other GPU tests)
from fcn8s_tensorflow_amd import optim  # noqa: E402

SMALL = (8, 16, 32, 64, 64, 128, 128)
W64 = (64,) * 7
K_STEPS = 4
SGD_LR = 1e-4          # (1e-2 leaves the finite range within four steps on these synthetic parameters)


def _L():
    from fcn8s_tensorflow_amd import _lib
    return _lib


def engine(widths=SMALL, precision='fp32', deterministic=True, seed=7):
    from fcn8s_tensorflow_amd.engine import Engine
    e = Engine(20, widths=widths, seed=seed, precision=precision)
    e.set_params(orc.init_params(20, widths, seed=1, decoder_std_scale=30.0, bias_std=0.05))
    if deterministic:
        e.set_option("deterministic", 1)
    return e


def batch(seed, n=2, h=64, w=64):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8), rng.integers(0, 20, (n, h, w), dtype=np.uint8)


def theta(e):
    return e.flat_params.detach().cpu().numpy().copy()


def state(e):
    m, v = e.get_opt_state()
    return theta(e), m, v


def same_bits(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def shadow_bound(snapshots, k):
    """4 k 2^-23 M, M the elementwise largest magnitude among the snapshots (the shadow is a convex combination of them)"""
    M = np.max(np.abs(np.stack(snapshots)), axis=0).astype(np.float64)
    return 4.0 * k * 2.0 ** -23 * M


def recursion(s0, thetas, decay, warmup, t0=0):
    s = s0.astype(np.float64)
    for i, th in enumerate(thetas, 1):
        s = optim.ema_step(s, th, optim.ema_omega(decay, t0 + i, warmup))
    return s


# ---- the average does not steer training ------------------------------------------------------------------------------------------------
def _three_updates(e, route):
    L = _L()
    for i in range(3):
        img, lab = batch(10 + i)
        if route == "adam":                       # the one-call route (fcn8s_train_step)
            e.train_step(img, lab, 1e-3, keep_prob=0.5)
        elif route == "sgd":                      # split phase, SGD-momentum
            e.train_step(img, lab, SGD_LR, keep_prob=0.5, optimizer=L.OPT_SGD_MOMENTUM)
        elif route == "sgd_clip":                 # ... with the device-scale kernel
            e.train_step(img, lab, SGD_LR, keep_prob=0.5, optimizer=L.OPT_SGD_MOMENTUM)
        else:                                     # clip + two micro-batches, TF-Adam with the device-scale kernel
            e.accumulate_step(*batch(20 + i), keep_prob=0.5)
            e.train_step(img, lab, 1e-3, keep_prob=0.5)


@pytest.mark.parametrize("route", ["adam", "sgd", "sgd_clip", "clip_accum"])
def test_training_does_not_notice_the_average(route):
    a, b = engine(), engine()
    b.set_ema(0.9)
    assert b.ema_config == dict(decay=0.9, warmup=True) and a.ema_config is None
    if route in ("clip_accum", "sgd_clip"):
        for e in (a, b):
            e.set_grad_clip(0.05)                 # bites: the scale comes from the device slab
    start = theta(a)
    _three_updates(a, route); _three_updates(b, route)
    if route in ("clip_accum", "sgd_clip"):
        assert a.update_stats()["clip_coef"] < 1.0
    sa, sb = state(a), state(b)
    assert not same_bits(sa[0], start) and all(np.isfinite(x).all() for x in sa)
    for x, y, what in zip(sa, sb, ("theta", "m", "v")):
        assert same_bits(x, y), (route, what)
    assert a.global_step == b.global_step == 3
    assert not same_bits(b.get_ema(), sb[0]) and not same_bits(b.get_ema(), start)
    a.close(); b.close()


def test_one_call_and_split_phase_give_the_same_shadow():
    a, b = engine(), engine()
    for e in (a, b):
        e.set_ema(0.9)
    for i in range(3):
        img, lab = batch(10 + i)
        a.train_step(img, lab, 1e-3, keep_prob=1.0)
        b.forward_backward(img, lab, keep_prob=1.0)
        b.apply_update(1e-3)
    assert same_bits(theta(a), theta(b)) and same_bits(a.get_ema(), b.get_ema())
    assert not same_bits(a.get_ema(), theta(a))
    a.close(); b.close()


# ---- the shadow follows the definition ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["adam", "sgd", "none"])
@pytest.mark.parametrize("warmup", [True, False])
def test_shadow_is_the_recursion_over_the_snapshots(warmup, route):
    L = _L()
    e = engine()
    e.set_ema(0.999, warmup)
    s0 = e.get_ema()
    assert same_bits(s0, theta(e))                              # s = theta when the average is switched on
    snaps = []
    gen = torch.Generator(device="cpu"); gen.manual_seed(5)
    for i in range(K_STEPS):
        img, lab = batch(30 + i)
        if route == "adam":
            e.train_step(img, lab, 1e-3, keep_prob=0.5)
        elif route == "sgd":
            e.train_step(img, lab, SGD_LR, keep_prob=0.5, optimizer=L.OPT_SGD_MOMENTUM)
        else:                                                   # the caller writes theta (a torch optimizer over the views), the library folds it
            e.freeze(False)
            e.flat_params.add_((torch.randn(e.flat_params.numel(), generator=gen) * 1e-2).to(e.flat_params.device))
            e.apply_update(0.0, optimizer=L.OPT_NONE)
        assert e.global_step == i + 1
        snaps.append(theta(e))
    got = e.get_ema().astype(np.float64)
    assert np.isfinite(got).all() and all(np.isfinite(x).all() for x in snaps) and not same_bits(snaps[-1], snaps[0])
    want = recursion(s0, snaps, 0.999, warmup)
    bound = shadow_bound([s0] + snaps, K_STEPS)
    err = np.abs(got - want)
    print("route %s warmup %s: worst error %.3f of the bound" % (route, warmup, float((err / np.maximum(bound, 1e-300)).max())))
    assert (err <= bound).all()
    # the other warm-up rule is far outside the bound (at t = 1 the weights are 9/11 and 0.001): a missing warm-up fails here
    other = recursion(s0, snaps, 0.999, not warmup)
    assert (np.abs(got - other) > bound).any()
    e.close()


# ---- guard and accumulation -----------------------------------------------------------------------------------------------------------------
def test_a_skipped_update_and_a_fold_leave_the_shadow_alone():
    L = _L()
    e = engine()
    e.set_ema(0.9)
    e.set_grad_clip(float("inf"))                               # the guard alone
    e.train_step(*batch(40), 1e-3, keep_prob=1.0)
    s1, st1 = e.get_ema(), state(e)
    assert not same_bits(s1, st1[0])
    # a NaN gradient: the update is skipped, the step advances, no bit of the shadow (nor of theta, m, v) changes
    for opt in (L.OPT_TF_ADAM, L.OPT_SGD_MOMENTUM, L.OPT_NONE):
        step = e.global_step
        e.forward_backward(*batch(41), keep_prob=1.0)
        e.flat_grads[12345 % e.flat_grads.numel()] = float("nan")
        e.apply_update(1e-3, optimizer=opt)
        assert e.global_step == step + 1
        assert same_bits(e.get_ema(), s1), opt
        for x, y in zip(state(e), st1):
            assert same_bits(x, y), opt
    assert e.update_stats()["skipped"] == 3
    # a micro-batch that is folded does not touch the shadow; the closing train_step moves it once
    step = e.global_step
    e.accumulate_step(*batch(42), keep_prob=1.0)
    assert same_bits(e.get_ema(), s1) and e.global_step == step
    e.train_step(*batch(43), 1e-3, keep_prob=1.0)
    assert e.global_step == step + 1
    th2 = theta(e)
    assert not same_bits(th2, st1[0])
    want = recursion(s1, [th2], 0.9, True, t0=step)
    assert (np.abs(e.get_ema().astype(np.float64) - want) <= shadow_bound([s1, th2], 1)).all()
    assert not same_bits(e.get_ema(), s1)
    e.close()


# ---- the fresh-model rule for the swap -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,widths", [("fp32", SMALL), ("f32x3", SMALL), ("bf16_train", W64)])
def test_swapped_model_predicts_like_a_fresh_one_with_the_shadow(precision, widths):
    from fcn8s_tensorflow_amd.engine import Engine
    e = engine(widths, precision, deterministic=False)
    e.set_ema(0.5, warmup=False)
    for i in range(2):
        e.train_step(*batch(50 + i), 1e-3, keep_prob=1.0)
    img = batch(59)[0]
    e.freeze(True)
    e.predict(img, argmax=False)
    p_raw = e.predict(img, argmax=False)                        # frozen, cached banks warm
    raw, shadow = theta(e), e.get_ema()
    assert not same_bits(raw, shadow)
    e.ema_swap()
    info = e.ema_info()
    assert info["swapped"] and info["has_shadow"] and e.get_option("frozen") == 0
    assert same_bits(theta(e), shadow) and same_bits(e.get_ema(), raw)
    p_avg = e.predict(img, argmax=False)
    f = Engine(20, widths=widths, precision=precision)
    f.flat_params.copy_(torch.from_numpy(shadow))
    p_fresh = f.predict(img, argmax=False)
    assert np.abs(p_fresh - p_raw).max() > 0, "the average did not move the prediction: the test has no force"
    assert same_bits(p_avg, p_fresh)
    got = f.get_params()
    for k, v in e.get_params().items():                         # fcn8s_get_param reads the averaged weights
        assert same_bits(v, got[k]), k
    f.close()
    # frozen again while swapped, then back: the raw prediction, bit for bit
    e.freeze(True)
    assert same_bits(e.predict(img, argmax=False), p_avg)
    e.ema_swap()
    assert not e.ema_info()["swapped"] and e.get_option("frozen") == 0
    assert same_bits(theta(e), raw) and same_bits(e.get_ema(), shadow)
    assert same_bits(e.predict(img, argmax=False), p_raw)
    e.close()


def test_swap_clears_an_fp8_calibration():
    e = engine(W64, "fp8_infer", deterministic=False)
    e.set_ema(0.9)                                              # accepted in the inference-only mode
    assert e.calibrate_fp8(batch(60)[0], reset=True) is not None
    e.ema_swap()
    assert e.fp8_calibration() is None
    e.ema_swap()
    e.close()


# ---- errors and defaults ----------------------------------------------------------------------------------------------------------------------
def test_errors_and_refusals():
    import ctypes as C
    L = _L()
    e = engine()
    for bad in (float("nan"), -0.1, 1.0, 2.0):
        assert L.lib.fcn8s_set_ema(e.h, bad, 1) == L.ERR_BAD_ARG
        with pytest.raises(ValueError):
            e.set_ema(bad)
    a = np.zeros(e.flat_params.numel(), np.float32)
    assert L.lib.fcn8s_ema_swap(e.h) == L.ERR_STATE
    assert L.lib.fcn8s_ema_reset(e.h) == L.ERR_STATE
    assert L.lib.fcn8s_get_ema(e.h, a.ctypes.data_as(C.c_void_p), a.size) == L.ERR_STATE
    assert e.ema_info() == dict(decay=0.0, warmup=True, has_shadow=False, swapped=False)
    with e.averaged_weights():                                  # no shadow: the block runs on the parameters as they are
        assert not e.ema_info()["swapped"]
    e.set_ema(0.9)
    e.train_step(*batch(70), 1e-3, keep_prob=1.0)
    e.accumulate_step(*batch(71), keep_prob=1.0); e.discard_accumulated()
    st, s, step = state(e), e.get_ema(), e.global_step
    # while swapped nothing trains, and nothing is touched by the attempt
    with e.averaged_weights():
        assert e.ema_info()["swapped"]
        with pytest.raises(L.Fcn8sError):
            e.train_step(*batch(72), 1e-3)
        with pytest.raises(L.Fcn8sError):
            e.train_step(*batch(72), 1e-3, optimizer=L.OPT_SGD_MOMENTUM)
        with pytest.raises(L.Fcn8sError):
            e.apply_update(1e-3)
        with pytest.raises(L.Fcn8sError):
            e.accumulate_step(*batch(72))
        with pytest.raises(L.Fcn8sError):
            e.ema_reset()
        assert L.lib.fcn8s_train_step(e.h, None, 0, None, 2, 64, 64, 1e-3, 1.0, 0.0, L.HOST, None, None) == L.ERR_STATE
        assert e.global_step == step and e.pending_micro_batches == 0
        assert same_bits(theta(e), s) and same_bits(e.get_ema(), st[0])          # (swapped: the shadow is live)
        m, v = e.get_opt_state()
        assert same_bits(m, st[1]) and same_bits(v, st[2])
    assert not e.ema_info()["swapped"]
    for x, y in zip(state(e), st):
        assert same_bits(x, y)
    assert same_bits(e.get_ema(), s)
    # off keeps the contents, on again continues from them, reset sets s = theta
    e.set_ema(None)
    assert e.ema_config is None and e.ema_info()["has_shadow"]
    e.train_step(*batch(73), 1e-3, keep_prob=1.0)
    assert same_bits(e.get_ema(), s)
    e.set_ema(0.9)
    assert same_bits(e.get_ema(), s)
    e.ema_reset()
    assert same_bits(e.get_ema(), theta(e))
    e.close()


def test_defaults_cost_nothing_and_the_groups_report_their_bytes():
    L = _L()
    e = engine()
    n = e.flat_params.numel()
    e.train_step(*batch(80), 1e-3, keep_prob=1.0)              # (the workspace, the slots)

    def step_profile(**kw):
        e.profile(1); e.profile_reset()
        before = e.get_option("workspace_allocations")
        e.train_step(*batch(81), 1e-3, keep_prob=1.0, **kw)
        prof = e.profile_results()
        e.profile(0)
        return prof, e.get_option("workspace_allocations") - before

    prof, allocs = step_profile()
    assert allocs == 0 and "ema_update" not in prof and "ema_swap" not in prof
    assert prof["adam"]["launches"] == 1 and prof["adam"]["bytes"] == 28.0 * n
    assert not [k for k in prof if k.startswith("kernel:") and "ema" in k]
    prof, _ = step_profile(optimizer=L.OPT_SGD_MOMENTUM)
    assert prof["sgd_momentum"]["bytes"] == 20.0 * n
    before = e.get_option("workspace_allocations")
    e.set_ema(0.9)
    assert e.get_option("workspace_allocations") == before + 1  # the shadow: one allocation, once
    prof, allocs = step_profile()
    assert allocs == 0 and prof["adam"]["launches"] == 1 and prof["adam"]["bytes"] == 36.0 * n and "ema_update" not in prof
    prof, allocs = step_profile(optimizer=L.OPT_SGD_MOMENTUM)
    assert allocs == 0 and prof["sgd_momentum"]["bytes"] == 28.0 * n
    e.profile(1); e.profile_reset()
    e.apply_update(0.0, optimizer=L.OPT_NONE)
    e.ema_swap(); e.ema_swap()
    prof = e.profile_results()
    e.profile(0)
    assert prof["ema_update"]["launches"] == 1 and prof["ema_update"]["bytes"] == 12.0 * n
    assert prof["ema_swap"]["launches"] == 2 and prof["ema_swap"]["bytes"] == 2 * 16.0 * n
    e.set_ema(None); e.set_ema(0.5)
    assert e.get_option("workspace_allocations") == before + 1
    # the setting and the shadow survive a precision change, an option and freezing
    s = e.get_ema()
    e.set_precision("f32x3"); e.set_option("winograd_tile", 4); e.freeze(True)
    assert e.ema_info() == dict(decay=0.5, warmup=True, has_shadow=True, swapped=False) and same_bits(e.get_ema(), s)
    e.close()


# ---- the facade ---------------------------------------------------------------------------------------------------------------------------------
def _cycle(batches):
    """a fixed, unshuffled generator: the same batches in the same order, for ever"""
    return itertools.cycle(batches)


def _model():
    from fcn8s_tensorflow_amd.fcn8s import FCN8s
    m = FCN8s(vgg16_dir='synthetic:3', num_classes=19, widths=SMALL)
    m.engine.set_option("deterministic", 1)
    return m


def _batches19():
    out = []
    for s in (90, 91):
        rng = np.random.default_rng(s)
        out.append((rng.integers(0, 256, (2, 64, 64, 3), dtype=np.uint8), rng.integers(0, 19, (2, 64, 64), dtype=np.uint8)))
    return out


def test_facade_trains_with_the_average_and_evaluates_it(tmp_path):
    from fcn8s_tensorflow_amd import tf_bundle
    from fcn8s_tensorflow_amd.fcn8s import FCN8s
    data = _batches19()
    kw = dict(epochs=1, steps_per_epoch=2, learning_rate_schedule=lambda s: 1e-3, keep_prob=0.5, record_summaries=False)
    plain = _model()
    plain.train(_cycle(data), **kw)
    raw = theta(plain.engine)
    plain.close()

    m = _model()
    g = _cycle(data)
    m.train(g, eval_dataset='train', eval_frequency=1, metrics={'loss', 'mean_iou'}, ema_decay=0.9, **kw)
    logged = list(m.metric_values)
    assert m.metric_names == ['loss', 'mean_iou']
    # the live weights are the raw ones, bit-equal to the run without the average; the previous setting (off) is back, the shadow stays
    info = m.engine.ema_info()
    assert same_bits(theta(m.engine), raw) and not info["swapped"] and info["has_shadow"] and info["decay"] == 0.0
    assert m.engine.ema_config is None
    shadow = m.engine.get_ema()
    assert not same_bits(shadow, raw)
    # the logged evaluation is the averaged weights' (the generator is back at its first batch: 2 for training + 2 for the evaluation)
    with m.averaged_weights():
        m.evaluate(g, 2, metrics={'loss', 'mean_iou'}, dataset='train')
        assert list(m.metric_values) == logged
    m.evaluate(g, 2, metrics={'loss', 'mean_iou'}, dataset='train')
    assert list(m.metric_values) != logged                     # ... and not the raw weights'
    assert same_bits(theta(m.engine), raw)

    # an evaluation that raises: the raw weights are live again, the previous setting is back
    def broken():
        raise RuntimeError("no validation data today")
        yield
    step = m.engine.global_step
    with pytest.raises(RuntimeError, match="no validation data today"):
        m.train(g, eval_dataset='val', val_generator=broken(), val_steps=1, eval_frequency=1, metrics={'loss'}, ema_decay=0.9, **kw)
    info = m.engine.ema_info()
    assert m.engine.global_step == step + 2 and not info["swapped"] and info["decay"] == 0.0
    again = _model()
    again.train(_cycle(data), **dict(kw, epochs=2))
    assert same_bits(theta(m.engine), theta(again.engine))
    again.close()

    # save -> load restores the shadow's bits and the settings
    m.engine.set_ema(0.75, warmup=False)
    shadow = m.engine.get_ema()
    m.variables_updated = True
    m.save(str(tmp_path), 'saved_model', name='ema', include_metrics=False, include_last_training_loss=False)
    m.export_tf_variables(str(tmp_path / "tf" / "variables"))
    unpadded = {k: m.engine.unpad(k, shadow[off:off + int(np.prod(shape))].reshape(shape)) for k, (shape, off) in m.engine.specs.items()}
    params = m.engine.get_params()
    m.close()
    m2 = FCN8s(model_load_dir=os.path.join(str(tmp_path), m.last_saved_model_name))
    assert m2.engine.ema_info() == dict(decay=0.75, warmup=False, has_shadow=True, swapped=False)
    assert m2.engine.ema_config == dict(decay=0.75, warmup=False)
    assert same_bits(m2.engine.get_ema(), shadow)
    m2.close()
    # the TensorFlow bundle carries every shadow tensor under tf.train.ExponentialMovingAverage's name, with the 19 logical classes
    back = tf_bundle.read_bundle(str(tmp_path / "tf" / "variables"))
    for k, v in unpadded.items():
        name = k + "/ExponentialMovingAverage"
        assert name in back and back[name].shape == params[k].shape and same_bits(back[name], v), k
    assert back["fc7_pool4_pool3_conv2d_trans/bias/ExponentialMovingAverage"].shape == (19,)
    m3 = _model()
    m3.load_variables(str(tmp_path / "tf" / "variables"))
    assert same_bits(m3.engine.get_ema(), shadow) and m3.engine.ema_info()["decay"] == 0.0
    m3.close()
