"""The focal loss inside the model on the GPU (fcn8s_set_focal; the definition is in include/fcn8s_hip.h, restated in fcn8s_tensorflow_amd/loss.py),
with the helpers and at the shapes of tests/test_entropy_term_model_gpu.py: 2 x 64 x 96 and 1 x 32 x 32, both logits layouts, fp32 and bf16_train.
The model is held to the float64 restatement on the fetched logits -- the loss, the `ce` term, the last bias gradient and (plain layout) dlogits --
alone and together with class weights, the U-Net boundary table, the Lovász term, a bound soft-target term and the entropy term; to itself across
the two logits layouts; to a model that never heard of the setting when gamma is 0; to its protocol; and to the default stream from a side stream.

Bars: those of tests/test_entropy_term_model_gpu.py -- 1e-5 relative for the loss and the term, 1e-5 of the restated scale for the last bias
gradient, 2e-6 of the largest entry for dlogits; each case prints the float32 restatement's own distance E to the float64 one next to the device's,
and where 8 E exceeds a bar, 8 E is the bar."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401

from fcn8s_tensorflow_amd import loss as LM
from oracle import fcn8s_oracle as orc
from tests.test_lovasz_gpu import LAST_BIAS, SMALL, W64, assert_bits, dev_softmax, engine, model_case
from tests.test_soft_targets_gpu import CW, SHAPES, _lib, as_device, device_bytes_live, teacher_softmax

pytestmark = pytest.mark.gpu

TABLE, RADIUS = LM.boundary_table(4.0, 3.0, 5), 5


def restated(logits, lab, n, gamma, K=20, cw=None, pw=None, ce=1.0, lov=0.0, kd=None, ent=0.0):
    """The whole training loss in float64 on the fetched logits, and the float32 restatement's distances E of the focal part."""
    P = lab.size
    g32 = np.float32(ce) * (np.float32(1.0) / np.float32(P))                  # gscale as compute_loss forms it
    r = LM.focal_restate(logits, lab, gamma, cw, pw, gscale=ce / P)
    r32 = LM.focal_restate(logits, lab, gamma, cw, pw, dtype=np.float32, gscale=g32)
    d = r["dlogits"].copy()
    loss = ce * r["loss"]
    scale = np.abs(r["dlogits"]).sum(0).max()
    if lov:
        rl = LM.lovasz_restate(dev_softmax(logits), lab, n, x_is='probs')
        d = d + lov * rl["grad_logits"]; loss += lov * rl["loss"]; scale += lov * np.abs(rl["grad_logits"]).sum(0).max()
    if kd is not None:
        rk = LM.soft_target_restate(logits, kd[0].reshape(-1, kd[0].shape[-1]), lab, kd[1], kd[2], 'valid', K)
        d = d + rk["dlogits"]; loss += rk["loss"]; scale += np.abs(rk["dlogits"]).sum(0).max()
    if ent:
        re = LM.entropy_restate(logits, lab, weight=ent, pixels='all', ncols=K, pixels_per_image=P // n)
        d = d + re["dlogits"]; loss += re["loss"]; scale += np.abs(re["dlogits"]).sum(0).max()
    dmax, col = max(np.abs(r["dlogits"]).max(), 1e-300), max(np.abs(r["dlogits"]).sum(0).max(), 1e-300)
    E = dict(term=abs(r32["loss"] - r["loss"]) / max(abs(r["loss"]), 1e-300), d=np.abs(r32["dlogits"] - r["dlogits"]).max() / dmax,
             bias=np.abs(r32["bias"] - r["bias"]).max() / col)
    return dict(loss=loss, term=r["loss"], dlogits=d, scale=scale, E=E, valid=int(r["valid"].sum()))


@pytest.mark.parametrize("precision,widths", [("fp32", SMALL), ("bf16_train", W64)])
@pytest.mark.parametrize("tconv_gemm", [0, 1])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_model_matches_restatement(precision, widths, tconv_gemm, shape):
    n, h, w = SHAPES[shape]
    P, img, lab = model_case(widths, n=n, h=h, w=w, seed=6)
    e = engine(widths, precision, tconv_gemm=tconv_gemm)
    e.set_params(P)
    tg = teacher_softmax(SHAPES[shape])
    for gamma, combined in ((2.0, False), (0.5, True), (5.0, False), (1.0, True)):
        ce, lov = (0.75, 0.5) if combined else (1.0, 0.0)
        e.set_loss(class_weights=CW if combined else None)
        e.set_boundary_loss(*((TABLE, RADIUS) if combined else ()))
        e.set_lovasz(lov, ce_weight=ce)
        e.set_soft_targets(0.5 if combined else 0.0, 2.0)
        if combined:
            e.bind_soft_targets(as_device(tg, False))
        e.set_entropy_term(0.3 if combined else 0.0, 'all')
        e.set_focal(gamma)
        assert e.focal_config == dict(gamma=gamma)
        loss = e.forward_backward(img, lab, keep_prob=1.0)
        terms = e.loss_terms()
        logits = e.activation("logits", (n, h, w, 20)).reshape(-1, 20)
        pw = np.asarray(TABLE, np.float32)[e.boundary_codes().reshape(-1)] if combined else None
        r = restated(logits, lab, n, gamma, 20, CW if combined else None, pw, ce, lov, (tg, 0.5, 2.0) if combined else None, 0.3 if combined else 0.0)
        db = e.get_grads()[LAST_BIAS]
        dev = dict(loss=abs(loss - r["loss"]) / abs(r["loss"]), term=abs(terms["ce"] - r["term"]) / max(abs(r["term"]), 1e-300),
                   bias=np.abs(db - r["dlogits"].sum(0)).max() / r["scale"])
        if tconv_gemm == 0:
            dl = e.activation("dlogits", (n, h, w, 20)).reshape(-1, 20)
            dev["d"] = np.abs(dl - r["dlogits"]).max() / np.abs(r["dlogits"]).max()
        print("%s %s tconv_gemm=%d gamma=%g combined=%d: device %s; float32 restatement E %s"
              % (precision, shape, tconv_gemm, gamma, combined, {k: "%.2e" % v for k, v in dev.items()}, {k: "%.2e" % v for k, v in r["E"].items()}))
        assert dev["loss"] <= max(1e-5, 8 * r["E"]["term"]), (loss, r["loss"])
        assert dev["term"] <= max(1e-5, 8 * r["E"]["term"]), (terms, r["term"])
        assert dev["bias"] <= max(1e-5, 8 * r["E"]["bias"]), (db, r["dlogits"].sum(0))
        if tconv_gemm == 0:
            assert dev["d"] <= max(2e-6, 8 * r["E"]["d"])
        assert e.loss_stats() == dict(valid=r["valid"], kept=r["valid"], threshold=0.0)
    e.close()


@pytest.mark.parametrize("tconv_gemm", [0, 1])
def test_nineteen_logical_classes(tconv_gemm):
    """K = 19 of C = 20: the padding class's -1e30 logit gives e = 0; its gradient column is exactly 0 and everything is finite."""
    from fcn8s_tensorflow_amd.engine import Engine
    n, h, w = 1, 32, 32
    rng = np.random.default_rng(12)
    P = orc.init_params(19, SMALL, seed=3, decoder_std_scale=3.0, bias_std=0.05)
    img = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    lab = rng.integers(0, 19, (n, h, w), dtype=np.uint8)
    lab[rng.random((n, h, w)) < 0.3] = 255
    e = Engine(20, widths=SMALL, device_id=0, seed=0, logical_classes=19, options=dict(tconv_gemm=tconv_gemm))
    e.set_params(P)
    e.set_focal(2.0)
    loss = e.forward_backward(img, lab, keep_prob=1.0)
    logits = e.activation("logits", (n, h, w, 20)).reshape(-1, 20)
    assert (logits[:, 19] < -1e29).all()
    r = restated(logits, lab, n, 2.0)
    assert np.isfinite(loss) and abs(loss - r["loss"]) <= max(1e-5, 8 * r["E"]["term"]) * r["loss"]
    g = e.get_grads()
    assert all(np.isfinite(v).all() for v in g.values())
    assert g[LAST_BIAS].shape == (19,) and not r["dlogits"][:, 19].any()      # (the engine hands out the logical classes' entries)
    assert np.abs(g[LAST_BIAS] - r["dlogits"].sum(0)[:19]).max() <= max(1e-5, 8 * r["E"]["bias"]) * r["scale"]
    if tconv_gemm == 0:
        dl = e.activation("dlogits", (n, h, w, 20)).reshape(-1, 20)
        assert (dl[:, 19] == 0).all() and np.isfinite(dl).all()               # exactly 0
        assert not dl[lab.reshape(-1) == 255].any()
        assert np.abs(dl - r["dlogits"]).max() <= max(2e-6, 8 * r["E"]["d"]) * np.abs(r["dlogits"]).max()
    e.close()


def focal_grads(e, P, img, lab, gamma=None):
    e.set_params(P)
    if gamma is not None:
        e.set_focal(gamma)
    loss = e.forward_backward(img, lab, keep_prob=1.0, l2_rate=0.0)
    return loss, {k: v.copy() for k, v in e.get_grads().items()}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_the_two_layouts_agree(shape):
    """All 42 gradients, `deterministic` = 1, at the bar of tests/test_entropy_term_model_gpu.py's test of the same name (1e-5 of the tensor's
    largest entry): a wrong slot -> pixel mapping in the blocked layout pairs logits with other pixels' labels and moves every gradient by its own size."""
    n, h, w = SHAPES[shape]
    P, img, lab = model_case(SMALL, n=n, h=h, w=w, seed=6, ignore=0.4)
    a = focal_grads(engine(tconv_gemm=0, deterministic=1), P, img, lab, 2.0)
    b = focal_grads(engine(tconv_gemm=1, deterministic=1), P, img, lab, 2.0)
    assert abs(a[0] - b[0]) <= 1e-5 * abs(a[0])
    assert len(a[1]) == len(b[1]) == 42
    for k in a[1]:
        assert np.abs(a[1][k] - b[1][k]).max() <= 1e-5 * np.abs(a[1][k]).max(), k


def test_gamma_zero_and_reset_are_bit_identical_to_a_fresh_engine():
    P, img, lab = model_case(SMALL, seed=5)
    fresh = engine(deterministic=1)
    ref = focal_grads(fresh, P, img, lab)
    # gamma 0 from the start: nothing launched, nothing allocated
    z = engine(deterministic=1)
    z.profile(True)
    z.set_params(P); z.forward_backward(img, lab, keep_prob=1.0)              # (the workspace of the shape exists)
    allocs, live = z.get_option("workspace_allocations"), device_bytes_live()
    assert_bits(ref, focal_grads(z, P, img, lab, 0.0))
    assert z.get_option("workspace_allocations") == allocs and device_bytes_live() == live and "focal_xent" not in z.profile_results()
    assert z.focal_config is None
    # a reset after use
    e = engine(deterministic=1)
    used = focal_grads(e, P, img, lab, 2.0)
    assert used[0] != ref[0] and 0 < used[0] < ref[0]                         # (1 - p_y)^2 <= 1 scales every pixel's loss down
    e.set_focal(0.0)
    assert e.focal_config is None
    e.profile(True)
    allocs, live = e.get_option("workspace_allocations"), device_bytes_live()
    assert_bits(ref, focal_grads(e, P, img, lab))
    prof = e.profile_results()
    assert e.get_option("workspace_allocations") == allocs and device_bytes_live() == live and "focal_xent" not in prof and "softmax_xent" in prof
    # ... and with gamma on the profile has its group in the cross-entropy's place; the allocations were made on first use and none after
    focal_grads(e, P, img, lab, 2.0)
    prof = e.profile_results()
    assert prof["focal_xent"]["launches"] == 1 and e.get_option("workspace_allocations") == allocs
    for x in (fresh, z, e):
        x.close()


def test_protocol():
    L = _lib()
    P, img, lab = model_case(SMALL, seed=11)
    e = engine(W64)                                                           # (widths every precision takes)
    e.set_params(orc.init_params(20, W64, seed=11, decoder_std_scale=3.0, bias_std=0.05))
    for g in (float("nan"), float("inf"), -1.0, -1e-6, 8.5):
        assert L.lib.fcn8s_set_focal(e.h, g) == L.ERR_BAD_ARG, g
        with pytest.raises(ValueError):
            e.set_focal(g)
    assert L.lib.fcn8s_set_focal(None, 2.0) == L.ERR_BAD_ARG and e.focal_config is None
    # both refusal orders with OHEM
    e.set_loss(ohem_thresh=0.7, ohem_min_kept=100)
    assert L.lib.fcn8s_set_focal(e.h, 2.0) == L.ERR_STATE
    with pytest.raises(ValueError):
        e.set_focal(2.0)
    assert L.lib.fcn8s_set_focal(e.h, 0.0) == L.OK                            # switching off is always allowed
    e.set_loss()
    e.set_focal(2.0)
    assert L.lib.fcn8s_set_loss(e.h, None, 0, 0.7, 100) == L.ERR_STATE
    with pytest.raises(Exception):
        e.set_loss(ohem_thresh=0.7)
    assert L.lib.fcn8s_set_loss(e.h, None, 0, 1.5, 100) == L.ERR_BAD_ARG     # a bad threshold is a bad argument whatever gamma is
    a = e.forward_backward(img, lab, keep_prob=1.0)
    ta = e.loss_terms()["ce"]
    st = e.loss_stats()
    assert st == dict(valid=int((lab < 20).sum()), kept=int((lab < 20).sum()), threshold=0.0)
    # evaluation keeps the reference's loss
    def evaluated():
        e.metrics_reset(); e.eval_step(img, lab); e.predict(img)
        return e.metrics_get()
    ev = evaluated()
    e.set_focal(0.0)
    assert ev == evaluated() and np.isfinite(ev[0])
    e.set_focal(2.0)
    # the setting survives the other settings
    e.set_precision("bf16_train"); e.set_precision("fp32")
    e.set_loss(class_weights=CW); e.set_loss()
    e.set_lovasz(0.5); e.set_lovasz(0.0)
    e.set_boundary_loss(TABLE, RADIUS); e.set_boundary_loss()
    e.set_soft_targets(0.5); e.set_soft_targets(0.0)
    e.set_entropy_term(0.5); e.set_entropy_term(0.0)
    e.set_option("deterministic", 1); e.set_option("deterministic", 0)
    assert e.focal_config == dict(gamma=2.0)
    b = e.forward_backward(img, lab, keep_prob=1.0)
    assert np.float32(a) == np.float32(b) and np.float32(ta) == np.float32(e.loss_terms()["ce"])
    # fp8_infer: switching on refuses, switching off does not; a setting made before survives and training refuses as ever
    e.set_precision("fp8_infer")
    assert L.lib.fcn8s_set_focal(e.h, 1.0) == L.ERR_STATE
    with pytest.raises(Exception):
        e.set_focal(1.0)
    with pytest.raises(Exception):
        e.forward_backward(img, lab)
    e.set_focal(0.0)
    e.set_precision("fp32")
    e.close()


def test_two_equal_sequences_give_identical_bits_and_close_frees_everything():
    """Three updates with three gammas, twice: the same bits (`deterministic` = 1 for the REST of the step; the focal kernels have no float atomics
    whatever the option says).  No allocation after the first use; close() frees all."""
    P, img, lab = model_case(SMALL, seed=13, ignore=0.3)
    base = device_bytes_live()
    out = []
    for _ in range(2):
        e = engine(deterministic=1)
        e.set_params(P)
        res = []
        for s in range(3):
            e.set_focal((0.5, 2.0, 5.0)[s])
            res.append((e.train_step(img, lab, 1e-3, keep_prob=1.0)[0], e.loss_terms()["ce"]))
            if s == 0:
                a = e.get_option("workspace_allocations")
        assert e.get_option("workspace_allocations") == a and device_bytes_live() > base
        out.append((res, {k: v.copy() for k, v in e.get_params().items()}))
        e.close()
        del e
    assert out[0][0] == out[1][0] and all(np.isfinite(x) for r in out[0][0] for x in r)
    for k in out[0][1]:
        np.testing.assert_array_equal(out[0][1][k].view(np.uint32), out[1][1][k].view(np.uint32), err_msg=k)
    assert device_bytes_live() == base


def test_accumulated_update_is_the_mean_of_its_micro_batches():
    P, img, lab = model_case(SMALL, n=4, seed=8, ignore=0.3)
    parts = []
    for i in (0, 1):
        e = engine(deterministic=1)
        parts.append(focal_grads(e, P, img[2 * i:2 * i + 2], lab[2 * i:2 * i + 2], 2.0)[1])
        e.close()
    e = engine(deterministic=1)
    e.set_params(P)
    e.set_focal(2.0)
    e.accumulate_step(img[:2], lab[:2], keep_prob=1.0)
    t0 = e.loss_terms()["ce"]
    assert e.pending_micro_batches == 1
    e.train_step(img[2:], lab[2:], 1e-3, keep_prob=1.0)
    assert e.loss_terms()["ce"] != t0                                         # each micro-batch's own term
    g = e.get_grads()                                                         # the flushed sum g_1 + g_2 (the update scales it by 1 / 2)
    for k in g:
        mean = 0.5 * (parts[0][k].astype(np.float64) + parts[1][k])
        assert np.abs(0.5 * g[k] - mean).max() <= 1e-5 * np.abs(mean).max(), k
    e.close()


# ---- a side stream ---------------------------------------------------------------------------------------------------------------------
from tests.test_streams_gpu import H, SHAPE_A, moved_params, params, run_both  # noqa: E402,F401  (H: the module-scoped harness fixture)


@pytest.mark.parametrize("tconv_gemm", [0, 1])
def test_a_step_with_the_focal_loss_on_a_side_stream_equals_the_default_stream(tconv_gemm, H):
    """Both skews of tests/test_streams_gpu.py: a launch that went to the NULL stream would read logits that are not written yet, or store dlogits
    after the backward pass has read them.  Two steps: the second finds the first one's partials in the scratch."""
    def step(e, i, l):
        return e.train_step(i, l, 1e-3, keep_prob=1.0), e.loss_terms(), e.loss_stats()

    def sequence(d):
        d.e.set_focal(2.0)
        out = [d.step(step, SHAPE_A, 31)]
        p = moved_params(d.e, params(1)[1].numpy())
        d.e.set_focal(0.5)
        out.append(d.step(step, SHAPE_A, 32))
        moved_params(d.e, p)
        return out
    run_both(H, "fp32", sequence, options=dict(tconv_gemm=tconv_gemm))
