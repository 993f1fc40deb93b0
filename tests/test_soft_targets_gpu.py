"""The soft-target (distillation) term on the GPU (fcn8s_set_soft_targets, fcn8s_bind_soft_targets, fcn8s_get_soft_target_term; the definition is
in include/fcn8s_hip.h, restated in fcn8s_tensorflow_amd/loss.py).  The kernel has no op-level entry: it is reached through the model, at tiny shapes,
and held to the float64 restatement on the fetched logits -- the loss, the term, the last bias gradient and (plain layout) dlogits itself --, to itself
across the two logits layouts, to exact identities, to its binding protocol, and to the default stream from a side stream.

Targets are spatially structured (another model's softmax, or sharpened random rows): neighbouring pixels get very different rows, so a wrong slot ->
pixel mapping in the blocked layout cannot hide.

Shapes: 2 x 64 x 96 = 48 exact tiles of 256 pixels in the plain layout, 58.5 tiles of slots in the blocked one; 1 x 32 x 32 = 4 tiles plain, 6.25
blocked, with slots outside the image on every side.

Bars: 1e-5 relative for the loss and the term, 1e-5 of the restated scale for the last bias gradient, 2e-6 of the largest entry for dlogits -- what
the same quantities have in test_lovasz_gpu.py / test_loss_gpu.py.  Each case prints the float32 restatement's own distance E to the float64 one next
to the device's; where 8 E exceeds a bar, 8 E is the bar (the project's rule)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from fcn8s_tensorflow_amd import loss as LM
from oracle import fcn8s_oracle as orc
from tests.test_lovasz_gpu import LAST_BIAS, SMALL, W64, assert_bits, dev_softmax, engine, model_case

pytestmark = pytest.mark.gpu
SHAPES = {"2x64x96": (2, 64, 96), "1x32x32": (1, 32, 32)}


def _lib():
    from fcn8s_tensorflow_amd import _lib
    return _lib


def device_bytes_live():
    L = _lib()
    v = C.c_int64()
    L.check(L.lib.fcn8s_get_option(None, b"device_bytes_live", C.byref(v)))
    return int(v.value)


@functools.lru_cache(maxsize=None)
def teacher_softmax(shape, seed=21):
    """Another model's softmax of the case's images: float32 [N, H, W, 20] on the host (computed once per shape)."""
    n, h, w = shape
    _, img, _ = model_case(SMALL, n=n, h=h, w=w, seed=6)
    t = engine(SMALL)
    t.set_params(orc.init_params(20, SMALL, seed=seed, decoder_std_scale=30.0, bias_std=0.05))
    sm = t.predict(img, argmax=False)
    t.close()
    sm.setflags(write=False)
    return sm


def sharpened_rows(shape, K, seed):
    rng = np.random.default_rng(seed)
    z = 4.0 * rng.standard_normal(shape + (K,))
    p = np.exp(z - z.max(-1, keepdims=True))
    return (p / p.sum(-1, keepdims=True)).astype(np.float32)


def as_device(t, strided):
    """The targets [N, H, W, K] on the device: contiguous, or a class-slice of a wider tensor (rows of K in strides of K + 1; NaN behind each row)."""
    t = np.array(t, np.float32)                                               # (a copy: the cached teacher rows are read-only)
    if not strided:
        return torch.from_numpy(t).cuda()
    wide = torch.full(t.shape[:3] + (t.shape[3] + 1,), float("nan")).cuda()
    wide[..., :t.shape[3]] = torch.from_numpy(t).cuda()
    v = wide[..., :t.shape[3]]
    assert not v.is_contiguous()
    return v


def restated(logits, lab, n, targets, weight, T, pixels, K, ce=1.0, lov=0.0, per_image=False, **loss_cfg):
    """The whole training loss in float64 on the fetched logits, and the float32 restatement's distances E to the soft-target part."""
    rc = LM.restate(logits, lab, **loss_cfg)
    d = ce * rc["dlogits"]
    loss = ce * rc["loss"]
    scale = ce * np.abs(rc["dlogits"]).sum(0).max()
    if lov:
        rl = LM.lovasz_restate(dev_softmax(logits), lab, n, per_image=per_image, x_is='probs')
        d = d + lov * rl["grad_logits"]; loss += lov * rl["loss"]; scale += lov * np.abs(rl["grad_logits"]).sum(0).max()
    tg = targets.reshape(-1, targets.shape[-1])
    r = LM.soft_target_restate(logits, tg, lab, weight, T, pixels, K)
    r32 = LM.soft_target_restate(logits, tg, lab, weight, T, pixels, K, dtype=np.float32)
    E = dict(term=abs(r32["term"] - r["term"]) / max(abs(r["term"]), 1e-300),
             d=np.abs(r32["dlogits"] - r["dlogits"]).max() / np.abs(r["dlogits"]).max(),
             bias=np.abs(r32["bias"] - r["bias"]).max() / np.abs(r["dlogits"]).sum(0).max())
    return dict(loss=loss + r["loss"], term=r["term"], dlogits=d + r["dlogits"], kd_dlogits=r["dlogits"],
                scale=scale + np.abs(r["dlogits"]).sum(0).max(), E=E, term32=r32["term"])


CW = np.random.default_rng(7).uniform(0.5, 2.0, 20).astype(np.float32)


@pytest.mark.parametrize("precision,widths", [("fp32", SMALL), ("bf16_train", W64)])
@pytest.mark.parametrize("tconv_gemm", [0, 1])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_model_matches_restatement(precision, widths, tconv_gemm, shape):
    n, h, w = SHAPES[shape]
    P, img, lab = model_case(widths, n=n, h=h, w=w, seed=6)
    e = engine(widths, precision, tconv_gemm=tconv_gemm)
    e.set_params(P)
    i = 0
    for T in (1.0, 2.0):
        for pixels in ("valid", "all"):
            for combined in (False, True):
                tg = teacher_softmax(SHAPES[shape]) if i % 2 == 0 else sharpened_rows(SHAPES[shape], 20, 30 + i)
                strided = (i // 2) % 2 == 1
                i += 1
                weight = 0.7
                cfg = dict(class_weights=CW, ohem_thresh=0.7, ohem_min_kept=100) if combined else {}
                ce, lov = (1.0, 0.5) if combined else (1.0, 0.0)
                e.set_loss(**cfg)
                e.set_lovasz(lov, ce_weight=ce)
                e.set_soft_targets(weight, T, pixels)
                e.bind_soft_targets(as_device(tg, strided))
                loss = e.forward_backward(img, lab, keep_prob=1.0)
                term = e.soft_target_term()
                logits = e.activation("logits", (n, h, w, 20)).reshape(-1, 20)
                r = restated(logits, lab, n, tg, weight, T, pixels, 20, ce, lov, **cfg)
                db = e.get_grads()[LAST_BIAS]
                dev = dict(loss=abs(loss - r["loss"]) / r["loss"], term=abs(term - r["term"]) / r["term"],
                           bias=np.abs(db - r["dlogits"].sum(0)).max() / r["scale"])
                if tconv_gemm == 0:
                    dl = e.activation("dlogits", (n, h, w, 20)).reshape(-1, 20)
                    dev["d"] = np.abs(dl - r["dlogits"]).max() / np.abs(r["dlogits"]).max()
                print("%s %s tconv_gemm=%d T=%g %s combined=%d strided=%d: device %s; float32 restatement E %s"
                      % (precision, shape, tconv_gemm, T, pixels, combined, strided, {k: "%.2e" % v for k, v in dev.items()},
                         {k: "%.2e" % v for k, v in r["E"].items()}))
                assert dev["loss"] <= max(1e-5, 8 * r["E"]["term"]), (loss, r["loss"])
                assert dev["term"] <= max(1e-5, 8 * r["E"]["term"]), (term, r["term"])
                assert dev["bias"] <= max(1e-5, 8 * r["E"]["bias"]), (db, r["dlogits"].sum(0))
                if tconv_gemm == 0:
                    assert dev["d"] <= max(2e-6, 8 * r["E"]["d"])
                t = e.loss_terms()
                assert set(t) == {"ce", "lovasz", "l2"}                       # as it was
    e.close()


@pytest.mark.parametrize("tconv_gemm", [0, 1])
@pytest.mark.parametrize("num_classes", [12, 24])
def test_model_matches_restatement_at_other_class_counts(num_classes, tconv_gemm):
    """C = K = 12 (image stride 12) and 24 (stride 28): the kernel's generic 16-byte path, which a model of 20 classes never takes.  The bars of
    test_model_matches_restatement."""
    from fcn8s_tensorflow_amd.engine import Engine
    n, h, w = SHAPES["1x32x32"]
    rng = np.random.default_rng(14)
    P = orc.init_params(num_classes, SMALL, seed=6, decoder_std_scale=3.0, bias_std=0.05)
    img = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    lab = rng.integers(0, num_classes, (n, h, w), dtype=np.uint8)
    lab[rng.random((n, h, w)) < 0.1] = 255
    e = Engine(num_classes, widths=SMALL, device_id=0, seed=0, options=dict(tconv_gemm=tconv_gemm))
    e.set_params(P)
    for i, (T, pixels) in enumerate(((1.0, "valid"), (2.0, "all"))):
        tg = sharpened_rows((n, h, w), num_classes, 40 + i)
        weight = 0.7
        e.set_soft_targets(weight, T, pixels)
        e.bind_soft_targets(as_device(tg, i == 1))
        loss = e.forward_backward(img, lab, keep_prob=1.0)
        term = e.soft_target_term()
        logits = e.activation("logits", (n, h, w, num_classes)).reshape(-1, num_classes)
        r = restated(logits, lab, n, tg, weight, T, pixels, num_classes)
        db = e.get_grads()[LAST_BIAS]
        dev = dict(loss=abs(loss - r["loss"]) / r["loss"], term=abs(term - r["term"]) / r["term"],
                   bias=np.abs(db - r["dlogits"].sum(0)).max() / r["scale"])
        if tconv_gemm == 0:
            dl = e.activation("dlogits", (n, h, w, num_classes)).reshape(-1, num_classes)
            dev["d"] = np.abs(dl - r["dlogits"]).max() / np.abs(r["dlogits"]).max()
        print("C = %d tconv_gemm=%d T=%g %s: device %s; float32 restatement E %s"
              % (num_classes, tconv_gemm, T, pixels, {k: "%.2e" % v for k, v in dev.items()}, {k: "%.2e" % v for k, v in r["E"].items()}))
        assert dev["loss"] <= max(1e-5, 8 * r["E"]["term"]), (loss, r["loss"])
        assert dev["term"] <= max(1e-5, 8 * r["E"]["term"]), (term, r["term"])
        assert dev["bias"] <= max(1e-5, 8 * r["E"]["bias"]), (db, r["dlogits"].sum(0))
        if tconv_gemm == 0:
            assert dev["d"] <= max(2e-6, 8 * r["E"]["d"])
    e.close()


@pytest.mark.parametrize("tconv_gemm", [0, 1])
@pytest.mark.parametrize("strided", [False, True])
def test_nineteen_logical_classes(tconv_gemm, strided):
    """K = 19 of C = 20 (the 4-byte target path, rows of 19 in strides of 19 or 20): the padding class's -1e30 logit takes no part."""
    from fcn8s_tensorflow_amd.engine import Engine
    n, h, w = 1, 32, 32
    rng = np.random.default_rng(12)
    P = orc.init_params(19, SMALL, seed=3, decoder_std_scale=3.0, bias_std=0.05)
    img = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    lab = rng.integers(0, 19, (n, h, w), dtype=np.uint8)
    lab[rng.random((n, h, w)) < 0.1] = 255
    e = Engine(20, widths=SMALL, device_id=0, seed=0, logical_classes=19, options=dict(tconv_gemm=tconv_gemm))
    e.set_params(P)
    tg = sharpened_rows((n, h, w), 19, 5)
    e.set_soft_targets(0.5, 2.0, 'valid')
    with pytest.raises(ValueError):
        e.bind_soft_targets(torch.zeros(n, h, w, 20).cuda())                 # the caller's logical classes, not the library's
    e.bind_soft_targets(as_device(tg, strided))
    loss = e.forward_backward(img, lab, keep_prob=1.0)
    logits = e.activation("logits", (n, h, w, 20)).reshape(-1, 20)
    assert (logits[:, 19] < -1e29).all()
    r = restated(logits[:, :19], lab, n, tg, 0.5, 2.0, 'valid', 19)
    assert np.isfinite(loss) and abs(loss - r["loss"]) <= max(1e-5, 8 * r["E"]["term"]) * r["loss"]
    assert abs(e.soft_target_term() - r["term"]) <= max(1e-5, 8 * r["E"]["term"]) * r["term"]
    g = e.get_grads()
    assert all(np.isfinite(v).all() for v in g.values())
    assert np.abs(g[LAST_BIAS] - r["dlogits"].sum(0)).max() <= max(1e-5, 8 * r["E"]["bias"]) * r["scale"]
    if tconv_gemm == 0:
        dl = e.activation("dlogits", (n, h, w, 20)).reshape(-1, 20)
        assert (dl[:, 19] == 0).all()                                         # exactly 0
        assert np.abs(dl[:, :19] - r["dlogits"]).max() <= max(2e-6, 8 * r["E"]["d"]) * np.abs(r["dlogits"]).max()
    e.close()


def kd_grads(e, P, img, lab, tg, weight=None, T=1.0, pixels='valid', strided=False, **lovasz):
    e.set_params(P)
    if lovasz:
        e.set_lovasz(**lovasz)
    if weight is not None:
        e.set_soft_targets(weight, T, pixels)
        if weight:
            e.bind_soft_targets(as_device(tg, strided))
    loss = e.forward_backward(img, lab, keep_prob=1.0, l2_rate=0.0)
    return loss, {k: v.copy() for k, v in e.get_grads().items()}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_the_two_layouts_agree(shape):
    """Column sums cannot see a permuted target row; the 42 gradients can.  `deterministic` = 1: the two layouts' backward passes differ by their own
    rounding whether the term is on or not, and at 2 x 64 x 96 that distance alone is close to the bar -- measured on the MI355X, worst tensor (a deep
    encoder filter), term off / on: 0.86e-5 / 0.91e-5 of its largest entry with `deterministic` = 1 (the same bits every run), 1.05e-5 .. 1.08e-5 /
    0.82e-5 .. 1.14e-5 with the float atomics of `deterministic` = 0; at 1 x 32 x 32 0.63e-5 / 0.60e-5.  A permuted target row moves the decoder's
    gradients by their own size."""
    n, h, w = SHAPES[shape]
    P, img, lab = model_case(SMALL, n=n, h=h, w=w, seed=6)
    tg = teacher_softmax(SHAPES[shape])
    a = kd_grads(engine(tconv_gemm=0, deterministic=1), P, img, lab, tg, 1.0, 2.0, 'all')
    b = kd_grads(engine(tconv_gemm=1, deterministic=1), P, img, lab, tg, 1.0, 2.0, 'all')
    assert abs(a[0] - b[0]) <= 1e-5 * abs(a[0])
    assert len(a[1]) == len(b[1]) == 42
    for k in a[1]:
        assert np.abs(a[1][k] - b[1][k]).max() <= 1e-5 * np.abs(a[1][k]).max(), k


@pytest.mark.parametrize("tconv_gemm", [0, 1])
def test_linear_wiring_is_exact(tconv_gemm):
    P, img, lab = model_case(SMALL, seed=4)
    tg = teacher_softmax(SHAPES["2x64x96"])
    half = kd_grads(engine(deterministic=1, tconv_gemm=tconv_gemm), P, img, lab, tg, 0.5, 2.0, lovasz_weight=0.0, ce_weight=1.0)
    dbl = kd_grads(engine(deterministic=1, tconv_gemm=tconv_gemm), P, img, lab, tg, 1.0, 2.0, lovasz_weight=0.0, ce_weight=2.0)
    assert_bits(half, dbl, scale=2.0)


def test_zero_weight_and_reset_are_bit_identical_to_a_fresh_engine():
    P, img, lab = model_case(SMALL, seed=5)
    tg = teacher_softmax(SHAPES["2x64x96"])
    fresh = engine(deterministic=1)
    ref = kd_grads(fresh, P, img, lab, tg)
    with pytest.raises(Exception):
        fresh.soft_target_term()
    # weight 0 from the start: nothing launched, nothing allocated
    z = engine(deterministic=1)
    z.profile(True)
    z.set_params(P); z.forward_backward(img, lab, keep_prob=1.0)              # (the workspace of the shape exists)
    allocs = z.get_option("workspace_allocations")
    assert_bits(ref, kd_grads(z, P, img, lab, tg, 0.0))
    assert z.get_option("workspace_allocations") == allocs and "soft_targets" not in z.profile_results()
    assert z.soft_target_config is None
    with pytest.raises(Exception):
        z.soft_target_term()
    # a reset after use
    e = engine(deterministic=1)
    used = kd_grads(e, P, img, lab, tg, 0.7, 2.0, 'all')
    assert used[0] != ref[0] and e.soft_target_term() > 0
    e.set_soft_targets(0.0)
    assert e.soft_target_config is None
    e.profile(True)
    allocs = e.get_option("workspace_allocations")
    assert_bits(ref, kd_grads(e, P, img, lab, tg))
    assert e.get_option("workspace_allocations") == allocs and "soft_targets" not in e.profile_results()
    with pytest.raises(Exception):
        e.soft_target_term()
    # ... and with the term on the profile has its group, one allocation was made on first use and none after
    e.set_soft_targets(0.7)
    kd_grads(e, P, img, lab, tg, 0.7)
    assert e.profile_results()["soft_targets"]["launches"] == 1 and e.get_option("workspace_allocations") == allocs
    for x in (fresh, z, e):
        x.close()


def test_own_prediction_as_target_leaves_the_cross_entropy_gradient():
    P, img, lab = model_case(SMALL, seed=9)
    n, h, w = lab.shape
    ce_only = kd_grads(engine(deterministic=1), P, img, lab, None)
    e = engine(deterministic=1)
    e.set_params(P)
    own = e.predict(torch.from_numpy(img).cuda(), argmax=False)                # float32 [N, H, W, 20] on the device
    e.set_soft_targets(1.0, 1.0, 'all')
    e.bind_soft_targets(own)
    e.forward_backward(img, lab, keep_prob=1.0)
    g = e.get_grads()
    for k in g:
        assert np.abs(g[k] - ce_only[1][k]).max() <= 1e-5 * np.abs(ce_only[1][k]).max(), k
    logits = e.activation("logits", (n, h, w, 20)).reshape(-1, 20)
    r = restated(logits, lab, n, own.cpu().numpy(), 1.0, 1.0, 'all', 20)
    term = e.soft_target_term()
    E_abs = abs(r["term32"] - r["term"])
    print("own prediction as target: L_kd device %.3e, float32 restatement %.3e, float64 %.3e" % (term, r["term32"], r["term"]))
    assert term <= r["term32"] + 8 * E_abs + 1e-7                              # (1e-7: a floor where both restatements round to the same tiny number)
    e.close()


def test_one_hot_targets_give_the_cross_entropy():
    P, img, lab = model_case(SMALL, seed=10)
    n, h, w = lab.shape
    onehot = np.zeros((n, h, w, 20), np.float32)
    v = lab < 20
    onehot[v, lab[v]] = 1.0
    onehot[~v, 0] = 1.0
    e = engine()
    kd_grads(e, P, img, lab, onehot, 1.0, 1.0, 'valid')
    ce = e.loss_terms()["ce"]
    assert abs(e.soft_target_term() - ce) <= 1e-5 * ce
    e.close()


def test_protocol():
    L = _lib()
    P, img, lab = model_case(SMALL, seed=11)
    n, h, w = lab.shape
    tg = as_device(teacher_softmax(SHAPES["2x64x96"]), False)
    e = engine(W64)                                                           # (widths every precision takes)
    e.set_params(orc.init_params(20, W64, seed=11, decoder_std_scale=3.0, bias_std=0.05))
    with pytest.raises(Exception):
        e.bind_soft_targets(tg)                                               # the term is off
    for kw in (dict(weight=-1.0), dict(weight=float("nan")), dict(weight=1.0, temperature=0.0), dict(weight=1.0, temperature=float("inf")),
               dict(weight=1.0, pixels="none")):
        with pytest.raises(ValueError):
            e.set_soft_targets(**kw)
    assert L.lib.fcn8s_set_soft_targets(e.h, -1.0, 1.0, 0) == L.ERR_BAD_ARG
    assert L.lib.fcn8s_set_soft_targets(e.h, float("inf"), 1.0, 0) == L.ERR_BAD_ARG
    assert L.lib.fcn8s_set_soft_targets(e.h, 1.0, 0.0, 0) == L.ERR_BAD_ARG
    assert L.lib.fcn8s_set_soft_targets(e.h, 1.0, float("nan"), 0) == L.ERR_BAD_ARG
    assert L.lib.fcn8s_set_soft_targets(e.h, 1.0, 1.0, 2) == L.ERR_BAD_ARG
    assert e.soft_target_config is None
    e.set_soft_targets(0.5, 2.0, 'all')
    assert e.soft_target_config == dict(weight=0.5, temperature=2.0, pixels='all')
    p = C.c_void_p(tg.data_ptr())
    assert L.lib.fcn8s_bind_soft_targets(e.h, None, n, h, w, 20, 20) == L.ERR_BAD_ARG
    assert L.lib.fcn8s_bind_soft_targets(e.h, p, n, h, w, 0, 20) == L.ERR_BAD_ARG
    assert L.lib.fcn8s_bind_soft_targets(e.h, p, n, h, w, 21, 21) == L.ERR_BAD_ARG
    assert L.lib.fcn8s_bind_soft_targets(e.h, p, n, h, w, 20, 19) == L.ERR_BAD_ARG
    assert L.lib.fcn8s_bind_soft_targets(e.h, p, 0, h, w, 20, 20) == L.ERR_SHAPE
    for bad in (tg.cpu(), tg.double(), tg[..., :19], tg.permute(0, 2, 1, 3), tg[:, ::2]):
        with pytest.raises(ValueError):
            e.bind_soft_targets(bad)
    # nothing bound: a training loss refuses, evaluation and prediction do not care
    for call in (lambda: e.forward_backward(img, lab), lambda: e.train_step(img, lab, 1e-3), lambda: e.accumulate_step(img, lab)):
        with pytest.raises(Exception) as ei:
            call()
        assert "bind_soft_targets" in str(ei.value)
    e.eval_step(img, lab); e.predict(img)
    # a binding for another shape is refused and stays; eval_step and predict between bind and step leave it alone; it is consumed once
    e.bind_soft_targets(tg)
    with pytest.raises(Exception):
        e.forward_backward(img[:1], lab[:1])
    e.eval_step(img, lab); e.predict(img); e.predict(img, argmax=False)
    a = e.forward_backward(img, lab, keep_prob=1.0)
    ta = e.soft_target_term()
    with pytest.raises(Exception):
        e.forward_backward(img, lab, keep_prob=1.0)
    # the setting survives the other settings
    e.set_precision("bf16_train"); e.set_precision("fp32")
    e.set_loss(class_weights=CW); e.set_loss()
    e.set_lovasz(0.5); e.set_lovasz(0.0)
    e.set_boundary_loss(LM.boundary_table(4.0, 3.0, 5), 5); e.set_boundary_loss()
    e.set_option("deterministic", 1); e.set_option("deterministic", 0)
    e.bind_soft_targets(tg)
    b = e.forward_backward(img, lab, keep_prob=1.0)
    assert np.float32(a) == np.float32(b) and np.float32(ta) == np.float32(e.soft_target_term())
    # fp8_infer: switching on refuses, switching off does not; a setting made before survives and training refuses as ever
    e.set_precision("fp8_infer")
    with pytest.raises(Exception):
        e.set_soft_targets(1.0)
    e.set_soft_targets(0.0)
    e.set_precision("fp32")
    e.close()


def test_two_equal_sequences_give_identical_bits_and_close_frees_everything():
    """Three updates with the term on, twice: the same bits (`deterministic` = 1 for the REST of the step, whose split-K routes use float
    atomics otherwise; the term's own kernels have none whatever the option says).  No allocation after the first use; close() frees all."""
    P, img, lab = model_case(SMALL, seed=13)
    tg = teacher_softmax(SHAPES["2x64x96"])
    base = device_bytes_live()
    out = []
    for _ in range(2):
        e = engine(deterministic=1)
        e.set_params(P)
        e.set_soft_targets(0.5, 2.0)
        res = []
        for s in range(3):
            e.bind_soft_targets(as_device(tg if s != 1 else sharpened_rows(lab.shape, 20, 3), s == 2))
            res.append((e.train_step(img, lab, 1e-3, keep_prob=1.0)[0], e.soft_target_term()))
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
    P, img, lab = model_case(SMALL, n=4, seed=8)
    tg = teacher_softmax((2, 64, 96))
    tgs = [tg, sharpened_rows((2, 64, 96), 20, 17)]
    parts = []
    for i in (0, 1):
        e = engine(deterministic=1)
        parts.append(kd_grads(e, P, img[2 * i:2 * i + 2], lab[2 * i:2 * i + 2], tgs[i], 0.7, 2.0)[1])
        e.close()
    e = engine(deterministic=1)
    e.set_params(P)
    e.set_soft_targets(0.7, 2.0)
    e.bind_soft_targets(as_device(tgs[0], False))
    e.accumulate_step(img[:2], lab[:2], keep_prob=1.0)
    with pytest.raises(Exception):                                            # each micro-batch binds its own
        e.train_step(img[2:], lab[2:], 0.0, keep_prob=1.0)
    e.bind_soft_targets(as_device(tgs[1], True))
    assert e.pending_micro_batches == 1
    e.train_step(img[2:], lab[2:], 1e-3, keep_prob=1.0)
    g = e.get_grads()                                                         # the flushed sum g_1 + g_2 (the update scales it by 1 / 2)
    for k in g:
        mean = 0.5 * (parts[0][k].astype(np.float64) + parts[1][k])
        assert np.abs(0.5 * g[k] - mean).max() <= 1e-5 * np.abs(mean).max(), k
    e.close()


# ---- a side stream ---------------------------------------------------------------------------------------------------------------------
from tests.test_streams_gpu import H, SHAPE_A, moved_params, params, run_both  # noqa: E402,F401  (H: the module-scoped harness fixture)


def _targets_of(images):
    """Spatially structured target rows made by torch on the CURRENT stream from the step's own images: behind whatever that stream waits for."""
    x = images.float()
    k = torch.arange(20, device=images.device, dtype=torch.float32)
    z = torch.sin(x[..., 0:1] * 0.11 + k) * 3.0 + torch.cos(x[..., 1:2] * 0.07 * (k + 1.0))
    return torch.softmax(z, -1).contiguous()


@pytest.mark.parametrize("tconv_gemm", [0, 1])
def test_a_step_with_the_term_on_a_side_stream_equals_the_default_stream(tconv_gemm, H):
    """Both skews of tests/test_streams_gpu.py: a launch or a clear that went to the NULL stream would read targets that are not written yet, or wipe the
    partials after they were produced.  Two steps: the second finds the first one's partials in the scratch."""
    def step(e, i, l):
        e.bind_soft_targets(_targets_of(i))
        return e.train_step(i, l, 1e-3, keep_prob=1.0), e.loss_terms(), e.soft_target_term()

    def sequence(d):
        d.e.set_soft_targets(0.7, 2.0, 'all')
        out = [d.step(step, SHAPE_A, 31)]
        p = moved_params(d.e, params(1)[1].numpy())
        out.append(d.step(step, SHAPE_A, 32))
        moved_params(d.e, p)
        return out
    run_both(H, "fp32", sequence, options=dict(tconv_gemm=tconv_gemm))
