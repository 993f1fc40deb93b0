"""The boundary-weighted cross-entropy inside the training step (fcn8s_set_boundary_loss, Engine.set_boundary_loss, FCN8s.train(boundary_*);
definitions in include/fcn8s_hip.h and fcn8s_tensorflow_amd/loss.py): exact identities of a whole step in the blocked and the plain logits
layout (an ignore band equals relabelling, a unit table changes nothing, a table of 2.0 doubles everything), the U-Net table against the
float64 restatement in fp32 and bf16_train with and without OHEM, the codes of every step against the NumPy route, order and lifetime of
the setting, bad arguments, and the facade.

The label maps are Voronoi maps with a painted ignore rectangle (noise would give every pixel code 1); every test first checks that its
own input has at least 10 % of the pixels valid inside the band and at least 10 % valid outside of it."""
import ctypes as C

import numpy as np
import pytest

from fcn8s_tensorflow_amd import loss as LM
from oracle import fcn8s_oracle as orc

pytestmark = pytest.mark.gpu
SMALL = (8, 16, 32, 64, 64, 128, 128)
W64 = (64, 64, 128, 256, 256, 256, 128)          # bf16_train needs channel widths % 64 == 0
LAST_BIAS = "fc7_pool4_pool3_conv2d_trans/bias"
IDS = np.concatenate([np.arange(20), [255]])     # train ids and the ignore id


def engine(widths=SMALL, precision="fp32", **opts):
    from fcn8s_tensorflow_amd.engine import Engine
    return Engine(20, widths=widths, device_id=0, seed=0, precision=precision, options=opts)


def voronoi(rng, H, W, n, labels):
    ys, xs = np.mgrid[:H, :W]
    py, px = rng.integers(0, H, n), rng.integers(0, W, n)
    lab = rng.choice(labels, n)
    return lab[np.argmin((ys[..., None] - py) ** 2 + (xs[..., None] - px) ** 2, -1)].astype(np.uint8)


def label_maps(seed, n=2, h=64, w=96, cells=8, ids=IDS, paint=True):
    """n different Voronoi maps of `cells` cells, each with a painted 255 rectangle.  2 x 64 x 96: 2 x 2 distance tiles (the right one
    partial), a 9 x 13 grid of 8 x 8 logit blocks with invalid half blocks on all sides, non-square, two different images."""
    rng = np.random.default_rng(seed)
    lab = np.stack([voronoi(rng, h, w, cells, ids) for _ in range(n)])
    for i in range(n):
        if paint:
            y, x = int(rng.integers(0, h - h // 4)), int(rng.integers(0, w - w // 4))
            lab[i, y:y + h // 6, x:x + w // 5] = 255
    return lab


def band_codes(lab, R, num_classes=20):
    """The NumPy codes, after the precondition on the input: no test passes on an empty band, or on an empty outside."""
    codes = LM.boundary_codes_numpy(lab, R)
    valid = lab < num_classes
    inside, outside = float((valid & (codes != 255)).mean()), float((valid & (codes == 255)).mean())
    assert inside >= 0.10 and outside >= 0.10, (R, inside, outside)
    return codes


def model_case(widths, seed=3, n=2, h=64, w=96, decoder_std_scale=30.0):
    P = orc.init_params(20, widths, seed=seed, decoder_std_scale=decoder_std_scale, bias_std=0.05)
    img = np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    return P, img, label_maps(seed, n, h, w)


def step_grads(e, P, img, lab, boundary=None, **loss_cfg):
    e.set_params(P)
    if loss_cfg:
        e.set_loss(**loss_cfg)
    if boundary is not None:
        e.set_boundary_loss(*boundary)
    loss = e.forward_backward(img, lab, keep_prob=1.0, l2_rate=0.0)
    return loss, {k: v.copy() for k, v in e.get_grads().items()}


def assert_bits(a, b, scale=1.0):
    assert np.float32(a[0]) * np.float32(scale) == np.float32(b[0]), (a[0], b[0])
    assert len(a[1]) == len(b[1]) == 42
    for k in a[1]:
        np.testing.assert_array_equal((a[1][k] * np.float32(scale)).view(np.uint32), b[1][k].view(np.uint32), err_msg=k)


def fresh_step(P, img, lab, boundary=None, **cfg):
    opts = cfg.pop("opts", dict(deterministic=1))
    e = engine(**opts)
    out = step_grads(e, P, img, lab, boundary, **cfg)
    e.close()
    return out


# ---- 1. the code indexing, exactly: weight 0 in the band = the band relabelled to "ignore" -------------------------------------------
@pytest.mark.parametrize("R", [3, 8])
@pytest.mark.parametrize("tconv_gemm", [0, 1])
def test_ignore_band_equals_relabelling_bit_for_bit(tconv_gemm, R):
    P, img, lab = model_case(SMALL, seed=5)
    codes = band_codes(lab, R)
    opts = dict(deterministic=1, tconv_gemm=tconv_gemm)
    got = fresh_step(P, img, lab, boundary=(LM.ignore_band_table(R), R), opts=opts)
    relab = lab.copy(); relab[codes != 255] = 255
    ref = fresh_step(P, img, relab, opts=opts)
    assert ref[0] > 0 and any(np.abs(g).max() > 0 for g in ref[1].values())
    assert_bits(ref, got)


# ---- 2. a table of ones ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tconv_gemm", [0, 1])
def test_a_unit_table_changes_no_bit(tconv_gemm):
    P, img, lab = model_case(SMALL, seed=6)
    band_codes(lab, 5)
    cw = np.random.default_rng(11).uniform(0.5, 2.0, 20)
    opts = dict(deterministic=1, tconv_gemm=tconv_gemm)
    for cfg in (dict(), dict(class_weights=cw), dict(class_weights=cw, ohem_thresh=0.7, ohem_min_kept=1500)):
        ref = fresh_step(P, img, lab, opts=opts, **cfg)
        got = fresh_step(P, img, lab, boundary=(np.ones(256, np.float32), 5), opts=opts, **cfg)
        assert_bits(ref, got)


# ---- 3. a table of twos ------------------------------------------------------------------------------------------------------------
def test_a_table_of_twos_doubles_loss_and_gradients_exactly():
    # Doubling is exact in fp32 only away from underflow.  A Voronoi batch holds a few of the 20 classes: with wide logits the others'
    # probabilities, and with them whole gradient entries, are denormal, and a rounded denormal does not double.  So: logits of a few tenths.
    P, img, lab = model_case(SMALL, seed=4, decoder_std_scale=3.0)
    band_codes(lab, 4)
    ref = fresh_step(P, img, lab)
    got = fresh_step(P, img, lab, boundary=(np.full(256, 2.0, np.float32), 4))
    assert_bits(ref, got, scale=2.0)


# ---- 4. the U-Net table against the float64 restatement -------------------------------------------------------------------------------
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


@pytest.mark.parametrize("precision,widths,tconv_gemm", [("fp32", SMALL, 0), ("fp32", SMALL, 1), ("bf16_train", W64, 1)])
def test_unet_table_matches_restatement(precision, widths, tconv_gemm):
    R = 6
    P, img, lab = model_case(widths, seed=6, decoder_std_scale=10.0)
    n, h, w = lab.shape
    T = LM.boundary_table(10, 2, R)
    b = T[band_codes(lab, R)].reshape(-1)
    assert b.max() > 5.0 and b.min() == 1.0
    cw = np.random.default_rng(7).uniform(0.5, 2.0, 20).astype(np.float32)
    e = engine(widths, precision, tconv_gemm=tconv_gemm)
    e.set_params(P)
    e.forward_backward(img, lab, keep_prob=1.0)
    logits = e.activation("logits", (n, h, w, 20)).reshape(-1, 20)
    valid = lab.reshape(-1) < 20
    tol = 4e-6 * max(1.0, float(np.abs(logits).max()))                # round-off of an fp32 l_p = m + log(s) - v
    by_tau, by_k = _gap_configs(LM.pixel_losses(logits, lab), valid, tol)
    e.set_boundary_loss(T, R)
    for cfg in (dict(), by_tau, by_k):
        e.set_loss(class_weights=cw, **cfg)
        loss = e.forward_backward(img, lab, keep_prob=1.0)
        logits = e.activation("logits", (n, h, w, 20)).reshape(-1, 20)
        r = LM.restate(logits, lab, class_weights=cw, pixel_weights=b, **cfg)
        plain = LM.restate(logits, lab, class_weights=cw, **cfg)
        assert abs(r["loss"] - plain["loss"]) > 0.05 * plain["loss"]              # (the weighting is far outside the bar below)
        print(precision, tconv_gemm, cfg, "loss", loss, "restated", r["loss"], "unweighted", plain["loss"])
        assert abs(loss - r["loss"]) <= 1e-5 * r["loss"] + tol, (cfg, loss, r["loss"])
        db = e.get_grads()[LAST_BIAS]
        ref = r["dlogits"].sum(0)
        assert np.abs(db - ref).max() <= 1e-5 * np.abs(r["dlogits"]).sum(0).max(), (cfg, db, ref)
        st = e.loss_stats()
        assert (st["valid"], st["kept"]) == (r["valid"], r["num_kept"]), (cfg, st, r["num_kept"])
        if cfg:
            assert r["num_kept"] < r["valid"]
    e.close()


# ---- 5. every step computes its own codes ---------------------------------------------------------------------------------------------
def test_the_step_computes_this_steps_codes():
    R = 8
    T = LM.boundary_table(10, 2.5, R)
    P, img, labA = model_case(SMALL, seed=8)
    labB = label_maps(18)
    labS = label_maps(28, 2, 32, 64, cells=4)
    imgS = np.ascontiguousarray(img[:, :32, :64])
    cA, cB, cS = band_codes(labA, R), band_codes(labB, R), band_codes(labS, R)
    assert (cA != cB).mean() > 0.10 and (labA != labB).mean() > 0.10
    params = []
    for _ in range(2):
        e = engine(deterministic=1)
        e.set_params(P)
        e.set_boundary_loss(T, R)
        for im, lb, ref in ((img, labA, cA), (img, labB, cB), (imgS, labS, cS), (img, labA, cA)):
            e.forward_backward(im, lb, keep_prob=1.0)
            got = e.boundary_codes()
            assert got.dtype == np.uint8 and got.shape == lb.shape
            np.testing.assert_array_equal(got, ref)
        e.accumulate_step(img, labA, keep_prob=1.0)
        np.testing.assert_array_equal(e.boundary_codes(), cA)
        e.train_step(img, labB, 1e-3, keep_prob=1.0)
        np.testing.assert_array_equal(e.boundary_codes(), cB)                     # the last micro-batch's
        a = e.get_option("workspace_allocations")
        for lb, ref in ((labA, cA), (labB, cB), (labA, cA)):
            l, _ = e.train_step(img, lb, 1e-3, keep_prob=1.0)
            assert np.isfinite(l)
            np.testing.assert_array_equal(e.boundary_codes(), ref)
        assert e.get_option("workspace_allocations") == a
        params.append({k: v.copy() for k, v in e.get_params().items()})
        e.close()
    for k in params[0]:
        np.testing.assert_array_equal(params[0][k].view(np.uint32), params[1][k].view(np.uint32), err_msg=k)


def test_nothing_is_allocated_while_the_weighting_is_off():
    P, img, lab = model_case(SMALL, seed=8)
    band_codes(lab, 3)
    e = engine(); e.set_params(P)
    e.forward_backward(img, lab, keep_prob=1.0)
    a = e.get_option("workspace_allocations")
    e.set_boundary_loss(LM.ignore_band_table(3), 3); e.set_boundary_loss()
    e.forward_backward(img, lab, keep_prob=1.0)
    assert e.get_option("workspace_allocations") == a
    e.set_boundary_loss(LM.ignore_band_table(3), 3)
    e.forward_backward(img, lab, keep_prob=1.0)
    assert e.get_option("workspace_allocations") == a + 2                         # the codes and the loss's state, once
    e.close()


# ---- 6. order and lifetime ------------------------------------------------------------------------------------------------------------
def test_order_and_lifetime_of_the_setting():
    R = 6
    T = LM.boundary_table(10, 2, R)
    P, img, lab = model_case(SMALL, seed=9)
    b = T[band_codes(lab, R)].reshape(-1)
    n, h, w = lab.shape
    cw = np.random.default_rng(12).uniform(0.5, 2.0, 20).astype(np.float32)

    def run(e):
        loss = e.forward_backward(img, lab, keep_prob=1.0, l2_rate=0.0)
        return loss, {k: v.copy() for k, v in e.get_grads().items()}

    default = fresh_step(P, img, lab)
    only = fresh_step(P, img, lab, boundary=(T, R))                               # boundary-only on a fresh engine
    both = fresh_step(P, img, lab, boundary=(T, R), class_weights=cw)             # set_loss, then set_boundary_loss
    assert only[0] != default[0] and both[0] != only[0]

    e = engine(deterministic=1); e.set_params(P)
    e.set_boundary_loss(T, R); e.set_loss(class_weights=cw)                       # the reverse order
    assert_bits(both, run(e))
    e.set_loss()                                                                  # the class weights go: ones, not the old weights
    assert_bits(only, run(e))
    st = e.loss_stats()
    assert st["valid"] == st["kept"] == int((lab < 20).sum()) and st["threshold"] == 0.0
    e.set_boundary_loss()
    assert e.boundary_config is None
    assert_bits(default, run(e))
    with pytest.raises(Exception, match="without the boundary weighting"):
        e.boundary_codes()
    e.close()

    e = engine(deterministic=1); e.set_params(P)
    e.set_loss(class_weights=cw); e.set_loss(); e.set_boundary_loss(T, R)         # old weights in the buffer, then boundary-only
    assert_bits(only, run(e))
    e.set_precision("f32x3"); e.set_precision("fp32")                             # survives a precision round trip ...
    e.set_option("tconv_gemm", 0); e.set_option("tconv_gemm", 1)                  # ... and an option
    assert e.boundary_config["radius"] == R
    assert_bits(only, run(e))
    # under the Lovász term it acts on the CE term only
    logits = e.activation("logits", (n, h, w, 20)).reshape(-1, 20)
    tol = 4e-6 * max(1.0, float(np.abs(logits).max()))
    r = LM.restate(logits, lab, pixel_weights=b)
    assert abs(only[0] - r["loss"]) <= 1e-5 * r["loss"] + tol
    e.set_lovasz(0.5)
    total = e.forward_backward(img, lab, keep_prob=1.0)
    t = e.loss_terms()
    assert t["lovasz"] > 0 and abs(t["ce"] - only[0]) <= 1e-5 * only[0] + tol, (t, only[0])
    assert abs(t["ce"] - default[0]) > 0.05 * default[0]
    assert abs(total - (t["ce"] + 0.5 * t["lovasz"])) <= 1e-5 * total
    np.testing.assert_array_equal(e.boundary_codes(), LM.boundary_codes_numpy(lab, R))
    e.set_lovasz(0)
    # evaluation keeps the reference's loss
    e.metrics_reset(); e.eval_step(img, lab); with_setting = e.metrics_raw()[1]
    e.set_boundary_loss()
    e.metrics_reset(); e.eval_step(img, lab); without = e.metrics_raw()[1]
    assert np.isfinite(with_setting) and with_setting == without
    e.close()


# ---- 7. bad arguments -----------------------------------------------------------------------------------------------------------------
def test_bad_arguments():
    from fcn8s_tensorflow_amd import _lib as L
    e = engine()
    T = LM.boundary_table(10, 2, 6)
    bad = T.copy(); bad[7] = -1.0
    nan = T.copy(); nan[200] = np.nan
    for args in ((T, None), (T, 0), (T, 16), (T, 2.5), (T, True), (None, 16), (None, -1), (T[:255], 6), (bad, 6), (nan, 6),
                 (np.full(256, np.inf), 6), (np.full(256, 1e39), 6)):
        with pytest.raises(ValueError):
            LM.validate_boundary(*args)
        with pytest.raises(ValueError):
            e.set_boundary_loss(*args)
    assert e.boundary_config is None

    def arr(t):
        return (C.c_float * 256)(*np.asarray(t, np.float32).tolist())
    assert L.lib.fcn8s_set_boundary_loss(e.h, 16, arr(T)) == L.ERR_BAD_ARG
    assert L.lib.fcn8s_set_boundary_loss(e.h, 0, arr(T)) == L.ERR_BAD_ARG         # a table without a radius
    assert L.lib.fcn8s_set_boundary_loss(e.h, 6, None) == L.ERR_BAD_ARG           # a radius without a table
    assert L.lib.fcn8s_set_boundary_loss(e.h, -1, arr(T)) == L.ERR_BAD_ARG
    assert L.lib.fcn8s_set_boundary_loss(e.h, 6, arr(nan)) == L.ERR_BAD_ARG
    assert L.lib.fcn8s_set_boundary_loss(e.h, 6, arr(bad)) == L.ERR_BAD_ARG
    assert b"fcn8s_set_boundary_loss" in L.lib.fcn8s_last_error(e.h)
    assert L.lib.fcn8s_set_boundary_loss(None, 6, arr(T)) == L.ERR_BAD_ARG
    # no weighted loss has run: the state error, before and after a default loss; a wrong size once one has
    buf = np.zeros(2 * 64 * 96, np.uint8)
    assert L.lib.fcn8s_get_boundary_codes(e.h, buf.ctypes.data_as(C.c_void_p), buf.size) == L.ERR_STATE
    with pytest.raises(L.Fcn8sError, match="without the boundary weighting"):
        e.boundary_codes()
    P, img, lab = model_case(SMALL, seed=3)
    band_codes(lab, 6)
    e.set_params(P)
    e.forward_backward(img, lab, keep_prob=1.0)
    with pytest.raises(L.Fcn8sError, match="without the boundary weighting"):
        e.boundary_codes()
    e.set_boundary_loss(T, 6)
    with pytest.raises(L.Fcn8sError, match="without the boundary weighting"):
        e.boundary_codes()                                                        # set, but no loss has run with it yet
    e.forward_backward(img, lab, keep_prob=1.0)
    assert L.lib.fcn8s_get_boundary_codes(e.h, buf.ctypes.data_as(C.c_void_p), buf.size - 1) == L.ERR_BAD_ARG
    assert L.lib.fcn8s_get_boundary_codes(e.h, None, buf.size) == L.ERR_BAD_ARG
    assert L.lib.fcn8s_get_boundary_codes(e.h, buf.ctypes.data_as(C.c_void_p), buf.size) == L.OK
    np.testing.assert_array_equal(buf.reshape(lab.shape), LM.boundary_codes_numpy(lab, 6))
    e.close()
    # fp8_infer refuses the call as it refuses the training calls (the mode needs channel widths that are multiples of 64)
    from fcn8s_tensorflow_amd.engine import Engine
    e = Engine(20, widths=(64,) * 7, seed=7)
    e.set_precision('fp8_infer')
    assert L.lib.fcn8s_set_boundary_loss(e.h, 6, arr(T)) == L.ERR_STATE
    assert b"fp8" in L.lib.fcn8s_last_error(e.h).lower()
    with pytest.raises(L.Fcn8sError):
        e.set_boundary_loss(T, 6)
    assert e.boundary_config is None
    e.close()


# ---- 8. the facade --------------------------------------------------------------------------------------------------------------------
def gen(n, h, w, seed):
    k = seed
    while True:
        k += 1000
        lab = label_maps(k, n, h, w, cells=4, ids=np.arange(19), paint=False)
        img = np.random.default_rng(k).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
        yield img, orc.one_hot(lab, 19)


def test_facade_train_with_boundary_weighting():
    from fcn8s_tensorflow_amd.fcn8s import FCN8s
    for k in (1000, 2000):                                                        # the two batches a training run below draws
        lab = label_maps(k, 2, 32, 64, cells=4, ids=np.arange(19), paint=False)
        band_codes(lab, 6, 19); band_codes(lab, 2, 19)
    m = FCN8s(vgg16_dir='synthetic:3', num_classes=19, widths=SMALL)
    for kw in (dict(boundary_weight=10), dict(boundary_sigma=2), dict(boundary_radius=4), dict(boundary_weight=10, boundary_sigma=2, boundary_radius=16),
               dict(boundary_weight=-1, boundary_sigma=2), dict(boundary_ignore_band=0), dict(boundary_ignore_band=16),
               dict(boundary_radius=4, boundary_ignore_band=2)):
        with pytest.raises(ValueError):
            m.train(gen(2, 32, 64, 0), 1, 1, lambda s: 1e-3, record_summaries=False, **kw)
    assert m.engine.global_step == 0                                              # ... before a step ran
    m.train(gen(2, 32, 64, 0), epochs=1, steps_per_epoch=2, learning_rate_schedule=lambda s: 1e-3, boundary_weight=10, boundary_sigma=2,
            metrics={'loss'}, eval_frequency=1, record_summaries=False)
    assert m.g_step == 2 and np.isfinite(m.training_loss)
    assert m.engine.boundary_config is None                                       # restored
    np.testing.assert_array_equal(m.engine.boundary_codes(),                       # the last training loss ran with the weighting, at the default radius
                                  LM.boundary_codes_numpy(label_maps(2000, 2, 32, 64, cells=4, ids=np.arange(19), paint=False), 6))
    m.train(gen(2, 32, 64, 0), epochs=1, steps_per_epoch=2, learning_rate_schedule=lambda s: 1e-3, boundary_ignore_band=2, ohem_thresh=0.7,
            ohem_min_kept=1000, record_summaries=False)
    assert m.g_step == 4 and np.isfinite(m.training_loss)
    assert m.engine.boundary_config is None and m.engine.loss_config is None
    st = m.engine.loss_stats()
    assert 0 < st["kept"] <= st["valid"] == 2 * 32 * 64
    # a configuration of the engine's own comes back after the call
    m.engine.set_boundary_loss(LM.ignore_band_table(3), 3)
    m.train(gen(2, 32, 64, 0), epochs=1, steps_per_epoch=1, learning_rate_schedule=lambda s: 1e-3, boundary_weight=4, boundary_sigma=1,
            record_summaries=False)
    assert m.engine.boundary_config["radius"] == 3
    np.testing.assert_array_equal(m.engine.boundary_config["table"], LM.ignore_band_table(3))
    m.engine.set_boundary_loss()
    m.evaluate(gen(2, 32, 64, 1), 1, metrics={'loss'})
    a = m.metric_values[0]
    m2 = FCN8s(vgg16_dir='synthetic:3', num_classes=19, widths=SMALL)
    m2.engine.set_params(m.engine.get_params())
    m2.evaluate(gen(2, 32, 64, 1), 1, metrics={'loss'})
    assert np.isfinite(a) and abs(a - m2.metric_values[0]) <= 1e-6 * abs(a)
