"""State coherence of a long-lived model on the MI355X.

The one rule this module checks: after ANY sequence of legal calls, a model's output equals that of a model created fresh and put directly
into the same end state -- the same flat parameters, precision, options and fp8 calibration vector.  The fresh model is the reference: it
never held a cache, and the rest of the suite holds fresh models to the float64 oracle in every precision.  A long-lived model is never
compared with itself.

What is under test is host-side state in csrc/model.hip, not a kernel: the banks that are valid for one version of the parameters, one
precision, one option set or one shape (u_cache, wbf16_cache, w8 / w8_valid, bank_stale / banks_stale, u_train, the padded and phase-packed
kernels of prepare_forward_weights, the per-shape padded copies xg16 / dyg16 / q8).  A stale bank gives plausible numbers, so no parity test
of a fresh model notices one.

Every comparison is bit for bit (the precondition test says why it may be).  Every step that changes parameters also asserts that the logits
moved, so no test passes because nothing happened.  The fp8 calibration is an input here: it is made once per parameter set on a fresh engine
and handed to long-lived and fresh engines alike through set_fp8_calibration."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import fcn8s_oracle as orc  # noqa: E402  (checker only: the initializer)

WIDTHS = (64, 64, 128, 128, 128, 128, 128)      # every precision takes them: all % 64, conv5 % 32, fc6 / fc7 % 128; fc6 stays 7x7
CLASSES = 20
PRECISIONS = ('fp32', 'f32x3', 'f32x2', 'bf16_fc', 'bf16_fwd', 'bf16_fwd_x2', 'bf16_train', 'fp8_infer')
TRAINING = PRECISIONS[:-1]
WINOGRAD = ('fp32', 'f32x3', 'f32x2', 'bf16_fc', 'bf16_fwd', 'bf16_fwd_x2')     # bf16_train / fp8_infer ride on the direct path
BF16 = ('bf16_fc', 'bf16_fwd', 'bf16_fwd_x2', 'bf16_train')
# Two shapes that differ in the map size AND in whether the batch is a single image: both decide the Winograd tile, hence a bank's key and shape
SHAPE_A, SHAPE_B = (2, 64, 96), (1, 128, 160)


def _images(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape + (3,), dtype=np.uint8)


A, B = _images(SHAPE_A, 1), _images(SHAPE_B, 2)
LABELS_A = np.random.default_rng(3).integers(0, CLASSES, SHAPE_A, dtype=np.uint8)


def _engine(precision, options=None):
    from fcn8s_tensorflow_amd.engine import Engine
    return Engine(CLASSES, widths=WIDTHS, precision=precision, options=options)


@functools.lru_cache(maxsize=None)
def params(seed):
    """The oracle's initializer for `seed`: (dict for set_params, the same values as the library lays them out flat, on the host)."""
    P = orc.init_params(CLASSES, WIDTHS, seed=seed, decoder_std_scale=6.0, bias_std=0.05)
    e = _engine('fp32'); e.set_params(P)
    flat = e.flat_params.detach().cpu().clone()
    e.close()
    return P, flat


@functools.lru_cache(maxsize=None)
def calibration(seed):
    """The fp8 calibration of parameter set `seed`, made once on a fresh engine (on B, so that a calibration on A is another vector)."""
    e = _engine('fp8_infer'); e.flat_params.copy_(params(seed)[1])
    cal = e.calibrate_fp8(B, reset=True).copy()
    e.close()
    return cal


def fresh(precision, flat, options=None, calibration=None):
    """A model that never held a cache, created directly in the end state."""
    e = _engine(precision, options)
    e.flat_params.copy_(torch.as_tensor(flat))
    if calibration is not None:
        e.set_fp8_calibration(calibration)
    return e


def logits(engine, images):
    return engine.predict(images, argmax=False)


def cal_for(precision, seed):
    return calibration(seed) if precision == 'fp8_infer' else None


def device_bytes_live():
    """Device bytes the library's models hold right now (process-wide)."""
    import ctypes as C
    from fcn8s_tensorflow_amd import _lib as L
    v = C.c_int64()
    L.check(L.lib.fcn8s_get_option(None, b"device_bytes_live", C.byref(v)))
    return int(v.value)


def moved(after, before):
    assert np.abs(after - before).max() > 0, "the parameter change did not move the logits: the test has no force"


def derived_work(prof):
    """Launch counts of everything a pass made from the parameters alone, by the names the profile itself reports: the count-only
    'derived:<kernel>' groups (Winograd filter transform, bf16 kernel relayouts, the padded / phase-packed kernels) and fp8's weight banks."""
    return {k: int(v["launches"]) for k, v in prof.items() if k.startswith("derived:") or k.startswith("fp8_quantize_w")}


def profiled(engine, images):
    engine.profile(2); engine.profile_reset()
    out = logits(engine, images)
    prof = engine.profile_results()
    engine.profile(0)
    return out, prof


# ---- precondition ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_two_fresh_models_agree_bit_for_bit(precision):
    """Two fresh engines in the same state give bit-identical logits on A and on B, in every precision with its default options:
    every comparison below relies on it."""
    flat = params(1)[1]
    e, f = fresh(precision, flat, calibration=cal_for(precision, 1)), fresh(precision, flat, calibration=cal_for(precision, 1))
    for img in (A, B):
        np.testing.assert_array_equal(logits(e, img), logits(f, img))
    e.close(); f.close()


# ---- 1. the frozen cache is used, and is right -----------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_frozen_cache_is_used_and_right(precision):
    """freeze(True), two passes on A, two on B: the second pass at each shape does no weight-derived work at all (so the cache is in use),
    and all four results are the fresh model's."""
    flat, cal = params(1)[1], cal_for(precision, 1)
    e, f = fresh(precision, flat, calibration=cal), fresh(precision, flat, calibration=cal)
    e.freeze(True)
    for i, img in enumerate((A, B)):
        want = logits(f, img)
        first, p1 = profiled(e, img)
        second, p2 = profiled(e, img)
        np.testing.assert_array_equal(first, want)
        np.testing.assert_array_equal(second, want)
        built, again = derived_work(p1), derived_work(p2)
        if i == 0:                               # the first frozen pass built what this precision keeps ...
            assert built.get("derived:prepare_forward_weights", 0) == 1, built
            if precision in WINOGRAD:
                assert built.get("derived:wino_filter_kernel", 0) > 0, built
            if precision in BF16:
                assert sum(n for k, n in built.items() if k.startswith("derived:w_to_bf16_")) > 0, built
            if precision == 'fp8_infer':
                assert sum(n for k, n in built.items() if k.startswith("fp8_quantize_w")) > 0, built
        for k in set(built) | set(again):         # ... and the second pass at the same shape builds nothing
            assert again.get(k, 0) == 0, (k, built, again)
    e.close(); f.close()


# ---- 2. a library write while frozen ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_library_write_while_frozen(precision):
    """freeze, predict, set_params(P2), predict = a fresh model at P2, and the model is no longer frozen.  Frozen again, the first pass does
    the work of a fresh model's first frozen pass and no more: nothing kept from P1 has to be found out and thrown away by the guard."""
    (_, flat1), (P2, flat2) = params(1), params(2)
    e = fresh(precision, flat1, calibration=cal_for(precision, 1))
    e.freeze(True)
    before = logits(e, A)
    logits(e, A)
    e.set_params(P2)
    if precision == 'fp8_infer':
        e.set_fp8_calibration(calibration(2))
    assert e.get_option("frozen") == 0
    f = fresh(precision, flat2, calibration=cal_for(precision, 2))
    after = logits(e, A)
    np.testing.assert_array_equal(after, logits(f, A))
    moved(after, before)
    e.freeze(True); f.freeze(True)
    got, pe = profiled(e, A)
    want, pf = profiled(f, A)
    np.testing.assert_array_equal(got, want)
    launches = lambda prof: {k: int(v["launches"]) for k, v in prof.items() if int(v["launches"])}      # noqa: E731
    assert launches(pe) == launches(pf)
    e.close(); f.close()


# ---- 3. a side-door write while frozen -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_side_door_write_while_frozen(precision):
    """freeze, two passes, flat_params.mul_(1.01) with no library call, two passes: both equal a fresh model holding a copy of the written
    buffer.  (fp8: with the same calibration vector -- that it no longer describes the weights is the caller's business; serving the old
    e4m3 weight banks would be the library's.)"""
    cal = cal_for(precision, 1)
    e = fresh(precision, params(1)[1], calibration=cal)
    e.freeze(True)
    before = logits(e, A)
    np.testing.assert_array_equal(logits(e, A), before)
    e.flat_params.mul_(1.01)
    f = fresh(precision, e.flat_params, calibration=cal)
    want = logits(f, A)
    moved(want, before)
    np.testing.assert_array_equal(logits(e, A), want)
    np.testing.assert_array_equal(logits(e, A), want)
    assert e.get_option("frozen") == 1
    e.close(); f.close()


# ---- 4. shape changes while frozen -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_shape_changes_while_frozen(precision):
    """A, B, A, A[:1] on one frozen model: each equals the fresh model's for that shape (the '#tile' bank keys of the Winograd precisions;
    the kept padded copies of bf16_train and fp8_infer, whose zero borders are cleared only on a geometry change)."""
    flat, cal = params(1)[1], cal_for(precision, 1)
    e, f = fresh(precision, flat, calibration=cal), fresh(precision, flat, calibration=cal)
    want = {id(img): logits(f, img) for img in (A, B)}
    f.close()
    e.freeze(True)
    for img in (A, B, A):
        np.testing.assert_array_equal(logits(e, img), want[id(img)])
    f = fresh(precision, flat, calibration=cal)                     # (a model that has seen no other shape)
    np.testing.assert_array_equal(logits(e, A[:1]), logits(f, A[:1]))
    np.testing.assert_array_equal(logits(e, B), want[id(B)])
    e.close(); f.close()


# ---- 5. precision round trips ----------------------------------------------------------------------------------------------------
ROUND_TRIPS = (('fp32', 'bf16_train', 'fp32'), ('fp32', 'fp8_infer', 'bf16_fwd'), ('bf16_train', 'fp8_infer', 'bf16_train'), ('f32x3', 'bf16_fc', 'f32x2'))


@pytest.mark.parametrize("frozen", (True, False), ids=("frozen", "unfrozen"))
@pytest.mark.parametrize("trip", ROUND_TRIPS, ids=lambda t: ">".join(t))
def test_precision_round_trip(trip, frozen):
    """predict in each mode along the way (freeze held throughout, or never on): the last predict equals a fresh model created directly in
    the last mode, and the caller's winograd_min_cin / winograd_fc6 -- which the direct modes take over while they are on -- read back
    unchanged."""
    mine = {"winograd_min_cin": 128, "winograd_fc6": 0}             # not the defaults (64, 1)
    flat, cal = params(1)[1], calibration(1)
    e = fresh(trip[0], flat, options=mine, calibration=cal)
    if frozen:
        e.freeze(True)
    for mode in trip:
        e.set_precision(mode)
        got_a, got_b = logits(e, A), logits(e, B)
    assert e.get_option("frozen") == int(frozen)
    f = fresh(trip[-1], flat, options=mine, calibration=cal)
    np.testing.assert_array_equal(got_a, logits(f, A))
    np.testing.assert_array_equal(got_b, logits(f, B))
    e.set_precision('fp32')                                          # (a direct mode reports what it keeps for the day it is left: leave it)
    assert (e.get_option("winograd_min_cin"), e.get_option("winograd_fc6")) == (128, 0)
    e.close(); f.close()


# ---- 6. options while frozen -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,option,value,default",
                         [(p, "winograd_tile", 4, 6) for p in WINOGRAD] + [(p, "winograd_min_cin", 0, 64) for p in WINOGRAD] +
                         [("bf16_train", "bf16_infer_copies", 0, 1)])
def test_option_change_while_frozen(precision, option, value, default):
    """freeze, predict, set_option, predict = a fresh model with that option; the option set back, = a fresh model again.  Only the precisions
    in which the option decides anything.  The banks of the old option value are gone as well: a bank's key carries what the option decides
    (the tile, the kernel's layout), so an old one is never read again -- it would only stay allocated until the model is unfrozen; the
    long-lived model holds no more device memory than a fresh one taken through the same frozen passes."""
    flat = params(1)[1]
    base = device_bytes_live()
    e = fresh(precision, flat)
    e.freeze(True)
    first = {id(img): logits(e, img) for img in (A, B)}
    e.set_option(option, value)
    got = {id(img): logits(e, img) for img in (A, B)}
    bytes_e = device_bytes_live() - base                              # all that e holds (no other model is alive between `base` and here)
    f = fresh(precision, flat, options={option: value})
    f.freeze(True)
    for img in (A, B):
        np.testing.assert_array_equal(got[id(img)], logits(f, img))
    bytes_f = device_bytes_live() - base - bytes_e                    # all that f holds
    # Both are frozen, hold the option's new value and last ran A, then B.  Expected equal: the optimizer / staging buffers of a new model, the
    # arena (set_option drops it, the next pass plans it exactly for its shape: B's plan under the new value in both), the banks of the new value
    # for A's and B's tiles, the bf16 kernels.  The shared scratch grows with the shape only, and both saw A and B.  What e could hold beyond
    # that is what it built under the OLD value: the banks set_option must drop.
    assert bytes_e <= bytes_f, (bytes_e, bytes_f)
    assert e.get_option("frozen") == 1
    e.set_option(option, default)
    for img in (A, B):
        np.testing.assert_array_equal(logits(e, img), first[id(img)])
    f.close()
    f = fresh(precision, flat)
    np.testing.assert_array_equal(logits(f, A), first[id(A)])
    e.close(); f.close()


# ---- 7. after predict_tta on a model that is not frozen --------------------------------------------------------------------------
@pytest.mark.parametrize("write", ("set_params", "side_door", "set_params_then_side_door"))
@pytest.mark.parametrize("precision", PRECISIONS)
def test_parameter_change_after_predict_tta(precision, write):
    """predict_tta keeps the storage of the banks it built on an unfrozen model, marked stale (bank_stale / banks_stale / g16_stale; fp8's
    w8_valid is cleared).  After a parameter change -- through the library, behind its back, or one after the other -- predict and
    predict_tta equal the fresh model's."""
    tta = dict(scales=(0.75, 1.0), flip=True, argmax=False)
    e = fresh(precision, params(1)[1], calibration=cal_for(precision, 1))
    before = e.predict_tta(A, **tta)
    cal = cal_for(precision, 1)
    if write.startswith("set_params"):
        e.set_params(params(2)[0])
        cal = cal_for(precision, 2)
        if cal is not None:
            e.set_fp8_calibration(cal)
    if write.endswith("side_door"):
        e.flat_params.mul_(1.01)
    f = fresh(precision, e.flat_params, calibration=cal)
    np.testing.assert_array_equal(logits(e, A), logits(f, A))
    after = e.predict_tta(A, **tta)
    np.testing.assert_array_equal(after, f.predict_tta(A, **tta))
    moved(after, before)
    np.testing.assert_array_equal(logits(e, B), logits(f, B))
    e.close(); f.close()


# ---- 8. training after serving ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("served_in", ("same", "other"))
@pytest.mark.parametrize("precision", TRAINING)
def test_training_after_serving(precision, served_in):
    """freeze, predict on B (in the training precision, or in another one first), then forward_backward on A: loss and all 42 gradients are
    bit for bit those of a fresh model that only ran that forward_backward (deterministic = 1 on both: the weight gradients' split sums
    otherwise meet in float atomics).  Then one train_step, freeze, predict = a fresh model loaded with the stepped parameters.  u_train: a
    mode whose forward pass does not refresh a bank must never find an old one; and training leaves the frozen state on its own."""
    flat = params(1)[1]
    det = {"deterministic": 1}
    other = 'bf16_train' if precision == 'fp32' else 'fp32'           # (fp32's training pass keeps a Winograd bank per layer in u_train)
    e = fresh(precision if served_in == "same" else other, flat, options=det)
    e.freeze(True)
    logits(e, B); logits(e, B)
    if served_in == "other":
        e.train_step(A, LABELS_A, 1e-3, keep_prob=1.0, l2_rate=1e-3)      # (leaves that mode's forward banks, of the parameters before the step, in u_train)
        e.freeze(True)
        logits(e, B)
        e.set_precision(precision)
    le = e.forward_backward(A, LABELS_A, keep_prob=1.0, l2_rate=1e-3)
    assert e.get_option("frozen") == 0
    ge = e.get_grads()
    f = fresh(precision, e.flat_params, options=det)
    lf = f.forward_backward(A, LABELS_A, keep_prob=1.0, l2_rate=1e-3)
    assert le == lf, (le, lf)
    gf = f.get_grads()
    assert len(gf) == 42
    for k in gf:
        np.testing.assert_array_equal(ge[k], gf[k], err_msg=k)
    before = logits(f, A)
    e.train_step(A, LABELS_A, 1e-3, keep_prob=1.0, l2_rate=1e-3)
    e.freeze(True)
    after = logits(e, A)
    f.close()
    f = fresh(precision, e.flat_params, options=det)
    np.testing.assert_array_equal(after, logits(f, A))
    moved(after, before)
    e.close(); f.close()


# ---- 9. calibration under freeze (fp8 only) --------------------------------------------------------------------------------------
def test_fp8_calibration_while_frozen():
    """While frozen: calibrate_fp8(A, reset=True) then predict = a fresh model given the resulting vector; set_fp8_calibration of another
    vector then predict = a fresh model with that one.  The activation scales follow the calibration; the weight banks, which do not depend
    on it, survive both (no fp8_quantize_w launch)."""
    flat = params(1)[1]
    e = fresh('fp8_infer', flat, calibration=calibration(1))
    e.freeze(True)
    base = logits(e, A)
    cal_a = e.calibrate_fp8(A, reset=True).copy()
    assert np.abs(cal_a - calibration(1)).max() > 0
    for cal in (cal_a, (cal_a * 1.5).astype(np.float32)):
        if cal is not cal_a:
            e.set_fp8_calibration(cal)
        assert e.get_option("frozen") == 1
        got, prof = profiled(e, A)
        f = fresh('fp8_infer', flat, calibration=cal)
        np.testing.assert_array_equal(got, logits(f, A))
        f.close()
        assert np.abs(got - base).max() > 0                          # the activation scales did change
        assert sum(n for k, n in derived_work(prof).items() if k.startswith("fp8_quantize_w")) == 0, derived_work(prof)
    e.close()


# ---- 10. a pass refused inside predict_tta ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("frozen", (True, False), ids=("frozen", "unfrozen"))
def test_refused_pass_inside_predict_tta(frozen):
    """An fp8_infer model that was never calibrated: predict_tta's first pass is refused by forward() (FCN8S_ERR_STATE, a host-side return)
    after the call has frozen the model for its passes.  The model is left as it was found -- frozen or not -- and, once calibrated, predicts
    bit for bit what a fresh model does that never saw the refused call; unfrozen, also after new parameters and a new calibration (the
    refused call marked the banks stale like any other)."""
    import ctypes as C
    from fcn8s_tensorflow_amd import _lib as L
    img = _images((1, 64, 64), 4)
    tta = dict(scales=(0.5, 1.0), argmax=False)                      # two passes, 32 x 32 and 64 x 64: not the identity shortcut

    def calibrated(flat):
        f = fresh('fp8_infer', flat)
        if frozen:
            f.freeze(True)
        f.calibrate_fp8(img, reset=True)
        return f
    e = fresh('fp8_infer', params(1)[1])
    if frozen:
        e.freeze(True)
    with pytest.raises(L.Fcn8sError, match="no FP8 calibration"):
        e.predict_tta(img, **tta)
    assert e.get_option("frozen") == int(frozen)
    out = np.empty((1, 64, 64, CLASSES), np.float32)
    rc = L.lib.fcn8s_predict_tta(e.h, img.ctypes.data_as(C.c_void_p), L.IMG_U8, 1, 64, 64, (C.c_float * 2)(0.5, 1.0), 2, 0, 0,
                                 out.ctypes.data_as(C.c_void_p), L.HOST)
    assert rc == L.ERR_STATE
    assert e.get_option("frozen") == int(frozen)
    e.calibrate_fp8(img, reset=True)
    f = calibrated(params(1)[1])
    first = e.predict_tta(img, **tta)
    np.testing.assert_array_equal(first, f.predict_tta(img, **tta))
    assert e.get_option("frozen") == int(frozen)
    f.close()
    if not frozen:
        e.set_params(params(2)[0])
        e.calibrate_fp8(img, reset=True)
        f = calibrated(params(2)[1])
        second = e.predict_tta(img, **tta)
        np.testing.assert_array_equal(second, f.predict_tta(img, **tta))
        moved(second, first)
        f.close()
    e.close()
