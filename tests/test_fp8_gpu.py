"""FCN8S_PREC_FP8_INFER ('fp8_infer') on the MI355X: the e4m3 conversion, the MX-MFMA convolution against float64 of the dequantized
operands, the model's FP8 layers against torch on the device's own operands, calibration and its state rules, batch invariance, workspace
reuse, and the facade."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import fcn8s_oracle as orc  # noqa: E402  (checker only)
from fcn8s_tensorflow_amd import fp8  # noqa: E402
from fcn8s_tensorflow_amd import _lib as L  # noqa: E402
from tests import hostile  # noqa: E402

WIDTHS = (64, 64, 128, 256, 256, 256, 128)


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def op_conv_fp8(x, w, b, x_exp, relu=1):
    """One call on tests/hostile.py's memory (the model-level tests of this module run on the model's own): x, w, b fenced by NaN bands and
    checked intact, y NaN inside its bands until written, verify() before the result is handed back."""
    N, H, W, Cin = x.shape
    K, Cout = w.shape[0], w.shape[-1]
    with hostile.session(L) as arena:
        xd, wd = arena.inp(x.astype(np.float32), "x"), arena.inp(w.astype(np.float32), "w")
        bd = arena.inp(b.astype(np.float32), "b") if b is not None else None
        y = arena.out((N, H, W, Cout), name="y")
        L.check(L.lib.fcn8s_op_conv2d_fp8(None, ptr(xd), ptr(wd), ptr(bd), ptr(y), relu, x_exp, N, H, W, Cin, Cout, K))
        torch.cuda.synchronize()
        return y.cpu().numpy()


def conv64(x, w):
    """float64 SAME convolution, NHWC x, HWIO w"""
    k = w.shape[0]
    xt = torch.as_tensor(np.asarray(x, np.float64)).permute(0, 3, 1, 2)
    wt = torch.as_tensor(np.asarray(w, np.float64)).permute(3, 2, 0, 1)
    return F.conv2d(xt, wt, padding=(k - 1) // 2).permute(0, 2, 3, 1).numpy()


def fp8_sweep():
    from tests.test_fp8_host import sweep
    return sweep()


def test_device_conversion_is_the_host_rule_bit_for_bit():
    """An identity 1x1 layer (w = I: ew = E(1) = -8, Wq = 256) returns 2^0 q(x) exactly: the device's q is the host's on every e4m3 code,
    its fp32 neighbours, the exact midpoints (ties to even), subnormals, +-0 and values beyond +-448 (which the explicit clamp saturates)."""
    v = fp8_sweep()
    n = (v.size + 63) // 64 * 64
    x = np.zeros(n, np.float32); x[:v.size] = v
    x = x.reshape(1, 1, n // 64, 64)
    y = op_conv_fp8(x, np.eye(64, dtype=np.float32).reshape(1, 1, 64, 64), None, 0, relu=0)
    want = fp8.q(x)
    # (bit patterns, except that the sign of a zero does not survive the sum: -0 x 256 + 63 x (+0) = +0)
    yv, wv = y.reshape(-1)[:v.size], want.reshape(-1)[:v.size]
    bad = np.nonzero((yv.view(np.uint32) != wv.view(np.uint32)) & ~((yv == 0) & (wv == 0)))[0]
    assert bad.size == 0, [(float(v[i]), float(y.reshape(-1)[i]), float(want.reshape(-1)[i])) for i in bad[:10]]
    # NaN stays NaN on both sides (a clamp through fminf / fmaxf would turn it into -448, a finite output): a pixel with a NaN input comes out
    # NaN in every channel (0 x NaN = NaN in the sum), a finite pixel next to it is untouched
    xn = np.ones((1, 1, 3, 64), np.float32); xn[0, 0, 0, 5] = np.nan; xn[0, 0, 1, 9] = -np.nan
    yn = op_conv_fp8(xn, np.eye(64, dtype=np.float32).reshape(1, 1, 64, 64), None, 0, relu=0)
    assert np.isnan(yn[0, 0, :2]).all() and (yn[0, 0, 2] == 1.0).all()
    assert np.isnan(fp8.q(xn)[0, 0, 0, 5]) and np.isnan(fp8.q(xn)[0, 0, 1, 9])


CASES = [
    # N, H, W, Cin, Cout, K
    (1, 9, 13, 64, 64, 3),
    (3, 8, 10, 128, 128, 3),
    (1, 5, 7, 512, 128, 3),
    (3, 6, 5, 64, 512, 7),
    (1, 4, 3, 512, 64, 7),
    (3, 7, 9, 128, 64, 1),
    (1, 4, 4, 512, 4096, 1),
]
# Measured on the MI355X: |y - ref| / sum|a b| reaches 2.0e-5 (1x1, Cin 128) and 1-7e-6 for the 3x3 / 7x7 cases -- well above what an fp32
# fmaf chain over the same exact e4m3 products gives (about 1e-7 at these depths, the bf16 kernels hold 1e-5): the MX instruction does not add
# its 64 products exactly before the fp32 accumulate.  The integer test below is exact, so this is rounding inside the sum, not a lane-map error.
TOL = 6e-5


@pytest.mark.parametrize("N,H,W,Cin,Cout,K", CASES)
def test_op_conv2d_fp8_against_float64_of_the_dequantized_operands(N, H, W, Cin, Cout, K):
    rng = np.random.default_rng(N * 1000 + Cin + Cout + K)
    x = np.maximum(rng.standard_normal((N, H, W, Cin)), 0).astype(np.float32) * 3
    w = (rng.standard_normal((K, K, Cin, Cout)) * np.sqrt(2.0 / (K * K * Cin)) * np.logspace(-1, 1, Cout)).astype(np.float32)
    b = (rng.standard_normal(Cout) * 0.1).astype(np.float32)
    ex = fp8.exponent(np.abs(x).max())
    y = op_conv_fp8(x, w, b, ex, relu=0)
    xq = fp8.quantize_activation(x, ex).numpy().astype(np.float64)
    wq, ew = fp8.quantize_weights(w)
    wd = wq.numpy().astype(np.float64) * np.ldexp(1.0, ew)
    ref = conv64(xq, wd) + b
    mag = conv64(np.abs(xq), np.abs(wd)) + np.abs(b)
    err = (np.abs(y - ref) / (mag + 1e-30)).max()
    print("fp8 conv %s: max |y - ref| / sum|ab| = %.3g" % ((N, H, W, Cin, Cout, K), err))
    assert err < TOL


@pytest.mark.parametrize("N,H,W,Cin,Cout,K", [(3, 7, 11, 64, 128, 3), (1, 5, 6, 128, 64, 7), (3, 5, 5, 128, 128, 1)])
def test_op_conv2d_fp8_integer_data_is_exact(N, H, W, Cin, Cout, K):
    """Integers |x| <= 8 and |w| <= 4 are e4m3 values (w scaled by 2^6 still is), every partial sum is an integer below 2^24: any lane-map
    error (A row / B column / channel pairing) shows up as a wrong integer.  B is asymmetric (random per column)."""
    rng = np.random.default_rng(K * 7 + Cin)
    x = rng.integers(-8, 9, (N, H, W, Cin)).astype(np.float32)
    w = rng.integers(-4, 5, (K, K, Cin, Cout)).astype(np.float32)
    w[0, 0, 0, :] = 4.0                                          # every column's max is 4: ew = -6, Wq = 64 w exactly
    y = op_conv_fp8(x, w, None, fp8.exponent(8.0), relu=0)
    ref = conv64(x, w)
    np.testing.assert_array_equal(y, ref.astype(np.float32))


# ---- the model ---------------------------------------------------------------------------------------------------------------------
def model(seed=0, num_classes=20):
    from fcn8s_tensorflow_amd.engine import Engine
    P = orc.init_params(num_classes, WIDTHS, seed=seed, decoder_std_scale=6.0, bias_std=0.05)
    e = Engine(num_classes, widths=WIDTHS, device_id=0)
    e.set_params(P)
    return e, P


def images(n=2, h=64, w=96, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


GEOM = {  # FP8 layer -> (down-sampling of its input map, width index of its input channels, K)
    "conv1_2": (1, 0, 3), "conv2_1": (2, 0, 3), "conv2_2": (2, 1, 3), "conv3_1": (4, 1, 3), "conv3_2": (4, 2, 3), "conv3_3": (4, 2, 3),
    "conv4_1": (8, 2, 3), "conv4_2": (8, 3, 3), "conv4_3": (8, 3, 3), "conv5_1": (16, 3, 3), "conv5_2": (16, 4, 3), "conv5_3": (16, 4, 3),
    "fc6": (32, 4, 7), "fc7": (32, 5, 1)}


def q8(e, layer, N, H, W):
    d, wi, _ = GEOM[layer]
    return e.activation("q8:" + layer, (N, H // d, W // d, WIDTHS[wi]))


def test_fp8_layers_equal_torch_on_the_devices_own_operands():
    """Each FP8 layer's output copy ("q8:<next>") equals torch evaluated on the device's quantized input and weights, quantized with the
    consumer's exponent.  Codes may differ only where the exact value lies within the measured sum rounding (TOL x sum |a b|) of an e4m3
    rounding midpoint; those elements are counted and bounded."""
    e, P = model()
    img = images()
    N, H, W, _ = img.shape
    e.set_precision('fp8_infer')
    amax = e.calibrate_fp8(img, reset=True)
    ex = fp8.exponents(amax)
    e.predict(img)
    layers = list(fp8.LAYERS)
    total = near = 0
    for Li, name in enumerate(layers):
        xin = torch.as_tensor(q8(e, name, N, H, W), dtype=torch.float64).permute(0, 3, 1, 2)
        wkey = name + ("/weights" if name.startswith("fc") else "/filter")
        wq, ew = fp8.quantize_weights(P[wkey])
        wd = torch.as_tensor(wq.numpy().astype(np.float64) * np.ldexp(1.0, ew))
        k = wd.shape[0]
        bias = torch.as_tensor(P[name + "/biases"], dtype=torch.float64)
        y = F.relu(F.conv2d(xin, wd.permute(3, 2, 0, 1), bias, padding=(k - 1) // 2))
        mag = F.conv2d(xin.abs(), wd.abs().permute(3, 2, 0, 1), bias.abs(), padding=(k - 1) // 2)      # sum |a b| + |b| per output
        if name == "fc7":
            got = e.activation("fc7", (N, H // 32, W // 32, WIDTHS[6]))
            ref = y.permute(0, 2, 3, 1).numpy()
            assert np.abs(got - ref).max() <= TOL * np.abs(ref).max()
            continue
        nxt = layers[Li + 1]
        last = name in ("conv1_2", "conv2_2", "conv3_3", "conv4_3", "conv5_3")
        if last:
            y, mag = F.max_pool2d(y, 2, 2), F.max_pool2d(mag, 2, 2)
        s = 2.0 ** -ex[Li + 1]
        want = fp8.codes((y * s).float()).permute(0, 2, 3, 1).numpy()
        got = fp8.codes(torch.as_tensor(q8(e, nxt, N, H, W)) * s).numpy()
        diff = got != want
        total += want.size
        if diff.any():
            # each differing element is a near-tie: the device's fp32 value lies within the measured sum rounding (TOL x sum |a b|) of the
            # exact one, and its code is one of the codes q takes on that interval (non-negative codes order like their values)
            v = (y * s).permute(0, 2, 3, 1).numpy()[diff]
            ms = (mag * s).permute(0, 2, 3, 1).numpy()[diff]
            lo = fp8.codes(torch.as_tensor(np.maximum(v - TOL * ms, 0.0)).float()).numpy()
            hi = fp8.codes(torch.as_tensor(v + TOL * ms).float()).numpy()
            g = got[diff]
            assert ((g >= lo) & (g <= hi)).all(), (name, int((g < lo).sum() + (g > hi).sum()))
            near += int(diff.sum())
    print("fp8 layers: %d of %d codes differ from the exact rounding, all at near-ties" % (near, total))
    assert near <= 1e-3 * total
    e.close()


def fp8_forward_t(P, img, amax, device_copy=None, stats=None):
    """torch restatement of the whole fp8_infer forward pass (float64 sums): fp32 conv1_1; every FP8 layer on q(x 2^-ex) with ex from the
    device's calibration and on the per-channel quantized weights (fp8.py); fp32 pools (the device's byte-max pool is the same thing after q,
    which is monotone); the fp32 decoder on pool3, pool4 and fc7.  Returns NCHW logits.
    device_copy(layer) -> the device's dequantized input copy of `layer` (NHWC): where the restatement's code differs from the device's, the
    element must be a rounding near-tie -- the device's code lies among the codes q takes within TOL x sum |a b| of the exact value -- and the
    restatement then takes the device's code (as smoke() follows the device's ReLU decisions at ties); stats counts those elements."""
    Pt = {k: torch.as_tensor(v, dtype=torch.float64) for k, v in P.items()}
    ex = fp8.exponents(amax)

    def quant(x, mag, name, L):
        xq = fp8.quantize_activation(x.float(), ex[L]).double()
        if device_copy is None:
            return xq
        s = 2.0 ** -ex[L]
        dq = torch.as_tensor(device_copy(name), dtype=torch.float64).permute(0, 3, 1, 2)
        diff = (xq != dq)
        if bool(diff.any()):
            v, ms = (x * s)[diff], (mag * s)[diff]
            lo = fp8.codes(torch.clamp(v - TOL * ms, min=0.0).float())
            hi = fp8.codes((v + TOL * ms).float())
            g = fp8.codes((dq * s)[diff].float())
            assert bool(((g >= lo) & (g <= hi)).all()), (name, "an e4m3 code differs from the restatement's away from a rounding tie")
            stats["ties"] = stats.get("ties", 0) + int(diff.sum())
        stats["codes"] = stats.get("codes", 0) + xq.numel()
        return dq

    def conv(x, w, b, relu=True):
        return orc.conv2d_same_t(x, w, b, relu=relu), orc.conv2d_same_t(x.abs(), w.abs(), b.abs())

    def conv8(x, mag, name, L):
        wq, ew = fp8.quantize_weights(P[name + ("/weights" if name.startswith("fc") else "/filter")])
        wd = torch.as_tensor(wq.numpy().astype(np.float64) * np.ldexp(1.0, ew))
        return conv(quant(x, mag, name, L), wd, Pt[name + "/biases"])

    x = orc.preprocess_t(torch.as_tensor(img.astype(np.float64))).permute(0, 3, 1, 2)
    x, mag = conv(x, Pt["conv1_1/filter"], Pt["conv1_1/biases"])
    L, pools = 0, {}
    for blk, nconv in enumerate(orc.CONVS_PER_BLOCK, start=1):
        for i in range(1, nconv + 1):
            if blk == 1 and i == 1:
                continue
            x, mag = conv8(x, mag, "conv%d_%d" % (blk, i), L); L += 1
        x, mag = orc.maxpool2x2_t(x), orc.maxpool2x2_t(mag)
        pools[blk] = x
    x, mag = conv8(x, mag, "fc6", 12)
    x, mag = conv8(x, mag, "fc7", 13)
    p3 = orc.conv2d_same_t(pools[3] * orc.POOL3_SCALE, Pt["pool3_1x1/kernel"], Pt["pool3_1x1/bias"])
    p4 = orc.conv2d_same_t(pools[4] * orc.POOL4_SCALE, Pt["pool4_1x1/kernel"], Pt["pool4_1x1/bias"])
    s7 = orc.conv2d_same_t(x, Pt["fc7_1x1/kernel"], Pt["fc7_1x1/bias"])
    a4 = orc.conv2d_transpose_same_t(s7, Pt["fc7_conv2d_trans/kernel"], Pt["fc7_conv2d_trans/bias"], 2) + p4
    a3 = orc.conv2d_transpose_same_t(a4, Pt["fc7_pool4_conv2d_trans/kernel"], Pt["fc7_pool4_conv2d_trans/bias"], 2) + p3
    return orc.conv2d_transpose_same_t(a3, Pt["fc7_pool4_pool3_conv2d_trans/kernel"], Pt["fc7_pool4_pool3_conv2d_trans/bias"], 8)


# Measured on the MI355X: with the restatement following the device at its e4m3 rounding near-ties, the logits agree to 1e-5 of their range or
# better.  Without that (each side rounding its own ties) the two drift apart chaotically: a code flip is a 6-12 % change of one element, it
# flips more codes in the next layer, and after thirteen layers the logits differed by 0.084 of their range -- about the size of the e4m3
# quantization itself (the same logits against the fp32 graph: 0.107).  So the decisions are checked to be ties and then followed.
E2E_TOL = 2e-4


def test_fp8_logits_against_a_torch_restatement_of_the_whole_fp8_forward():
    """The device's logits against fp8_forward_t fed by the same image and the device's calibration (every e4m3 code the device chose away from
    the restatement's checked to be a rounding near-tie, and their count bounded), within E2E_TOL of the logits' range; argmax identical
    wherever the top-2 margin exceeds twice that."""
    e, P = model(seed=5)
    img = images(seed=5)
    N, H, W, _ = img.shape
    e.set_precision('fp8_infer')
    amax = e.calibrate_fp8(img, reset=True)
    e.predict(img)
    got = e.activation("logits", (N, H, W, 20))
    stats = {}
    ref = fp8_forward_t(P, img, amax, device_copy=lambda name: q8(e, name, N, H, W), stats=stats).permute(0, 2, 3, 1).numpy()
    rng_ = np.abs(ref).max()
    err = np.abs(got - ref).max() / rng_
    srt = np.sort(ref, -1)
    safe = (srt[..., -1] - srt[..., -2]) > 2 * E2E_TOL * rng_
    agree = (np.argmax(got, -1) == np.argmax(ref, -1))
    # for the record: the FP8 logits against the fp32 graph (the oracle), i.e. what quantization itself costs on this model
    f32 = orc.forward_t({k: torch.as_tensor(v) for k, v in P.items()}, torch.as_tensor(img.astype(np.float32))).permute(0, 2, 3, 1).numpy()
    print("fp8 e2e: max |dev - restatement| = %.3g of the logits' range; %d of %d codes followed at ties; argmax checked on %d / %d pixels; "
          "vs fp32: %.3g of the range, argmax agreement %.4f" % (err, stats.get("ties", 0), stats["codes"], int(safe.sum()), safe.size,
                                                                  np.abs(got - f32).max() / np.abs(f32).max(),
                                                                  float((np.argmax(got, -1) == np.argmax(f32, -1)).mean())))
    assert stats.get("ties", 0) <= 1e-3 * stats["codes"]
    assert err < E2E_TOL
    assert safe.mean() > 0.5 and agree[safe].all()
    e.close()


def test_winograd_options_do_not_reach_the_fp8_pass():
    """fp8_infer rides on the direct path like bf16_train: winograd_min_cin / winograd_fc6 set while it is on are kept for later (get_option
    reports them) and do not switch conv1_1 into conv1_2's input transform, whose fp32 output the FP8 pass needs."""
    e, P = model(seed=6)
    img = images(seed=6)
    e.set_precision('fp8_infer')
    e.calibrate_fp8(img, reset=True)
    base = e.predict(img, argmax=False)
    e.set_option("winograd_min_cin", 64)
    e.set_option("winograd_fc6", 1)
    assert e.get_option("winograd_min_cin") == 64 and e.get_option("winograd_fc6") == 1
    np.testing.assert_array_equal(e.predict(img, argmax=False), base)
    e.calibrate_fp8(img, reset=True)
    np.testing.assert_array_equal(e.predict(img, argmax=False), base)
    e.set_precision('fp32')
    assert e.get_option("winograd_min_cin") == 64 and e.get_option("winograd_fc6") == 1
    e.close()


def test_calibration_state_rules():
    e, P = model(seed=1)
    img1, img2 = images(seed=1), images(seed=2)
    with pytest.raises(L.Fcn8sError):
        e.calibrate_fp8(img1)                                   # not in the mode
    e.set_precision('fp8_infer')
    with pytest.raises(L.Fcn8sError, match="calibration"):
        e.predict(img1)                                         # no calibration yet
    a1 = e.calibrate_fp8(img1, reset=True)
    # the maxima are those of the fp32 forward pass
    _, acts = orc.forward_t({k: torch.as_tensor(v) for k, v in P.items()}, torch.as_tensor(img1.astype(np.float32)), keep=True)
    ref = np.array([float(acts[n].abs().max()) for n in fp8.INPUTS], np.float32)
    np.testing.assert_allclose(a1, ref, rtol=1e-4)
    for a, r in zip(a1, ref):
        e_b = 448.0 * 2.0 ** fp8.exponent(r)
        if abs(r - e_b) > 1e-5 * r and abs(r - e_b / 2) > 1e-5 * r:
            assert fp8.exponent(a) == fp8.exponent(r)
    # accumulation and reset: deterministic maxima
    a2 = e.calibrate_fp8(img2, reset=True)
    e.calibrate_fp8(img1, reset=True)
    a12 = e.calibrate_fp8(img2)
    np.testing.assert_array_equal(a12, np.maximum(a1, a2))
    np.testing.assert_array_equal(e.calibrate_fp8(img1, reset=True), a1)
    p1 = e.predict(img1, argmax=False)
    # get / set round trip
    cal = e.fp8_calibration()
    e.set_fp8_calibration(a2)
    e.set_fp8_calibration(cal)
    np.testing.assert_array_equal(e.predict(img1, argmax=False), p1)
    # survives a set_precision round trip
    e.set_precision('bf16_train'); e.set_precision('fp8_infer')
    np.testing.assert_array_equal(e.fp8_calibration(), cal)
    np.testing.assert_array_equal(e.predict(img1, argmax=False), p1)
    # training in the mode is refused, and leaves the calibration alone
    lab = np.zeros(img1.shape[:3], np.uint8)
    with pytest.raises(L.Fcn8sError, match="inference only"):
        e.train_step(img1, lab, 1e-4, keep_prob=1.0)
    with pytest.raises(L.Fcn8sError, match="inference only"):
        e.forward_backward(img1, lab)
    np.testing.assert_array_equal(e.fp8_calibration(), cal)
    # writing parameters clears it
    e.set_params({"conv1_1/biases": P["conv1_1/biases"]})
    assert e.fp8_calibration() is None
    with pytest.raises(L.Fcn8sError, match="calibration"):
        e.predict(img1)
    e.close()


def test_invariance_and_reuse():
    e, P = model(seed=3)
    img = images(n=3, seed=3)
    e.set_precision('fp8_infer')
    e.calibrate_fp8(img, reset=True)
    full = e.predict(img, argmax=False)
    for i in range(3):
        np.testing.assert_array_equal(e.predict(img[i:i + 1], argmax=False)[0], full[i])
    np.testing.assert_array_equal(e.predict_tta(img, scales=(1.0,), flip=False, argmax=False), full)
    e.predict_tta(img[:, :50, :70], scales=(0.75, 1.0, 1.25), flip=True)
    n0 = e.get_option("workspace_allocations")
    r1 = e.predict_tta(img[:, :50, :70], scales=(0.75, 1.0, 1.25), flip=True)
    assert e.get_option("workspace_allocations") == n0
    np.testing.assert_array_equal(e.predict_tta(img[:, :50, :70], scales=(0.75, 1.0, 1.25), flip=True), r1)
    # a frozen model quantizes its weight banks once
    e.freeze(True)
    e.profile(True); e.profile_reset()
    e.predict(img); e.predict(img)
    res = e.profile_results()
    assert res["fp8_quantize_w"]["launches"] == 14
    assert res["conv3x3_fwd_fp8"]["launches"] == 2 * 12
    e.freeze(False); e.profile(False)
    # eval_step's confusion matrix is the one of the FP8 predictions
    lab = np.random.default_rng(4).integers(0, 20, img.shape[:3], dtype=np.uint8)
    pred = e.predict(img)
    e.metrics_reset()
    e.eval_step(img, orc.one_hot(lab, 20))
    cm, _, _ = e.metrics_raw()
    want = np.zeros((20, 20), np.int64)
    np.add.at(want, (lab.reshape(-1).astype(np.int64), pred.reshape(-1)), 1)
    np.testing.assert_array_equal(cm, want)
    e.close()


def test_facade_calibrate_save_load(tmp_path):
    from fcn8s_tensorflow_amd.fcn8s import FCN8s

    def gen(seed):
        rng = np.random.default_rng(seed)
        while True:
            img = rng.integers(0, 256, (2, 64, 96, 3), dtype=np.uint8)
            yield img, orc.one_hot(rng.integers(0, 20, (2, 64, 96), dtype=np.uint8), 20)

    m = FCN8s(vgg16_dir='synthetic:3', num_classes=20, widths=WIDTHS)
    cal = m.calibrate_fp8(gen(0), 2)
    assert m.engine.precision == 'fp8_infer' and cal.shape == (14,)
    img = next(gen(5))[0]
    pred = m.predict(img, argmax=False)
    with pytest.raises(ValueError, match="fp8_infer"):
        m.train(gen(1), epochs=1, steps_per_epoch=1, learning_rate_schedule=lambda s: 1e-4)
    m.save(str(tmp_path), 'saved_model', tags=['default'], force_save=True)
    saved = [d for d in (tmp_path.iterdir()) if d.is_dir()]
    m.close()
    m2 = FCN8s(model_load_dir=str(saved[0]), tags=['default'])
    np.testing.assert_array_equal(m2.engine.fp8_calibration(), cal)
    m2.engine.set_precision('fp8_infer')
    np.testing.assert_array_equal(m2.predict(img, argmax=False), pred)
    m2.close()
