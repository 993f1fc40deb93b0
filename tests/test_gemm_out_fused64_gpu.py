"""Option gemm_out_fused64 (default 1): conv1_2's forward -- the 64 position GEMMs of F(6x6,3x3), the output transform, bias, ReLU and the
2x2/2 max-pool with its argmax bytes -- as ONE kernel (csrc/wino_fused64.hip: wino_gemm_out64_kernel; M is never written), against the two-kernel
route (option 0) on seeded inputs.  The fused epilogue runs the fma chains of wino_output_kernel in their order, so the only arithmetic difference
is the summation order of the 64-term position GEMMs: everything agrees to round-off.

A narrow model (widths[0] = 64 puts conv1_2 on the route, the rest as small as smoke()'s) on the two shapes that walk the kernel's edge cases:
  1 x 64x64: 11 x 11 = 121 tiles -- seven full blocks of 16 tiles and one of 9 (clamped loads, skipped stores), partial edge tiles both ways (64 = 10 * 6 + 4)
  2 x 32x64: 6 x 11 = 66 tiles per image, 132 in all -- the block of tiles 64..79 straddles the two images
(The kernel alone -- launches of fewer than 16 tiles, every (H % 6, W % 6) edge, the argmax bytes against a rule of their own, the second filter
bank -- is held to float64 at op level in tests/test_gemm_out_fused64_ops_gpu.py; this module is the route inside a model.  Since the rule implies
that the pool is routed in the transform, no pass of a model on this route can ask for conv1_2's full-resolution activation: of the two declining
cases only the precision can be exercised: f32x3 and bf16_fc.)

Tolerances are those of test_model_gpu.py::test_conv1_1_inside_conv1_2_input_transform, the same kind of change (a summation order inside block 1)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import fcn8s_oracle as orc  # noqa: E402  (checker only)

WIDTHS = (64, 16, 32, 64, 64, 128, 128)
SHAPES = ((1, 64, 64), (2, 32, 64))
SEED = 31
KERNEL = "wino_gemm_out64_kernel"


@functools.lru_cache(maxsize=None)
def params():
    return orc.init_params(20, WIDTHS, seed=SEED, decoder_std_scale=6.0, bias_std=0.05)


@functools.lru_cache(maxsize=None)
def inputs(n, h, w):
    rng = np.random.default_rng(SEED + 100)
    img = rng.integers(0, 256, (2, h, w, 3), dtype=np.uint8)          # (image 0 is the same whatever n)
    lab = rng.integers(0, 20, (2, h, w), dtype=np.uint8)
    return img[:n], lab[:n]


@functools.lru_cache(maxsize=None)
def reference(n, h, w):
    """float64: conv1_2 before its ReLU (NHWC) and pool1, from the oracle's conv1_1."""
    import torch
    P = params()
    img, _ = inputs(n, h, w)
    _, acts = orc.forward(P, img, dtype=torch.float64, keep=True)
    x = torch.as_tensor(acts["conv1_1"]).permute(0, 3, 1, 2)
    z = orc.conv2d_same_t(x, torch.as_tensor(P["conv1_2/filter"]).double(), torch.as_tensor(P["conv1_2/biases"]).double())
    z = z.permute(0, 2, 3, 1).contiguous().numpy()
    pool = np.asarray(acts["pool1"], np.float64)
    win = z.reshape(n, h // 2, 2, w // 2, 2, 64).transpose(0, 1, 3, 5, 2, 4).reshape(n, h // 2, w // 2, 64, 4)
    assert np.abs(np.maximum(win.max(-1), 0) - pool).max() < 1e-12
    return z, pool, win


def value_tol(pool):
    return 2e-5 * max(1.0, float(np.abs(pool).max()))


def ambiguous(n, h, w):
    """Windows whose argmax byte round-off may decide: the two largest entries, or the largest and 0, closer than the value tolerance."""
    _, pool, win = reference(n, h, w)
    tol = value_tol(pool)
    srt = np.sort(np.maximum(win, 0), -1)
    return ((srt[..., 3] - srt[..., 2] < tol) & (srt[..., 3] > 0)) | (np.abs(win.max(-1)) < tol)


@functools.lru_cache(maxsize=None)
def run(n, h, w, fused, precision="fp32", deterministic=0):
    from fcn8s_tensorflow_amd.engine import Engine
    img, lab = inputs(n, h, w)
    e = Engine(20, widths=WIDTHS, device_id=0, precision=precision, options={"gemm_out_fused64": fused, "deterministic": deterministic})
    assert e.get_option("gemm_out_fused64") == fused
    e.set_params(params())
    e.profile(2); e.profile_reset()
    r = {}
    r["loss"] = e.forward_backward(img, orc.one_hot(lab, 20), keep_prob=1.0, l2_rate=1e-3)
    r["train_kernels"] = [k for k in e.profile_results() if k.startswith("kernel:")]
    e.profile_reset()
    r["grads"] = e.get_grads()
    r["pool1"] = e.activation("pool1", (n, h // 2, w // 2, 64))
    r["bytes"] = e.pool_routes((n, h, w))["pool1"]
    r["logits"] = e.activation("logits", (n, h, w, 20))
    # the same pass again: identical bits
    r["loss2"] = e.forward_backward(img, orc.one_hot(lab, 20), keep_prob=1.0, l2_rate=1e-3)
    r["pool1_2"] = e.activation("pool1", (n, h // 2, w // 2, 64))
    r["bytes_2"] = e.pool_routes((n, h, w))["pool1"]
    e.profile_reset()
    r["pred"] = e.predict(img, argmax=False)                        # inference: no argmax bytes, V in the shared scratch
    r["infer_kernels"] = [k for k in e.profile_results() if k.startswith("kernel:")]
    e.profile(0)
    e.freeze(True); r["pred_frozen"] = (e.predict(img, argmax=False), e.predict(img, argmax=False)); e.freeze(False)      # the kept bank, made and reused
    e.close()
    return r


def ran(kernels):
    return any(KERNEL in k for k in kernels)


@pytest.mark.parametrize("n,h,w", SHAPES)
def test_the_seed_leaves_few_windows_to_round_off(n, h, w):
    """The reference alone: far fewer than the 0.1 % of windows the byte comparison may exclude are within the value tolerance of a tie."""
    amb = ambiguous(n, h, w)
    print("ambiguous windows: %d of %d" % (int(amb.sum()), amb.size))
    assert amb.mean() < 2e-4


@pytest.mark.parametrize("n,h,w", SHAPES)
def test_fused_against_two_kernels(n, h, w):
    """pool1, logits, loss, every gradient, the predictions: round-off apart.  Against the float64 oracle on pool1 the fused form's largest error
    is at most twice the two-kernel form's (both are 64-term fp32 chains with one worst-case bound).  The argmax bytes are equal except in windows
    within the value tolerance of a tie (at most 0.1 % of them)."""
    f, u = run(n, h, w, 1), run(n, h, w, 0)
    assert ran(f["train_kernels"]) and ran(f["infer_kernels"]), f["train_kernels"]
    assert not ran(u["train_kernels"]) and not ran(u["infer_kernels"]), u["train_kernels"]
    _, ref, _ = reference(n, h, w)
    tol = value_tol(ref)
    d = float(np.abs(f["pool1"] - u["pool1"]).max())
    ef, eu = float(np.abs(f["pool1"] - ref).max()), float(np.abs(u["pool1"] - ref).max())
    print("%d x %dx%d pool1: fused - two-kernel %.3g (tolerance %.3g); against float64: fused %.3g, two kernels %.3g; largest |pool1| %.3g"
          % (n, h, w, d, tol, ef, eu, float(np.abs(ref).max())))
    assert d <= tol
    assert ef <= 2.0 * eu
    assert abs(f["loss"] - u["loss"]) <= 2e-6 * abs(u["loss"])
    assert np.abs(f["logits"] - u["logits"]).max() <= 2e-5 * max(1.0, np.abs(u["logits"]).max())
    assert np.abs(f["pred"] - u["pred"]).max() <= 2e-5
    for k in u["grads"]:
        a, b = np.asarray(f["grads"][k], np.float64), np.asarray(u["grads"][k], np.float64)
        assert np.linalg.norm(a - b) <= 3e-2 * np.linalg.norm(b) + 1e-12, (k, np.linalg.norm(a - b) / np.linalg.norm(b))
    differ = f["bytes"] != u["bytes"]
    amb = ambiguous(n, h, w)
    print("argmax bytes: %d of %d differ, %d windows excluded as ties" % (int(differ.sum()), differ.size, int(amb.sum())))
    assert amb.mean() <= 1e-3
    assert not (differ & ~amb).any()
    # the frozen model's kept bank: made in one prediction, reused in the next
    np.testing.assert_array_equal(f["pred_frozen"][0], f["pred"]); np.testing.assert_array_equal(f["pred_frozen"][1], f["pred"])


@pytest.mark.parametrize("n,h,w", SHAPES)
def test_two_identical_runs_give_identical_bits(n, h, w):
    """The layer's outputs, pass after pass; the loss too where the library joins its reductions in a fixed order (deterministic = 1: the default
    joins the loss partials of these narrow widths with atomics, with or without the fused kernel)."""
    f, d = run(n, h, w, 1), run(n, h, w, 1, deterministic=1)
    np.testing.assert_array_equal(f["pool1"], f["pool1_2"])
    np.testing.assert_array_equal(f["bytes"], f["bytes_2"])
    np.testing.assert_array_equal(d["pool1"], d["pool1_2"])
    np.testing.assert_array_equal(d["bytes"], d["bytes_2"])
    print("loss, two passes: default %r %r (two kernels: %r %r), deterministic %r %r" % (f["loss"], f["loss2"], run(n, h, w, 0)["loss"], run(n, h, w, 0)["loss2"], d["loss"], d["loss2"]))
    assert d["loss"] == d["loss2"]


def test_an_image_does_not_depend_on_its_batch():
    """Image 0's pool1 and bytes at N = 1 are image 0's at N = 2 (the second image shares blocks with the first: 121 tiles per image)."""
    one, two = run(1, 64, 64, 1), run(2, 64, 64, 1)
    assert ran(two["train_kernels"])
    np.testing.assert_array_equal(one["pool1"][0], two["pool1"][0])
    np.testing.assert_array_equal(one["bytes"][0], two["bytes"][0])


@pytest.mark.parametrize("n,h,w", SHAPES)
def test_deterministic_changes_nothing_in_this_forward(n, h, w):
    a, b = run(n, h, w, 1), run(n, h, w, 1, deterministic=1)
    assert ran(b["train_kernels"])
    np.testing.assert_array_equal(a["pool1"], b["pool1"])
    np.testing.assert_array_equal(a["bytes"], b["bytes"])
    np.testing.assert_array_equal(a["pred"], b["pred"])


@pytest.mark.parametrize("precision", ["f32x3", "bf16_fc"])
def test_other_precisions_decline_and_return_the_two_kernel_bits(precision):
    """Only the fp32 precision takes the fused kernel: f32x3 asks for other GEMM arithmetic than it has, and the bf16 modes keep the arithmetic they
    were bounded with.  The call site declines, the two kernels run, bit for bit."""
    n, h, w = SHAPES[1]
    a, b = run(n, h, w, 1, precision=precision, deterministic=1), run(n, h, w, 0, precision=precision, deterministic=1)      # (deterministic: the loss's own reduction order is fixed)
    assert not ran(a["train_kernels"]) and not ran(a["infer_kernels"]), a["train_kernels"]
    assert a["loss"] == b["loss"]
    np.testing.assert_array_equal(a["pool1"], b["pool1"])
    np.testing.assert_array_equal(a["bytes"], b["bytes"])
    np.testing.assert_array_equal(a["pred"], b["pred"])
