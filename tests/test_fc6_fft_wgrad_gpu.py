"""fc6's weight gradient in the 14x14 real-DFT domain (option fc6_fft_wgrad, csrc/fft_fc6.hip: fft_fc6_dfilter_kernel) against the
F(4x4,4x4) / direct weight gradient and float64 over the same operands; bit reproducibility under deterministic mode; the forward
activation and the data gradient unchanged by it; the path the bench shape takes."""
import numpy as np
import pytest
import torch

from oracle import fcn8s_oracle as orc

pytestmark = pytest.mark.gpu
WIDTHS = (16, 32, 64, 128, 128, 256, 128)        # fc6: 128 -> 256 channels (Cin % 16 == 0, Cout % 128 == 0)


def rng_batch(n, h, w, seed=0):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8), rng.integers(0, 20, (n, h, w), dtype=np.uint8)


def run(P, img, lab, opts):
    from fcn8s_tensorflow_amd.engine import Engine
    n, h, w = img.shape[:3]
    e = Engine(20, widths=WIDTHS, device_id=0, seed=0, options=dict(opts, keep_output_gradients=1))
    e.set_params(P)
    e.profile(1); e.profile_reset()
    e.forward_backward(img, lab, keep_prob=1.0)
    groups = set(e.profile_results())
    out = {"groups": groups,
           "fc6": e.activation("fc6", (n, h // 32, w // 32, WIDTHS[5])).copy(),
           "pool5": e.activation("pool5", (n, h // 32, w // 32, WIDTHS[4])).copy(),
           "dy": e.activation("dy:fc6", (n, h // 32, w // 32, WIDTHS[5])).copy(),
           "grads": {k: v.copy() for k, v in e.get_grads().items()}}
    e.close()
    return out


def wgrad64(x, dy):
    """float64 7x7 SAME weight and bias gradient of the same operands: [7][7][Cin][Cout], [Cout]."""
    nchw = lambda a: torch.from_numpy(a.astype(np.float64)).permute(0, 3, 1, 2).contiguous()
    dw = torch.nn.grad.conv2d_weight(nchw(x), (dy.shape[3], x.shape[3], 7, 7), nchw(dy), padding=3)
    return dw.permute(2, 3, 1, 0).numpy(), dy.astype(np.float64).sum(axis=(0, 1, 2))


def err(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("h,w", [(256, 512), (320, 416)])      # pool5 8x16 (whole tiles; F(4x4,4x4) otherwise) and 10x13 (partial edge tiles; direct otherwise)
def test_dft_weight_gradient_matches_the_other_paths_and_float64(h, w):
    P = orc.init_params(20, WIDTHS, seed=8, decoder_std_scale=30.0, bias_std=0.05)
    img, lab = rng_batch(2, h, w, seed=4)
    new = run(P, img, lab, {"fc6_fft_wgrad": 2})
    old = run(P, img, lab, {"fc6_fft_wgrad": 0})
    assert "fc6_fft_gemm_wgrad" in new["groups"] and "fc6_fft_gemm_wgrad" not in old["groups"]
    assert not any(g.startswith("wino_gemm_fc6_wgrad") for g in new["groups"])
    np.testing.assert_array_equal(new["pool5"], old["pool5"])
    assert err(new["dy"], old["dy"]) < 1e-5           # (the head's weight gradients add with atomics outside deterministic mode: fc6's dY differs in the last bits)
    for r in (new, old):                               # each against float64 over its own operands
        dw, db = wgrad64(r["pool5"], r["dy"])
        assert err(r["grads"]["fc6/weights"], dw) <= 1e-5
        assert err(r["grads"]["fc6/biases"], db) <= 1e-5
    assert err(new["grads"]["fc6/weights"], old["grads"]["fc6/weights"]) <= 1e-5
    assert err(new["grads"]["fc6/biases"], old["grads"]["fc6/biases"]) <= 1e-5


def test_forward_and_data_gradient_are_bit_identical_and_dw_reproducible():
    P = orc.init_params(20, WIDTHS, seed=9, decoder_std_scale=30.0, bias_std=0.05)
    img, lab = rng_batch(2, 256, 512, seed=5)
    a = run(P, img, lab, {"fc6_fft_wgrad": 2, "deterministic": 1})
    b = run(P, img, lab, {"fc6_fft_wgrad": 2, "deterministic": 1})
    old = run(P, img, lab, {"fc6_fft_wgrad": 0, "deterministic": 1})
    assert "fc6_fft_gemm_wgrad" in a["groups"]
    for k in a["grads"]:
        np.testing.assert_array_equal(a["grads"][k], b["grads"][k], err_msg=k)
    np.testing.assert_array_equal(a["fc6"], old["fc6"])
    np.testing.assert_array_equal(a["dy"], old["dy"])
    # fc6's data gradient feeds every gradient below it (conv5_3 down to conv1_1); the head's do not depend on fc6's backward pass
    for k in a["grads"]:
        if not k.startswith("fc6/"):
            np.testing.assert_array_equal(a["grads"][k], old["grads"][k], err_msg=k)


def test_small_tile_counts_keep_winograd_by_default():
    P = orc.init_params(20, WIDTHS, seed=10, decoder_std_scale=30.0, bias_std=0.05)
    img, lab = rng_batch(2, 256, 512, seed=6)                          # 4 tiles: below the rule's threshold
    r = run(P, img, lab, {})
    assert "fc6_fft_gemm_fwd" in r["groups"] and "fc6_fft_gemm_wgrad" not in r["groups"]
    assert any(g.startswith("wino_gemm_fc6_wgrad") for g in r["groups"])


def test_bench_shape_takes_the_dft_weight_gradient():
    from fcn8s_tensorflow_amd.engine import Engine
    img, lab = rng_batch(16, 512, 1024, seed=7)
    e = Engine(20, device_id=0, seed=0)
    e.init_params(0)
    e.profile(1); e.profile_reset()
    e.forward_backward(img, lab, keep_prob=0.5)
    groups = set(e.profile_results())
    g = e.get_grads()["fc6/weights"]
    e.close()
    assert {"fc6_fft_gemm_fwd", "fc6_fft_gemm_wgrad", "fc6_fft_gemm_dgrad"} <= groups, groups
    assert not any(k.startswith("wino_gemm_fc6") for k in groups), groups
    assert np.isfinite(g).all() and np.abs(g).max() > 0
