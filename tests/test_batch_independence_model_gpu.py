"""An image's logits do not depend on its batch, through the whole forward pass of a model (csrc/split_route.h states the invariant;
tests/test_batch_independence_ops_gpu.py holds it route by route)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import fcn8s_oracle as orc  # noqa: E402  (parameters only)

CASES = {
    # precision: (widths, H, W).  Each is sized so that one forward launch, by the inline formula its rule replaced, changed its K split between a
    # batch of two and a batch of five:
    #   bf16_train  conv4_2 / conv4_3 (256 -> 256 on a 24x32 map, 884 padded positions an image, 24 K-tiles) on conv_bf16_rows_kernel<64>:
    #               7 row tiles x 4 column tiles = 28 blocks -> 4 slabs at N = 2; 18 x 4 = 72 blocks -> one pass at N = 5  (bf16_rows_slabs)
    #   fp32        the score head of fc7 (4096 -> 20 on a 16x26 map, 416 rows an image) on head_fwd_kernel: 26 blocks of 32 rows -> 8 slabs at
    #               N = 2; 65 blocks -> one pass at N = 5  (head_fwd_splits)
    "bf16_train": ((64, 64, 128, 256, 256, 256, 256), 192, 256),
    "fp32": ((8, 16, 32, 64, 64, 128, 4096), 512, 832),
}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("precision", sorted(CASES))
def test_logits_of_two_images_are_their_bits_in_a_batch_of_five(precision):
    """forward_backward (keep_prob = 1) on five images, then on images 1..2 of them: the two images' logits are bit-identical.  The launch whose
    split used to change between the two batch sizes is named in CASES; with it the logits of both images differed in their last bits.
    And the looser property every mode had: the loss of the five is the mean over its images (here: over the sub-batches [0, 1] and [2, 3, 4],
    weighted by their sizes: batches of two or more, so that no single-image exception enters) to 1e-6 relative."""
    from fcn8s_tensorflow_amd.engine import Engine
    widths, h, w = CASES[precision]
    P = orc.init_params(20, widths, seed=5, decoder_std_scale=6.0, bias_std=0.05)
    rng = np.random.default_rng(77)
    img = rng.integers(0, 256, (5, h, w, 3), dtype=np.uint8)
    lab = rng.integers(0, 20, (5, h, w), dtype=np.uint8)
    e = Engine(20, widths=widths, precision=precision)
    try:
        e.set_params(P)
        loss5 = e.forward_backward(img, lab, keep_prob=1.0)
        five = e.activation("logits", (5, h, w, 20))[1:3].copy()
        e.forward_backward(img[1:3], lab[1:3], keep_prob=1.0)
        two = e.activation("logits", (2, h, w, 20))
        differ = int((bits(two) != bits(five)).sum())
        print("%s: %d of %d logits differ between the batch of five and the batch of two (largest |logit| %.3g)" % (precision, differ, two.size, float(np.abs(five).max())))
        assert np.isfinite(five).all() and five.std() > 0
        assert differ == 0
        loss_a = e.forward_backward(img[0:2], lab[0:2], keep_prob=1.0)
        loss_b = e.forward_backward(img[2:5], lab[2:5], keep_prob=1.0)
        mean = (2.0 * loss_a + 3.0 * loss_b) / 5.0
        print("%s: loss of five %.9g, mean over its images %.9g" % (precision, loss5, mean))
        assert abs(loss5 - mean) <= 1e-6 * abs(mean)
    finally:
        e.close()
