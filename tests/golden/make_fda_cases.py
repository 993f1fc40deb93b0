"""Writes tests/golden/fda_cases.npz: inputs and float64 results of Fourier domain adaptation (`fcn8s_op_fda_transfer`; the definition is in
include/fcn8s_hip.h) by the PUBLISHED route (Yang & Soatto, CVPR 2020, FDA_source_to_target_np): np.fft.fft2 of source and target, amplitude and
phase, fftshift of the amplitudes, the centred window [c - b : c + b + 1] (c = H // 2, W // 2) of the source's amplitude overwritten with the
target's, ifftshift, ifft2 of amplitude * exp(i phase), real part.  Written from that description; it shares nothing with
fcn8s_tensorflow_amd/fda.py or the kernel, which use the matrix formulation.

python tests/golden/make_fda_cases.py  (a second)

Cases: H x W in {2x2, 3x5, 7x16, 8x63, 33x129}, each with one source and one target, at b = 0, b = 1 where it fits and the largest b that fits; one
batch N = 3, M = 2 of 16 x 24 at b = 2 with pair = [1, 0, 1] (rotated, one target repeated).  Sources and targets alternate between uint8 noise and
a smooth image plus noise.  The script asserts that every source amplitude inside every window is at least 1e-3 H W: the references are
well-conditioned (a phase of a vanishing coefficient is noise in this route too)."""
import os

import numpy as np

SHAPES = [(2, 2), (3, 5), (7, 16), (8, 63), (33, 129)]
FLOOR = 1e-3


def noise(rng, H, W):
    return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)


def smooth(rng, H, W):
    y, x = np.mgrid[0:H, 0:W]
    out = np.empty((H, W, 3))
    for c in range(3):
        a, p, q = rng.uniform(40, 90), rng.uniform(0.3, 1.7), rng.uniform(0.3, 1.7)
        out[:, :, c] = 128 + a * np.sin(p * np.pi * y / max(H - 1, 1) + c) * np.cos(q * np.pi * x / max(W - 1, 1) - c) + rng.normal(0, 12, (H, W))
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def published(src, trg, b):
    """[H, W, 3] uint8 x 2 -> float64 [H, W, 3], and the smallest source amplitude inside the window over H W."""
    H, W = src.shape[:2]
    fs = np.fft.fft2(src.astype(np.float64), axes=(0, 1))
    ft = np.fft.fft2(trg.astype(np.float64), axes=(0, 1))
    amp_s, pha_s, amp_t = np.abs(fs), np.angle(fs), np.abs(ft)
    a_s, a_t = np.fft.fftshift(amp_s, axes=(0, 1)), np.fft.fftshift(amp_t, axes=(0, 1))
    ch, cw = H // 2, W // 2
    window = (slice(ch - b, ch + b + 1), slice(cw - b, cw + b + 1))
    floor = a_s[window].min() / (H * W)
    a_s[window] = a_t[window]
    a_s = np.fft.ifftshift(a_s, axes=(0, 1))
    return np.real(np.fft.ifft2(a_s * np.exp(1j * pha_s), axes=(0, 1))), floor


def main():
    rng = np.random.default_rng(20201)
    cases = []
    for k, (H, W) in enumerate(SHAPES):
        src = (noise if k % 2 == 0 else smooth)(rng, H, W)[None]
        trg = (smooth if k % 2 == 0 else noise)(rng, H, W)[None]
        fit = (min(H, W) - 1) // 2
        for b in sorted({0, min(1, fit), fit}):
            cases.append(("%dx%d b=%d" % (H, W, b), src, trg, b, np.array([0], np.int32)))
    H, W = 16, 24
    src = np.stack([noise(rng, H, W), smooth(rng, H, W), noise(rng, H, W)])
    trg = np.stack([smooth(rng, H, W), noise(rng, H, W)])
    cases.append(("batch 3+2 16x24 b=2", src, trg, 2, np.array([1, 0, 1], np.int32)))

    out = {"names": np.array([c[0] for c in cases])}
    worst = np.inf
    for i, (name, src, trg, b, pair) in enumerate(cases):
        ys = []
        for n in range(src.shape[0]):
            y, floor = published(src[n], trg[pair[n]], b)
            assert floor >= FLOOR, (name, n, floor)
            worst = min(worst, floor)
            ys.append(y)
        out["c%d_images" % i], out["c%d_targets" % i], out["c%d_b" % i], out["c%d_pair" % i] = src, trg, np.int32(b), pair
        out["c%d_y" % i] = np.stack(ys)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fda_cases.npz")
    np.savez_compressed(path, **out)
    print("%d cases, smallest source amplitude in a window %.2e H W, %d bytes" % (len(cases), worst, os.path.getsize(path)))


if __name__ == "__main__":
    main()
