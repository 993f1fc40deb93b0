"""Float64 model of fc6's weight gradient in the 14x14 real-DFT domain (csrc/fft_fc6.hip: fft_fc6_dfilter_kernel): the transpose of the
filter transform, written the way the kernel computes it (Gauss stage, column DFT adjoint, row DFT adjoint, flip), checked as an exact adjoint
of the forward filter transform and, composed with the plane GEMMs dUf[p] = Xf[p]^T dYf[p], against a direct 7x7 weight gradient.  Numpy only."""
import numpy as np

from tests.test_fc6_fft_host import CPLX, K, P, REAL, conv_direct, filter_planes, input_planes, output_adjoint, tiles


def plane_of(u, v):
    """(first plane, real?) of stored frequency (u, v), the kernel's cplx() / realp() order."""
    if (u, v) in REAL:
        return 3 * len(CPLX) + REAL.index((u, v)), True
    return 3 * CPLX.index((u, v)), False


def dfilter(duf):
    """[P][Cin][Cout] -> dw [7][7][Cin][Cout], column by column as fft_fc6_dfilter_kernel runs."""
    c = lambda k: np.cos(2 * np.pi * k / 14)
    s = lambda k: np.sin(2 * np.pi * k / 14)
    dg = np.zeros((K, K) + duf.shape[1:])
    for v in range(8):
        us = range(14 if 1 <= v <= 6 else 8)
        R, I = {}, {}
        for u in us:
            p, real = plane_of(u, v)
            if real:
                R[u], I[u] = duf[p], 0.0
            else:
                R[u], I[u] = duf[p] - duf[p + 1] + duf[p + 2], duf[p + 1] + duf[p + 2]
        for a in range(K):
            dr = sum(R[u] * c(u * a) - I[u] * s(u * a) for u in us)
            di = sum(R[u] * s(u * a) + I[u] * c(u * a) for u in us)
            for b in range(K):
                dg[6 - a, 6 - b] += dr * c(v * b) - di * s(v * b)
    return dg


def wgrad_direct(x, dz):
    H, W, Ci = x.shape
    xp = np.zeros((H + 6, W + 6, Ci)); xp[3:3 + H, 3:3 + W] = x
    dw = np.zeros((K, K, Ci, dz.shape[2]))
    for ky in range(K):
        for kx in range(K):
            dw[ky, kx] = np.tensordot(xp[ky:ky + H, kx:kx + W], dz, axes=([0, 1], [0, 1]))
    return dw


def test_dfilter_is_the_exact_adjoint_of_the_filter_transform():
    rng = np.random.default_rng(3)
    w = rng.standard_normal((K, K, 3, 5)); g = rng.standard_normal((P, 3, 5))
    lhs = np.vdot(filter_planes(w), g); rhs = np.vdot(w, dfilter(g))
    assert abs(lhs - rhs) < 1e-12 * max(1.0, abs(lhs))


def test_dft_weight_gradient_matches_direct_correlation():
    rng = np.random.default_rng(4)
    for H, W in ((16, 32), (10, 13), (5, 9)):           # exact tiling, partial edge tiles, a map smaller than one tile
        th, tw = tiles(H, W)
        x = rng.standard_normal((H, W, 4)); dz = rng.standard_normal((H, W, 6))
        duf = np.einsum("ptc,pto->pco", input_planes(x), output_adjoint(dz, th, tw))
        ref = wgrad_direct(x, dz)
        assert np.abs(dfilter(duf) - ref).max() < 1e-12 * np.abs(ref).max(), (H, W)
    # the same weight gradient is the gradient of <conv(x, w), dz> with respect to w
    assert abs(np.vdot(conv_direct(x, ref), dz) - np.vdot(ref, ref)) < 1e-9 * np.vdot(ref, ref)


def test_float32_round_off():
    rng = np.random.default_rng(5)
    x = np.maximum(rng.standard_normal((16, 32, 32)), 0).astype(np.float32)
    dz = (rng.standard_normal((16, 32, 8)) * 1e-3).astype(np.float32)
    duf = np.einsum("ptc,pto->pco", input_planes(x), output_adjoint(dz, 2, 4).astype(np.float32)).astype(np.float32)
    ref = wgrad_direct(x.astype(np.float64), dz.astype(np.float64))
    assert np.abs(dfilter(duf) - ref).max() < 1e-5 * np.abs(ref).max()
