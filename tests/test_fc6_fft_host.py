"""Float64 model of fc6's 14x14 real-DFT plane set (csrc/fft_fc6.hip): 292 real GEMM planes with Gauss's three-product complex multiply.
Checks the forward algorithm against a direct 7x7 SAME correlation, the data-gradient transforms as exact adjoints of the forward ones,
and the float32 round-off of the same arithmetic.  Numpy only."""
import numpy as np

TILE, OUT, K = 14, 8, 7


def freqs():
    """Stored frequencies in plane order: (u, v, real?) -> plane index of the first plane."""
    cplx, real = [], []
    for v in range(8):
        for u in range(14 if 1 <= v <= 6 else 8):
            (real if (v in (0, 7) and u in (0, 7)) else cplx).append((u, v))
    real.sort(key=lambda uv: (uv[1] == 7, uv[0] == 7))
    return cplx, real


CPLX, REAL = freqs()
P = 3 * len(CPLX) + len(REAL)


def dft_rows(x):
    """Forward 2-D DFT of the leading two axes at the stored frequencies: complex [len(CPLX)], real [len(REAL)] (+ trailing axes)."""
    n = np.arange(TILE)
    out = {}
    for u, v in CPLX + REAL:
        e = np.exp(-2j * np.pi * (u * n[:, None] + v * n[None, :]) / TILE)
        out[(u, v)] = np.tensordot(e, x, axes=([0, 1], [0, 1]))
    return out


def filter_planes(w):
    wf = np.zeros((TILE, TILE) + w.shape[2:], w.dtype)
    wf[:K, :K] = w[::-1, ::-1]
    F = dft_rows(wf)
    pl = []
    for uv in CPLX:
        c, d = F[uv].real, F[uv].imag
        pl += [c, d - c, c + d]
    pl += [F[uv].real for uv in REAL]
    return np.stack(pl).astype(w.dtype)                     # [P][Cin][Cout]


def tiles(H, W):
    return -(-H // OUT), -(-W // OUT)


def input_planes(x):
    """x [H][W][C] -> [P][T][C], patches of origin 8t - 3."""
    H, W, C = x.shape
    th, tw = tiles(H, W)
    xp = np.zeros((th * OUT + 6, tw * OUT + 6, C), x.dtype)
    xp[3:3 + H, 3:3 + W] = x
    out = np.zeros((P, th * tw, C), x.dtype)
    for ty in range(th):
        for tx in range(tw):
            F = dft_rows(xp[8 * ty:8 * ty + TILE, 8 * tx:8 * tx + TILE])
            pl = []
            for uv in CPLX:
                a, b = F[uv].real, F[uv].imag
                pl += [a + b, a, b]
            pl += [F[uv].real for uv in REAL]
            out[:, ty * tw + tx] = np.stack(pl)
    return out


def coef(u, v, n, m):
    return 2 * np.pi * (u * n + v * m) / TILE


def output_from_planes(yf, H, W):
    """[P][T][Co] -> y [H][W][Co]: real = k1 - k3, imag = k1 + k2, inverse real DFT, last 8x8 of each tile."""
    th, tw = tiles(H, W)
    Co = yf.shape[2]
    y = np.zeros((th * OUT, tw * OUT, Co), yf.dtype)
    n = np.arange(6, 14)
    for i, (u, v) in enumerate(CPLX + REAL):
        if i < len(CPLX):
            k1, k2, k3 = yf[3 * i], yf[3 * i + 1], yf[3 * i + 2]
            R, I, beta = k1 - k3, k1 + k2, 2.0
        else:
            R, I, beta = yf[3 * len(CPLX) + i - len(CPLX)], 0.0 * yf[0], 1.0
        th_ = coef(u, v, n[:, None], n[None, :])
        cs, sn = (beta / 196 * np.cos(th_)).astype(yf.dtype), (beta / 196 * np.sin(th_)).astype(yf.dtype)
        for t in range(th * tw):
            ty, tx = divmod(t, tw)
            y[8 * ty:8 * ty + 8, 8 * tx:8 * tx + 8] += cs[:, :, None] * R[t] - sn[:, :, None] * I[t]
    return y[:H, :W]


def output_adjoint(dz, th, tw):
    """Transpose of output_from_planes: dz [H][W][Co] -> [P][T][Co]."""
    H, W, Co = dz.shape
    d = np.zeros((th * OUT, tw * OUT, Co)); d[:H, :W] = dz
    out = np.zeros((P, th * tw, Co))
    n = np.arange(6, 14)
    for i, (u, v) in enumerate(CPLX + REAL):
        beta = 2.0 if i < len(CPLX) else 1.0
        th_ = coef(u, v, n[:, None], n[None, :])
        for t in range(th * tw):
            ty, tx = divmod(t, tw)
            blk = d[8 * ty:8 * ty + 8, 8 * tx:8 * tx + 8]
            dR = beta / 196 * np.tensordot(np.cos(th_), blk, axes=([0, 1], [0, 1]))
            dI = -beta / 196 * np.tensordot(np.sin(th_), blk, axes=([0, 1], [0, 1]))
            if i < len(CPLX):
                out[3 * i, t], out[3 * i + 1, t], out[3 * i + 2, t] = dR + dI, dI, -dR
            else:
                out[3 * len(CPLX) + i - len(CPLX), t] = dR
    return out


def input_adjoint(dxf, H, W):
    """Transpose of input_planes: [P][T][C] -> dx [H][W][C] (patch gradients overlap-added at stride 8)."""
    th, tw = tiles(H, W)
    C = dxf.shape[2]
    dxp = np.zeros((th * OUT + 6, tw * OUT + 6, C))
    n = np.arange(TILE)
    for i, (u, v) in enumerate(CPLX + REAL):
        if i < len(CPLX):
            A, B = dxf[3 * i] + dxf[3 * i + 1], dxf[3 * i] + dxf[3 * i + 2]
        else:
            A, B = dxf[3 * len(CPLX) + i - len(CPLX)], np.zeros_like(dxf[0])
        th_ = coef(u, v, n[:, None], n[None, :])
        for t in range(th * tw):
            ty, tx = divmod(t, tw)
            dxp[8 * ty:8 * ty + TILE, 8 * tx:8 * tx + TILE] += np.cos(th_)[:, :, None] * A[t] - np.sin(th_)[:, :, None] * B[t]
    return dxp[3:3 + H, 3:3 + W]


def conv_fft(x, w):
    H, W, _ = x.shape
    xf, uf = input_planes(x), filter_planes(w)
    return output_from_planes(np.einsum("ptc,pco->pto", xf, uf), H, W)


def conv_direct(x, w):
    H, W, _ = x.shape
    xp = np.zeros((H + 6, W + 6, x.shape[2])); xp[3:3 + H, 3:3 + W] = x
    y = np.zeros((H, W, w.shape[3]))
    for ky in range(K):
        for kx in range(K):
            y += xp[ky:ky + H, kx:kx + W] @ w[ky, kx]
    return y


def test_plane_count():
    assert len(CPLX) == 96 and len(REAL) == 4 and P == 292


def test_forward_matches_direct_correlation():
    rng = np.random.default_rng(0)
    for H, W in ((16, 32), (20, 13), (5, 9)):           # exact tiling, partial edge tiles, a map smaller than one tile
        x = rng.standard_normal((H, W, 6)); w = rng.standard_normal((K, K, 6, 5))
        ref = conv_direct(x, w)
        assert np.abs(conv_fft(x, w) - ref).max() < 1e-12 * np.abs(ref).max(), (H, W)


def test_data_gradient_transforms_are_exact_adjoints():
    rng = np.random.default_rng(1)
    H, W, C = 20, 13, 3
    th, tw = tiles(H, W)
    x = rng.standard_normal((H, W, C)); g = rng.standard_normal((P, th * tw, C))
    lhs = np.vdot(input_planes(x), g); rhs = np.vdot(x, input_adjoint(g, H, W))
    assert abs(lhs - rhs) < 1e-12 * max(1.0, abs(lhs))
    yf = rng.standard_normal((P, th * tw, C)); dz = rng.standard_normal((H, W, C))
    lhs = np.vdot(output_from_planes(yf, H, W), dz); rhs = np.vdot(yf, output_adjoint(dz, th, tw))
    assert abs(lhs - rhs) < 1e-12 * max(1.0, abs(lhs))
    # the whole data gradient: input^T((output^T dz) Uf^T) equals the direct correlation with the flipped, transposed kernel
    w = rng.standard_normal((K, K, C, 4)); dz = rng.standard_normal((H, W, 4))
    dx = input_adjoint(np.einsum("pto,pco->ptc", output_adjoint(dz, th, tw), filter_planes(w)), H, W)
    ref = conv_direct(dz, w[::-1, ::-1].transpose(0, 1, 3, 2))
    assert np.abs(dx - ref).max() < 1e-12 * np.abs(ref).max()


def test_float32_round_off():
    rng = np.random.default_rng(2)
    x = np.maximum(rng.standard_normal((16, 32, 64)), 0).astype(np.float32)
    w = (rng.standard_normal((K, K, 64, 8)) / np.sqrt(49 * 64)).astype(np.float32)
    ref = conv_direct(x.astype(np.float64), w.astype(np.float64))
    y = conv_fft(x, w)
    assert y.dtype == np.float32
    assert np.abs(y - ref).max() < 1e-6 * (ref.max() - ref.min())
