"""Fourier domain adaptation of the labelled batch (FDA: Yang & Soatto, CVPR 2020): the low-frequency amplitudes of every source image are replaced
by those of a target image, the phases stay.  The NumPy restatement of `fcn8s_op_fda_transfer`, the half-width rule, the validation of
`FCN8s.train(fda_beta=...)` and the device wrapper.

The definition is in include/fcn8s_hip.h at `fcn8s_op_fda_transfer`.  Inputs are N source and M target images, uint8 [., H, W, 3] of one H x W;
pair[n] in [0, M) names the target of source n (None: n mod M); b is the half-width, 0 <= b <= 96 and B = 2 b + 1 <= min(H, W).  Per source n,
target t = pair[n] and channel, for u, v in {-b .. b}:

    F_s(u,v) = sum_h sum_w x_s[h,w] exp(-2 pi i (u h / H + v w / W)),  F_t likewise from x_t
    A_s = |F_s|, A_t = |F_t|, phi = F_s / A_s (phi = 1 where A_s = 0: numpy's angle(0) = 0)
    Delta(u,v) = phi (A_t - A_s)
    y[h,w] = x_s[h,w] + 1 / (H W) Re sum_u sum_v Delta(u,v) exp(+2 pi i (u h / H + v w / W))
    out_f32 = y, out_u8 = clamp(rint(y), 0, 255)

Only a (2 b + 1)^2 window of coefficients changes, so no FFT is needed: a partial DFT is two skinny matrix products per image and channel, the
synthesis two more.  Every twiddle exp(+-2 pi i k / n) comes from the integer-reduced phase (f index) mod n.  Spectra of equal bytes are equal
bits, so a source whose target holds the same bytes comes back exactly.  Where A_s lies below the rounding of its own sum (a constant source at
b >= 1) the phase is noise, as in the published float64 code: such outputs are finite, no more."""
from __future__ import annotations

import math

import numpy as np

MAX_BATCH = 256
MAX_HALF_WIDTH = 96
MAX_BETA = 0.09


def half_width(H, W, beta):
    """b = floor(min(H, W) beta): the published rule."""
    return int(math.floor(min(int(H), int(W)) * float(beta)))


def _check_b(H, W, b):
    if isinstance(b, bool) or not isinstance(b, (int, np.integer)):
        raise ValueError("the half-width b is an integer, got {!r}".format(b))
    b = int(b)
    if not 0 <= b <= MAX_HALF_WIDTH or 2 * b + 1 > min(H, W):
        raise ValueError("the half-width b must satisfy 0 <= b <= {} and 2 b + 1 <= min(H, W); got b = {} for {}x{}".format(MAX_HALF_WIDTH, b, H, W))
    return b


check_half_width = _check_b          # (H, W, b) -> b, or ValueError: what `FCN8s.train(fda_beta=...)` asks as soon as a batch shows its size


def _check_arrays(images, targets):
    images, targets = np.asarray(images), np.asarray(targets)
    for a, what in ((images, "images"), (targets, "targets")):
        if a.dtype != np.uint8 or a.ndim != 4 or a.shape[-1] != 3 or 0 in a.shape:
            raise ValueError("{} are uint8 [N, H, W, 3]".format(what))
    if images.shape[1:] != targets.shape[1:]:
        raise ValueError("images {} and targets {} must have one height and width".format(images.shape, targets.shape))
    N, H, W = images.shape[:3]
    if N > MAX_BATCH or targets.shape[0] > MAX_BATCH or H * W >= 1 << 31:
        raise ValueError("a batch has at most {} images and an image fewer than 2^31 pixels".format(MAX_BATCH))
    return images, targets


def _check_pair(pair, N, M):
    if pair is None:
        return np.arange(N, dtype=np.int64) % M
    p = np.asarray(pair)
    if p.dtype.kind not in 'iu' or p.shape != (N,):
        raise ValueError("`pair` holds one integer per source image ({}), got {!r}".format(N, pair))
    p = p.astype(np.int64)
    if (p < 0).any() or (p >= M).any():
        raise ValueError("`pair` names targets in [0, {}), got {}".format(M, p.tolist()))
    return p


def _twiddles(n, b, dtype):
    """E[f + b, k] = exp(-2 pi i ((f k) mod n) / n) for f in -b .. b, k in 0 .. n - 1: the phase is reduced in integers, the sine and cosine are
    taken in float64 and rounded to `dtype`."""
    f = np.arange(-b, b + 1, dtype=np.int64)[:, None]
    k = np.arange(n, dtype=np.int64)[None, :]
    ph = 2.0 * np.pi * ((f * k) % n).astype(np.float64) / n
    ctype = np.complex128 if dtype == np.float64 else np.complex64
    return (np.cos(ph) - 1j * np.sin(ph)).astype(ctype)


def transfer_numpy(images, targets, b, pair=None, dtype=np.float64):
    """y [N, H, W, 3] in `dtype` (np.float64 or np.float32): the matrix formulation above, every product and sum in `dtype`."""
    dtype = np.dtype(dtype).type
    if dtype not in (np.float64, np.float32):
        raise ValueError("`dtype` is np.float64 or np.float32")
    images, targets = _check_arrays(images, targets)
    N, H, W = images.shape[:3]
    M = targets.shape[0]
    b = _check_b(H, W, b)
    pair = _check_pair(pair, N, M)
    Eh, Ew = _twiddles(H, b, dtype), _twiddles(W, b, dtype)                   # [B, H], [B, W]
    Ewt, Ehc, Ewc = np.ascontiguousarray(Ew.T), np.ascontiguousarray(Eh.conj().T), np.ascontiguousarray(Ew.conj())

    def spectrum(x):                                                          # [H, W, 3] uint8 -> [3, B, B]
        return np.stack([Eh @ (x[:, :, c].astype(dtype) @ Ewt) for c in range(3)])
    Ft = {int(t): spectrum(targets[t]) for t in np.unique(pair)}              # a target is analysed once
    out = np.empty(images.shape, dtype)
    scale = dtype(1.0) / dtype(H * W)
    one = np.ones((), Eh.dtype)
    for n in range(N):
        Fs = spectrum(images[n])
        As, At = np.abs(Fs), np.abs(Ft[int(pair[n])])
        phi = np.where(As > 0, Fs / np.where(As > 0, As, 1), one)
        delta = (phi * (At - As)).astype(Eh.dtype)
        for c in range(3):
            out[n, :, :, c] = images[n, :, :, c].astype(dtype) + (Ehc @ delta[c] @ Ewc).real.astype(dtype) * scale
    return out


def to_uint8(y):
    """out_u8 of the op from its float output: clamp(rint(y), 0, 255)."""
    return np.clip(np.rint(y), 0, 255).astype(np.uint8)


def validate(beta, has_generator=True):
    """`FCN8s.train`'s `fda_beta` -> None (off) or the float, which lies in (0, 0.09]."""
    if beta is None:
        return None
    if isinstance(beta, bool) or not isinstance(beta, (int, float, np.integer, np.floating)) or not 0.0 < float(beta) <= MAX_BETA:
        raise ValueError("`fda_beta` must be None or a number in (0, {}], got {!r}".format(MAX_BETA, beta))
    if not has_generator:
        raise ValueError("`fda_beta` needs an `unlabeled_generator`: its images are the style source.")
    return float(beta)


# ---- the call on device tensors ------------------------------------------------------------------------------------------------------------
def work_bytes(N, M, H, W, b):
    from . import _lib as L
    return int(L.lib.fcn8s_op_fda_work_bytes(int(N), int(M), int(H), int(W), int(b)))


def flag_of(work):
    """The flag word of the most recent call on `work` (1: a pair[n] was out of range and counted as n mod M); synchronises."""
    off = (-work.data_ptr()) % 16
    return int(work[off:off + 4].cpu().numpy().view(np.uint32)[0])


def transfer_device(images, targets, b, pair=None, out_float=False, work=None):
    """One `fcn8s_op_fda_transfer` call on uint8 device tensors [N,H,W,3] and [M,H,W,3], on the current stream: (out, work), out uint8 or -- with
    `out_float` -- float32 [N,H,W,3].  `pair`: None = n mod M, a sequence of N ints in [0, M), or an int32 device tensor of N (not checked: an
    entry out of range counts as n mod M and sets the flag).  `work`: a uint8 device tensor to reuse (a larger one is made when it is too
    small) -- returned."""
    import ctypes as C
    import torch
    from . import _lib as L
    for t, what in ((images, "images"), (targets, "targets")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.uint8 or t.dim() != 4 or not t.is_contiguous() or t.shape[-1] != 3 \
                or t.numel() == 0:
            raise ValueError("%s have to be a contiguous uint8 tensor [N,H,W,3] on the GPU" % what)
    if tuple(images.shape[1:]) != tuple(targets.shape[1:]) or images.device != targets.device:
        raise ValueError("images {} and targets {} must have one height and width and live on one device".format(tuple(images.shape), tuple(targets.shape)))
    N, H, W = (int(x) for x in images.shape[:3])
    M = int(targets.shape[0])
    if N > MAX_BATCH or M > MAX_BATCH or H * W >= 1 << 31:
        raise ValueError("a batch has at most {} images and an image fewer than 2^31 pixels".format(MAX_BATCH))
    b = _check_b(H, W, b)
    dev = images.device
    if pair is None:
        pair_t = None
    elif isinstance(pair, torch.Tensor):
        if pair.dtype != torch.int32 or pair.numel() != N or pair.device != dev or not pair.is_contiguous():
            raise ValueError("a pair tensor is N contiguous int32 on the images' device")
        pair_t = pair
    else:
        pair_t = torch.from_numpy(_check_pair(pair, N, M).astype(np.int32)).to(dev)
    nbytes = work_bytes(N, M, H, W, b)
    if work is None or work.numel() < nbytes or work.device != dev:
        work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = torch.empty(images.shape, dtype=torch.float32 if out_float else torch.uint8, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    optr = C.c_void_p(out.data_ptr())
    L.check(L.lib.fcn8s_op_fda_transfer(stream, C.c_void_p(images.data_ptr()), N, C.c_void_p(targets.data_ptr()), M, H, W, b,
                                        C.c_void_p(pair_t.data_ptr()) if pair_t is not None else None, C.c_void_p(work.data_ptr()),
                                        None if out_float else optr, optr if out_float else None))
    return out, work
