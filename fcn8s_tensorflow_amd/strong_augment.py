"""Strong photometric augmentation of the unlabelled batch (DACS, Tranheden et al., WACV 2021; ClassMix, Olsson et al., WACV 2021: the student
sees the mixed image after colour jitter and Gaussian blur, the labeler the clean one): the NumPy restatement of `fcn8s_op_strong_augment`, the
blur's tap table, the validation of `FCN8s.train(unlabeled_augment=...)` and the device wrapper.

The definition is in include/fcn8s_hip.h at `fcn8s_op_strong_augment`.  Per image n, seven Philox words u_0..u_6 of (seed, draw, n) decide
everything: a gated colour step (contrast about the input's mean grey with a 16.16 factor; saturation and brightness with 16.16 factors and a
hue shift in OpenCV's 8-bit HSV, through `cv2_compat.rgb2hsv` / `hsv2rgb`) and a gated separable blur with 11-bit taps and reflect-101 borders.
Integers plus the float32 steps of HSV -> RGB: `augment_numpy` and the kernel agree with `==`.

Settings: `jitter` = None or five ints {gate, Cs, Ss, Bs, Hs}; `blur` = None or (gate, taps) with taps uint16 [Q, R + 1] as `taps_table`
makes them.  Gates lie in 0..65536 (65536 = always); Cs, Ss, Bs in 0..65536 are the half-widths of the 16.16 factors around 1; Hs in 0..90 is
the half-width of the hue shift in OpenCV's hue units (180 per turn)."""
from __future__ import annotations

import numpy as np

from . import cv2_compat
from .class_mix import MAX_BATCH, MAX_DRAW, philox_u32

STREAM = 0x53415547          # the Philox stream of the draws ("SAUG")
ONE = 1 << 16
TAP_SUM = 2048
MAX_LEVELS = 16
MAX_RADIUS = 7
# DACS's settings as recalled (they cannot be checked offline; the README says so): ColorJitter(0.25, 0.25, 0.25, 0.25) with p = 0.8 -- a hue of
# 0.25 taken as a quarter of the +-90 units that this op allows --, GaussianBlur with p = 0.5 and sigma in [0.15, 1.15]
DEFAULTS = dict(jitter_p=0.8, brightness=0.25, contrast=0.25, saturation=0.25, hue=0.25, blur_p=0.5, sigma=(0.15, 1.15), levels=16, radius=4)


def taps_table(sigma_min, sigma_max, levels, radius):
    """uint16 [levels, radius + 1]: level q holds the one-sided taps of a Gaussian with sigma_q evenly spaced over [sigma_min, sigma_max]
    (one level: sigma_min), w[i] = rint(2048 g_i / sum g) for i >= 1 and the centre takes the remainder, so that w[0] + 2 sum w[1:] = 2048.
    Raises if the centre falls below w[1] (sigma too large for the radius)."""
    Q, R = int(levels), int(radius)
    if not 1 <= Q <= MAX_LEVELS or not 1 <= R <= MAX_RADIUS:
        raise ValueError("a tap table has 1..{} levels and a radius of 1..{}, got {} and {}".format(MAX_LEVELS, MAX_RADIUS, levels, radius))
    lo, hi = float(sigma_min), float(sigma_max)
    if not (0.0 < lo <= hi) or not np.isfinite(hi):
        raise ValueError("sigma must satisfy 0 < sigma_min <= sigma_max, got {!r} and {!r}".format(sigma_min, sigma_max))
    out = np.zeros((Q, R + 1), np.uint16)
    i = np.arange(-R, R + 1, dtype=np.float64)
    for q in range(Q):
        sigma = lo if Q == 1 else lo + (hi - lo) * q / (Q - 1)
        g = np.exp(-(i * i) / (2.0 * sigma * sigma))
        w = np.rint(TAP_SUM * g[R + 1:] / g.sum()).astype(np.int64)
        centre = TAP_SUM - 2 * int(w.sum())
        if centre < w[0]:
            raise ValueError("sigma {} is too wide for radius {}: the centre tap {} falls below its neighbour {}".format(sigma, R, centre, int(w[0])))
        out[q, 0], out[q, 1:] = centre, w
    return out


def _check_call(seed, draw, jitter, blur):
    """-> (jitter int64[5] | None, (gate, taps int64 [Q, R + 1]) | None); raises ValueError for what the op refuses with BAD_ARG."""
    if not 0 <= int(draw) < MAX_DRAW:
        raise ValueError("`draw` must lie in [0, 2^48), got {!r}".format(draw))
    if not 0 <= int(seed) < 1 << 64:
        raise ValueError("`seed` must lie in [0, 2^64), got {!r}".format(seed))
    if jitter is not None:
        j = np.asarray(jitter)
        if j.shape != (5,) or j.dtype.kind not in 'iu':
            raise ValueError("`jitter` is five integers {gate, contrast, saturation, brightness, hue}")
        j = j.astype(np.int64)
        if (j < 0).any() or (j[:4] > ONE).any() or j[4] > 90:
            raise ValueError("`jitter`: the gate and the contrast, saturation and brightness strengths lie in 0..65536, the hue strength in 0..90; got {}"
                             .format(j.tolist()))
        jitter = j
    if blur is not None:
        if not isinstance(blur, (tuple, list)) or len(blur) != 2 or isinstance(blur[0], bool) or not isinstance(blur[0], (int, np.integer)):
            raise ValueError("`blur` is (gate, taps [Q, R + 1])")
        gate, taps = int(blur[0]), np.asarray(blur[1])
        if not 0 <= gate <= ONE:
            raise ValueError("the blur gate lies in 0..65536, got {}".format(gate))
        if taps.ndim != 2 or taps.dtype.kind not in 'iu' or not 1 <= taps.shape[0] <= MAX_LEVELS or not 1 <= taps.shape[1] - 1 <= MAX_RADIUS:
            raise ValueError("the taps are integers [Q, R + 1] with 1 <= Q <= {} and 1 <= R <= {}".format(MAX_LEVELS, MAX_RADIUS))
        taps = taps.astype(np.int64)
        if (taps < 0).any() or (taps[:, 0] + 2 * taps[:, 1:].sum(1) != TAP_SUM).any() or (np.diff(taps, axis=1) > 0).any():
            raise ValueError("every row of taps has w[0] + 2 sum(w[1:]) = 2048 and does not increase")
        blur = (gate, taps)
    return jitter, blur


def _uniform(u, S):
    """-S + ((u (2 S + 1)) >> 32): a uniform integer in [-S, S] from a 32-bit word."""
    return -int(S) + ((int(u) * (2 * int(S) + 1)) >> 32)


def draws(N, seed, draw):
    """uint32 [N, 7]: u_j = philox_u32(draw 2^16 + n 2^8 + j, seed, STREAM)."""
    idx = (np.uint64(int(draw) << 16) + (np.arange(int(N), dtype=np.uint64)[:, None] << np.uint64(8)) + np.arange(7, dtype=np.uint64)[None, :])
    return philox_u32(idx, seed, STREAM)


def _grey_mean(image):
    """m: the rounded mean of cv2_compat.rgb2gray over the image, (2 G + P) // (2 P)."""
    g = int(cv2_compat.rgb2gray(image).astype(np.int64).sum())
    P = int(image.shape[0]) * int(image.shape[1])
    return (2 * g + P) // (2 * P)


def _check_images(images, blur):
    images = np.asarray(images)
    if images.dtype != np.uint8 or images.ndim != 4 or images.shape[-1] != 3 or 0 in images.shape:
        raise ValueError("images are uint8 [N, H, W, 3]")
    N, H, W = images.shape[:3]
    if N > MAX_BATCH or H * W >= 1 << 31:
        raise ValueError("a batch has at most {} images and an image fewer than 2^31 pixels".format(MAX_BATCH))
    if blur is not None and min(H, W) <= blur[1].shape[1] - 1:
        raise ValueError("the blur needs H > R and W > R, got {}x{} with R = {}".format(H, W, blur[1].shape[1] - 1))
    return images


def params_numpy(images, seed=0, draw=0, jitter=None, blur=None):
    """int32 [N, 8] as the op writes `params_out`: per image {colour step ran, c16, s16, b16, dh, m, blur ran, q}, 0 for what did not run."""
    jitter, blur = _check_call(seed, draw, jitter, blur)
    images = _check_images(images, blur)
    N = images.shape[0]
    u = draws(N, seed, draw)
    out = np.zeros((N, 8), np.int32)
    for n in range(N):
        if jitter is not None and (int(u[n, 0]) >> 16) < jitter[0]:
            out[n, 0] = 1
            if jitter[1]:
                out[n, 1] = ONE + _uniform(u[n, 1], jitter[1])
                out[n, 5] = _grey_mean(images[n])
            if jitter[2] | jitter[3] | jitter[4]:
                out[n, 2] = ONE + _uniform(u[n, 2], jitter[2])
                out[n, 3] = ONE + _uniform(u[n, 3], jitter[3])
                out[n, 4] = _uniform(u[n, 4], jitter[4])
        if blur is not None and (int(u[n, 5]) >> 16) < blur[0]:
            out[n, 6] = 1
            out[n, 7] = (int(u[n, 6]) * blur[1].shape[0]) >> 32
    return out


def _colour(image, p, contrast, hsv):
    x = image.astype(np.int64)
    if contrast:
        c16, m = int(p[1]), int(p[5])
        x = np.clip((x * c16 + m * (ONE - c16) + 32768) >> 16, 0, 255)
    if hsv:
        t = cv2_compat.rgb2hsv(x.astype(np.uint8)).astype(np.int64)
        t[..., 0] = (t[..., 0] + 180 + int(p[4])) % 180
        t[..., 1] = np.minimum(255, (t[..., 1] * int(p[2]) + 32768) >> 16)
        t[..., 2] = np.minimum(255, (t[..., 2] * int(p[3]) + 32768) >> 16)
        x = cv2_compat.hsv2rgb(t.astype(np.uint8))
    return x.astype(np.uint8)


def _blur(image, w):
    R = len(w) - 1
    H, W = image.shape[:2]
    x = np.pad(image.astype(np.int64), ((R, R), (R, R), (0, 0)), mode='reflect')            # reflect-101
    a = sum(int(w[abs(i)]) * x[:, R + i:R + i + W] for i in range(-R, R + 1))
    b = sum(int(w[abs(i)]) * a[R + i:R + i + H] for i in range(-R, R + 1))
    return ((b + (1 << 21)) >> 22).astype(np.uint8)


def augment_numpy(images, seed=0, draw=0, jitter=None, blur=None):
    """(out_images uint8 [N, H, W, 3], params int32 [N, 8]) as `fcn8s_op_strong_augment` writes them."""
    params = params_numpy(images, seed, draw, jitter, blur)
    jitter, blur = _check_call(seed, draw, jitter, blur)
    images = np.asarray(images)
    out = images.copy()
    for n in range(images.shape[0]):
        p = params[n]
        if p[0]:
            out[n] = _colour(out[n], p, bool(jitter[1]), bool(jitter[2] | jitter[3] | jitter[4]))
        if p[6]:
            out[n] = _blur(out[n], blur[1][int(p[7])])
    return out, params


def validate(augment, has_generator=True):
    """`FCN8s.train`'s `unlabeled_augment` -> None (off) or dict(jitter int32[5] | None, blur (gate, taps) | None).  True takes DEFAULTS, a dict
    overrides its fields: `jitter_p` and `blur_p` (probabilities; 0 switches the stage off), `brightness`, `contrast`, `saturation` (0..1: the
    half-width of the factor around 1), `hue` (0..1: the share of the +-90 hue units), `sigma` (min, max), `levels`, `radius`."""
    if augment is None or augment is False:
        return None
    if not has_generator:
        raise ValueError("`unlabeled_augment` needs an `unlabeled_generator`.")
    if augment is True:
        augment = {}
    if not isinstance(augment, dict):
        raise ValueError("`unlabeled_augment` must be None, True or a dict of settings, got {!r}".format(augment))
    if set(augment) - set(DEFAULTS):
        raise ValueError("`unlabeled_augment` takes {}; got {}".format(sorted(DEFAULTS), sorted(set(augment) - set(DEFAULTS))))
    s = dict(DEFAULTS, **augment)

    def unit(name):
        v = s[name]
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not 0.0 <= float(v) <= 1.0:
            raise ValueError("`unlabeled_augment[{!r}]` must be a number in [0, 1], got {!r}".format(name, v))
        return float(v)
    gate_j, gate_b = int(np.rint(unit('jitter_p') * ONE)), int(np.rint(unit('blur_p') * ONE))
    jitter = blur = None
    if gate_j:
        jitter = np.array([gate_j, np.rint(unit('contrast') * ONE), np.rint(unit('saturation') * ONE), np.rint(unit('brightness') * ONE),
                           np.rint(unit('hue') * 90)], np.int32)
    else:
        for name in ('contrast', 'saturation', 'brightness', 'hue'):
            unit(name)
    sigma = s['sigma']
    if not isinstance(sigma, (tuple, list)) or len(sigma) != 2:
        raise ValueError("`unlabeled_augment['sigma']` is (sigma_min, sigma_max), got {!r}".format(sigma))
    for name in ('levels', 'radius'):
        if isinstance(s[name], bool) or not isinstance(s[name], (int, np.integer)):
            raise ValueError("`unlabeled_augment[{!r}]` must be an integer, got {!r}".format(name, s[name]))
    taps = taps_table(sigma[0], sigma[1], s['levels'], s['radius'])
    if gate_b:
        blur = (gate_b, taps)
    if jitter is None and blur is None:
        raise ValueError("`unlabeled_augment` with `jitter_p` = 0 and `blur_p` = 0 does nothing; pass None.")
    return dict(jitter=jitter, blur=blur)


# ---- the call on device tensors ------------------------------------------------------------------------------------------------------------
def work_bytes(N):
    from . import _lib as L
    return int(L.lib.fcn8s_op_strong_augment_work_bytes(int(N)))


def augment_device(images, seed=0, draw=0, jitter=None, blur=None, params=False, work=None):
    """One `fcn8s_op_strong_augment` call on a uint8 device tensor [N,H,W,3], on the current stream: (images', params int32 [N, 8] | None, work).
    `work`: a uint8 device tensor to reuse (a larger one is made when it is too small) -- returned."""
    import ctypes as C
    import torch
    from . import _lib as L
    if not isinstance(images, torch.Tensor) or not images.is_cuda or images.dtype != torch.uint8 or images.dim() != 4 or not images.is_contiguous() \
            or images.shape[-1] != 3 or images.numel() == 0:
        raise ValueError("images have to be a contiguous uint8 tensor [N,H,W,3] on the GPU")
    jitter, blur = _check_call(seed, draw, jitter, blur)
    N, H, W = (int(x) for x in images.shape[:3])
    if N > MAX_BATCH or H * W >= 1 << 31:
        raise ValueError("a batch has at most {} images and an image fewer than 2^31 pixels".format(MAX_BATCH))
    if blur is not None and min(H, W) <= blur[1].shape[1] - 1:
        raise ValueError("the blur needs H > R and W > R, got {}x{} with R = {}".format(H, W, blur[1].shape[1] - 1))
    dev = images.device
    nbytes = work_bytes(N)
    if work is None or work.numel() < nbytes or work.device != dev:
        work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = torch.empty_like(images)
    par = torch.empty((N, 8), dtype=torch.int32, device=dev) if params else None
    jit_h = (C.c_int32 * 5)(*[int(v) for v in jitter]) if jitter is not None else None
    blur_h = taps_h = None
    if blur is not None:
        Q, R1 = blur[1].shape
        blur_h = (C.c_int32 * 3)(blur[0], Q, R1 - 1)
        taps_h = (C.c_uint16 * (Q * R1))(*[int(v) for v in blur[1].reshape(-1)])
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    L.check(L.lib.fcn8s_op_strong_augment(stream, C.c_void_p(images.data_ptr()), N, H, W, int(seed), int(draw), jit_h, blur_h, taps_h,
                                          C.c_void_p(work.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(par.data_ptr()) if params else None))
    return out, par, work
