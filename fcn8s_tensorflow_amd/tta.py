"""Multi-scale / left-right-flip prediction (test-time augmentation, fcn8s_predict_tta): the pass-shape rule, argument validation and a
float64 restatement of how the library composes its passes, for the tests.

A call with scales (s_0, ..., s_k) and `flip` makes P = nscales * (1 + flip) passes, in the order (s_0, s_0 mirrored, s_1, ...).  Pass
of scale s on an H x W batch: the network sees the image resized to Hs x Ws = max(1, floor(H s + 0.5)) x max(1, floor(W s + 0.5)) (cv2
INTER_LINEAR on uint8), mirrored on a flipped pass, padded bottom / right with the mean colour to Hp x Wp (multiples of 32).  Its logits
over [0,Hs)x[0,Ws), un-mirrored, are resized to H x W with half-pixel centres and softmaxed; the result is the mean over the passes.
The scale is taken as float32, as the C ABI receives it.
"""
import math

import numpy as np

MAX_SCALES = 8
MAX_SCALE = 4.0


def validate(scales, flip=False):
    """-> the scales as a tuple of float32-rounded floats; ValueError for what fcn8s_predict_tta rejects with FCN8S_ERR_BAD_ARG."""
    try:
        seq = [float(s) for s in scales]
    except TypeError:
        raise ValueError("`scales` must be a sequence of numbers, got {!r}".format(scales))
    if not 1 <= len(seq) <= MAX_SCALES:
        raise ValueError("`scales` must hold between 1 and {} scales, got {}".format(MAX_SCALES, len(seq)))
    out = []
    for s in seq:
        s32 = float(np.float32(s)) if math.isfinite(s) and abs(s) < 1e30 else s
        if not math.isfinite(s32) or not 0.0 < s32 <= MAX_SCALE:
            raise ValueError("every scale must be a finite number in (0, {}], got {!r}".format(MAX_SCALE, s))
        out.append(s32)
    if flip not in (True, False, 0, 1):
        raise ValueError("`flip` must be a bool, got {!r}".format(flip))
    return tuple(out)


def pass_shape(H, W, scale):
    """(Hs, Ws, Hp, Wp) of one pass: the resized size and the padded size the network runs at."""
    s = float(np.float32(scale))
    hs = max(1, int(math.floor(H * s + 0.5)))
    ws = max(1, int(math.floor(W * s + 0.5)))
    return hs, ws, -(-hs // 32) * 32, -(-ws // 32) * 32


def passes(H, W, scales, flip=False):
    """[(scale, flipped, Hs, Ws, Hp, Wp)] in the library's pass order."""
    out = []
    for s in scales:
        shp = pass_shape(H, W, s)
        out.append((s, False) + shp)
        if flip:
            out.append((s, True) + shp)
    return out


def resizes(H, W, scales):
    """Whether any pass resizes the image (float32 images are then refused)."""
    return any(pass_shape(H, W, s)[:2] != (H, W) for s in scales)


def is_identity(H, W, scales, flip=False):
    """scales (1,), no flip and H, W multiples of 32: the call is exactly fcn8s_predict."""
    return not flip and len(scales) == 1 and pass_shape(H, W, scales[0]) == (H, W, H, W)


def _axis_taps(dst, src):
    """Half-pixel source taps (F.interpolate(mode='bilinear', align_corners=False)): i0, i1, weight of i1 per output index."""
    r = np.maximum((np.arange(dst, dtype=np.float64) + 0.5) * (src / dst) - 0.5, 0.0)
    i0 = np.minimum(np.floor(r).astype(np.int64), src - 1)
    i1 = np.minimum(i0 + 1, src - 1)
    return i0, i1, r - i0


def resize_bilinear(x, H, W):
    """x [N,h,w,C] -> [N,H,W,C], bilinear with half-pixel centres, in float64."""
    x = np.asarray(x, np.float64)
    y0, y1, ly = _axis_taps(H, x.shape[1])
    x0, x1, lx = _axis_taps(W, x.shape[2])
    ly = ly[None, :, None, None]; lx = lx[None, None, :, None]
    top = x[:, y0][:, :, x0] * (1 - lx) + x[:, y0][:, :, x1] * lx
    bot = x[:, y1][:, :, x0] * (1 - lx) + x[:, y1][:, :, x1] * lx
    return top * (1 - ly) + bot * ly


def softmax(x):
    x = np.asarray(x, np.float64)
    e = np.exp(x - x.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def compose(pass_logits, flips, H, W):
    """The mean softmax [N,H,W,C] (float64) of passes whose valid logits [N,Hs,Ws,C] are `pass_logits`, as the network produced them
    (i.e. still mirrored on a flipped pass)."""
    acc = None
    for lg, f in zip(pass_logits, flips):
        lg = np.asarray(lg, np.float64)
        if f:
            lg = lg[:, :, ::-1]
        p = softmax(resize_bilinear(lg, H, W))
        acc = p if acc is None else acc + p
    return acc / len(pass_logits)
