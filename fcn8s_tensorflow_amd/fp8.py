"""The arithmetic of the 'fp8_infer' precision (FCN8S_PREC_FP8_INFER, include/fcn8s_hip.h), restated on the host.

- e4m3 is OCP E4M3FN (what gfx950 uses; not the MI300 `fnuz` format): max 448, min subnormal 2^-9, no infinities.
- q(v) = clamp v to [-448, 448], then round to nearest even e4m3; NaN stays NaN.  The clamp is explicit: torch's float8_e4m3fn
  conversion does not saturate (500.0 converts to NaN).
- E(a) = the smallest integer e with a <= 448 * 2^e, E(0) = 0.  Scales are powers of two, so every scaling below is exact and this
  module reproduces the device's operands bit for bit.
- Weights, per layer and output channel co: ew[co] = E(max |W[..., co]|), Wq = q(W * 2^-ew[co]).
- Activations, per FP8 layer L (the inputs of conv1_2 .. conv5_3, fc6, fc7): ex[L] = E(amax[L]) from calibration; the layer reads
  q(x * 2^-ex[L]).
- Output: y[co] = 2^(ex[L] + ew[co]) * sum Xq * Wq + b[co], then ReLU, fp32 products and sums.
"""
from __future__ import annotations

import math

import numpy as np

E4M3_MAX = 448.0
LAYERS = ("conv1_2", "conv2_1", "conv2_2", "conv3_1", "conv3_2", "conv3_3", "conv4_1", "conv4_2", "conv4_3",
          "conv5_1", "conv5_2", "conv5_3", "fc6", "fc7")
# the fp32 tensor each FP8 layer reads (the pool of a block feeds the next block's first conv; amax(pool) = amax(its conv))
INPUTS = ("conv1_1", "pool1", "conv2_1", "pool2", "conv3_1", "conv3_2", "pool3", "conv4_1", "conv4_2", "pool4",
          "conv5_1", "conv5_2", "pool5", "fc6")


def exponent(a):
    """E(a): the smallest integer e with a <= 448 * 2^e; E(0) = 0."""
    a = float(a)
    if not a > 0.0:
        return 0
    e = math.frexp(a)[1] - 1 - 8
    while a > math.ldexp(E4M3_MAX, e):
        e += 1
    while a <= math.ldexp(E4M3_MAX, e - 1):
        e -= 1
    return e


def q(v):
    """q(v) as float32 values (torch tensor or array in, same kind out): clamp to [-448, 448], round to nearest even e4m3."""
    import torch
    t = v if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v, dtype=np.float32))
    r = t.float().clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn).float()
    return r if isinstance(v, torch.Tensor) else r.numpy()


def codes(v):
    """The e4m3 bit patterns (uint8) of q(v)."""
    import torch
    t = v if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v, dtype=np.float32))
    return t.float().clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn).view(torch.uint8)


def quantize_activation(x, ex):
    """Dequantized values of a layer input: 2^ex * q(x * 2^-ex) (exact in fp32)."""
    import torch
    t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x, dtype=np.float32))
    return q(t.float() * (2.0 ** -ex)) * (2.0 ** ex)


def quantize_weights(w):
    """HWIO weights -> (Wq as float32 values, ew int array per output channel)."""
    import torch
    t = w if isinstance(w, torch.Tensor) else torch.as_tensor(np.asarray(w, dtype=np.float32))
    t = t.float()
    amax = t.abs().reshape(-1, t.shape[-1]).amax(0)
    ew = np.array([exponent(a) for a in amax.cpu().numpy()], np.int64)
    scale = torch.as_tensor(np.ldexp(1.0, -ew).astype(np.float32), device=t.device)
    return q(t * scale), ew


def exponents(amax):
    """ex[L] for a calibration (14 maxima)."""
    return [exponent(a) for a in amax]
