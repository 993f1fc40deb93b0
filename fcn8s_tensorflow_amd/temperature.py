"""Temperature scaling (Guo et al., ICML 2017): one scalar T, fitted on a validation set by minimising the NLL of the calibrated distribution,
applied to whatever distribution a prediction route returns.  It never changes the argmax.

The definition is in include/fcn8s_hip.h at `fcn8s_op_temperature_nll`; for beta = 1 / T and a row p of C floats:

    l_c = log(max(p_c, FLT_MIN));   m = max_c l_c;   d_c = l_c - m
    e_c = exp(beta * d_c);          s = sum_c e_c   folded in class order from 0
    q_c = e_c / s                                   the calibrated distribution
    nll(beta) = log(s) - beta * d_t                 t = the true class

`nll_numpy` and `apply_numpy` restate it in that operation order, in float32 (the device's arithmetic) or float64 (the reference of the tests).
The fit (`fit`) is a bracketing grid search, safe because nll is convex in beta: every sweep over the validation set evaluates one grid of K
candidates (`fcn8s_op_temperature_nll` does that in one pass over each softmax, where it already is), `refine` puts the next grid between the
two neighbours of the minimum.  `Fitter` owns the device tables of one sweep; `FCN8s.fit_temperature` feeds it a directory.

Tables of one sweep (int64): nll [K] = sum over the counted pixels of rint(nll(beta_k) * 2^16), count [1], bad [2] (pixels whose true class is
>= C and not 255 = ignore; pixels with a p_c that is not finite).  On the device they are one tensor of K + 3 integers in that order.
"""
from __future__ import annotations

import ctypes as C
import json
import math
import os
from collections import OrderedDict

import numpy as np

MAX_CANDIDATES = 32          # FCN8S_TS_MAX_CANDIDATES
TILE_PIXELS = 256            # FCN8S_TS_TILE_PIXELS: pixels per block and trip of the kernels
MAX_BLOCKS = 1024            # FCN8S_TS_MAX_BLOCKS: beyond TILE_PIXELS * MAX_BLOCKS pixels a block takes a second trip
BETA_MIN, BETA_MAX = 2.0 ** -6, 2.0 ** 6
Q_NLL = float(2 ** 16)
_FLT_MIN = np.float32(np.finfo(np.float32).tiny)


def validate(betas):
    """The candidates of one `temperature_nll` call as float32[K]: 1 <= K <= MAX_CANDIDATES, every beta finite and in [2^-6, 2^6]."""
    b = np.asarray(betas, dtype=np.float64).reshape(-1)
    if not 1 <= b.size <= MAX_CANDIDATES:
        raise ValueError("between 1 and {} candidate values of beta = 1 / T, got {}".format(MAX_CANDIDATES, b.size))
    if not (np.isfinite(b).all() and (b >= BETA_MIN).all() and (b <= BETA_MAX).all()):
        raise ValueError("every beta = 1 / T must be finite and in [2^-6, 2^6], got {}".format(b.tolist()))
    return b.astype(np.float32)


def validate_temperature(temperature):
    """float(T) for a temperature whose beta = 1 / T the ops take; ValueError otherwise."""
    try:
        T = float(temperature)
    except (TypeError, ValueError):
        raise ValueError("`temperature` must be a number, got {!r}".format(temperature))
    if not (math.isfinite(T) and T > 0 and BETA_MIN <= 1.0 / T <= BETA_MAX):
        raise ValueError("`temperature` must be finite and in [2^-6, 2^6], got {!r}".format(temperature))
    return T


def validate_fit(passes, candidates, t_min, t_max):
    if not (isinstance(passes, (int, np.integer)) and 1 <= int(passes) <= 8):
        raise ValueError("`passes` must be an integer in 1..8, got {!r}".format(passes))
    if not (isinstance(candidates, (int, np.integer)) and 3 <= int(candidates) <= MAX_CANDIDATES):
        raise ValueError("`candidates` must be an integer in 3..{}, got {!r}".format(MAX_CANDIDATES, candidates))
    t_min, t_max = validate_temperature(t_min), validate_temperature(t_max)
    if not t_min < t_max:
        raise ValueError("`t_min` must be below `t_max`, got {!r} and {!r}".format(t_min, t_max))
    return int(passes), int(candidates), t_min, t_max


def _check_lut(lut):
    lut = np.asarray(lut)
    if lut.dtype != np.uint8 or lut.shape != (256,):
        raise ValueError("`lut` must be 256 uint8 entries")
    return lut


def nll_numpy(prob, gt, lut, betas, dtype=np.float32):
    """The definition from NumPy in `dtype` (float32: the device's operation order; float64: the reference).  prob [..., C] float32, gt [...]
    uint8, lut 256 uint8, betas as `validate` takes them.  Returns (terms, nll, count, bad): terms [n, K] in `dtype`, nll(beta_k) of the n
    counted pixels in their order; nll int64[K] = sum of rint(terms * 2^16); count = n; bad int64[2]."""
    prob = np.asarray(prob)
    if prob.dtype != np.float32 or prob.ndim < 2:
        raise ValueError("`prob` must be float32 [..., C]")
    Cn = int(prob.shape[-1])
    if Cn < 2:
        raise ValueError("temperature scaling needs at least 2 classes, got {}".format(Cn))
    b = validate(betas).astype(dtype)
    lut = _check_lut(lut)
    gt = np.asarray(gt)
    if gt.dtype != np.uint8 or gt.shape != prob.shape[:-1]:
        raise ValueError("`gt` must be uint8 of shape {}, got {} {}".format(prob.shape[:-1], gt.dtype, gt.shape))
    bad = np.zeros(2, np.int64)
    t = lut[gt.reshape(-1)].astype(np.int64)
    bad[0] = int(((t >= Cn) & (t != 255)).sum())
    sel = np.flatnonzero(t < Cn)
    p = prob.reshape(-1, Cn)[sel]
    t = t[sel]
    fin = np.isfinite(p).all(-1)                     # tested on p_c, before the clamp
    bad[1] = int((~fin).sum())
    p, t = p[fin].astype(dtype), t[fin]
    n = len(t)
    with np.errstate(all="ignore"):
        l = np.log(np.fmax(p, dtype(_FLT_MIN)))
        d = l - l.max(-1, keepdims=True)
        s = np.zeros((n, b.size), dtype)
        for c in range(Cn):                          # the fold in class order; the product is rounded before the exponential
            x = d[:, c:c + 1] * b[None, :]
            s = s + np.exp(x)
        bd = d[np.arange(n), t][:, None] * b[None, :]
        terms = np.log(s) - bd
        q = np.rint(terms * dtype(Q_NLL)).astype(np.int64)
    return terms, q.sum(0), n, bad


def apply_numpy(prob, beta, dtype=np.float32):
    """(q, h) of `fcn8s_op_temperature_apply` from NumPy in `dtype`: the calibrated distribution [..., C] and its entropy [...].  A row with a
    p_c that is not finite is NaN throughout."""
    prob = np.asarray(prob)
    if prob.dtype != np.float32 or prob.ndim < 2:
        raise ValueError("`prob` must be float32 [..., C]")
    b = dtype(validate([beta])[0])
    Cn = int(prob.shape[-1])
    p = prob.astype(dtype)
    with np.errstate(all="ignore"):
        fin = np.isfinite(p).all(-1)
        l = np.log(np.fmax(np.where(np.isfinite(p), p, 1), dtype(_FLT_MIN)))
        d = l - l.max(-1, keepdims=True)
        e = np.exp(d * b)
        s = np.zeros(p.shape[:-1], dtype)
        for c in range(Cn):
            s = s + e[..., c]
        q = e / s[..., None]
        h = np.zeros(p.shape[:-1], dtype)
        for c in range(Cn):                          # mc_dropout._entropy's fold: h - fl(q_c * log(max(q_c, FLT_MIN)))
            h = h - q[..., c] * np.log(np.fmax(q[..., c], dtype(_FLT_MIN)))
    q[~fin] = np.nan; h[~fin] = np.nan
    return q, h


# ---------------------------------------------------------------------------------------------------------
# the grids of the fit (temperatures in ascending order; beta = float32(1 / T) is what the ops see)
# ---------------------------------------------------------------------------------------------------------
def candidate_grid(t_min, t_max, k):
    """k log-spaced temperatures from t_min to t_max.  The grid always contains T = 1 (beta = 1, the uncalibrated model, so that "before"
    is reported from the same sweep): an interior point that is the nearest to 1 is moved onto it; if 1 lies outside the range or an end point
    is the nearest, k - 1 points span the range and 1 is the k-th."""
    t_min, t_max = validate_temperature(t_min), validate_temperature(t_max)
    if not (isinstance(k, (int, np.integer)) and 3 <= int(k) <= MAX_CANDIDATES and t_min < t_max):
        raise ValueError("a grid needs 3..{} points and t_min < t_max".format(MAX_CANDIDATES))
    k = int(k)
    g = np.geomspace(t_min, t_max, k)
    g[0], g[-1] = t_min, t_max
    j = int(np.argmin(np.abs(np.log(g))))
    if 0 < j < k - 1:
        g[j] = 1.0
    elif not (g == 1.0).any():
        g = np.geomspace(t_min, t_max, k - 1)
        g[0], g[-1] = t_min, t_max
        g = np.sort(np.append(g, 1.0))
    return g


def refine(temperatures, nll, k):
    """The next grid: k log-spaced temperatures that span the two neighbours of the minimum of `nll` over the ascending `temperatures` (convexity
    puts the optimum between them).  Returns (grid, end): end is None, or 'min' / 'max' when the minimum is the grid's first / last point --
    the next grid then spans that end and its one neighbour, and cannot leave the range."""
    T = np.asarray(temperatures, np.float64)
    v = np.asarray(nll)
    if T.ndim != 1 or T.size < 2 or v.shape != T.shape or not (np.diff(T) > 0).all():
        raise ValueError("`temperatures` must be ascending, with one nll each")
    j = int(np.argmin(v))
    lo, hi = max(j - 1, 0), min(j + 1, T.size - 1)
    g = np.geomspace(T[lo], T[hi], int(k))
    g[0], g[-1] = T[lo], T[hi]
    return g, ('min' if j == 0 else 'max' if j == T.size - 1 else None)


def betas_of(temperatures):
    """float32 beta = 1 / T per temperature: what `temperature_nll` is given, and what `temperature_apply` forms from a fitted T."""
    return (1.0 / np.asarray(temperatures, np.float64)).astype(np.float32)


def fit(sweep, passes=2, candidates=32, t_min=0.125, t_max=8.0):
    """The bracketing grid search.  `sweep(betas)` evaluates one grid over the whole validation set and returns (nll int64[K], count, bad[2]) --
    `Fitter` on the device, `nll_numpy` on the host.  Returns the dict `FCN8s.fit_temperature` returns, without 'nbPixels' and 'route'."""
    passes, k, t_min, t_max = validate_fit(passes, candidates, t_min, t_max)
    grid = candidate_grid(t_min, t_max, k)
    history, before, count = [], None, 0
    for i in range(passes):
        nll, count, bad = sweep(betas_of(grid))
        nll = np.asarray(nll, np.int64)
        if np.asarray(bad).any():
            raise ValueError("{} pixels hold a class id outside the model's classes and {} a probability that is not finite".format(int(bad[0]), int(bad[1])))
        if count <= 0:
            raise ValueError("no pixel was counted: every label is ignored")
        mean = nll / (float(count) * Q_NLL)
        history.append([(float(t), float(m)) for t, m in zip(grid, mean)])
        if i == 0:
            before = float(mean[int(np.flatnonzero(grid == 1.0)[0])])
        j = int(np.argmin(nll))
        best, after = float(grid[j]), float(mean[j])
        if i + 1 < passes:
            grid, _ = refine(grid, nll, k)
    return OrderedDict([("temperature", best), ("atBound", bool(best <= t_min or best >= t_max)), ("nllBefore", before), ("nllAfter", after),
                        ("candidates", history), ("pixels", int(count))])


# ---------------------------------------------------------------------------------------------------------
# the device side
# ---------------------------------------------------------------------------------------------------------
def new_tables_device(k, device):
    import torch
    return torch.zeros(int(k) + 3, dtype=torch.int64, device=device)


def nll_device(prob, gt, lut, betas, tables=None):
    """One `fcn8s_op_temperature_nll` call on tensors that live on the GPU, accumulating into `tables` (int64 [K + 3] on the device: nll [K],
    count, bad [2]; None: a new, zeroed one).  prob float32 [N,...,C], gt uint8 [N,...], lut uint8[256] (a device tensor or anything
    `np.asarray` takes), betas as `validate` takes them (host).  Nothing comes back to the host; returns the tables."""
    import torch
    from . import _lib as L
    if not (isinstance(prob, torch.Tensor) and prob.is_cuda and prob.dtype == torch.float32 and prob.dim() >= 2):
        raise ValueError("`prob` must be a float32 tensor [N, ..., C] on the GPU")
    dev = prob.device
    Cn = int(prob.shape[-1])
    if Cn < 2:
        raise ValueError("temperature scaling needs at least 2 classes, got {}".format(Cn))
    b = validate(betas)
    if not isinstance(gt, torch.Tensor):
        gt = torch.as_tensor(np.asarray(gt))
    if gt.dtype != torch.uint8 or tuple(gt.shape) != tuple(prob.shape[:-1]):
        raise ValueError("`gt` must be uint8 of shape {}, got {} {}".format(tuple(prob.shape[:-1]), gt.dtype, tuple(gt.shape)))
    gt = gt.to(dev).contiguous(); prob = prob.contiguous()
    if not isinstance(lut, torch.Tensor):
        lut = torch.from_numpy(_check_lut(lut).copy())
    if lut.dtype != torch.uint8 or tuple(lut.shape) != (256,):
        raise ValueError("`lut` must be 256 uint8 entries")
    lut = lut.to(dev).contiguous()
    if tables is None:
        tables = new_tables_device(b.size, dev)
    if not (isinstance(tables, torch.Tensor) and tables.device == dev and tables.dtype == torch.int64 and tuple(tables.shape) == (b.size + 3,)
            and tables.is_contiguous()):
        raise ValueError("`tables` must be a contiguous int64 tensor of {} entries on the prediction's device".format(b.size + 3))
    if gt.numel() == 0:
        return tables
    N = 1 if gt.dim() <= 1 else int(gt.shape[0])
    P = gt.numel() // N
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    at = lambda i: C.c_void_p(tables.data_ptr() + 8 * i)
    L.check(L.lib.fcn8s_op_temperature_nll(stream, C.c_void_p(prob.data_ptr()), C.c_void_p(gt.data_ptr()), C.c_void_p(lut.data_ptr()), N, P, Cn,
                                           b.ctypes.data_as(L._fp), int(b.size), at(0), at(b.size), at(b.size + 1)))
    return tables


def apply_device(prob, temperature, entropy=False, out=None):
    """One `fcn8s_op_temperature_apply` call on a float32 tensor [N,...,C] on the GPU: the distribution calibrated at `temperature` into `out`
    (None: a new tensor; `prob` itself: in place; False: not written) and, with `entropy`, its entropy [N,...].  Returns (out | None,
    entropy | None)."""
    import torch
    from . import _lib as L
    if not (isinstance(prob, torch.Tensor) and prob.is_cuda and prob.dtype == torch.float32 and prob.dim() >= 2 and prob.is_contiguous()):
        raise ValueError("`prob` must be a contiguous float32 tensor [N, ..., C] on the GPU")
    beta = float(betas_of([validate_temperature(temperature)])[0])
    Cn = int(prob.shape[-1])
    if Cn < 2:
        raise ValueError("temperature scaling needs at least 2 classes, got {}".format(Cn))
    if out is None:
        out = torch.empty_like(prob)
    elif out is False:
        out = None
    elif not (isinstance(out, torch.Tensor) and out.device == prob.device and out.dtype == torch.float32 and out.shape == prob.shape and out.is_contiguous()):
        raise ValueError("`out` must be a contiguous float32 tensor of the shape of `prob` on its device")
    if out is None and not entropy:
        raise ValueError("neither the distribution nor its entropy was asked for")
    ent = torch.empty(prob.shape[:-1], dtype=torch.float32, device=prob.device) if entropy else None
    if prob.numel() == 0:
        return out, ent
    N = 1 if prob.dim() <= 2 else int(prob.shape[0])
    P = prob.numel() // Cn // N
    stream = C.c_void_p(torch.cuda.current_stream(prob.device).cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    L.check(L.lib.fcn8s_op_temperature_apply(stream, ptr(prob), N, P, Cn, beta, ptr(out), ptr(ent)))
    return out, ent


class Fitter:
    """The device tables of one sweep of the fit: `add(prob, gt)` is one `temperature_nll` call on a prediction that is on the GPU, `result()`
    downloads the K + 3 integers once and returns (nll int64[K], count, bad int64[2])."""

    def __init__(self, betas, lut, num_classes=20):
        self.betas = validate(betas)
        self.lut = _check_lut(lut).copy()
        self.num_classes = int(num_classes)
        self._tables = None
        self._lut_dev = None

    def add(self, prob, gt):
        import torch
        if int(prob.shape[-1]) != self.num_classes:
            raise ValueError("a softmax of {} classes for a fitter of {}".format(int(prob.shape[-1]), self.num_classes))
        if self._tables is None:
            self._tables = new_tables_device(self.betas.size, prob.device)
            self._lut_dev = torch.from_numpy(self.lut).to(prob.device)
        nll_device(prob, gt, self._lut_dev, self.betas, self._tables)

    def result(self):
        K = self.betas.size
        t = np.zeros(K + 3, np.int64) if self._tables is None else self._tables.cpu().numpy()
        return t[:K].copy(), int(t[K]), t[K + 1:].copy()


def write_result_json(res, path):
    """The result of `fit` / `FCN8s.fit_temperature` as JSON."""
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    with open(path, 'w') as f:
        f.write(json.dumps(res, indent=4))
