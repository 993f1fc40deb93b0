"""What a softmax and its uncertainty maps are worth against ground truth: calibration (expected / maximum calibration error and the
reliability diagram, Guo et al., ICML 2017; NLL; Brier score) and error detection (AUROC, AUPR, risk-coverage and AURC / E-AURC of
"uncertainty predicts a wrong pixel": Hendrycks & Gimpel, ICLR 2017; Geifman & El-Yaniv, NeurIPS 2017).

Two halves.  The counting half turns pixels into four integer tables -- `fcn8s_op_reliability_pair` on the GPU (include/fcn8s_hip.h has
the definition), `counts_numpy` here in the device's float32 operation order, so the two agree exactly (the q_nll sum up to the two
`logf`s' last bits).  The measuring half takes every figure from the tables in float64 (`measures`).  `Evaluator` accumulates over images,
on the GPU when it is fed device tensors; `FCN8s.evaluate_reliability` feeds it a directory.

Tables (all int64; C classes, B confidence bins, M = SCORE_BINS uncertainty bins, J caller-supplied scores):
    calib [B][3]      per confidence bin b = min(B - 1, int(conf * B)): pixels, correct pixels, sum of q_conf = rint(conf * 2^24)
    sums  [4]         pixels, correct pixels, sum of q_nll = rint(-log(max(p_t, FLT_MIN)) * 2^16), sum of q_brier = rint(sum_c (p_c - [c == t])^2 * 2^23)
    hist  [1 + J][M][2]   per score and bin in ascending uncertainty: correct pixels, wrong pixels.  Score 0 is 1 - conf at scale M (the maximum
                      softmax probability), score j >= 1 the caller's map j - 1 at scale M / score_max: bin = min(M - 1, int(s * scale)), 0 for s <= 0
    bad   [2]         pixels whose true class is >= C (and not 255 = ignore); pixels whose confidence or a score is not finite
"""
from __future__ import annotations

import ctypes as C
import json
import math
import os
from collections import OrderedDict

import numpy as np

SCORE_BINS = 1024            # FCN8S_REL_SCORE_BINS
TILE_PIXELS = 256            # FCN8S_REL_TILE_PIXELS: pixels per block and trip of the kernel
MAX_BLOCKS = 1024            # FCN8S_REL_MAX_BLOCKS: beyond TILE_PIXELS * MAX_BLOCKS pixels a block takes a second trip
MAX_BINS = 64
MAX_SCORES = 3
Q_CONF, Q_NLL, Q_BRIER = float(2 ** 24), float(2 ** 16), float(2 ** 23)
_FLT_MIN = np.float32(np.finfo(np.float32).tiny)


def cityscapes_lut():
    """label id -> this project's train id (labels.py), train id 0 (void) -> 255: the pixels the official evaluation ignores are ignored
    here too.  Ids above 33 -> 255."""
    from . import cityscapes_eval as ce
    lut = np.full(256, 255, np.uint8)
    t = ce.IDS_TO_TRAINIDS_ARRAY[:ce.NUM_IDS]
    lut[:ce.NUM_IDS] = np.where(t == 0, 255, t)
    return lut


def identity_lut():
    """gt already holds class ids; 255 stays the ignore value."""
    return np.arange(256, dtype=np.uint8)


def _check_common(C_, bins, nscores, scales):
    if C_ < 2:
        raise ValueError("reliability counts need at least 2 classes, got {}".format(C_))
    if not (isinstance(bins, (int, np.integer)) and 1 <= int(bins) <= MAX_BINS):
        raise ValueError("`bins` must be an integer in 1..{}, got {!r}".format(MAX_BINS, bins))
    if nscores > MAX_SCORES:
        raise ValueError("at most {} uncertainty maps, got {}".format(MAX_SCORES, nscores))
    if len(scales) != nscores:
        raise ValueError("{} scores with {} scales".format(nscores, len(scales)))
    for s in scales:
        if not (math.isfinite(float(s)) and float(s) > 0):
            raise ValueError("a score's scale must be finite and positive, got {!r}".format(s))


def _check_lut(lut):
    lut = np.asarray(lut)
    if lut.dtype != np.uint8 or lut.shape != (256,):
        raise ValueError("`lut` must be 256 uint8 entries")
    return lut


def new_tables(bins, nscores):
    return (np.zeros((bins, 3), np.int64), np.zeros(4, np.int64), np.zeros((1 + nscores, SCORE_BINS, 2), np.int64), np.zeros(2, np.int64))


def _bins_of(x, nbins):
    """min(nbins - 1, int(x)) for x >= 0 (float32), 0 below; no value outside int's range is converted."""
    top = x >= np.float32(nbins)
    return np.where(top, nbins - 1, np.where(x > 0, np.where(top, 0, x), 0).astype(np.int64)).astype(np.int64)


def counts_numpy(prob, gt, lut, scores=(), scales=(), bins=15):
    """The tables of `fcn8s_op_reliability_pair` from NumPy, float32 arithmetic in the device's operation order.  prob [..., C] float32,
    gt [...] uint8, lut 256 uint8, scores: up to 3 float32 maps of gt's shape with their float32 scales.  Returns (calib, sums, hist, bad)."""
    prob = np.asarray(prob)
    if prob.dtype != np.float32 or prob.ndim < 2:
        raise ValueError("`prob` must be float32 [..., C]")
    Cn = int(prob.shape[-1])
    scores = list(scores); scales = list(scales)
    _check_common(Cn, bins, len(scores), scales)
    bins = int(bins)
    lut = _check_lut(lut)
    gt = np.asarray(gt)
    if gt.dtype != np.uint8 or gt.shape != prob.shape[:-1]:
        raise ValueError("`gt` must be uint8 of shape {}, got {} {}".format(prob.shape[:-1], gt.dtype, gt.shape))
    sc = []
    for s in scores:
        s = np.asarray(s)
        if s.dtype != np.float32 or s.shape != gt.shape:
            raise ValueError("a score must be float32 of shape {}, got {} {}".format(gt.shape, s.dtype, s.shape))
        sc.append(s.reshape(-1))
    calib, sums, hist, bad = new_tables(bins, len(sc))
    if gt.size == 0:
        return calib, sums, hist, bad
    t = lut[gt.reshape(-1)].astype(np.int64)
    bad[0] = int(((t >= Cn) & (t != 255)).sum())
    sel = np.flatnonzero(t < Cn)
    p = prob.reshape(-1, Cn)[sel]
    t = t[sel]
    sc = [s[sel] for s in sc]
    f32 = np.float32
    with np.errstate(all="ignore"):
        conf = p[:, 0].copy(); k = np.zeros(len(sel), np.int64)
        for c in range(1, Cn):                       # c replaces the running maximum only if p_c > it: lowest index on ties, NaN at c > 0 never wins
            m = p[:, c] > conf
            conf[m] = p[m, c]; k[m] = c
        fin = np.isfinite(conf)
        for s in sc:
            fin &= np.isfinite(s)
        bad[1] = int((~fin).sum())
        p, t, conf, k = p[fin], t[fin], conf[fin], k[fin]
        sc = [s[fin] for s in sc]
        n = len(t)
        ok = k == t
        b = _bins_of(conf * f32(bins), bins)
        q_conf = np.rint(conf * f32(Q_CONF)).astype(np.int64)
        pt = p[np.arange(n), t]
        q_nll = np.rint(-np.log(np.fmax(pt, _FLT_MIN)) * f32(Q_NLL)).astype(np.int64)
        br = np.zeros(n, f32)
        for c in range(Cn):                          # the fold in class order; the square is rounded before it is added
            d = p[:, c] - (t == c).astype(f32)
            sq = d * d
            br = br + sq
        q_brier = np.rint(br * f32(Q_BRIER)).astype(np.int64)
        u = f32(1) - conf
        idx = [np.where(u > 0, _bins_of(u * f32(SCORE_BINS), SCORE_BINS), 0)]
        for s, g in zip(sc, scales):
            idx.append(np.where(s > 0, _bins_of(s * f32(g), SCORE_BINS), 0))
    np.add.at(calib[:, 0], b, 1); np.add.at(calib[:, 1], b, ok.astype(np.int64)); np.add.at(calib[:, 2], b, q_conf)
    sums[:] = (n, int(ok.sum()), int(q_nll.sum()), int(q_brier.sum()))
    wrong = (~ok).astype(np.int64)
    for j, i in enumerate(idx):
        np.add.at(hist[j].reshape(-1), i * 2 + wrong, 1)
    return calib, sums, hist, bad


def new_tables_device(bins, nscores, device):
    import torch
    return tuple(torch.zeros(t.shape, dtype=torch.int64, device=device) for t in new_tables(bins, nscores))


def counts_device(prob, gt, lut, scores=(), scales=(), bins=15, tables=None):
    """One `fcn8s_op_reliability_pair` call on tensors that live on the GPU, accumulating into `tables` (calib, sums, hist, bad: int64 device
    tensors as `new_tables_device` makes them; None: new, zeroed ones).  prob float32 [N,...,C], gt uint8 [N,...], lut uint8[256] (a tensor on
    the device or anything `np.asarray` takes), scores float32 of gt's shape.  Nothing comes back to the host; returns the tables."""
    import torch
    from . import _lib as L
    if not (isinstance(prob, torch.Tensor) and prob.is_cuda and prob.dtype == torch.float32 and prob.dim() >= 2):
        raise ValueError("`prob` must be a float32 tensor [N, ..., C] on the GPU")
    dev = prob.device
    Cn = int(prob.shape[-1])
    scores = list(scores); scales = [float(s) for s in scales]
    _check_common(Cn, bins, len(scores), scales)
    bins = int(bins)
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
    sc = []
    for s in scores:
        if not (isinstance(s, torch.Tensor) and s.dtype == torch.float32 and tuple(s.shape) == tuple(gt.shape)):
            raise ValueError("a score must be a float32 tensor of shape {}".format(tuple(gt.shape)))
        sc.append(s.to(dev).contiguous())
    if tables is None:
        tables = new_tables_device(bins, len(sc), dev)
    calib, sums, hist, bad = tables
    want = [t.shape for t in new_tables(bins, len(sc))]
    for t, w in zip(tables, want):
        if not (isinstance(t, torch.Tensor) and t.device == dev and t.dtype == torch.int64 and tuple(t.shape) == tuple(w) and t.is_contiguous()):
            raise ValueError("`tables` must be contiguous int64 tensors on the prediction's device of shapes {}".format([tuple(w) for w in want]))
    if gt.numel() == 0:
        return tables
    N = 1 if gt.dim() <= 1 else int(gt.shape[0])
    P = gt.numel() // N
    ptrs = (C.c_void_p * max(len(sc), 1))(*[s.data_ptr() for s in sc])
    scl = (C.c_float * max(len(sc), 1))(*scales)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    L.check(L.lib.fcn8s_op_reliability_pair(stream, ptr(prob), ptr(gt), ptr(lut), N, P, Cn, ptrs, scl, len(sc), bins,
                                            ptr(calib), ptr(sums), ptr(hist), ptr(bad)))
    return tables


# ---------------------------------------------------------------------------------------------------------
# the measures, float64, from the tables alone
# ---------------------------------------------------------------------------------------------------------
def _div(a, b):
    return float(a) / float(b) if b else float('nan')


def calibration_measures(calib, sums):
    calib = np.asarray(calib, np.int64); sums = np.asarray(sums, np.int64)
    n = int(sums[0])
    cnt = calib[:, 0].astype(np.float64)
    with np.errstate(all="ignore"):
        acc = np.where(cnt > 0, calib[:, 1] / cnt, np.nan)
        cf = np.where(cnt > 0, calib[:, 2] / (cnt * Q_CONF), np.nan)
    gap = np.abs(acc - cf)
    full = cnt > 0
    return OrderedDict([
        ("pixels", n),
        ("accuracy", _div(int(sums[1]), n)),
        ("meanConfidence", _div(int(calib[:, 2].sum()), n * Q_CONF)),
        ("nll", _div(int(sums[2]), n * Q_NLL)),
        ("brier", _div(int(sums[3]), n * Q_BRIER)),
        ("ece", float((cnt[full] / n * gap[full]).sum()) if n else float('nan')),
        ("mce", float(gap[full].max()) if n else float('nan')),
        ("reliabilityDiagram", OrderedDict([("count", calib[:, 0].tolist()), ("accuracy", acc.tolist()), ("meanConfidence", cf.tolist())])),
    ])


def detection_measures(hist2):
    """One score's histogram [M][2] (correct, wrong; bins in ascending uncertainty), wrong = the positive class."""
    h = np.asarray(hist2, np.int64)
    cor, wr = h[:, 0].astype(np.float64), h[:, 1].astype(np.float64)
    nb = cor + wr
    W, K = float(wr.sum()), float(cor.sum())
    n = W + K
    below = np.cumsum(cor) - cor                                           # correct pixels in lower bins
    auroc = float((wr * (below + cor / 2)).sum()) / (W * K) if W and K else float('nan')
    wr_ge = np.cumsum(wr[::-1])[::-1]; n_ge = np.cumsum(nb[::-1])[::-1]
    wr_le = np.cumsum(wr); n_le = np.cumsum(nb)
    with np.errstate(all="ignore"):
        prec = np.where(n_ge > 0, wr_ge / n_ge, 0.0)
        risk = np.where(n_le > 0, wr_le / n_le, 0.0)
    aupr = float((wr / W * prec).sum()) if W else float('nan')
    aurc = float((nb / n * risk).sum()) if n else float('nan')
    r = _div(W, n)
    if n:
        best = r + ((1 - r) * math.log(1 - r) if r < 1 else 0.0)           # the AURC of a perfect ranking at this error rate
        eaurc = aurc - best
    else:
        eaurc = float('nan')
    at = np.flatnonzero(nb > 0)
    return OrderedDict([("auroc", auroc), ("aupr", aupr), ("aurc", aurc), ("eaurc", eaurc),
                        ("riskCoverage", OrderedDict([("bin", at.tolist()), ("coverage", (n_le[at] / n).tolist() if n else []),
                                                      ("risk", risk[at].tolist())]))])


def measures(calib, sums, hist, bad, score_names=()):
    """Every figure from the tables: the calibration block, per score ('maxProb' first, then `score_names`) the detection block, and the raw
    tables themselves."""
    hist = np.asarray(hist, np.int64)
    names = ["maxProb"] + list(score_names)
    if len(names) != hist.shape[0]:
        raise ValueError("{} score names for {} histograms".format(len(names), hist.shape[0]))
    res = calibration_measures(calib, sums)
    res["errorRate"] = _div(int(sums[0]) - int(sums[1]), int(sums[0]))
    res["scores"] = OrderedDict((nm, detection_measures(hist[j])) for j, nm in enumerate(names))
    res["tables"] = OrderedDict([("calib", np.asarray(calib, np.int64)), ("sums", np.asarray(sums, np.int64)), ("hist", hist),
                                 ("bad", np.asarray(bad, np.int64))])
    return res


class Evaluator:
    """Accumulates the tables over `add` calls and reports `measures`.  `score_names`: the caller's uncertainty maps in the order `add`
    receives them; `score_max`: one positive number per map (or one for all), the value that lands in the last bin -- scale = float32(M) /
    float32(score_max); default ln(num_classes), the largest entropy.  Device tensors are counted on the GPU and the tables stay there
    until `results` (or `tables`) downloads them once; NumPy arrays are counted by `counts_numpy`.  One evaluator takes one kind."""

    def __init__(self, bins=15, num_classes=20, lut=None, score_names=(), score_max=None):
        self.score_names = tuple(score_names)
        self.num_classes = int(num_classes)
        J = len(self.score_names)
        if score_max is None:
            score_max = math.log(self.num_classes) if self.num_classes > 1 else 1.0
        smax = [score_max] * J if np.isscalar(score_max) else list(score_max)
        if len(smax) != J:
            raise ValueError("{} score names with {} values of `score_max`".format(J, len(smax)))
        for s in smax:
            if not (math.isfinite(float(s)) and float(s) > 0):
                raise ValueError("`score_max` must be finite and positive, got {!r}".format(s))
        self.score_max = [float(s) for s in smax]
        self.scales = [np.float32(SCORE_BINS) / np.float32(s) for s in smax]
        _check_common(self.num_classes, bins, J, self.scales)
        self.bins = int(bins)
        self.lut = _check_lut(identity_lut() if lut is None else lut).copy()
        self._host = new_tables(self.bins, J)
        self._dev = None
        self._lut_dev = None
        self._fed_host = False

    def add(self, prob, gt, scores=()):
        scores = list(scores)
        if len(scores) != len(self.score_names):
            raise ValueError("expected the scores {}, got {} maps".format(self.score_names, len(scores)))
        if int(prob.shape[-1]) != self.num_classes:
            raise ValueError("a softmax of {} classes for an evaluator of {}".format(int(prob.shape[-1]), self.num_classes))
        from .cityscapes_eval import _is_cuda_tensor
        if _is_cuda_tensor(prob):
            if self._fed_host:
                raise ValueError("this evaluator has been fed host arrays; device tensors need one of their own")
            import torch
            if self._dev is None:
                self._dev = new_tables_device(self.bins, len(scores), prob.device)
                self._lut_dev = torch.from_numpy(self.lut).to(prob.device)
            counts_device(prob, gt, self._lut_dev, scores, self.scales, self.bins, self._dev)
        else:
            if self._dev is not None:
                raise ValueError("this evaluator has been fed device tensors; host arrays need one of their own")
            to_np = lambda a: a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
            for acc, t in zip(self._host, counts_numpy(to_np(prob), to_np(gt), self.lut, [to_np(s) for s in scores], self.scales, self.bins)):
                acc += t
            self._fed_host = True

    def tables(self):
        """(calib, sums, hist, bad) as int64 ndarrays; one download when they are on the GPU."""
        if self._dev is not None:
            return tuple(t.cpu().numpy() for t in self._dev)
        return tuple(t.copy() for t in self._host)

    def results(self):
        res = measures(*self.tables(), score_names=self.score_names)
        res["bins"] = self.bins
        res["scoreMax"] = OrderedDict(zip(self.score_names, self.score_max))
        return res


def result_dict(res):
    """`res` with arrays as lists: what `write_result_json` writes."""
    def plain(o):
        if isinstance(o, dict):
            return OrderedDict((k, plain(v)) for k, v in o.items())
        if isinstance(o, np.ndarray):
            return o.tolist()
        if isinstance(o, (list, tuple)):
            return [plain(v) for v in o]
        if isinstance(o, np.generic):
            return o.item()
        return o
    return plain(res)


def write_result_json(res, path):
    """The result of `Evaluator.results` / `FCN8s.evaluate_reliability` as JSON, the raw tables included (NaN is written as NaN)."""
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    with open(path, 'w') as f:
        f.write(json.dumps(result_dict(res), indent=4))
