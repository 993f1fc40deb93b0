"""Class-balanced pseudo-labelling of unlabelled images (self-training on hard labels with one confidence threshold per class: CBST,
Zou et al., ECCV 2018): the NumPy restatement of `fcn8s_op_pseudo_label`, the host half of the threshold fit, and the device wrapper.

The definition is in include/fcn8s_hip.h at `fcn8s_op_pseudo_label`.  Two sweeps over the unlabelled set: the first fills, per predicted
class, a histogram of the maximum softmax probability in BINS = 1024 bins (`hist`), `thresholds_from_hist` puts each class's threshold on
the bin edge above which the asked portion of its pixels lies, and the second writes label maps that hold the class where it clears its
threshold and `ignore_id` elsewhere.  BINS is a power of two, so conf * BINS is exact in float32 and, for a threshold j / BINS,
conf >= j / BINS <=> bin(conf) >= j for every conf in [0, 1): the kept count of a class in the second sweep equals the tail sum of its
histogram from the first, exactly.  Everything that decides anything is an integer; `tables_numpy` and the kernel agree with `==`."""
from __future__ import annotations

import ctypes as C
import fnmatch
import json
import math
import os
from collections import OrderedDict
from fractions import Fraction

import numpy as np

from . import sweeps

BINS = 1024                  # FCN8S_PL_BINS
TILE_PIXELS = 256            # FCN8S_PL_TILE_PIXELS: pixels per block and trip of the kernel
MAX_BLOCKS = 512             # FCN8S_PL_MAX_BLOCKS: beyond TILE_PIXELS * MAX_BLOCKS pixels a block takes a second trip
MAX_CLASSES = 255
TABLE_NAMES = ("hist", "counts", "misc")


def new_tables(num_classes, hist=True):
    Cn = int(num_classes)
    return OrderedDict([("hist", np.zeros((Cn, BINS), np.int64) if hist else None), ("counts", np.zeros((Cn, 2), np.int64)),
                        ("misc", np.zeros(3, np.int64))])


def _check_classes(Cn):
    if not 2 <= Cn <= MAX_CLASSES:
        raise ValueError("pseudo-labelling takes 2..{} classes, got {}".format(MAX_CLASSES, Cn))


def _check_id(value, name):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not 0 <= int(value) <= 255:
        raise ValueError("`{}` must be an integer in 0..255, got {!r}".format(name, value))
    return int(value)


def _check_thresholds(thresholds, Cn):
    if thresholds is None:
        return None
    t = np.asarray(thresholds, np.float32).reshape(-1)
    if t.size != Cn:
        raise ValueError("`thresholds` must hold one value per class ({}), got {}".format(Cn, t.size))
    if np.isnan(t).any():
        raise ValueError("a threshold is NaN")
    return np.ascontiguousarray(t)


def _check_out_ids(out_ids, Cn):
    if out_ids is None:
        return None
    o = np.asarray(out_ids)
    if o.dtype.kind not in "iu" or o.reshape(-1).size != Cn or o.min() < 0 or o.max() > 255:
        raise ValueError("`out_ids` must hold one label in 0..255 per class ({})".format(Cn))
    return np.ascontiguousarray(o.reshape(-1).astype(np.uint8))


def _check_gate(score_given, score_max):
    if not score_given:
        if score_max is not None:
            raise ValueError("`score_max` without a `score` map")
        return None
    if score_max is None or not math.isfinite(float(score_max)):
        raise ValueError("a `score` map needs a finite `score_max`, got {!r}".format(score_max))
    return np.float32(score_max)


def bins_of(conf):
    """b = conf > 0 ? min(BINS - 1, (int)(conf * BINS)) : 0 for finite float32 `conf`; no value outside int's range is converted."""
    conf = np.asarray(conf, np.float32)
    with np.errstate(all="ignore"):
        x = conf * np.float32(BINS)
        top = x >= np.float32(BINS)
        return np.where(top, BINS - 1, np.where((conf > 0) & ~top, x, 0).astype(np.int64)).astype(np.int64)


def tables_numpy(prob, thresholds=None, out_ids=None, ignore_id=255, base=None, base_fill=None, score=None, score_max=None):
    """`fcn8s_op_pseudo_label` from NumPy, float32 arithmetic exactly as the header defines it.  prob [..., C] float32; thresholds float32[C]
    or None (all 0); out_ids [C] in 0..255 or None (the class itself); base uint8 [...] with `base_fill`, or None; score float32 [...] with
    `score_max`, or None.  Returns (labels uint8 [...], hist int64 [C, BINS], counts int64 [C, 2], misc int64 [3])."""
    prob = np.asarray(prob)
    if prob.dtype != np.float32 or prob.ndim < 2:
        raise ValueError("`prob` must be float32 [..., C]")
    Cn = int(prob.shape[-1])
    _check_classes(Cn)
    shape = prob.shape[:-1]
    thr = _check_thresholds(thresholds, Cn)
    if thr is None:
        thr = np.zeros(Cn, np.float32)
    oid = _check_out_ids(out_ids, Cn)
    if oid is None:
        oid = np.arange(Cn, dtype=np.uint8)
    ignore_id = _check_id(ignore_id, "ignore_id")
    p = prob.reshape(-1, Cn)
    T = p.shape[0]
    if base is not None:
        base = np.asarray(base)
        if base.dtype != np.uint8 or base.shape != shape:
            raise ValueError("`base` must be uint8 of shape {}, got {} {}".format(shape, base.dtype, base.shape))
        base_fill = _check_id(base_fill, "base_fill")
    elif base_fill is not None:
        raise ValueError("`base_fill` without a `base` map")
    if score is not None:
        score = np.asarray(score)
        if score.dtype != np.float32 or score.shape != shape:
            raise ValueError("`score` must be float32 of shape {}, got {} {}".format(shape, score.dtype, score.shape))
    smax = _check_gate(score is not None, score_max)
    t = new_tables(Cn)
    hist, counts, misc = t["hist"], t["counts"], t["misc"]
    labels = np.full(T, ignore_id, np.uint8)
    todo = np.ones(T, bool)
    if base is not None:                                  # 1. pass-through
        b = base.reshape(-1)
        through = b != base_fill
        labels[through] = b[through]
        misc[1] = int(through.sum())
        todo &= ~through
    with np.errstate(all="ignore"):
        conf = p[:, 0].copy(); k = np.zeros(T, np.int64)  # 2. c replaces the running maximum only if p_c > it
        for c in range(1, Cn):
            m = p[:, c] > conf
            conf[m] = p[m, c]; k[m] = c
        bad = todo & ~np.isfinite(conf)
        misc[0] = int(bad.sum())
        todo &= ~bad
        if score is not None:                             # 3. a NaN score fails the gate
            gated = todo & ~(score.reshape(-1) <= smax)
            misc[2] = int(gated.sum())
            np.add.at(counts[:, 1], k[gated], 1)
            todo &= ~gated
        sel = np.flatnonzero(todo)
        conf, k = conf[sel], k[sel]
        np.add.at(hist.reshape(-1), k * BINS + bins_of(conf), 1)      # 4.
        keep = conf >= thr[k]                                         # 5.
    np.add.at(counts[:, 0], k[keep], 1)
    np.add.at(counts[:, 1], k[~keep], 1)
    labels[sel[keep]] = oid[k[keep]]
    return labels.reshape(shape), hist, counts, misc


def portions_of(portion, num_classes):
    """`portion` (one value in (0, 1] or one per class) as exact rationals: fractions.Fraction(p).limit_denominator(10**6) each."""
    Cn = int(num_classes)
    vals = np.asarray(portion, np.float64).reshape(-1)
    if vals.size == 1:
        vals = np.repeat(vals, Cn)
    if vals.size != Cn:
        raise ValueError("`portion` must be one value or one per class ({}), got {}".format(Cn, vals.size))
    out = []
    for v in vals:
        if not (math.isfinite(v) and 0.0 < v <= 1.0):
            raise ValueError("`portion` must lie in (0, 1], got {!r}".format(float(v)))
        f = Fraction(float(v)).limit_denominator(10 ** 6)
        if f <= 0:
            raise ValueError("`portion` {!r} is smaller than 1e-6".format(float(v)))
        out.append(f)
    return out


def _clamp_bins(t_min, t_max):
    t_min = float(t_min)
    t_max = 1.0 if t_max is None else float(t_max)
    if not (math.isfinite(t_min) and math.isfinite(t_max) and 0.0 <= t_min <= t_max <= 1.0):
        raise ValueError("`t_min` and `t_max` must satisfy 0 <= t_min <= t_max <= 1, got {!r} and {!r}".format(t_min, t_max))
    lo = -((-Fraction(t_min) * BINS) // 1)                # ceil(t_min * BINS), exact
    hi = (Fraction(t_max) * BINS) // 1                    # floor(t_max * BINS)
    if lo > hi:
        raise ValueError("no bin edge lies in [t_min, t_max] = [{!r}, {!r}]".format(t_min, t_max))
    return int(lo), int(hi)


def thresholds_from_hist(hist, portion, t_min=0.0, t_max=None):
    """The thresholds of the fit.  For class k with n_k = sum_b hist[k][b] pixels: m_k = ceil(portion_k * n_k) in integers,
    S_k(b) = sum_{j >= b} hist[k][j] (S_k(BINS) = 0), j_k = the largest b in 0..BINS with S_k(b) >= m_k -- BINS for a class that was never
    predicted --, clamped to [ceil(t_min * BINS), floor(t_max * BINS)] (t_max = None: BINS); thr_k = float32(j_k / BINS).  Returns
    (thresholds float32[C], bins int64[C])."""
    hist = np.asarray(hist)
    if hist.ndim != 2 or hist.shape[1] != BINS or hist.dtype.kind not in "iu":
        raise ValueError("`hist` must be an integer table [C, {}]".format(BINS))
    if (hist < 0).any():
        raise ValueError("`hist` holds a negative count")
    Cn = int(hist.shape[0])
    por = portions_of(portion, Cn)
    lo, hi = _clamp_bins(t_min, t_max)
    js = np.zeros(Cn, np.int64)
    for k in range(Cn):
        row = [int(v) for v in hist[k]]
        n = sum(row)
        need = por[k] * n
        m = -((-need.numerator) // need.denominator)      # ceil in integers
        j, tail = BINS, 0                                 # S_k(BINS) = 0
        while tail < m:                                   # m <= n = S_k(0): ends at j >= 0
            j -= 1
            tail += row[j]
        js[k] = min(max(j, lo), hi)
    return (js.astype(np.float64) / BINS).astype(np.float32), js


def tail_sums(hist, bins):
    """sum_{b >= bins[k]} hist[k][b] per class: what a sweep with the edge thresholds bins / BINS keeps (for conf in [0, 1))."""
    hist = np.asarray(hist, np.int64)
    return np.array([int(hist[k, int(j):].sum()) for k, j in enumerate(np.asarray(bins).reshape(-1))], np.int64)


def validate(num_classes, portion=0.2, t_min=0.0, t_max=None, thresholds=None, ignore_id=255, id_space='train', base_search=None, base_fill=None,
             samples=None, mi_max=None, temperature=None, passes=False, resize=False):
    """The arguments of `FCN8s.fit_pseudo_label_thresholds` / `predict_and_export_pseudo_labels`; raises ValueError for what they refuse.
    Returns dict(portions, bins_range, thresholds, ignore_id, base_fill, mi_max)."""
    Cn = int(num_classes)
    _check_classes(Cn)
    por = portions_of(portion, Cn)
    rng = _clamp_bins(t_min, t_max)
    thr = _check_thresholds(thresholds, Cn)
    ignore_id = _check_id(ignore_id, "ignore_id")
    if id_space not in ('train', 'label'):
        raise ValueError("`id_space` must be 'train' or 'label', got {!r}".format(id_space))
    if id_space == 'label' and Cn != 20:
        raise ValueError("id_space='label' maps the 20 Cityscapes train ids to label ids; this model has {} classes.".format(Cn))
    if (base_search is None) != (base_fill is None):
        raise ValueError("`base_search` and `base_fill` go together: the maps to complete and the value that marks their pixels to fill")
    if base_fill is not None:
        base_fill = _check_id(base_fill, "base_fill")
        if resize:
            raise ValueError("`base_search` with `resize`: the base maps have the files' size, the prediction the resized one")
    mi_max = sweeps.check_route(passes, samples, temperature, mi_max)
    return dict(portions=por, bins_range=rng, thresholds=thr, ignore_id=ignore_id, base_fill=base_fill, mi_max=mi_max)


def summary(hist, counts, misc, thresholds=None):
    """A plain dict (json.dumps takes it) of what the tables say: per class the pixels predicted, kept and dropped, the kept share and the
    threshold; and the totals.  `hist` may be None (an export sweep keeps none)."""
    counts = np.asarray(counts, np.int64); misc = np.asarray(misc, np.int64)
    Cn = int(counts.shape[0])
    thr = None if thresholds is None else np.asarray(thresholds, np.float32).reshape(-1)
    classes = []
    for k in range(Cn):
        kept, dropped = int(counts[k, 0]), int(counts[k, 1])
        row = OrderedDict([("class", k), ("predicted", kept + dropped), ("kept", kept), ("dropped", dropped),
                           ("keptShare", kept / (kept + dropped) if kept + dropped else None),
                           ("threshold", None if thr is None else float(thr[k]))])
        if hist is not None:
            row["inHistogram"] = int(np.asarray(hist[k], np.int64).sum())
        classes.append(row)
    kept, dropped = int(counts[:, 0].sum()), int(counts[:, 1].sum())
    totals = OrderedDict([("predicted", kept + dropped), ("kept", kept), ("dropped", dropped),
                          ("keptShare", kept / (kept + dropped) if kept + dropped else None),
                          ("badRows", int(misc[0])), ("passedThrough", int(misc[1])), ("droppedByScore", int(misc[2])),
                          ("pixels", kept + dropped + int(misc[0]) + int(misc[1]))])
    return OrderedDict([("classes", classes), ("totals", totals)])


def find_base(image_path, base_files):
    """The one base label map of an image: `evaluate_cityscapes` pairs a ground-truth file `<city>_<seq>_<frame>_<type>.png` with the image
    `<city>_<seq>_<frame>*`; this is that rule in the other direction -- among `base_files` the one whose basename is
    `<city>_<seq>_<frame>_*` for the image's city, sequence and frame.  Raises ValueError when there is none or more than one."""
    from . import cityscapes_eval as ce
    city, seq, frame = ce.cs_file_info(image_path)
    pattern = "{}_{}_{}_*".format(city, seq, frame)
    found = [f for f in base_files if fnmatch.fnmatch(os.path.basename(f), pattern)]
    if not found:
        raise ValueError("Found no base label map for image {}".format(image_path))
    if len(found) > 1:
        raise ValueError("Found multiple base label maps for image {}".format(image_path))
    return found[0]


def write_result_json(res, path):
    """A result of `FCN8s.fit_pseudo_label_thresholds` / `predict_and_export_pseudo_labels` as JSON (arrays as lists)."""
    def plain(v):
        if isinstance(v, np.ndarray):
            return v.tolist()
        if isinstance(v, (np.integer,)):
            return int(v)
        if isinstance(v, (np.floating,)):
            return float(v)
        if isinstance(v, dict):
            return OrderedDict((k, plain(x)) for k, x in v.items())
        if isinstance(v, (list, tuple)):
            return [plain(x) for x in v]
        return v
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    with open(path, 'w') as f:
        f.write(json.dumps(plain(res), indent=4))


# ---------------------------------------------------------------------------------------------------------
# the device side
# ---------------------------------------------------------------------------------------------------------
def new_tables_device(num_classes, device, hist=True):
    import torch
    return OrderedDict((k, None if v is None else torch.zeros(v.shape, dtype=torch.int64, device=device)) for k, v in new_tables(num_classes, hist).items())


def labels_device(prob, thresholds=None, out_ids=None, ignore_id=255, base=None, base_fill=None, score=None, score_max=None, labels=True,
                  tables=None):
    """One `fcn8s_op_pseudo_label` call on tensors that live on the GPU, on the current stream.  prob float32 [N,...,C]; thresholds float32[C]
    and out_ids uint8[C] (device tensors, or anything `np.asarray` takes: uploaded) or None; base uint8 [N,...] with `base_fill`; score
    float32 [N,...] with `score_max`; `labels`: write the uint8 label map [N,...] (False: tables only, the fit sweep).  The counts are
    accumulated into `tables`, a dict of int64 device tensors hist [C, BINS] (or None: not kept), counts [C, 2], misc [3]; None makes zeroed
    ones.  Nothing comes back to the host; returns (labels | None, tables)."""
    import torch
    from . import _lib as L
    if not (isinstance(prob, torch.Tensor) and prob.is_cuda and prob.dtype == torch.float32 and prob.dim() >= 2):
        raise ValueError("`prob` must be a float32 tensor [N, ..., C] on the GPU")
    dev = prob.device
    Cn = int(prob.shape[-1])
    _check_classes(Cn)
    shape = tuple(prob.shape[:-1])
    prob = prob.contiguous()
    ignore_id = _check_id(ignore_id, "ignore_id")

    def small(v, check, dtype):
        if v is None:
            return None
        if isinstance(v, torch.Tensor):
            if v.dtype != dtype or v.numel() != Cn:
                raise ValueError("a per-class tensor must hold {} values of {}".format(Cn, dtype))
            return v.to(dev).contiguous()
        return torch.from_numpy(check(v, Cn).copy()).to(dev)
    thr = small(thresholds, _check_thresholds, torch.float32)
    oid = small(out_ids, _check_out_ids, torch.uint8)
    if base is not None:
        if not labels:
            raise ValueError("`base` maps are completed: that needs `labels`")
        if not (isinstance(base, torch.Tensor) and base.dtype == torch.uint8 and tuple(base.shape) == shape):
            raise ValueError("`base` must be a uint8 tensor of shape {}".format(shape))
        base = base.to(dev).contiguous()
        base_fill = _check_id(base_fill, "base_fill")
    elif base_fill is not None:
        raise ValueError("`base_fill` without a `base` map")
    if score is not None:
        if not (isinstance(score, torch.Tensor) and score.dtype == torch.float32 and tuple(score.shape) == shape):
            raise ValueError("`score` must be a float32 tensor of shape {}".format(shape))
        score = score.to(dev).contiguous()
    smax = _check_gate(score is not None, score_max)
    if tables is None:
        tables = new_tables_device(Cn, dev)
    want = new_tables(Cn)
    if set(tables) != set(TABLE_NAMES):
        raise ValueError("`tables` must be a dict of {}".format(TABLE_NAMES))
    for name in TABLE_NAMES:
        t = tables[name]
        if t is None and name == "hist":
            continue
        if not (isinstance(t, torch.Tensor) and t.device == dev and t.dtype == torch.int64 and tuple(t.shape) == want[name].shape and t.is_contiguous()):
            raise ValueError("`tables[{!r}]` must be a contiguous int64 tensor of shape {} on the prediction's device".format(name, want[name].shape))
    if not labels and tables["hist"] is None:
        raise ValueError("neither labels nor a histogram was asked for")
    out = torch.empty(shape, dtype=torch.uint8, device=dev) if labels else None
    if prob.numel() == 0:
        return out, tables
    N = 1 if len(shape) <= 1 else int(shape[0])
    P = (prob.numel() // Cn) // N
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    L.check(L.lib.fcn8s_op_pseudo_label(stream, ptr(prob), N, P, Cn, ptr(thr), ptr(oid), ignore_id, ptr(base), base_fill if base is not None else 0,
                                        ptr(score), float(smax) if smax is not None else 0.0, ptr(out),
                                        ptr(tables["hist"]), ptr(tables["counts"]), ptr(tables["misc"])))
    return out, tables


def tables_to_host(tables, num_classes):
    """The device tables as NumPy int64 arrays (hist None stays None); `tables` None: zeroed ones."""
    if tables is None:
        return new_tables(num_classes)
    return OrderedDict((k, None if v is None else v.cpu().numpy()) for k, v in tables.items())
