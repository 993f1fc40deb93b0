"""Class-weighted and hard-pixel-mined (OHEM) cross-entropy for training (fcn8s_set_loss): argument validation shared with the engine,
a float64 restatement of both modes for the tests, and class-weight recipes computed from label counts on the host.

P = pixels of the batch, V = the valid pixels (label id < C), l_p = the per-pixel loss m + log(sum exp(v - m)) - v[y_p] (>= 0),
w_c = the class weights.
Weighted: L = sum_{p in V} w_{y_p} l_p / P; dlogits_p = (w_{y_p} / P)(softmax_p - onehot_p).
OHEM (thresh in (0, 1], a probability): tau = float32(-log(thresh)), k = min(min_kept, |V|), t = min(tau, l_(k)) (the k-th largest l_p
over V) if k > 0 else tau, K = {p in V : l_p >= t}; L = sum_{p in K} w_{y_p} l_p / |K| (0 for an empty K); dlogits_p =
(w_{y_p} / |K|)(softmax_p - onehot_p) on K, 0 elsewhere.  The threshold is taken as float32, as the C ABI receives it.
"""
import math

import numpy as np


def validate(class_weights, ohem_thresh, ohem_min_kept, num_classes):
    """-> (float32 weights or None, float32 threshold (0.0 = off), int min_kept); ValueError for what fcn8s_set_loss rejects."""
    w = None
    if class_weights is not None:
        w = np.asarray(class_weights, dtype=np.float64).reshape(-1)
        if w.size != num_classes:
            raise ValueError("`class_weights` must hold num_classes = %d weights, got %d" % (num_classes, w.size))
        if not np.isfinite(w).all() or (w < 0).any():
            raise ValueError("class weights must be finite and >= 0")
        w = w.astype(np.float32)
        if not (w > 0).any():
            raise ValueError("class weights must not all be zero")
    t = 0.0
    if ohem_thresh is not None and ohem_thresh != 0:
        try:
            t = float(np.float32(ohem_thresh))
        except (TypeError, ValueError):
            raise ValueError("`ohem_thresh` must be a number in (0, 1], got {!r}".format(ohem_thresh))
        if not (math.isfinite(t) and 0.0 < t <= 1.0):
            raise ValueError("`ohem_thresh` must be in (0, 1] (a probability) or None, got {!r}".format(ohem_thresh))
    if isinstance(ohem_min_kept, bool) or int(ohem_min_kept) != ohem_min_kept or ohem_min_kept < 0:
        raise ValueError("`ohem_min_kept` must be an integer >= 0, got {!r}".format(ohem_min_kept))
    return w, t, int(ohem_min_kept)


def tau(ohem_thresh):
    """The loss threshold of a probability threshold, as the library computes it: float32(-log(float64(float32(thresh))))."""
    return float(np.float32(-math.log(float(np.float32(ohem_thresh)))))


def pixel_losses(logits, labels):
    """float64 l_p of (P, C) logits and (P,) labels (ids >= C: NaN)."""
    x = np.asarray(logits, np.float64)
    lab = np.asarray(labels).reshape(-1).astype(np.int64)
    C = x.shape[1]
    m = x.max(1)
    lse = m + np.log(np.exp(x - m[:, None]).sum(1))
    valid = lab < C
    out = np.full(x.shape[0], np.nan)
    out[valid] = lse[valid] - x[np.nonzero(valid)[0], lab[valid]]
    return out


def restate(logits, labels, class_weights=None, ohem_thresh=None, ohem_min_kept=100000, pixel_loss=None):
    """Both modes in float64.  logits (P, C), labels (P,) class ids; `pixel_loss` (P,) = precomputed l_p (e.g. the device's own, so that
    the selection can be compared exactly), else computed here.  -> dict(loss, dlogits (P, C), kept (P,) bool, valid, num_kept, threshold)
    (threshold 0.0 in the weighted mode)."""
    x = np.asarray(logits, np.float64)
    P, C = x.shape
    lab = np.asarray(labels).reshape(-1).astype(np.int64)
    valid = lab < C
    w = np.ones(C) if class_weights is None else np.asarray(class_weights, np.float64)
    l = pixel_losses(x, lab) if pixel_loss is None else np.asarray(pixel_loss, np.float64).reshape(-1)
    V = int(valid.sum())
    if ohem_thresh is None or ohem_thresh == 0:
        keep, den, t = valid, float(P), 0.0
    else:
        t = tau(ohem_thresh)
        k = min(int(ohem_min_kept), V)
        if k > 0:
            t = min(t, float(np.sort(l[valid])[::-1][k - 1]))
        keep = valid & (np.where(valid, l, -np.inf) >= t)
        den = float(keep.sum())
    wy = np.where(keep, w[np.where(valid, lab, 0)], 0.0)
    loss = float((wy * np.where(keep, l, 0.0)).sum() / den) if den > 0 else 0.0
    sm = np.exp(x - x.max(1, keepdims=True))
    sm /= sm.sum(1, keepdims=True)
    onehot = np.zeros_like(sm)
    onehot[np.nonzero(valid)[0], lab[valid]] = 1.0
    d = (wy / den)[:, None] * (sm - onehot) if den > 0 else np.zeros_like(sm)
    return dict(loss=loss, dlogits=d, kept=keep, valid=V, num_kept=int(keep.sum()), threshold=t)


def class_pixel_counts(label_batches, num_classes):
    """Pixel counts per class over an iterable of label-id batches ((N, H, W) or (H, W); ids >= num_classes ignored).
    -> (counts, image_counts), int64 [num_classes]: image_counts[c] = the labelled pixels of the images in which class c occurs (the
    denominator of median-frequency balancing)."""
    counts = np.zeros(num_classes, np.int64)
    image_counts = np.zeros(num_classes, np.int64)
    for batch in label_batches:
        b = np.asarray(batch)
        if b.ndim == 2:
            b = b[None]
        for img in b.reshape(b.shape[0], -1):
            ids = img[img < num_classes].astype(np.int64)
            c = np.bincount(ids, minlength=num_classes)
            counts += c
            image_counts[c > 0] += ids.size
    return counts, image_counts


def median_frequency_weights(counts, image_counts):
    """Median-frequency balancing (Eigen & Fergus; SegNet): freq_c = counts[c] / image_counts[c], w_c = median(freq) / freq_c over the
    classes that occur; a class that never occurs gets weight 0."""
    counts = np.asarray(counts, np.float64)
    image_counts = np.asarray(image_counts, np.float64)
    present = counts > 0
    if not present.any():
        raise ValueError("no class occurs in the counts")
    freq = np.zeros_like(counts)
    freq[present] = counts[present] / image_counts[present]
    w = np.zeros_like(counts)
    w[present] = np.median(freq[present]) / freq[present]
    return w.astype(np.float32)


def enet_weights(counts, c=1.02):
    """ENet's class weights: w_c = 1 / ln(c + p_c), p_c = counts[c] / sum(counts)."""
    counts = np.asarray(counts, np.float64)
    if counts.sum() <= 0:
        raise ValueError("the counts are all zero")
    if not c > 1.0:
        raise ValueError("`c` must be > 1 (the weights are 1 / ln(c + p))")
    return (1.0 / np.log(c + counts / counts.sum())).astype(np.float32)
