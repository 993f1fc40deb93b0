"""Class-weighted and hard-pixel-mined (OHEM) cross-entropy for training (fcn8s_set_loss): argument validation shared with the engine,
a float64 restatement of both modes for the tests, and class-weight recipes computed from label counts on the host.  The Lovász-softmax
term (fcn8s_set_lovasz) has its validation and float64 restatement behind the boundary-weighted cross-entropy
(fcn8s_set_boundary_loss; fcn8s_op_boundary_distance, fcn8s_op_softmax_xent_px): its table builders, the NumPy route of its distance codes,
its validation and the facade's argument rule (resolve_boundary).  The soft-target term (fcn8s_set_soft_targets) follows with its
validation and its float64 and float32 restatements, the entropy term (fcn8s_set_entropy_term) comes next in the same way, and the focal loss (fcn8s_set_focal) closes the file.

P = pixels of the batch, V = the valid pixels (label id < C), l_p = the per-pixel loss m + log(sum exp(v - m)) - v[y_p] (>= 0),
w_c = the class weights.
Weighted: L = sum_{p in V} w_{y_p} l_p / P; dlogits_p = (w_{y_p} / P)(softmax_p - onehot_p).
OHEM (thresh in (0, 1], a probability): tau = float32(-log(thresh)), k = min(min_kept, |V|), t = min(tau, l_(k)) (the k-th largest l_p
over V) if k > 0 else tau, K = {p in V : l_p >= t}; L = sum_{p in K} w_{y_p} l_p / |K| (0 for an empty K); dlogits_p =
(w_{y_p} / |K|)(softmax_p - onehot_p) on K, 0 elsewhere.  The threshold is taken as float32, as the C ABI receives it.
Boundary weighting: b_p = table[code(p)], code(p) = the squared distance of p to the nearest pixel of another label id if <= R^2, else 255;
every w_{y_p} above becomes w_p = float32(w_{y_p} * b_p); the OHEM selection stays on the unweighted l_p.
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


def restate(logits, labels, class_weights=None, ohem_thresh=None, ohem_min_kept=100000, pixel_loss=None, pixel_weights=None):
    """Both modes in float64.  logits (P, C), labels (P,) class ids; `pixel_loss` (P,) = precomputed l_p (e.g. the device's own, so that
    the selection can be compared exactly), else computed here; `pixel_weights` (P,) = the float32 b_p of the boundary weighting: the
    weight of a pixel is then the float32 product float32(w_{y_p}) * b_p, as the kernel forms it, and everything after it is float64.
    -> dict(loss, dlogits (P, C), kept (P,) bool, valid, num_kept, threshold) (threshold 0.0 in the weighted mode)."""
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
    if pixel_weights is not None:
        b = np.asarray(pixel_weights, np.float32).reshape(-1)
        if b.size != P:
            raise ValueError("`pixel_weights` must hold one weight per pixel (%d), got %d" % (P, b.size))
        wy = (wy.astype(np.float32) * b).astype(np.float64)
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


# ---- boundary-weighted cross-entropy (the definition is in include/fcn8s_hip.h at fcn8s_op_softmax_xent_px) -----------------------------
MAX_BOUNDARY_RADIUS = 15          # codes are one byte: d2 <= 225, 255 = farther than R
FAR_CODE = 255


def _boundary_radius(radius):
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 1 <= int(radius) <= MAX_BOUNDARY_RADIUS:
        raise ValueError("the boundary radius must be an integer in 1..%d, got %r" % (MAX_BOUNDARY_RADIUS, radius))
    return int(radius)


def default_boundary_radius(sigma):
    """min(15, ceil(3 sigma)): beyond three sigma the Gaussian adds less than 1.2 % of `weight`."""
    return max(1, min(MAX_BOUNDARY_RADIUS, int(math.ceil(3.0 * float(sigma)))))


def boundary_table(weight, sigma, radius):
    """U-Net's weight map as a table over the distance codes: float32[256], T[d2] = float32(1 + weight * exp(-d2 / (2 sigma^2)))
    (computed in float64) for 1 <= d2 <= radius^2, 1.0 elsewhere (farther than the radius, and the codes that do not occur)."""
    R = _boundary_radius(radius)
    try:
        w, s = float(weight), float(sigma)
    except (TypeError, ValueError):
        raise ValueError("`weight` and `sigma` must be numbers, got {!r}, {!r}".format(weight, sigma))
    if not (math.isfinite(w) and w >= 0.0):
        raise ValueError("the boundary weight must be finite and >= 0, got {!r}".format(weight))
    if not (math.isfinite(s) and s > 0.0):
        raise ValueError("the boundary sigma must be finite and > 0, got {!r}".format(sigma))
    T = np.ones(256, np.float32)
    d2 = np.arange(1, R * R + 1, dtype=np.float64)
    T[1:R * R + 1] = (1.0 + w * np.exp(-d2 / (2.0 * s * s))).astype(np.float32)
    return T


def ignore_band_table(width):
    """Weight 0 within `width` pixels of a boundary (d2 <= width^2), 1.0 elsewhere; its radius is `width`."""
    R = _boundary_radius(width)
    T = np.ones(256, np.float32)
    T[1:R * R + 1] = 0.0
    return T


def boundary_codes_numpy(labels, radius):
    """The NumPy route of fcn8s_op_boundary_distance's definition: uint8 codes of one label map (H, W) or a stack (N, H, W), code = d2 (the
    squared distance to the nearest pixel of the same image with another label id) if d2 <= radius^2, else 255."""
    from .cityscapes_eval import _nearest_other_label
    R = _boundary_radius(radius)
    lab = np.asarray(labels)
    if lab.ndim not in (2, 3) or lab.size == 0:
        raise ValueError("`labels` must be a label map (H, W) or a stack (N, H, W), got shape {}".format(lab.shape))
    maps = lab[None] if lab.ndim == 2 else lab
    out = np.empty(maps.shape, np.uint8)
    for n in range(maps.shape[0]):
        d2 = _nearest_other_label(maps[n], R)
        out[n] = np.where(d2 <= R * R, d2, FAR_CODE).astype(np.uint8)
    return out[0] if lab.ndim == 2 else out


def validate_boundary(table, radius):
    """-> (float32 table [256] or None, radius (0 = off)); ValueError for a table or radius outside the definition.  No table, or radius None /
    0 with no table, is "off"; a table needs a radius."""
    if table is None:
        if radius not in (None, 0):
            _boundary_radius(radius)
        return None, 0
    if radius is None:
        raise ValueError("a boundary table needs its radius")
    R = _boundary_radius(radius)
    T = np.asarray(table, dtype=np.float64).reshape(-1)
    if T.size != 256:
        raise ValueError("the boundary table must hold 256 weights (one per distance code), got %d" % T.size)
    if not np.isfinite(T).all() or (T < 0).any():
        raise ValueError("the boundary table's entries must be finite and >= 0")
    with np.errstate(over='ignore'):
        T32 = T.astype(np.float32)
    if not np.isfinite(T32).all():
        raise ValueError("the boundary table's entries must be finite in float32")
    return T32, R


def resolve_boundary(weight=None, sigma=None, radius=None, ignore_band=None):
    """The facade's arguments (FCN8s.train(boundary_*)) -> (table, radius) for Engine.set_boundary_loss; a pure function.
    `weight` + `sigma`: U-Net's table (boundary_table), `radius` defaulting to default_boundary_radius(sigma); `ignore_band` = k: weight 0
    within k pixels of a boundary (ignore_band_table); both: the U-Net table with the entries d2 <= k^2 set to 0, radius max(radius, k);
    nothing: (None, 0).  ValueError for `weight` without `sigma` or the reverse, a `radius` without them, and whatever the builders reject."""
    if (weight is None) != (sigma is None):
        raise ValueError("`boundary_weight` and `boundary_sigma` go together: got weight {!r}, sigma {!r}".format(weight, sigma))
    if weight is None:
        if radius is not None:
            raise ValueError("`boundary_radius` needs `boundary_weight` and `boundary_sigma` (an ignore band's radius is its width)")
        if ignore_band is None:
            return None, 0
        k = _boundary_radius(ignore_band)
        return ignore_band_table(k), k
    if radius is None:
        if not (isinstance(sigma, (int, float, np.integer, np.floating)) and not isinstance(sigma, bool) and math.isfinite(sigma) and sigma > 0):
            raise ValueError("the boundary sigma must be finite and > 0, got {!r}".format(sigma))
        radius = default_boundary_radius(sigma)
    R = _boundary_radius(radius)
    if ignore_band is None:
        return boundary_table(weight, sigma, R), R
    k = _boundary_radius(ignore_band)
    R = max(R, k)
    T = boundary_table(weight, sigma, R)
    T[1:k * k + 1] = 0.0
    return T, R


# ---- Lovász-softmax (fcn8s_set_lovasz; the definition is in include/fcn8s_hip.h) -------------------------------------------------------
def validate_lovasz(lovasz_weight, ce_weight=1.0, per_image=False, classes='present', num_classes=None):
    """-> (ce_weight, lovasz_weight, per_image 0/1, classes_all 0/1, uint8 mask [num_classes]); ValueError for what fcn8s_set_lovasz
    rejects.  `classes`: 'present', 'all' or a list of class ids (participating whether present or not, as the published code's list)."""
    def weight(v, name):
        try:
            f = float(v)
        except (TypeError, ValueError):
            raise ValueError("`{}` must be a number, got {!r}".format(name, v))
        if not math.isfinite(f) or f < 0:
            raise ValueError("`{}` must be finite and >= 0, got {!r}".format(name, v))
        return float(np.float32(f))
    lov, ce = weight(lovasz_weight, 'lovasz_weight'), weight(ce_weight, 'ce_weight')
    if lov == 0.0 and ce == 0.0:
        raise ValueError("`lovasz_weight` and `ce_weight` must not both be 0")
    if per_image not in (0, 1, False, True):
        raise ValueError("`per_image` must be a bool, got {!r}".format(per_image))
    mask = np.ones(num_classes, np.uint8)
    if isinstance(classes, str):
        if classes not in ('present', 'all'):
            raise ValueError("`classes` must be 'present', 'all' or a list of class ids, got {!r}".format(classes))
        classes_all = int(classes == 'all')
    else:
        ids = np.asarray(list(classes) if not isinstance(classes, np.ndarray) else classes).reshape(-1)
        if ids.size == 0 or ids.dtype.kind not in 'iu' or (ids < 0).any() or (ids >= num_classes).any():
            raise ValueError("`classes` must be a non-empty list of class ids in [0, {}), got {!r}".format(num_classes, classes))
        mask[:] = 0
        mask[ids] = 1
        classes_all = 1
    return ce, lov, int(bool(per_image)), classes_all, mask


def lovasz_grad(fg_sorted):
    """The Jaccard gradient g_r of a sorted foreground indicator in closed form (exact integer counts, float64):
    foreground 1 / U_r, background I_r / (U_{r-1} U_r) with U_0 = G; G = 0: g_1 = 1, all other 0."""
    fg = np.asarray(fg_sorted).astype(np.int64).reshape(-1)
    n = fg.size
    g = np.zeros(n)
    if n == 0:
        return g
    G = int(fg.sum())
    if G == 0:
        g[0] = 1.0
        return g
    r = np.arange(1, n + 1, dtype=np.int64)
    f = np.cumsum(fg)
    U = (G + r - f).astype(np.float64)
    Uprev = (G + r - 1 - (f - fg)).astype(np.float64)
    I = (G - f).astype(np.float64)
    return np.where(fg == 1, 1.0 / U, I / (Uprev * U))


def lovasz_grad_cumsum(fg_sorted):
    """The published form: J_r = 1 - I_r / U_r from cumulative sums, g = J_r - J_{r-1} (float64 here)."""
    fg = np.asarray(fg_sorted, np.float64).reshape(-1)
    if fg.size == 0:
        return fg.copy()
    gts = fg.sum()
    inter = gts - np.cumsum(fg)
    union = gts + np.cumsum(1.0 - fg)
    j = 1.0 - inter / union
    j[1:] = j[1:] - j[:-1]
    return j


def lovasz_restate(x, labels, N, per_image=False, classes='present', x_is='logits', num_classes=None):
    """The Lovász-softmax loss in float64 with the closed-form gradient.  x (P, C): logits (torch's float64 softmax), or 'probs' (probabilities;
    pass the device's fp32 ones so that the errors, e = float32(1 - p) for the foreground and p otherwise, and thus the order, are the
    device's own).  labels (P,) ids (>= C: ignore); N images of P / N pixels each.
    -> dict(loss, class_loss (S, C) (0 outside C_s), participating (S, C) bool, grad_prob (P, C) = d L / d prob, grad_logits (P, C) =
    the softmax Jacobian applied to it)."""
    x = np.asarray(x)
    P, C = x.shape
    lab = np.asarray(labels).reshape(-1).astype(np.int64)
    _, _, _, classes_all, mask = validate_lovasz(1.0, 1.0, per_image, classes, num_classes or C)
    if x_is == 'logits':
        import torch                      # (torch's float64 softmax: the probabilities, and so the ties, of a torch restatement)
        p = torch.softmax(torch.from_numpy(x.astype(np.float64)), 1).numpy()
        pf = p
    elif x_is == 'probs':
        pf = x.astype(np.float32)
        p = pf.astype(np.float64)
    else:
        raise ValueError("x_is must be 'logits' or 'probs'")
    S = int(N) if per_image else 1
    L = P // S
    class_loss = np.zeros((S, C))
    part = np.zeros((S, C), bool)
    gp = np.zeros((P, C))
    total = 0.0
    for s in range(S):
        off = s * L
        idx = off + np.nonzero(lab[off:off + L] < C)[0]
        ls = lab[idx]
        G = np.array([(ls == c).sum() for c in range(C)])
        on = (mask[:C] > 0) & ((G > 0) | bool(classes_all))
        part[s] = on
        ncs = int(on.sum())
        seg = 0.0
        for c in np.nonzero(on)[0]:
            fg = ls == c
            if x_is == 'probs':
                e = np.where(fg, (np.float32(1.0) - pf[idx, c]).astype(np.float32), pf[idx, c]).astype(np.float64)
            else:
                e = np.where(fg, 1.0 - p[idx, c], p[idx, c])
            order = np.argsort(-e, kind='stable')
            g = lovasz_grad(fg[order])
            lc = float(np.dot(e[order], g))
            class_loss[s, c] = lc
            seg += lc
            sgn = np.sign(p[idx[order], c] - fg[order])
            gp[idx[order], c] = g * sgn / (S * ncs)
        total += seg / ncs if ncs else 0.0
    valid = lab < C
    gz = p * (gp - (gp * p).sum(1, keepdims=True))
    gz[~valid] = 0.0
    return dict(loss=total / S, class_loss=class_loss, participating=part, grad_prob=gp, grad_logits=gz)


# ---- soft targets (fcn8s_set_soft_targets, fcn8s_bind_soft_targets; the definition is in include/fcn8s_hip.h) ----------------------------
def validate_soft_targets(weight=None, temperature=1.0, pixels='valid'):
    """-> (float32 weight (0.0 = off), float32 temperature, all_pixels 0/1); ValueError for what fcn8s_set_soft_targets rejects.  `weight`
    None or 0 is "off"; `pixels` is 'valid' (the pixels with a label id < C) or 'all'."""
    def number(v, name):
        if isinstance(v, bool):
            raise ValueError("`{}` must be a number, got {!r}".format(name, v))
        try:
            with np.errstate(over='ignore'):
                return float(np.float32(v))
        except (TypeError, ValueError):
            raise ValueError("`{}` must be a number, got {!r}".format(name, v))
    w = 0.0 if weight is None else number(weight, 'weight')
    if not math.isfinite(w) or w < 0:
        raise ValueError("the soft-target weight must be finite and >= 0, got {!r}".format(weight))
    t = number(temperature, 'temperature')
    if not (math.isfinite(t) and t > 0):
        raise ValueError("the soft-target temperature must be finite and > 0, got {!r}".format(temperature))
    if pixels not in ('valid', 'all'):
        raise ValueError("`pixels` must be 'valid' or 'all', got {!r}".format(pixels))
    return w, t, int(pixels == 'all')


def soft_target_restate(logits, targets, labels, weight=1.0, temperature=1.0, pixels='valid', ncols=None, dtype=np.float64):
    """The soft-target term restated: logits (P, C), targets (P, >= K) rows of probabilities (columns >= K = `ncols`, default C, do not take
    part), labels (P,) ids (>= C: outside U under 'valid').  `dtype` float64: the definition in float64 (the reference of the tests);
    float32: every operation rounded to float32 in the kernel's order (classes summed in order, no fused product), kd_p summed in float64 --
    its distance to the float64 result is the scale of what fp32 can be asked for.
    -> dict(term = L_kd, loss = weight * L_kd, kd (P,) (0 outside U), dlogits (P, C) = weight (T / P) (s - q), bias (C,) = its column sums
    (float64 sums), used (P,) bool)."""
    w, T, all_pixels = validate_soft_targets(weight, temperature, pixels)
    ft = np.dtype(dtype).type
    if ft not in (np.float64, np.float32):
        raise ValueError("dtype must be float64 or float32")
    z = np.asarray(logits)
    P, C = z.shape
    K = C if ncols is None else int(ncols)
    if not 1 <= K <= C:
        raise ValueError("`ncols` must be in 1..%d, got %r" % (C, ncols))
    t = np.asarray(targets)
    if t.ndim != 2 or t.shape[0] != P or t.shape[1] < K:
        raise ValueError("`targets` must be (%d, >= %d), got %s" % (P, K, t.shape))
    lab = np.asarray(labels).reshape(-1).astype(np.int64)
    used = np.ones(P, bool) if all_pixels else lab < C
    z = z[:, :K].astype(ft)
    t = t[:, :K].astype(ft)
    beta = ft(1.0) / ft(T)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        fin = np.isfinite(t).all(1)
        l = np.log(np.maximum(np.where(np.isfinite(t), t, ft(1.0)), ft(np.finfo(np.float32).tiny))).astype(ft)
        a = (beta * (l - l.max(1, keepdims=True))).astype(ft)
        b = (beta * (z - z.max(1, keepdims=True))).astype(ft)
        ea, eb = np.exp(a).astype(ft), np.exp(b).astype(ft)
        Sq, Ss = np.zeros(P, ft), np.zeros(P, ft)
        for c in range(K):                                    # classes summed in order
            Sq = (Sq + ea[:, c]).astype(ft)
            Ss = (Ss + eb[:, c]).astype(ft)
        q, s = (ea / Sq[:, None]).astype(ft), (eb / Ss[:, None]).astype(ft)
        lq, ls = (a - np.log(Sq).astype(ft)[:, None]).astype(ft), (b - np.log(Ss).astype(ft)[:, None]).astype(ft)
        kd = np.zeros(P, ft)
        for c in range(K):
            kd = (kd + (q[:, c] * (lq[:, c] - ls[:, c]).astype(ft)).astype(ft)).astype(ft)
        coef = ft(w) * (ft(T) / ft(P))
        g = (coef * (s - q).astype(ft)).astype(ft)
    kd = np.where(fin, kd, ft(np.nan))
    g[~fin] = np.nan
    kd = np.where(used, kd, ft(0.0))
    g[~used] = 0.0
    d = np.zeros((P, C), ft)
    d[:, :K] = g
    term = float(kd.astype(np.float64).sum() * (float(T) * float(T) / P))
    if ft is np.float32:
        term = float(np.float32(term))
    return dict(term=term, loss=w * term, kd=kd, dlogits=d, bias=d.astype(np.float64).sum(0), used=used)


# ---- the entropy term (fcn8s_set_entropy_term, fcn8s_op_entropy_term; the definition is in include/fcn8s_hip.h) --------------------------
ENTROPY_PIXEL_SETS = ('unlabeled', 'valid', 'all')      # the index is the C ABI's pixel_set


def validate_entropy_term(weight=None, pixels='unlabeled', first_image=0):
    """-> (float32 weight (0.0 = off; negative = the confidence penalty), pixel_set 0/1/2, first_image); ValueError for what
    fcn8s_set_entropy_term rejects.  `weight` None or 0 is "off"; `pixels` is 'unlabeled' (label id >= C), 'valid' (< C) or 'all'."""
    if weight is None:
        w = 0.0
    else:
        if isinstance(weight, bool):
            raise ValueError("`weight` must be a number, got {!r}".format(weight))
        try:
            with np.errstate(over='ignore'):
                w = float(np.float32(weight))
        except (TypeError, ValueError):
            raise ValueError("`weight` must be a number, got {!r}".format(weight))
    if not math.isfinite(w):
        raise ValueError("the entropy weight must be finite, got {!r}".format(weight))
    if not isinstance(pixels, str) or pixels not in ENTROPY_PIXEL_SETS:
        raise ValueError("`pixels` must be 'unlabeled', 'valid' or 'all', got {!r}".format(pixels))
    if isinstance(first_image, bool) or not isinstance(first_image, (int, np.integer)) or not 0 <= int(first_image) < 1 << 31:
        raise ValueError("`first_image` must be an integer in [0, 2^31), got {!r}".format(first_image))
    return w, ENTROPY_PIXEL_SETS.index(pixels), int(first_image)


def entropy_restate(logits, labels, weight=1.0, pixels='unlabeled', ncols=None, first_image=0, pixels_per_image=None, dtype=np.float64):
    """The entropy term restated: logits (P, C), labels (P,) ids, K = `ncols` (default C) logical classes, U = the pixels of the images >=
    `first_image` (an image = `pixels_per_image` consecutive pixels; None: the batch is one image) whose label is >= C ('unlabeled'), < C
    ('valid') or anything ('all').  `dtype` float64: the definition in float64 (the reference of the tests); float32: every operation rounded
    to float32 in the kernel's order (classes summed in order, no fused product), h_p summed in float64 -- its distance to the float64 result
    is the scale of what fp32 can be asked for.
    -> dict(term = L_ent, loss = weight * L_ent, h (P,) (0 outside U), dlogits (P, C) = coef (-s (b - m)), m = sum s b, bias (C,) = its column sums
    (float64 sums), used (P,) bool)."""
    w, pset, first = validate_entropy_term(weight, pixels, first_image)
    ft = np.dtype(dtype).type
    if ft not in (np.float64, np.float32):
        raise ValueError("dtype must be float64 or float32")
    z = np.asarray(logits)
    if z.ndim != 2:
        raise ValueError("`logits` must be (P, C), got %s" % (z.shape,))
    P, C = z.shape
    K = C if ncols is None else int(ncols)
    if not 2 <= K <= C:
        raise ValueError("`ncols` must be in 2..%d, got %r" % (C, ncols))
    lab = np.asarray(labels).reshape(-1).astype(np.int64)
    if lab.size != P:
        raise ValueError("`labels` must hold one id per row of `logits` (%d), got %d" % (P, lab.size))
    ppi = P if pixels_per_image is None else int(pixels_per_image)
    if ppi < 1 or P % ppi:
        raise ValueError("`pixels_per_image` must divide the number of pixels (%d), got %r" % (P, pixels_per_image))
    used = np.arange(P) >= min(first, P // ppi) * ppi
    if pset == 0:
        used &= lab >= C
    elif pset == 1:
        used &= lab < C
    z = z[:, :K].astype(ft)
    den = float(P) * math.log(float(K))
    coef = ft(np.float32(w / den)) if ft is np.float32 else ft(w / den)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        b = (z - z.max(1, keepdims=True)).astype(ft)
        e = np.exp(b).astype(ft)
        S = np.zeros(P, ft)
        for c in range(K):                                    # classes summed in order
            S = (S + e[:, c]).astype(ft)
        s = (e / S[:, None]).astype(ft)
        ls = (b - np.log(S).astype(ft)[:, None]).astype(ft)
        acc = np.zeros(P, ft)
        for c in range(K):
            acc = (acc + (s[:, c] * ls[:, c]).astype(ft)).astype(ft)
        h = -acc
        mb = np.zeros(P, ft)                                  # m_p = sum_c s_c b_c: ls_c + h_p is taken as b_c - m_p (see the header)
        for c in range(K):
            mb = (mb + (s[:, c] * b[:, c]).astype(ft)).astype(ft)
        g = (coef * (-(s * (b - mb[:, None]).astype(ft)).astype(ft))).astype(ft)
    h = np.where(used, h, ft(0.0))
    g[~used] = 0.0
    d = np.zeros((P, C), ft)
    d[:, :K] = g
    term = float(h.astype(np.float64).sum() / den)
    if ft is np.float32:
        term = float(np.float32(term))
    return dict(term=term, loss=w * term, h=h, dlogits=d, bias=d.astype(np.float64).sum(0), used=used)


# ---- the focal loss (fcn8s_set_focal, fcn8s_op_focal_xent; the definition is in include/fcn8s_hip.h) -------------------------------------
FOCAL_GAMMA_MAX = 8.0


def validate_focal(gamma, ohem_thresh=None):
    """-> float32 gamma as a float (0.0 = off); ValueError for what fcn8s_set_focal rejects: a gamma that is no number, not finite, negative or
    above 8, and gamma > 0 together with an OHEM threshold (both address the easy pixels; the library refuses the pair with FCN8S_ERR_STATE).
    `gamma` None or 0 is "off"."""
    if gamma is None:
        g = 0.0
    else:
        if isinstance(gamma, bool):
            raise ValueError("`gamma` must be a number, got {!r}".format(gamma))
        try:
            with np.errstate(over='ignore'):
                g = float(np.float32(gamma))
        except (TypeError, ValueError):
            raise ValueError("`gamma` must be a number, got {!r}".format(gamma))
    if not math.isfinite(g) or g < 0.0 or g > FOCAL_GAMMA_MAX:
        raise ValueError("the focal gamma must be 0 (off) or in (0, 8], got {!r}".format(gamma))
    if g > 0.0 and ohem_thresh is not None and ohem_thresh != 0:
        raise ValueError("the focal loss (gamma = {!r}) does not combine with OHEM (ohem_thresh = {!r}): use one of them".format(gamma, ohem_thresh))
    return g


def focal_restate(logits, labels, gamma, class_weights=None, pixel_weights=None, dtype=np.float64, gscale=None):
    """The focal loss restated: logits (P, C), labels (P,) ids (>= C: ignored), `gamma` in (0, 8], `class_weights` (C,) or None (all 1),
    `pixel_weights` (P,) = the float32 b_p of the boundary weighting or None: the weight of a pixel is the float32 product float32(w_{y_p}) * b_p,
    as the kernel forms it.  `dtype` float32: the header's definition step by step, every operation rounded to float32 (classes summed in order, no
    fused product), w_p (f l) summed in float64; float64: the same formulas in double -- the reference of the tests, and its distance to the float32
    form is the scale of what fp32 can be asked for.  `gscale` (default 1 / P, formed in `dtype`) = ce_weight / P of the model.
    -> dict(loss = L_foc, dlogits (P, C), bias (C,) = its column sums (float64 sums), f (P,) = t u, a (P,) (both 0 on ignored pixels), valid (P,) bool)."""
    g = validate_focal(gamma)
    if g == 0.0:
        raise ValueError("gamma = 0 is the plain cross-entropy (loss.restate)")
    ft = np.dtype(dtype).type
    if ft not in (np.float64, np.float32):
        raise ValueError("dtype must be float64 or float32")
    z = np.asarray(logits)
    if z.ndim != 2:
        raise ValueError("`logits` must be (P, C), got %s" % (z.shape,))
    P, C = z.shape
    lab = np.asarray(labels).reshape(-1).astype(np.int64)
    if lab.size != P:
        raise ValueError("`labels` must hold one id per row of `logits` (%d), got %d" % (P, lab.size))
    valid = lab < C
    y = np.where(valid, lab, 0)
    w = np.ones(P, np.float32) if class_weights is None else np.asarray(class_weights, np.float32).reshape(-1)[y]
    if pixel_weights is not None:
        b = np.asarray(pixel_weights, np.float32).reshape(-1)
        if b.size != P:
            raise ValueError("`pixel_weights` must hold one weight per pixel (%d), got %d" % (P, b.size))
        w = (w * b).astype(np.float32)
    w = w.astype(ft)
    gam = ft(g)
    gs = (ft(1.0) / ft(P)) if gscale is None else ft(gscale)
    tiny = ft(np.finfo(np.float32).tiny)                       # FLT_MIN in both forms
    z = z.astype(ft)
    rows = np.arange(P)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore', under='ignore'):
        m = z.max(1)
        e = np.exp((z - m[:, None]).astype(ft)).astype(ft)
        S = np.zeros(P, ft)
        R = np.zeros(P, ft)
        for c in range(C):                                    # classes summed in order; R skips y
            S = (S + e[:, c]).astype(ft)
            R = np.where(y == c, R, (R + e[:, c]).astype(ft))
        l = ((m + np.log(S).astype(ft)).astype(ft) - z[rows, y]).astype(ft)
        u = (R / S).astype(ft)
        sy = (e[rows, y] / S).astype(ft)
        t = np.exp(((gam - ft(1.0)) * np.log(np.maximum(u, tiny)).astype(ft)).astype(ft)).astype(ft)
        f = (t * u).astype(ft)
        a = (t * (u + (gam * (l * sy).astype(ft)).astype(ft)).astype(ft)).astype(ft)
        zero = u == 0
        f = np.where(zero, ft(0.0), f)
        a = np.where(zero, ft(0.0), a)
        fl = (f * l).astype(ft)
        cp = ((gs * w).astype(ft) * a).astype(ft)
        d = (e * (cp / S).astype(ft)[:, None]).astype(ft)
        d[rows, y] = -((cp * u).astype(ft))
    d[~valid] = 0.0
    f = np.where(valid, f, ft(0.0))
    a = np.where(valid, a, ft(0.0))
    loss = float(np.where(valid, w.astype(np.float64) * fl.astype(np.float64), 0.0).sum() / float(P))      # (zeros, not a selection: one summation order)
    if ft is np.float32:
        loss = float(np.float32(loss))
    return dict(loss=loss, dlogits=d, bias=d.astype(np.float64).sum(0), f=f, a=a, valid=valid)
