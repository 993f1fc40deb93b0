"""Official Cityscapes pixel-level scoring of FCN-8s predictions.

`FCN8s.evaluate()` reproduces the reference's in-graph metric -- `tf.metrics.mean_iou` over the 20
train ids *including* void (fcn8s_tensorflow.py:291-293).  The number comparable with the literature is
the 19-class score of `cityscapesscripts/evaluation/evalPixelLevelSemanticLabeling.py`: predictions are
mapped back to label ids, a 34x34 confusion matrix conf[gt, pred] is accumulated over all pixels
(:173-182, native loop addToConfusionMatrix_impl.c:10-16), and per label
    IoU = tp / (tp + fp + fn),   fp counted only on pixels whose ground truth is NOT ignored (:229-255),
averaged over the labels with a defined score (:286-295).

The label table is the reference author's modified one (`cityscapesscripts/helpers/labels.py:62-99`:
trainId 0 = every ignored label, 1..19 = the evaluated classes).  The confusion matrix is accumulated by
the library's HIP kernel when the inputs live on the GPU, by NumPy otherwise.

The instance-level half of the evaluator (`evalInstLevelScore`, on by default there: generateInstanceStats :184-215, the instance
loop of evaluatePair :595-635, getInstanceIouScoreForLabel :258-278, getInstanceIouScoreForCategory :332-351) is here as
`instance_level=True`: per image an exact integer table (v, size, tp, cattp) of the instance values v > 1000 -- counted by
`fcn8s_op_cityscapes_pair` in the same pass as the confusion matrix when the maps are on the GPU (include/fcn8s_hip.h has the definition),
by NumPy otherwise -- and then, on the host for both routes, the evaluator's float64 sums in its own order (`instance_stats_add`).
"""
from __future__ import annotations

import ctypes as C
import fnmatch
import json
import math
import os
from collections import OrderedDict

import numpy as np

#        name                    id  trainId  category        catId  hasInstances ignoreInEval  color
LABELS = [
    ('unlabeled',             0,  0, 'void',          0, False, True,  (0, 0, 0)),
    ('ego vehicle',           1,  0, 'void',          0, False, True,  (0, 0, 0)),
    ('rectification border',  2,  0, 'void',          0, False, True,  (0, 0, 0)),
    ('out of roi',            3,  0, 'void',          0, False, True,  (0, 0, 0)),
    ('static',                4,  0, 'void',          0, False, True,  (0, 0, 0)),
    ('dynamic',               5,  0, 'void',          0, False, True,  (111, 74, 0)),
    ('ground',                6,  0, 'void',          0, False, True,  (81, 0, 81)),
    ('road',                  7,  1, 'flat',          1, False, False, (128, 64, 128)),
    ('sidewalk',              8,  2, 'flat',          1, False, False, (244, 35, 232)),
    ('parking',               9,  0, 'flat',          1, False, True,  (250, 170, 160)),
    ('rail track',           10,  0, 'flat',          1, False, True,  (230, 150, 140)),
    ('building',             11,  3, 'construction',  2, False, False, (70, 70, 70)),
    ('wall',                 12,  4, 'construction',  2, False, False, (102, 102, 156)),
    ('fence',                13,  5, 'construction',  2, False, False, (190, 153, 153)),
    ('guard rail',           14,  0, 'construction',  2, False, True,  (180, 165, 180)),
    ('bridge',               15,  0, 'construction',  2, False, True,  (150, 100, 100)),
    ('tunnel',               16,  0, 'construction',  2, False, True,  (150, 120, 90)),
    ('pole',                 17,  6, 'object',        3, False, False, (153, 153, 153)),
    ('polegroup',            18,  0, 'object',        3, False, True,  (153, 153, 153)),
    ('traffic light',        19,  7, 'object',        3, False, False, (250, 170, 30)),
    ('traffic sign',         20,  8, 'object',        3, False, False, (220, 220, 0)),
    ('vegetation',           21,  9, 'nature',        4, False, False, (107, 142, 35)),
    ('terrain',              22, 10, 'nature',        4, False, False, (152, 251, 152)),
    ('sky',                  23, 11, 'sky',           5, False, False, (70, 130, 180)),
    ('person',               24, 12, 'human',         6, True,  False, (220, 20, 60)),
    ('rider',                25, 13, 'human',         6, True,  False, (255, 0, 0)),
    ('car',                  26, 14, 'vehicle',       7, True,  False, (0, 0, 142)),
    ('truck',                27, 15, 'vehicle',       7, True,  False, (0, 0, 70)),
    ('bus',                  28, 16, 'vehicle',       7, True,  False, (0, 60, 100)),
    ('caravan',              29,  0, 'vehicle',       7, True,  True,  (0, 0, 90)),
    ('trailer',              30,  0, 'vehicle',       7, True,  True,  (0, 0, 110)),
    ('train',                31, 17, 'vehicle',       7, True,  False, (0, 80, 100)),
    ('motorcycle',           32, 18, 'vehicle',       7, True,  False, (0, 0, 230)),
    ('bicycle',              33, 19, 'vehicle',       7, True,  False, (119, 11, 32)),
    ('license plate',        -1,  0, 'vehicle',       7, False, True,  (0, 0, 142)),
]
NUM_IDS = 34                                                   # label ids 0..33 (license plate has id -1)

# labels.py:185-192 -- id -> trainId (35 entries; the last one is the -1 label) and trainId -> id
IDS_TO_TRAINIDS_ARRAY = np.zeros(35, np.uint8)
for _n, _id, _tid, *_rest in LABELS:
    IDS_TO_TRAINIDS_ARRAY[_id] = _tid
TRAINIDS_TO_IDS_ARRAY = np.zeros(20, np.uint8)
for _n, _id, _tid, *_rest in LABELS:
    if _tid > 0:
        TRAINIDS_TO_IDS_ARRAY[_tid] = _id
# labels.py:218 -- overlay colours for predict_and_save (alpha 127; void transparent)
TRAINIDS_TO_RGBA_DICT = {0: (0, 0, 0, 0)}
TRAINIDS_TO_RGBA_DICT.update({tid: tuple(col) + (127,) for _n, _id, tid, _c, _ci, _h, _ig, col in LABELS if tid > 0})

IGNORED_IDS = np.array([i for _n, i, *_r in LABELS if i >= 0 and _r[4]], dtype=np.int64)
EVAL_IDS = np.array([i for _n, i, *_r in LABELS if i >= 0 and not _r[4]], dtype=np.int64)       # the 19 evaluated labels
ID_TO_NAME = {i: n for n, i, *_r in LABELS}
CATEGORY_TO_IDS = OrderedDict()
for _n, _id, _tid, _cat, *_r in LABELS:
    if _id >= 0:
        CATEGORY_TO_IDS.setdefault(_cat, []).append(_id)


def confusion_add(conf, gt_ids, pred_ids):
    """conf[gt, pred] += 1 over all pixels.  gt_ids / pred_ids: label-id maps of equal shape (NumPy, or torch
    tensors on the GPU: then the library's confusion kernel is used); conf: (34, 34) int64 array, updated in place."""
    try:
        import torch
        on_gpu = isinstance(gt_ids, torch.Tensor) and gt_ids.is_cuda
    except Exception:
        on_gpu = False
    if on_gpu:
        import torch
        from . import _lib as L
        g = gt_ids.to(torch.uint8).contiguous().view(-1)
        p = pred_ids.to(device=g.device, dtype=torch.int64).contiguous().view(-1)
        d = torch.zeros(NUM_IDS * NUM_IDS, dtype=torch.int64, device=g.device)
        stream = C.c_void_p(torch.cuda.current_stream(g.device).cuda_stream)
        L.check(L.lib.fcn8s_op_confusion(stream, C.c_void_p(g.data_ptr()), C.c_void_p(p.data_ptr()), g.numel(),
                                         C.c_void_p(d.data_ptr()), NUM_IDS))
        conf += d.cpu().numpy().reshape(NUM_IDS, NUM_IDS)
        return conf
    g = np.asarray(gt_ids).astype(np.int64).ravel(); p = np.asarray(pred_ids).astype(np.int64).ravel()
    ok = (g >= 0) & (g < NUM_IDS) & (p >= 0) & (p < NUM_IDS)
    conf += np.bincount(g[ok] * NUM_IDS + p[ok], minlength=NUM_IDS * NUM_IDS).reshape(NUM_IDS, NUM_IDS)
    return conf


def iou_for_label(label, conf):
    """evalPixelLevelSemanticLabeling.py:229-255"""
    if label in IGNORED_IDS:
        return float('nan')
    tp = int(conf[label, label])
    fn = int(conf[label, :].sum()) - tp
    not_ignored = [l for l in EVAL_IDS if l != label]
    fp = int(conf[not_ignored, label].sum())
    denom = tp + fp + fn
    return float('nan') if denom == 0 else tp / denom


def iou_for_category(category, conf):
    """evalPixelLevelSemanticLabeling.py:298-335: tp/fn over the category's non-ignored labels, fp from every other
    non-ignored label predicted as one of them."""
    ids = [l for l in CATEGORY_TO_IDS[category] if l not in IGNORED_IDS]
    if not ids:
        return float('nan')
    tp = int(conf[np.ix_(ids, ids)].sum())
    fn = int(conf[ids, :].sum()) - tp
    others = [l for l in EVAL_IDS if l not in ids]
    fp = int(conf[np.ix_(others, ids)].sum())
    denom = tp + fp + fn
    return float('nan') if denom == 0 else tp / denom


def score_average(scores):
    """nan-aware mean (:286-295)"""
    vals = [s for s in scores.values() if not math.isnan(s)]
    return float('nan') if not vals else sum(vals) / len(vals)


# ---------------------------------------------------------------------------------------------------------
# instance-level scores (iIoU)
# ---------------------------------------------------------------------------------------------------------
AVG_CLASS_SIZE = {                                             # evalPixelLevelSemanticLabeling.py:148-159
    "bicycle":     4672.3249222261,
    "caravan":    36771.8241758242,
    "motorcycle":  6298.7200839748,
    "rider":       3930.4788056518,
    "bus":        35732.1511111111,
    "train":      67583.7075812274,
    "car":        12794.0202738185,
    "person":      3462.4756337644,
    "truck":      27855.1264367816,
    "trailer":    16926.9763313609,
}
HAS_INSTANCES_IDS = [i for _n, i, _t, _c, _ci, has, _ig, _col in LABELS if i >= 0 and has]
INSTANCE_LABEL_IDS = [i for i in HAS_INSTANCES_IDS if i not in IGNORED_IDS]           # person .. bicycle without caravan / trailer
ID_TO_CATEGORY = {i: c for _n, i, _t, c, *_r in LABELS}
# generateInstanceStats :195-213: the categories all of whose labels (id >= 0) have instances, with ALL those ids (ignored ones included)
INSTANCE_CATEGORY_TO_IDS = OrderedDict((c, ids) for c, ids in CATEGORY_TO_IDS.items() if all(i in HAS_INSTANCES_IDS for i in ids))
DEFAULT_MAX_ENTRIES = 1024                                     # per image; a Cityscapes image holds a few hundred instances at most


def new_instance_stats():
    """generateInstanceStats (:184-215)"""
    zero = lambda: OrderedDict((k, 0.0) for k in ("tp", "tpWeighted", "fn", "fnWeighted"))
    return {"classes": OrderedDict((ID_TO_NAME[l], zero()) for l in INSTANCE_LABEL_IDS),
            "categories": OrderedDict((c, zero()) for c in INSTANCE_CATEGORY_TO_IDS)}


def instance_value_kind(v):
    """What the evaluator does with a value v > 1000 of an instance map: 'count', 'skip' (ignoreInEval, :605) or 'bad' (its KeyError:
    an evaluated label without instances, or no label at all)."""
    label = int(v) // 1000
    if label in INSTANCE_LABEL_IDS:
        return 'count'
    return 'skip' if label in IGNORED_IDS else 'bad'


def _bad_instance_value(v):
    return ValueError("Instance id {} in the ground truth: label {} is evaluated but has no instances (or does not exist).".format(int(v), int(v) // 1000))


def instance_entries_numpy(pred_ids, inst):
    """The integer half of the instance loop (:601-635) for one image: int64 rows (v, size, tp, cattp), ascending v, for the values
    v > 1000 of `inst` whose label is counted.  pred_ids: label ids of the same shape."""
    inst = np.asarray(inst); pred_ids = np.asarray(pred_ids)
    if inst.shape != pred_ids.shape:
        raise ValueError("Instance map of shape {} against a prediction of shape {}.".format(inst.shape, pred_ids.shape))
    sel = inst > 1000
    v = inst[sel].astype(np.int64); p = pred_ids[sel].astype(np.int64)
    vals = np.unique(v)
    kinds = [instance_value_kind(x) for x in vals]
    for x, k in zip(vals, kinds):
        if k == 'bad':
            raise _bad_instance_value(x)
    n = int(vals.max()) + 1 if vals.size else 0
    lab = v // 1000
    incat = np.zeros(v.shape, bool)
    for ids in INSTANCE_CATEGORY_TO_IDS.values():
        incat |= np.isin(lab, ids) & np.isin(p, ids)
    size = np.bincount(v, minlength=n); tp = np.bincount(v[p == lab], minlength=n); cattp = np.bincount(v[incat], minlength=n)
    keep = np.array([x for x, k in zip(vals, kinds) if k == 'count'], np.int64)
    return np.stack([keep, size[keep], tp[keep], cattp[keep]], axis=1).astype(np.int64) if keep.size else np.zeros((0, 4), np.int64)


def instance_stats_add(stats, entries):
    """The float64 half of the instance loop (:609-635) for one image's rows (v, size, tp, cattp) in ascending v: the evaluator's own
    operations in its own order, so the sums carry its bits whichever route counted the integers."""
    for v, size, tp, cattp in np.asarray(entries, dtype=np.int64).reshape(-1, 4).tolist():
        label = v // 1000
        name = ID_TO_NAME[label]
        weight = AVG_CLASS_SIZE[name] / float(size)
        c = stats["classes"][name]
        fn = size - tp
        c["tp"] += tp; c["fn"] += fn
        c["tpWeighted"] += float(tp) * weight; c["fnWeighted"] += float(fn) * weight
        category = ID_TO_CATEGORY[label]
        if category in stats["categories"]:
            k = stats["categories"][category]
            catfn = size - cattp
            k["tp"] += cattp; k["fn"] += catfn
            k["tpWeighted"] += float(cattp) * weight; k["fnWeighted"] += float(catfn) * weight
    return stats


def instance_iou_for_label(label, conf, stats):
    """getInstanceIouScoreForLabel (:258-278)"""
    if label in IGNORED_IDS or ID_TO_NAME[label] not in stats["classes"]:
        return float('nan')
    tp = stats["classes"][ID_TO_NAME[label]]["tpWeighted"]
    fn = stats["classes"][ID_TO_NAME[label]]["fnWeighted"]
    not_ignored = [l for l in EVAL_IDS if l != label]
    fp = int(conf[not_ignored, label].sum())
    denom = tp + fp + fn
    return float('nan') if denom == 0 else float(tp) / denom


def instance_iou_for_category(category, conf, stats):
    """getInstanceIouScoreForCategory (:332-351)"""
    if category not in stats["categories"]:
        return float('nan')
    ids = INSTANCE_CATEGORY_TO_IDS[category]
    tp = stats["categories"][category]["tpWeighted"]
    fn = stats["categories"][category]["fnWeighted"]
    others = [l for l in EVAL_IDS if ID_TO_CATEGORY[int(l)] != category]
    fp = int(conf[np.ix_(others, ids)].sum())
    denom = tp + fp + fn
    return float('nan') if denom == 0 else float(tp) / denom


def _is_cuda_tensor(x):
    try:
        import torch
    except ImportError:
        return False
    return isinstance(x, torch.Tensor) and x.is_cuda


def pair_counts_device(pred, gt_label_ids, gt_instance_ids=None, max_entries=DEFAULT_MAX_ENTRIES):
    """One `fcn8s_op_cityscapes_pair` call on maps that live on the GPU: `pred` int64 train ids (as `predict` returns them; consumed as
    they are) or uint8 label ids, `gt_label_ids` uint8, `gt_instance_ids` 16-bit (torch.int16 holding the uint16 bits, or torch.uint16) or
    None; shapes (H, W) or (N, H, W).  Returns (conf (34, 34) int64 ndarray of this call, [entries (K_n, 4) int64 per image] or None).
    Only the matrix, the three counters per image and the entries come back to the host.  More instances than `max_entries` in an image:
    the call is repeated once with the reported count."""
    import torch
    from . import _lib as L
    dev = pred.device
    if pred.dtype == torch.int64:
        kind = 0
    elif pred.dtype == torch.uint8:
        kind = 1
    else:
        raise ValueError("`pred` must hold int64 train ids or uint8 label ids, not {}".format(pred.dtype))
    if gt_label_ids.dtype != torch.uint8:
        raise ValueError("`gt_label_ids` must be uint8, not {}".format(gt_label_ids.dtype))
    if tuple(gt_label_ids.shape) != tuple(pred.shape) or pred.dim() not in (2, 3):
        raise ValueError("prediction of shape {} against ground truth of shape {}".format(tuple(pred.shape), tuple(gt_label_ids.shape)))
    N = 1 if pred.dim() == 2 else int(pred.shape[0])
    P = pred.numel() // max(N, 1)
    pred = pred.contiguous(); gt = gt_label_ids.to(dev).contiguous()
    inst = None
    if gt_instance_ids is not None:
        inst = gt_instance_ids.to(dev)
        if inst.element_size() != 2 or inst.is_floating_point():
            raise ValueError("`gt_instance_ids` must be a 16-bit integer tensor (the uint16 instance map's bits), not {}".format(inst.dtype))
        if tuple(inst.shape) != tuple(pred.shape):
            raise ValueError("instance map of shape {} against a prediction of shape {}".format(tuple(inst.shape), tuple(pred.shape)))
        inst = inst.contiguous()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    counts = torch.empty((N, 3), dtype=torch.int64, device=dev)
    work = torch.empty(L.lib.fcn8s_op_cityscapes_work_bytes(N), dtype=torch.uint8, device=dev) if inst is not None else None
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    for _attempt in range(2):
        conf = torch.zeros(NUM_IDS * NUM_IDS, dtype=torch.int64, device=dev)
        entries = torch.empty((N, max(int(max_entries), 1), 4), dtype=torch.int32, device=dev) if inst is not None else None
        L.check(L.lib.fcn8s_op_cityscapes_pair(stream, ptr(gt), ptr(inst), ptr(pred), kind, N, P, ptr(conf), ptr(work), ptr(entries),
                                               int(max_entries), ptr(counts)))
        cnt = counts.cpu().numpy()
        if int(cnt[:, 0].max()) <= max_entries:
            break
        max_entries = int(cnt[:, 0].max())
    if cnt[:, 1].any():
        bad_gt = int(gt.max()) >= NUM_IDS
        raise ValueError("Unknown label with id {:}".format(int(gt.max())) if bad_gt else
                         "{} predicted pixels hold an id outside the {}".format(int(cnt[:, 1].sum()), "train ids 0..19" if kind == 0 else "label ids 0..33"))
    if cnt[:, 2].any():
        vals = torch.unique(inst.view(torch.int16).to(torch.int32) & 0xFFFF).cpu().numpy()
        raise _bad_instance_value([v for v in vals if v > 1000 and instance_value_kind(v) == 'bad'][0])
    conf_np = conf.cpu().numpy().reshape(NUM_IDS, NUM_IDS)
    if inst is None:
        return conf_np, None
    e = entries[:, :max(int(cnt[:, 0].max()), 1)].cpu().numpy().astype(np.int64)
    return conf_np, [e[n, :int(cnt[n, 0])] for n in range(N)]


def pair_counts_numpy(pred, gt_label_ids, gt_instance_ids=None, pred_is_train_ids=True):
    """The NumPy route of the same definition, for one image or a stack of them: (conf (34, 34) int64, [entries per image] or None)."""
    pred = np.asarray(pred); gt = np.asarray(gt_label_ids)
    if pred.shape != gt.shape or pred.ndim not in (2, 3):
        raise ValueError("prediction of shape {} against ground truth of shape {}".format(pred.shape, gt.shape))
    if pred.size and (pred.min() < 0 or pred.max() >= (20 if pred_is_train_ids else NUM_IDS)):
        raise ValueError("predicted pixels hold an id outside the {}".format("train ids 0..19" if pred_is_train_ids else "label ids 0..33"))
    if gt.size and gt.max() >= NUM_IDS:
        raise ValueError("Unknown label with id {:}".format(int(gt.max())))
    pred_ids = TRAINIDS_TO_IDS_ARRAY[pred.astype(np.int64)] if pred_is_train_ids else pred
    conf = confusion_add(np.zeros((NUM_IDS, NUM_IDS), np.int64), gt, pred_ids)
    if gt_instance_ids is None:
        return conf, None
    inst = np.asarray(gt_instance_ids)
    if inst.shape != pred.shape:
        raise ValueError("instance map of shape {} against a prediction of shape {}".format(inst.shape, pred.shape))
    if pred.ndim == 2:
        return conf, [instance_entries_numpy(pred_ids, inst)]
    return conf, [instance_entries_numpy(pred_ids[n], inst[n]) for n in range(pred.shape[0])]


# ---------------------------------------------------------------------------------------------------------
# boundary measures: trimap IoU and boundary F-score
# ---------------------------------------------------------------------------------------------------------
# IoU over all pixels is dominated by the interiors of road, building and sky; a CRF or a test-time ensemble moves a few pixels around
# every contour.  Two measures look only there (the definition, all integers, is in include/fcn8s_hip.h at fcn8s_op_boundary_pair):
#   trimap IoU (Kraehenbuehl & Koltun 2011; Chen et al. 2015): the IoU restricted to the pixels within r of a ground-truth boundary;
#   boundary F-score (Csurka et al., BMVC 2013): precision / recall of the predicted against the true contours of a class under a
#   distance tolerance.
# The counts are taken by `fcn8s_op_boundary_pair` when the maps are on the GPU, by NumPy otherwise; the scores are float64 on the host.
MAX_BOUNDARY_RADIUS = 16
BAD_ID = 255                                                   # what an id out of range takes part as


def _check_radius(radius):
    R = int(radius)
    if R != radius or not 1 <= R <= MAX_BOUNDARY_RADIUS:
        raise ValueError("`boundary_radius` must be an integer in 1..{}, not {!r}".format(MAX_BOUNDARY_RADIUS, radius))
    return R


def ring_of(d2, R):
    """Smallest k >= 0 with k*k >= d2, R + 1 beyond R (and for 'nothing found', any d2 > R*R)."""
    d2 = np.asarray(d2)
    k = np.full(d2.shape, R + 1, np.int64)
    for r in range(R, -1, -1):
        k[d2 <= r * r] = r
    return k


def boundary_set(M):
    """B(M): the pixels with a 4-neighbour inside the image that holds another value."""
    M = np.asarray(M)
    b = np.zeros(M.shape, bool)
    v = M[:-1] != M[1:]; b[:-1] |= v; b[1:] |= v
    h = M[:, :-1] != M[:, 1:]; b[:, :-1] |= h; b[:, 1:] |= h
    return b


def _half_disk(R):
    """The offsets (d2, dy, dx) of one half of the disk of radius R without its centre (the other half is their negatives), ascending d2."""
    return sorted((dy * dy + dx * dx, dy, dx) for dy in range(0, R + 1) for dx in range(-R, R + 1)
                  if (dy > 0 or dx > 0) and dy * dy + dx * dx <= R * R)


def _nearest_other_label(G, R):
    """d2(p) = min |q - p|^2 over q != p inside the image with G[q] != G[p], R*R + 1 if there is none within R: shifted array
    comparisons over the disk's offsets in ascending distance (a pair p, q that differs is a hit for both of them)."""
    H, W = G.shape
    big = R * R + 1
    d2 = np.full((H, W), big, np.uint16)
    for dd, dy, dx in _half_disk(R):
        if dy >= H or abs(dx) >= W:
            continue
        a = (slice(0, H - dy), slice(max(0, -dx), W - max(0, dx)))                 # p
        b = (slice(dy, H), slice(max(0, dx), W - max(0, -dx)))                     # q = p + (dy, dx)
        hit = G[a] != G[b]
        val = np.where(hit, np.uint16(dd), np.uint16(big))
        np.minimum(d2[a], val, out=d2[a]); np.minimum(d2[b], val, out=d2[b])
    return d2.astype(np.int64)


def _nearest_contour_of_class(src, src_sel, tgt, tgt_b, R):
    """For every pixel p of the mask `src_sel` with c = src[p]: min |q - p|^2 over q in tgt_b with tgt[q] == c (q = p allowed), R*R + 1 if
    none within R.  Returns (classes, d2) over the selected pixels in np.nonzero order; only those pixels are searched."""
    H, W = src.shape
    ys, xs = np.nonzero(src_sel)
    c = src[ys, xs]
    big = R * R + 1
    d2 = np.full(c.shape, big, np.int64)
    pad = np.full((H + 2 * R, W + 2 * R), 254, np.uint8)                             # 254: no contour pixel of any class here
    pad[R:R + H, R:R + W] = np.where(tgt_b, tgt, 254)
    idx = np.arange(c.size)
    half = _half_disk(R)
    offsets = sorted([(0, 0, 0)] + half + [(dd, -dy, -dx) for dd, dy, dx in half])
    for dd, dy, dx in offsets:
        if idx.size == 0:
            break
        hit = pad[ys[idx] + (R + dy), xs[idx] + (R + dx)] == c[idx]
        d2[idx[hit]] = dd                                                         # ascending: the first hit is the nearest
        idx = idx[~hit]
    return c, d2


def boundary_tables_numpy(G, P, R):
    """The definition for ONE image on label-id maps (uint8, an id out of range already replaced by BAD_ID = 255):
    (rings [R + 1, 34, 34], bprec [R + 2, 34], brec [R + 2, 34], bad), int64."""
    G = np.ascontiguousarray(G, dtype=np.uint8); P = np.ascontiguousarray(P, dtype=np.uint8)
    if G.ndim != 2 or G.shape != P.shape or G.size == 0:
        raise ValueError("ground truth of shape {} against a prediction of shape {}".format(G.shape, P.shape))
    ok = (G < NUM_IDS) & (P < NUM_IDS)
    g = G[ok].astype(np.int64); p = P[ok].astype(np.int64)
    k = ring_of(_nearest_other_label(G, R), R)[ok]
    rings = np.bincount((k - 1) * NUM_IDS * NUM_IDS + g * NUM_IDS + p, minlength=(R + 1) * NUM_IDS * NUM_IDS).reshape(R + 1, NUM_IDS, NUM_IDS)
    BG, BP = boundary_set(G), boundary_set(P)
    c, e2 = _nearest_contour_of_class(P, BP & ok, G, BG, R)
    bprec = np.bincount(ring_of(e2, R) * NUM_IDS + c, minlength=(R + 2) * NUM_IDS).reshape(R + 2, NUM_IDS)
    c, e2 = _nearest_contour_of_class(G, BG & ok, P, BP, R)
    brec = np.bincount(ring_of(e2, R) * NUM_IDS + c, minlength=(R + 2) * NUM_IDS).reshape(R + 2, NUM_IDS)
    return rings.astype(np.int64), bprec.astype(np.int64), brec.astype(np.int64), int(ok.size - ok.sum())


def boundary_counts_numpy(pred, gt, radius, pred_is_train_ids=True):
    """The NumPy route of fcn8s_op_boundary_pair's definition for one image (H, W) or a stack (N, H, W): `pred` train ids 0..19 (or, with
    `pred_is_train_ids=False`, label ids 0..33) against the label ids `gt`.  Returns the int64 tables (rings [R + 1, 34, 34],
    bprec [R + 2, 34], brec [R + 2, 34]) summed over the images.  An id out of range is refused."""
    R = _check_radius(radius)
    pred = np.asarray(pred); gt = np.asarray(gt)
    if pred.shape != gt.shape or pred.ndim not in (2, 3) or pred.size == 0:
        raise ValueError("prediction of shape {} against ground truth of shape {}".format(pred.shape, gt.shape))
    if pred.min() < 0 or pred.max() >= (20 if pred_is_train_ids else NUM_IDS):
        raise ValueError("predicted pixels hold an id outside the {}".format("train ids 0..19" if pred_is_train_ids else "label ids 0..33"))
    if gt.min() < 0 or gt.max() >= NUM_IDS:
        raise ValueError("Unknown label with id {:}".format(int(gt.max())))
    ids = TRAINIDS_TO_IDS_ARRAY[pred.astype(np.int64)] if pred_is_train_ids else pred.astype(np.uint8)
    gt = gt.astype(np.uint8)
    if pred.ndim == 2:
        ids, gt = ids[None], gt[None]
    rings = np.zeros((R + 1, NUM_IDS, NUM_IDS), np.int64); bprec = np.zeros((R + 2, NUM_IDS), np.int64); brec = np.zeros((R + 2, NUM_IDS), np.int64)
    for n in range(ids.shape[0]):
        r, bp, br, _bad = boundary_tables_numpy(gt[n], ids[n], R)
        rings += r; bprec += bp; brec += br
    return rings, bprec, brec


def boundary_counts_device(pred, gt_label_ids, radius):
    """One `fcn8s_op_boundary_pair` call on maps that live on the GPU: `pred` int64 train ids (as `predict` returns them) or uint8 label
    ids, `gt_label_ids` uint8, shapes (H, W) or (N, H, W).  Returns the int64 ndarrays (rings, bprec, brec) of this call, summed over the
    images; only they and the count of out-of-range pixels come back to the host.  An id out of range is refused."""
    import torch
    from . import _lib as L
    R = _check_radius(radius)
    dev = pred.device
    if pred.dtype == torch.int64:
        kind = 0
    elif pred.dtype == torch.uint8:
        kind = 1
    else:
        raise ValueError("`pred` must hold int64 train ids or uint8 label ids, not {}".format(pred.dtype))
    if gt_label_ids.dtype != torch.uint8:
        raise ValueError("`gt_label_ids` must be uint8, not {}".format(gt_label_ids.dtype))
    if tuple(gt_label_ids.shape) != tuple(pred.shape) or pred.dim() not in (2, 3) or pred.numel() == 0:
        raise ValueError("prediction of shape {} against ground truth of shape {}".format(tuple(pred.shape), tuple(gt_label_ids.shape)))
    N = 1 if pred.dim() == 2 else int(pred.shape[0])
    H, W = int(pred.shape[-2]), int(pred.shape[-1])
    pred = pred.contiguous(); gt = gt_label_ids.to(dev).contiguous()
    nr, nb = (R + 1) * NUM_IDS * NUM_IDS, (R + 2) * NUM_IDS
    out = torch.zeros(nr + 2 * nb + 1, dtype=torch.int64, device=dev)                # rings | bprec | brec | bad: one clear, one download
    base = out.data_ptr()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    L.check(L.lib.fcn8s_op_boundary_pair(stream, C.c_void_p(gt.data_ptr()), C.c_void_p(pred.data_ptr()), kind, N, H, W, R, C.c_void_p(base),
                                         C.c_void_p(base + 8 * nr), C.c_void_p(base + 8 * (nr + nb)), C.c_void_p(base + 8 * (nr + 2 * nb))))
    o = out.cpu().numpy()
    if o[-1]:
        bad_gt = int(gt.max()) >= NUM_IDS
        raise ValueError("Unknown label with id {:}".format(int(gt.max())) if bad_gt else
                         "{} predicted pixels hold an id outside the {}".format(int(o[-1]), "train ids 0..19" if kind == 0 else "label ids 0..33"))
    return o[:nr].reshape(R + 1, NUM_IDS, NUM_IDS).copy(), o[nr:nr + nb].reshape(R + 2, NUM_IDS).copy(), o[nr + nb:nr + 2 * nb].reshape(R + 2, NUM_IDS).copy()


def trimap_scores(rings):
    """Trimap IoU from a rings table [R + 1, 34, 34]: the evaluator's own scores (`iou_for_label`, `iou_for_category`, `score_average`) on
    the confusion matrix of the pixels within r of a ground-truth boundary, i.e. on the sum of the first r ring matrices.  Every list has
    R + 1 entries: index r - 1 is the band of width r = 1..R, the last one is the whole image (all rings: the ordinary IoU)."""
    rings = np.asarray(rings)
    if rings.ndim != 3 or rings.shape[1:] != (NUM_IDS, NUM_IDS) or rings.shape[0] < 2:
        raise ValueError("a rings table is [R + 1, 34, 34], not {}".format(rings.shape))
    bands = np.cumsum(rings.astype(np.int64), axis=0)
    cls = [OrderedDict((ID_TO_NAME[l], iou_for_label(l, b)) for l in range(NUM_IDS)) for b in bands]
    cat = [OrderedDict((c, iou_for_category(c, b)) for c in CATEGORY_TO_IDS) for b in bands]
    return {"trimapScoreClasses": [score_average(s) for s in cls],
            "trimapScoreCategories": [score_average(s) for s in cat],
            "trimapClassScores": OrderedDict((ID_TO_NAME[l], [s[ID_TO_NAME[l]] for s in cls]) for l in range(NUM_IDS))}


def boundary_f_scores(bprec, brec):
    """Boundary F-score from the tables bprec / brec [R + 2, 34].  For label c and tolerance t = 0..R: precision = sum(bprec[0..t, c]) /
    sum(bprec[:, c]) (the share of c's predicted contour pixels that lie within t of a true contour pixel of c), recall likewise from brec,
    F = 2 P R / (P + R); NaN where a denominator is 0 and for the labels the evaluation ignores.  `boundaryFScoreClasses[t]` is the mean
    over the evaluated labels whose F is not NaN.  The counts are accumulated over all images before the division (the dataset-level
    protocol of the Cityscapes IoU), not averaged per image as Csurka et al. do."""
    bprec = np.asarray(bprec).astype(np.int64); brec = np.asarray(brec).astype(np.int64)
    if bprec.ndim != 2 or bprec.shape[1] != NUM_IDS or bprec.shape[0] < 3 or brec.shape != bprec.shape:
        raise ValueError("bprec / brec are [R + 2, 34] tables, not {} / {}".format(bprec.shape, brec.shape))
    R = bprec.shape[0] - 2
    nan = float('nan')
    per = OrderedDict()
    for l in range(NUM_IDS):
        if l in IGNORED_IDS:
            per[ID_TO_NAME[l]] = OrderedDict((k, [nan] * (R + 1)) for k in ("precision", "recall", "f"))
            continue
        np_, nr_ = int(bprec[:, l].sum()), int(brec[:, l].sum())
        hp, hr = np.cumsum(bprec[:R + 1, l]), np.cumsum(brec[:R + 1, l])
        prec = [int(h) / np_ if np_ else nan for h in hp]
        rec = [int(h) / nr_ if nr_ else nan for h in hr]
        f = [nan if (math.isnan(a) or math.isnan(b) or a + b == 0) else 2 * a * b / (a + b) for a, b in zip(prec, rec)]
        per[ID_TO_NAME[l]] = OrderedDict((("precision", prec), ("recall", rec), ("f", f)))
    mean = [score_average({n: s["f"][t] for n, s in per.items()}) for t in range(R + 1)]
    return {"boundaryFScoreClasses": mean, "boundaryClassScores": per}


class PixelLevelEvaluator:
    """Accumulates the official confusion matrix from FCN-8s predictions (train ids, as `FCN8s.predict`
    returns them) and Cityscapes `*_gtFine_labelIds` ground truth, and reports the 19-class scores; with `instance_level`, the
    instance statistics from `*_gtFine_instanceIds` maps and the iIoU scores as well (the evaluator's default table); with
    `boundary_radius=R` (1..16), the trimap IoU for the band widths 1..R and the boundary F-score for the tolerances 0..R as well; with
    `panoptic=4` or `8` (needs `instance_level`), panoptic quality with the predicted things split into connected components of that
    connectivity (panoptic.py has the definition and its caveat)."""

    def __init__(self, instance_level=False, boundary_radius=None, panoptic=None):
        self.conf = np.zeros((NUM_IDS, NUM_IDS), np.int64)
        self.instance_level = bool(instance_level)
        self.inst_stats = new_instance_stats() if self.instance_level else None
        self.boundary_radius = None if boundary_radius is None else _check_radius(boundary_radius)
        if self.boundary_radius is not None:
            R = self.boundary_radius
            self.rings = np.zeros((R + 1, NUM_IDS, NUM_IDS), np.int64)
            self.bprec = np.zeros((R + 2, NUM_IDS), np.int64)
            self.brec = np.zeros((R + 2, NUM_IDS), np.int64)
        self.panoptic = _check_panoptic(panoptic, self.instance_level)
        if self.panoptic is not None:
            from . import panoptic as pq
            self.panoptic_stats = pq.new_stats()
            self._panoptic_work = None

    def add_panoptic_rows(self, rows, bad):
        """The rows of `panoptic.pair_rows_numpy` / `pair_rows_device` for one image or a list of images, in file order."""
        from . import panoptic as pq
        if isinstance(rows, np.ndarray):
            rows, bad = [rows], [bad]
        if int(np.sum(bad)):
            raise ValueError("{} pixels of the instance map hold a value whose label is beyond 33 (or the prediction an id out of range).".format(int(np.sum(bad))))
        for r in rows:
            pq.stats_add(self.panoptic_stats, r)

    def add_boundary_tables(self, tables):
        rings, bprec, brec = tables
        self.rings += rings; self.bprec += bprec; self.brec += brec

    def add(self, pred_train_ids, gt_label_ids, gt_instance_ids=None, pred_is_train_ids=True, max_entries=DEFAULT_MAX_ENTRIES):
        """One image (H, W) or a stack (N, H, W).  Maps on the GPU (torch tensors; the prediction decides) are counted there by one
        `fcn8s_op_cityscapes_pair` call and stay there; NumPy maps are counted by NumPy.  `pred_is_train_ids=False`: `pred_train_ids`
        holds label ids 0..33 (uint8 on the GPU) instead."""
        if self.instance_level and gt_instance_ids is None:
            raise ValueError("an instance-level evaluation needs the ground truth's instance-id map (*_gtFine_instanceIds.png)")
        if not self.instance_level:
            gt_instance_ids = None
        if _is_cuda_tensor(pred_train_ids):
            import torch
            pred = pred_train_ids
            if pred_is_train_ids and pred.dtype != torch.int64:
                pred = pred.long()
            elif not pred_is_train_ids and pred.dtype != torch.uint8:
                raise ValueError("label ids on the GPU must be uint8")
            gt = gt_label_ids if isinstance(gt_label_ids, torch.Tensor) else torch.as_tensor(np.asarray(gt_label_ids))
            gt = gt.to(device=pred.device, dtype=torch.uint8)
            inst = gt_instance_ids
            if inst is not None and not isinstance(inst, torch.Tensor):
                inst = instance_map_tensor(inst, pred.device)
            conf, entries = pair_counts_device(pred, gt, inst, max_entries)
            if self.boundary_radius is not None:
                self.add_boundary_tables(boundary_counts_device(pred, gt, self.boundary_radius))
            if self.panoptic is not None:
                from . import panoptic as pq
                rows, bad, self._panoptic_work = pq.pair_rows_device(pred, inst, connectivity=self.panoptic, work=self._panoptic_work)
                self.add_panoptic_rows(rows, bad)
        else:
            to_np = lambda a: a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
            inst = None
            if gt_instance_ids is not None:
                inst = to_np(gt_instance_ids)
                if inst.dtype == np.int16:
                    inst = inst.view(np.uint16)
            conf, entries = pair_counts_numpy(to_np(pred_train_ids), to_np(gt_label_ids), inst, pred_is_train_ids)
            if self.boundary_radius is not None:
                self.add_boundary_tables(boundary_counts_numpy(to_np(pred_train_ids), to_np(gt_label_ids), self.boundary_radius, pred_is_train_ids))
            if self.panoptic is not None:
                from . import panoptic as pq
                self.add_panoptic_rows(*pq.pair_rows_numpy(to_np(pred_train_ids), inst, self.panoptic, pred_is_train_ids))
        self.conf += conf
        if entries is not None:
            for e in entries:
                instance_stats_add(self.inst_stats, e)

    def class_scores(self):
        return OrderedDict((ID_TO_NAME[int(l)], iou_for_label(int(l), self.conf)) for l in range(NUM_IDS))

    def category_scores(self):
        return OrderedDict((c, iou_for_category(c, self.conf)) for c in CATEGORY_TO_IDS)

    def class_inst_scores(self):
        return OrderedDict((ID_TO_NAME[int(l)], instance_iou_for_label(int(l), self.conf, self.inst_stats)) for l in range(NUM_IDS))

    def category_inst_scores(self):
        return OrderedDict((c, instance_iou_for_category(c, self.conf, self.inst_stats)) for c in CATEGORY_TO_IDS)

    def results(self):
        cs, cat = self.class_scores(), self.category_scores()
        res = {"classScores": cs, "averageScoreClasses": score_average(cs),
               "categoryScores": cat, "averageScoreCategories": score_average(cat)}
        if self.instance_level:
            ics, icat = self.class_inst_scores(), self.category_inst_scores()
            res.update({"classInstScores": ics, "averageScoreInstClasses": score_average(ics),
                        "categoryInstScores": icat, "averageScoreInstCategories": score_average(icat),
                        "instStats": self.inst_stats})
        if self.boundary_radius is not None:
            R = self.boundary_radius
            tri = trimap_scores(self.rings)
            res.update({"boundaryRadius": R,
                        "trimapScoreClasses": tri["trimapScoreClasses"][:R], "trimapScoreCategories": tri["trimapScoreCategories"][:R],
                        "trimapClassScores": OrderedDict((n, v[:R]) for n, v in tri["trimapClassScores"].items()),
                        "trimapRings": self.rings, "boundaryPrecisionCounts": self.bprec, "boundaryRecallCounts": self.brec})
            res.update(boundary_f_scores(self.bprec, self.brec))
        if self.panoptic is not None:
            from . import panoptic as pq
            res["panopticConnectivity"] = self.panoptic
            res.update(pq.results(self.panoptic_stats))
        return res


def instance_map_tensor(inst, device):
    """A uint16 instance-id map (NumPy) as the 16-bit tensor `fcn8s_op_cityscapes_pair` reads: the same bits, uploaded as torch.int16."""
    import torch
    a = np.ascontiguousarray(np.asarray(inst))
    if a.dtype not in (np.uint16, np.int16):
        if a.size and (a.min() < 0 or a.max() > 65535):
            raise ValueError("instance ids do not fit 16 bits")
        a = a.astype(np.uint16)
    return torch.from_numpy(a.view(np.int16)).to(device)


PANOPTIC_RESULT_KEYS = ("panopticConnectivity", "panopticQuality", "panopticClassScores", "panopticTp", "panopticFp", "panopticFn", "panopticIouSum")


def _check_panoptic(panoptic, instance_level):
    if panoptic is None:
        return None
    if isinstance(panoptic, bool) or panoptic not in (4, 8):
        raise ValueError("`panoptic` is None or the connectivity of the predicted things' components, 4 or 8, not {!r}".format(panoptic))
    if not instance_level:
        raise ValueError("`panoptic` takes its ground-truth segments from the instance-id maps: needs instance_level=True.")
    return int(panoptic)


BOUNDARY_RESULT_KEYS = ("boundaryRadius", "trimapScoreClasses", "trimapScoreCategories", "trimapClassScores", "boundaryFScoreClasses",
                        "boundaryClassScores", "trimapRings", "boundaryPrecisionCounts", "boundaryRecallCounts")


def result_dict(res):
    """createResultDict (:355-376) of an instance-level result: the layout of the evaluator's resultPixelLevelSemanticLabeling.json."""
    if "classInstScores" not in res or "confMatrix" not in res:
        raise ValueError("result_dict needs the result of an instance-level evaluation of files (evaluate_file_pairs / evaluate_directory with instance_level=True)")
    conf = np.asarray(res["confMatrix"])
    whole = OrderedDict()
    whole["confMatrix"] = conf.tolist()
    whole["priors"] = OrderedDict(); whole["labels"] = OrderedDict()
    total = float(conf.sum())
    for label in range(NUM_IDS):
        whole["priors"][ID_TO_NAME[label]] = float(conf[label, :].sum()) / total if total else float('nan')
        whole["labels"][ID_TO_NAME[label]] = label
    for k in ("classScores", "classInstScores", "categoryScores", "categoryInstScores"):
        whole[k] = OrderedDict(res[k])
    for k in ("averageScoreClasses", "averageScoreInstClasses", "averageScoreCategories", "averageScoreInstCategories"):
        whole[k] = res[k]
    for k in BOUNDARY_RESULT_KEYS + PANOPTIC_RESULT_KEYS:          # not the evaluator's: present only after an evaluation that asked for them
        if k in res:
            whole[k] = res[k].tolist() if isinstance(res[k], np.ndarray) else res[k]
    return whole


def write_result_json(res, path):
    """writeJSONFile (:378-383): `result_dict(res)` as JSON, interchangeable with the evaluator's result file."""
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    with open(path, 'w') as f:
        f.write(json.dumps(result_dict(res), default=lambda o: o.__dict__, sort_keys=True, indent=4))


# ---------------------------------------------------------------------------------------------------------
# files either side of the scoring: label-id PNG export and the evaluator's prediction / ground-truth file loop
# ---------------------------------------------------------------------------------------------------------
def save_label_id_png(path, pred_train_ids):
    """Write one prediction (train ids, (H,W), as `FCN8s.predict` returns them) as the single-channel uint8 label-id PNG the
    official evaluator reads (evalPixelLevelSemanticLabeling.py:553-555; ids via labels.py:188-192)."""
    from PIL import Image
    a = np.asarray(pred_train_ids)
    if a.ndim != 2:
        raise ValueError("expected one (H, W) map of train ids, got shape {}".format(a.shape))
    Image.fromarray(TRAINIDS_TO_IDS_ARRAY[a.astype(np.int64)]).save(path)


def cs_file_info(file_name):
    """csHelpers.getCsFileInfo: (city, sequenceNb, frameNb) of `<city>_<seq>_<frame>_<type>[_<type2>].<ext>`."""
    parts = os.path.basename(file_name).split('_')
    if len(parts) < 4:
        raise ValueError("Cannot parse given filename ({}). Does not seem to be a valid Cityscapes file.".format(file_name))
    return parts[0], parts[1], parts[2]


def walk_predictions(prediction_path):
    return [(root, files) for root, _, files in os.walk(prediction_path)]


def find_prediction(prediction_path, ground_truth_file, walk=None, extension='png'):
    """evalPixelLevelSemanticLabeling.py:72-106: the one file `<city>_<seq>_<frame>*.png` anywhere below `prediction_path`
    (`walk`: a walk_predictions() result to reuse, as the evaluator walks the tree once)."""
    if walk is None:
        walk = walk_predictions(prediction_path)
    city, seq, frame = cs_file_info(ground_truth_file)
    pattern = "{}_{}_{}*.{}".format(city, seq, frame, extension)
    found = None
    for root, files in walk:
        for f in fnmatch.filter(files, pattern):
            if found is not None:
                raise ValueError("Found multiple predictions for ground truth {}".format(ground_truth_file))
            found = os.path.join(root, f)
    if found is None:
        raise ValueError("Found no prediction for ground truth {}".format(ground_truth_file))
    return found


def instance_file_of(ground_truth_file):
    """The instance-id map that belongs to a `*_labelIds.png` (:564)."""
    return ground_truth_file.replace("labelIds", "instanceIds")


def evaluate_file_pairs(prediction_files, ground_truth_files, device=None, instance_level=False, boundary_radius=None, panoptic=None):
    """evaluateImgLists / evaluatePair (evalPixelLevelSemanticLabeling.py:454-498, 550-635): accumulate conf[gt, pred] over
    pairs of label-id PNGs with the evaluator's checks, then the class / category scores.  `device`: a torch cuda device
    to count on the GPU (the library's kernels), None = NumPy.  `instance_level`: also read each ground truth's `*_instanceIds.png`
    and report the iIoU scores (`classInstScores`, `categoryInstScores`, their averages, `instStats`).  `boundary_radius=R`: also the
    trimap IoU for the band widths 1..R around the ground-truth boundaries and the boundary F-score for the tolerances 0..R (the
    `trimap*` / `boundary*` keys; `trimap_scores`, `boundary_f_scores`).  `panoptic=4` or `8` (needs `instance_level`): also panoptic
    quality, the predicted things split into connected components of that connectivity (the `panoptic*` keys; panoptic.py)."""
    from PIL import Image
    if len(prediction_files) != len(ground_truth_files):
        raise ValueError("List of images for prediction and groundtruth are not of equal size.")
    ev = PixelLevelEvaluator(instance_level=instance_level, boundary_radius=boundary_radius, panoptic=panoptic)
    pixels = 0
    for pf, gf in zip(prediction_files, ground_truth_files):
        pred, gt = np.array(Image.open(pf)), np.array(Image.open(gf))
        inst = None
        if instance_level:
            inf = instance_file_of(gf)
            if inf == gf or not os.path.isfile(inf):
                raise ValueError("Unable to load " + inf)
            inst = np.array(Image.open(inf))
        if pred.ndim != 2:
            raise ValueError("Predicted image has multiple channels.")
        if pred.shape[1] != gt.shape[1]:
            raise ValueError("Image widths of " + pf + " and " + gf + " are not equal.")
        if pred.shape[0] != gt.shape[0]:
            raise ValueError("Image heights of " + pf + " and " + gf + " are not equal.")
        if gt.max() >= NUM_IDS:
            raise ValueError("Unknown label with id {:}".format(int(gt.max())))
        if instance_level:
            if inst.shape != gt.shape:
                raise ValueError("Image sizes of " + instance_file_of(gf) + " and " + gf + " are not equal.")
            if pred.max() >= NUM_IDS:
                raise ValueError("Unknown label with id {:} in {}".format(int(pred.max()), pf))
            if device is not None:
                import torch
                ev.add(torch.from_numpy(pred.astype(np.uint8)).to(device), gt.astype(np.uint8), inst, pred_is_train_ids=False)
            else:
                ev.add(pred, gt, inst, pred_is_train_ids=False)
        elif device is not None:
            import torch
            confusion_add(ev.conf, torch.from_numpy(gt.astype(np.uint8)).to(device), torch.from_numpy(pred.astype(np.int64)).to(device))
        else:
            confusion_add(ev.conf, gt, pred)
        if boundary_radius is not None and not instance_level:         # (with instance_level, ev.add has counted them)
            if device is not None:
                import torch
                if pred.max() >= NUM_IDS:
                    raise ValueError("Unknown label with id {:} in {}".format(int(pred.max()), pf))
                ev.add_boundary_tables(boundary_counts_device(torch.from_numpy(pred.astype(np.uint8)).to(device),
                                                              torch.from_numpy(gt.astype(np.uint8)).to(device), boundary_radius))
            else:
                ev.add_boundary_tables(boundary_counts_numpy(pred, gt, boundary_radius, pred_is_train_ids=False))
        pixels += pred.size
        if int(ev.conf.sum()) != pixels:
            raise ValueError("Number of analyzed pixels and entries in confusion matrix disagree: contMatrix {}, pixels {}".format(int(ev.conf.sum()), pixels))
    res = ev.results()
    res["confMatrix"] = ev.conf
    res["nbPixels"] = pixels
    return res


def evaluate_directory(ground_truth_search, prediction_path, device=None, instance_level=False, boundary_radius=None, panoptic=None):
    """The evaluator's no-argument mode (:667-676): every ground-truth file matching the glob (the official one is
    `<cityscapes>/gtFine/val/*/*_gtFine_labelIds.png`) against its prediction below `prediction_path`."""
    from . import sweeps
    gts, predictions = sweeps.paired_files(prediction_path, ground_truth_search, 'png')
    return evaluate_file_pairs(predictions, gts, device, instance_level, boundary_radius, panoptic)
