"""Instance-level AP of a semantic prediction against a Cityscapes instance map, and the official instance-level result format
(fcn8s_op_instance_pair; the definition is in include/fcn8s_hip.h).

The other half of the Cityscapes evaluation beside the pixel-level one (cityscapes_eval.py): AP over the overlaps 0.5 .. 0.95 and AP50% per
thing class and on average.  Train ids are those of `panoptic.py`: 0 = void, 1..11 = stuff, 12..19 = things.  Per image and pixel p:

  * `labels[p]`, a uint8 train id: the class the pixel ended up with -- the argmax of the softmax, possibly after `regions_clean`;
    `comp[p]`, the connected component of p in that map (`regions.components_numpy` / `fcn8s_op_regions_label`); `prob[p]`, float32 rows
    of C >= 20 classes as `predict*(argmax=False)` leaves them; `v[p]`, the uint16 ground-truth instance value (0 without ground truth:
    the export route).
  * Predicted key: a label in 12..19 gives kp = 2^31 | comp << 5 | label (panoptic's thing key; images of at most 2^26 pixels); every other
    label gives kp = 0, "no instance", and a label >= 20 is counted as bad besides.
  * Ground-truth key: the raw value v.  Not panoptic's `kg`, which sends every ignoreInEval label to 0: here a caravan instance 29001 is
    neither void nor a match; only values that equal an ignored label id (v < 1000) are void.
  * Confidence: where kp != 0, q = prob[p][labels[p]] and the term t = rint(q * 2^24) as an integer (float32 product, the fixed point of
    `reliability_pair`); a q that is not in [0, 1] (NaN fails the test) gives t = 0 and is counted.
  * The table holds every distinct (kp, v) of the image, kp = 0 included, with n = its pixel count and s = the sum of its terms.  Rows are
    int64 (kp, v, n, s) in ascending (kp, v); the counts sum to H * W.
  * Host half, float64.  Area of a predicted instance = sum_v n; confidence = sum_v s / (area * 2^24); void intersection = sum of n over the
    void v; intersection with a ground-truth instance = n(kp, v) for the v whose label (v if v < 1000 else v // 1000) is the instance's
    class; ground-truth pixel count of v = sum_kp n; v // 1000 > 33 is refused.  Then the official matching: for each of the ten overlaps
    and each class, a ground-truth instance (v >= 1000, at least 100 pixels) is matched by the predictions whose IoU with it exceeds the
    overlap -- the best-scored one is the true positive, the others are false positives; a ground-truth instance without a match is a hard
    false negative; a prediction without a match (groups and small instances count as matches here) is a false positive unless its share
    of ignored pixels -- void, groups (v < 1000 of the class) and instances below 100 pixels -- exceeds the overlap.  AP is the step-wise
    integral of the precision-recall curve over the distinct scores; a class with ground truth and no prediction has AP 0, one without
    ground truth NaN; the averages skip NaN.  The distance-based variants (AP50m, AP100m) are not taken: they need disparity.

Caveat.  Connected components are the naive way to turn a semantic map into instances: touching cars are one instance.  AP under this rule
measures the semantic model plus that rule.  It is a baseline and a speck detector -- what calibration, averaging and `min_region` cleanup do
to the ranking of segments -- not an instance-segmentation method.

`pair_rows_numpy` restates the table in NumPy; `pair_rows_device` takes it on the GPU; `image_tables` / `image_instances`, `new_stats` /
`stats_add` / `results` are the host half for both; `write_export` / `read_export` / `evaluate_directory` are the official file format.
"""
from __future__ import annotations

import os
import warnings
from collections import OrderedDict

import numpy as np

from . import regions
from .cityscapes_eval import LABELS, NUM_IDS, TRAINIDS_TO_IDS_ARRAY

FIRST_THING = 12                                             # train ids 12..19 have instances
NUM_TRAIN_IDS = 20
MAX_PIXELS = 1 << 26
THING_BIT = 1 << 31
CONF_ONE = 1 << 24                                           # the fixed point of a confidence term
DEFAULT_MAX_ROWS = 4096
MIN_REGION_SIZE = 100                                        # ground-truth instances below it are ignore regions
OVERLAPS = np.arange(0.5, 1., 0.05)
INST_LABEL_IDS = [int(TRAINIDS_TO_IDS_ARRAY[t]) for t in range(FIRST_THING, NUM_TRAIN_IDS)]      # 24, 25, 26, 27, 28, 31, 32, 33
INST_LABEL_NAMES = [n for n, i, *_r in LABELS if i in INST_LABEL_IDS]
VOID_IDS = np.array([i for _n, i, *_r in LABELS if i >= 0 and _r[4]], dtype=np.int64)            # label ids that are ignored in the evaluation
assert INST_LABEL_IDS == sorted(INST_LABEL_IDS) and len(INST_LABEL_NAMES) == 8


# ---- the NumPy restatement of the table ---------------------------------------------------------------------------------------------------
def confidence_terms(q):
    """t of every q: float32 in, int64 out; (t, out of range)."""
    q = np.asarray(q, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        ok = (q >= 0) & (q <= 1)
        t = np.rint(np.where(ok, q, np.float32(0)) * np.float32(CONF_ONE)).astype(np.int64)
    return t, ~ok


def _rows_one(prob, labels, comp, inst):
    if labels.ndim != 2 or labels.size == 0 or prob.shape[:2] != labels.shape or prob.ndim != 3 or prob.shape[2] < NUM_TRAIN_IDS:
        raise ValueError("a softmax of shape {} against a label map of shape {}".format(prob.shape, labels.shape))
    if labels.size > MAX_PIXELS:
        raise ValueError("instances: an image has at most 2^26 pixels, got {}".format(labels.size))
    lab = labels.astype(np.int64).ravel()
    thing = (lab >= FIRST_THING) & (lab < NUM_TRAIN_IDS)
    kp = np.where(thing, THING_BIT | (comp.astype(np.int64).ravel() << 5) | lab, 0)
    v = np.zeros(lab.size, np.int64) if inst is None else inst.astype(np.int64).ravel()
    q = prob.reshape(lab.size, -1)[np.arange(lab.size), np.where(thing, lab, 0)]
    t, out = confidence_terms(q)
    t = np.where(thing, t, 0)
    both = kp.astype(np.uint64) << np.uint64(32) | v.astype(np.uint64)
    uniq, inv, n = np.unique(both, return_inverse=True, return_counts=True)      # ascending (kp, v)
    s = np.zeros(uniq.size, np.int64)
    np.add.at(s, inv.ravel(), t)
    rows = np.stack([(uniq >> np.uint64(32)).astype(np.int64), (uniq & np.uint64(0xFFFFFFFF)).astype(np.int64), n.astype(np.int64), s], axis=1)
    return rows.reshape(-1, 4), np.array([int((lab >= NUM_TRAIN_IDS).sum()), int((out & thing).sum())], np.int64)


def pair_rows_numpy(prob, labels, inst=None, connectivity=4, comp=None):
    """(rows, bad) of one image (prob [H, W, C] float32, labels [H, W] uint8 train ids, inst [H, W] uint16 or None), or (list of rows,
    list of bad) of a stack [N, ...]: rows int64 [K, 4] = (kp, v, pixels, sum of terms) in ascending (kp, v), bad = int64 (pixels with a
    label >= 20, pixels with q out of range).  `comp`: the component ids of `labels`; None takes `regions.components_numpy`."""
    regions._check(connectivity)
    prob = np.asarray(prob); labels = np.asarray(labels)
    if prob.dtype != np.float32 or labels.dtype != np.uint8 or labels.ndim not in (2, 3):
        raise ValueError("the softmax is float32 and the labels are uint8 [H, W] or [N, H, W], got {} {} and {} {}".format(prob.dtype, prob.shape, labels.dtype, labels.shape))
    if inst is not None:
        inst = np.asarray(inst)
        if inst.dtype == np.int16:
            inst = inst.view(np.uint16)
        if inst.dtype.kind not in "iu" or inst.shape != labels.shape:
            raise ValueError("the instance map is an integer array of the labels' shape, got {} {}".format(inst.dtype, inst.shape))
    if comp is None:
        comp, _area = regions.components_numpy(labels, connectivity)
    comp = np.asarray(comp)
    if comp.shape != labels.shape:
        raise ValueError("the components have the labels' shape, got {}".format(comp.shape))
    if labels.ndim == 2:
        return _rows_one(prob, labels, comp, inst)
    if prob.ndim != 4 or prob.shape[0] != labels.shape[0]:
        raise ValueError("a softmax of shape {} against labels of shape {}".format(prob.shape, labels.shape))
    res = [_rows_one(prob[i], labels[i], comp[i], None if inst is None else inst[i]) for i in range(labels.shape[0])]
    return [r[0] for r in res], [r[1] for r in res]


# ---- the table on the GPU ----------------------------------------------------------------------------------------------------------------
def _pow2_at_least(x):
    return 1 << max(0, int(x) - 1).bit_length()


def default_slots(H, W):
    """A 32nd of the pixels, at least 256: a Cityscapes image has a few hundred pairs, and a slot is 32 bytes that the clear kernel writes and
    the compaction reads in every call (measured at 16 x 1024x512 on Cityscapes-like maps: 178.7 us with an eighth of the pixels, 162.9 us with a 32nd).  A map salted at 5 % has one
    pair per twenty pixels; the table is then doubled once and the next call on the same `work` starts there."""
    return _pow2_at_least(max(256, (int(H) * int(W) + 31) // 32))


def _shape(prob, labels, comp, inst):
    import torch
    if labels.dtype != torch.uint8 or labels.dim() not in (2, 3) or not labels.is_contiguous() or labels.numel() == 0:
        raise ValueError("the labels are a contiguous uint8 tensor [H, W] or [N, H, W]")
    N = 1 if labels.dim() == 2 else int(labels.shape[0])
    H, W = int(labels.shape[-2]), int(labels.shape[-1])
    if prob.dtype != torch.float32 or not prob.is_contiguous() or prob.device != labels.device or prob.dim() != labels.dim() + 1 or tuple(prob.shape[:-1]) != tuple(labels.shape):
        raise ValueError("the softmax is a contiguous float32 tensor of the labels' shape plus the classes, on their device")
    C_ = int(prob.shape[-1])
    if C_ < NUM_TRAIN_IDS:
        raise ValueError("instances: the softmax has at least 20 classes, got {}".format(C_))
    if comp.dtype != torch.int32 or tuple(comp.shape) != tuple(labels.shape) or not comp.is_contiguous() or comp.device != labels.device:
        raise ValueError("the components are a contiguous int32 tensor of the labels' shape on their device")
    if inst is not None and (inst.element_size() != 2 or inst.is_floating_point() or tuple(inst.shape) != tuple(labels.shape) or not inst.is_contiguous() or inst.device != labels.device):
        raise ValueError("the instance map is a contiguous 16-bit integer tensor of the labels' shape on their device")
    return N, H, W, C_


def raw_pair_device(prob, labels, comp, inst, slots_per_image, max_rows, table=None, rows=None):
    """One `fcn8s_op_instance_pair` call on device tensors: (rows [N, max_rows, 4] int64, counts [N, 5] int64, table) as device tensors, in
    the op's own order and with whatever it reports; nothing is downloaded.  `table` / `rows`: tensors to reuse when they are large enough."""
    import ctypes as C
    import torch
    from . import _lib as L
    N, H, W, C_ = _shape(prob, labels, comp, inst)
    nbytes = int(L.lib.fcn8s_op_instance_work_bytes(N, int(slots_per_image)))
    if nbytes == 0:
        raise ValueError("instances: slots_per_image has to be a power of two in 1..2^28, got %r" % (slots_per_image,))
    if int(max_rows) < 1:
        raise ValueError("instances: max_rows has to be positive, got %r" % (max_rows,))
    if table is None or table.numel() < nbytes:
        table = torch.empty(nbytes, dtype=torch.uint8, device=labels.device)
    if rows is None or rows.numel() < N * int(max_rows) * 4:
        rows = torch.empty(N * int(max_rows) * 4, dtype=torch.int64, device=labels.device)
    counts = torch.empty((N, 5), dtype=torch.int64, device=labels.device)
    stream = C.c_void_p(torch.cuda.current_stream(labels.device).cuda_stream)
    L.check(L.lib.fcn8s_op_instance_pair(stream, C.c_void_p(prob.data_ptr()), C_, C.c_void_p(labels.data_ptr()), C.c_void_p(comp.data_ptr()),
                                         C.c_void_p(inst.data_ptr() if inst is not None else None), N, H, W,
                                         C.c_void_p(table.data_ptr()), int(slots_per_image), C.c_void_p(rows.data_ptr()), int(max_rows),
                                         C.c_void_p(counts.data_ptr())))
    return rows[:N * int(max_rows) * 4].view(N, int(max_rows), 4), counts, table


def sort_rows(rows):
    """Rows (kp, v, n, s) in ascending (kp, v): one sort on the 64-bit key kp << 32 | v (both are below 2^32, and a table holds a pair once)."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 4)
    return rows[np.argsort(rows[:, 0].astype(np.uint64) << np.uint64(32) | rows[:, 1].astype(np.uint64), kind="stable")]


def pair_rows_device(prob, labels, comp, inst=None, slots_per_image=None, max_rows=None, work=None):
    """The table of device tensors (prob float32 [.., H, W, C], labels uint8 and comp int32 [H, W] or [N, H, W], inst a 16-bit device
    tensor, a NumPy uint16 map that is uploaded, or None): one `fcn8s_op_instance_pair` call.  When the op reports a hash table that was
    too small or more rows than `max_rows`, the call is repeated with twice the slots / the reported row count; a table of 2 H W slots
    cannot be too small, so the repeats are bounded.  Returns (list of rows per image, sorted ascending as `pair_rows_numpy` gives them;
    int64 array [N, 2] of bad pixels per image; work) -- `work`: a dict of device scratch to hand to the next call."""
    import torch
    from .cityscapes_eval import instance_map_tensor
    if inst is not None:
        if not isinstance(inst, torch.Tensor):
            inst = instance_map_tensor(inst, labels.device)
        inst = inst.to(labels.device).contiguous()
    N, H, W, _C = _shape(prob, labels, comp, inst)
    if H * W > MAX_PIXELS:
        raise ValueError("instances: an image has at most 2^26 pixels, got {}".format(H * W))
    work = {} if work is None else work
    full = _pow2_at_least(2 * H * W)
    slots = min(full, max(default_slots(H, W), work.get("slots", 0))) if slots_per_image is None else int(slots_per_image)
    rows_cap = max(DEFAULT_MAX_ROWS, work.get("max_rows", 0)) if max_rows is None else int(max_rows)
    while True:
        rows, counts, work["table"] = raw_pair_device(prob, labels, comp, inst, slots, rows_cap, table=work.get("table"), rows=work.get("rows"))
        work["rows"] = rows.view(-1)
        cnt = counts.cpu().numpy()
        if cnt[:, 2].any():
            if slots >= full:
                raise RuntimeError("instances: a hash table of 2 H W slots reported an overflow")
            slots = min(full, slots * 2)
            continue
        if int(cnt[:, 0].max()) > rows_cap:
            rows_cap = int(cnt[:, 0].max())                                     # exact: the table held every pair
            continue
        break
    work["slots"], work["max_rows"] = slots, rows_cap
    if (cnt[:, 3] != H * W).any():
        raise RuntimeError("instances: the counted pixels do not add up to the image: {}".format(cnt.tolist()))
    host = rows[:, :max(int(cnt[:, 0].max()), 1)].cpu().numpy()
    return [sort_rows(host[n, :int(cnt[n, 0])]) for n in range(N)], cnt[:, [1, 4]].copy(), work


# ---- the host half -----------------------------------------------------------------------------------------------------------------------
def _value_labels(v):
    lab = np.where(v < 1000, v, v // 1000)
    if (lab >= NUM_IDS).any():
        raise ValueError("Unknown label with id {:}".format(int(lab.max())))
    return lab


def image_tables(rows, min_instance_pixels=0):
    """One image's rows (kp, v, n, s), ascending (kp, v), as the arrays of the matching: predictions in ascending kp (pred_kp, pred_label,
    pred_pix, pred_conf, pred_void), ground-truth values in ascending v (gt_id, gt_label, gt_pix), and the matches (m_pred, m_gt, m_inter:
    a prediction and a value of its label that share pixels) in ascending (prediction, value).  Predictions of fewer than
    `min_instance_pixels` pixels are dropped; their pixels still count for the ground truth."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 4)
    kp, v, n, s = rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3]
    both = kp.astype(np.uint64) << np.uint64(32) | v.astype(np.uint64)
    if (both[1:] <= both[:-1]).any():
        raise ValueError("instance rows have to be in ascending (kp, v) order")
    uv, iv = np.unique(v, return_inverse=True)
    iv = iv.ravel()
    glab = _value_labels(uv)
    gpix = np.bincount(iv, weights=n, minlength=uv.size).astype(np.int64)                       # (sums of at most 2^26 pixels: exact in float64)
    m = kp != 0
    kpt, nt, st, ivt = kp[m], n[m], s[m], iv[m]
    head = np.ones(kpt.size, bool)
    head[1:] = kpt[1:] != kpt[:-1]                                                              # kp ascends: an instance is a stretch of rows
    starts = np.flatnonzero(head)
    gid = np.cumsum(head) - 1
    if starts.size:
        area, total = np.add.reduceat(nt, starts), np.add.reduceat(st, starts)
        void = np.add.reduceat(np.where(np.isin(v[m], VOID_IDS), nt, 0), starts)
    else:
        area = total = void = np.zeros(0, np.int64)
    keep = area >= int(min_instance_pixels)
    new_index = np.cumsum(keep) - 1
    plabel = TRAINIDS_TO_IDS_ARRAY[kpt[starts] & 31].astype(np.int64)
    match = keep[gid] & (glab[ivt] == plabel[gid]) if kpt.size else np.zeros(0, bool)
    return dict(pred_kp=kpt[starts][keep], pred_label=plabel[keep], pred_pix=area[keep], pred_void=void[keep],
                pred_conf=total[keep].astype(np.float64) / (area[keep] * CONF_ONE).astype(np.float64),
                gt_id=uv, gt_label=glab, gt_pix=gpix, m_pred=new_index[gid[match]], m_gt=ivt[match], m_inter=nt[match])


def tables_as_lists(t):
    """The arrays of `image_tables` as the two lists of the matching: predictions, each a dict(kp, labelID, pixelCount, confidence,
    voidIntersection, matchedGt = [(instID, pixelCount of it, intersection), ..] in ascending instID over the values of the prediction's
    label, groups included); ground truth over every value of the image, each a dict(instID, labelID, pixelCount, matchedPred =
    [(index into predictions, intersection), ..])."""
    preds = [dict(kp=None if t["pred_kp"] is None else int(t["pred_kp"][i]), labelID=int(t["pred_label"][i]), pixelCount=int(t["pred_pix"][i]),
                  confidence=float(t["pred_conf"][i]), voidIntersection=int(t["pred_void"][i]), matchedGt=[]) for i in range(t["pred_label"].size)]
    gts = [dict(instID=int(t["gt_id"][i]), labelID=int(t["gt_label"][i]), pixelCount=int(t["gt_pix"][i]), matchedPred=[]) for i in range(t["gt_id"].size)]
    for p, g, inter in zip(t["m_pred"].tolist(), t["m_gt"].tolist(), t["m_inter"].tolist()):
        preds[p]["matchedGt"].append((gts[g]["instID"], gts[g]["pixelCount"], inter))
        gts[g]["matchedPred"].append((p, inter))
    return preds, gts


def image_instances(rows, min_instance_pixels=0):
    """One image's rows as the predicted and ground-truth instance lists with their intersections: `tables_as_lists(image_tables(...))`."""
    return tables_as_lists(image_tables(rows, min_instance_pixels))


def new_stats():
    return {"images": []}


def stats_add(stats, rows, min_instance_pixels=0):
    """One image's rows into the running tables (images in file order)."""
    stats["images"].append(image_tables(rows, min_instance_pixels))
    return stats


def _average_precision(y_true, y_score, hard_fns):
    """The step-wise integral of the precision-recall curve over the distinct scores; the curve starts at (recall 0, precision 1)."""
    if y_score.size == 0:
        return 0.0                                                              # ground truth that nothing matched and no false positive
    order = np.argsort(y_score, kind="stable")
    score, true = y_score[order], y_true[order]
    cum = np.cumsum(true)
    _thr, first = np.unique(score, return_index=True)
    below = np.where(first > 0, cum[first - 1], 0.)                              # the true examples scored below each threshold
    tp = cum[-1] - below
    fp = score.size - first - tp
    fn = below + hard_fns
    precision = np.append(tp / (tp + fp), 1.)
    recall = np.append(tp / (tp + fn), 0.)
    ext = np.concatenate([recall[:1], recall, [0.]])
    widths = 0.5 * (ext[:-2] - ext[2:])
    return float(np.dot(precision, widths))


def _class_view(t, label):
    """What one image holds of one class, whatever the overlap: its predictions, its matches, the ignored pixels of every prediction
    (void, groups, instances below the minimum size), the ground-truth instances that are evaluated."""
    mine = np.flatnonzero(t["pred_label"] == label)
    sel = t["pred_label"][t["m_pred"]] == label
    mp, mg, inter = t["m_pred"][sel], t["m_gt"][sel], t["m_inter"][sel]
    gp, pp = t["gt_pix"][mg], t["pred_pix"][mp]
    weight = inter * ((t["gt_id"][mg] < 1000).astype(np.int64) + (gp < MIN_REGION_SIZE).astype(np.int64))
    ignored = t["pred_void"] + np.bincount(mp, weights=weight, minlength=t["pred_label"].size).astype(np.int64)
    real = (t["gt_label"] == label) & (t["gt_id"] >= 1000) & (t["gt_pix"] >= MIN_REGION_SIZE)
    iou = inter.astype(np.float64) / (gp + pp - inter)
    return dict(mine=mine, mp=mp, mg=mg, iou=iou, real=np.flatnonzero(real), is_real=real[mg], conf=t["pred_conf"], npred=t["pred_label"].size,
                share=ignored[mine].astype(np.float64) / t["pred_pix"][mine])


def _class_examples(c, overlap):
    """One image, one class, one overlap: (y_true, y_score, hard false negatives)."""
    hit = c["iou"] > overlap
    true, score = [], []
    on_real = np.flatnonzero(hit & c["is_real"])                                 # ascending (prediction, value)
    by_gt = {}
    for i in on_real.tolist():
        by_gt.setdefault(int(c["mg"][i]), []).append(float(c["conf"][c["mp"][i]]))
    for g in c["real"].tolist():
        confs = by_gt.get(g)
        if not confs:
            continue
        best = confs[0]
        for conf in confs[1:]:                                                  # a second match: the lower score is a false positive
            true.append(0.); score.append(min(best, conf))
            best = max(best, conf)
        true.append(1.); score.append(best)
    hard = int(c["real"].size - len(by_gt))
    found = np.bincount(c["mp"][hit], minlength=c["npred"]) > 0                  # (groups and small instances count as found here)
    spare = c["mine"][~found[c["mine"]] & (c["share"] <= overlap)]
    true += [0.] * spare.size; score += c["conf"][spare].tolist()
    return true, score, hard


def results(stats):
    """The result: `ap` float64 [8 classes, 10 overlaps]; `averages` {allAp, allAp50%, classes: {name: {ap, ap50%}}}, `overlaps`,
    `minRegionSizes`, `instLabels` and `resultApMatrix` [1][8][10] in the layout of resultInstanceLevelSemanticLabeling.json; and the raw
    tables `nbImages`, `nbPredictions` / `nbGroundTruth` (int64 [8]: predictions, and ground-truth instances that are evaluated)."""
    ap = np.zeros((len(INST_LABEL_IDS), OVERLAPS.size), np.float64)
    npred = np.zeros(len(INST_LABEL_IDS), np.int64); ngt = np.zeros(len(INST_LABEL_IDS), np.int64)
    for li, label in enumerate(INST_LABEL_IDS):
        views = [_class_view(t, label) for t in stats["images"]]
        npred[li] = sum(c["mine"].size for c in views); ngt[li] = sum(c["real"].size for c in views)
        for oi, overlap in enumerate(OVERLAPS):
            if ngt[li] and npred[li]:
                true, score, hard = [], [], 0
                for c in views:
                    t, s, h = _class_examples(c, overlap)
                    true += t; score += s; hard += h
                ap[li, oi] = _average_precision(np.array(true, np.float64), np.array(score, np.float64), hard)
            elif ngt[li]:
                ap[li, oi] = 0.0
            else:
                ap[li, oi] = float('nan')
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)                          # a mean over nothing is NaN, as the official table has it
        averages = OrderedDict((("allAp", float(np.nanmean(ap))), ("allAp50%", float(np.nanmean(ap[:, 0]))), ("classes", OrderedDict())))
        for li, name in enumerate(INST_LABEL_NAMES):
            averages["classes"][name] = OrderedDict((("ap", float(np.mean(ap[li]))), ("ap50%", float(ap[li, 0]))))
    return {"ap": ap, "averages": averages, "overlaps": OVERLAPS.tolist(), "minRegionSizes": [MIN_REGION_SIZE], "instLabels": list(INST_LABEL_NAMES),
            "resultApMatrix": [ap.tolist()], "nbImages": len(stats["images"]), "nbPredictions": npred, "nbGroundTruth": ngt}


def result_dict(res):
    """The JSON-serialisable part of `results`, in the layout of resultInstanceLevelSemanticLabeling.json."""
    return {k: res[k] for k in ("averages", "overlaps", "minRegionSizes", "instLabels", "resultApMatrix")}


def write_result_json(res, path):
    import json
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    with open(path, 'w') as f:
        f.write(json.dumps(result_dict(res), sort_keys=True, indent=4))


# ---- the official result format -----------------------------------------------------------------------------------------------------------
def write_export(results_dir, name, comp, rows, min_instance_pixels=0):
    """One image in the official instance-level result format: `<results_dir>/<name>.txt` with one line
    `<relative mask path> <label id> <confidence>` per predicted instance, in ascending kp, and one binary mask PNG (0 / 255) per instance
    under `<name>_masks/`.  `comp`: the int32 component map [H, W] the rows were taken with; `rows`: the image's rows (a table taken
    without ground truth is enough).  The confidence is written with `repr`, so it reads back exactly.  Returns the path of the text file."""
    from PIL import Image
    comp = np.asarray(comp)
    preds, _gts = image_instances(rows, min_instance_pixels)
    os.makedirs(os.path.join(results_dir, name + "_masks"), exist_ok=True)
    lines = []
    for k, p in enumerate(preds):
        mask = comp == ((p["kp"] & (THING_BIT - 1)) >> 5)
        if int(mask.sum()) != p["pixelCount"]:
            raise ValueError("the component map does not belong to the rows: instance {} has {} pixels, its mask {}".format(k, p["pixelCount"], int(mask.sum())))
        rel = os.path.join(name + "_masks", "%05d.png" % k)
        Image.fromarray(mask.astype(np.uint8) * 255).save(os.path.join(results_dir, rel))
        lines.append("{} {} {}\n".format(rel, p["labelID"], repr(p["confidence"])))
    path = os.path.join(results_dir, name + ".txt")
    with open(path, 'w') as f:
        f.writelines(lines)
    return path


def read_export(path):
    """The predictions of one result text file, in file order: a list of (mask bool [H, W], label id, confidence)."""
    from PIL import Image
    out = []
    with open(path) as f:
        for line in f:
            parts = line.split(" ")
            if len(parts) != 3:
                raise ValueError("Invalid prediction file. Expected content: relPathPrediction1 labelIDPrediction1 confidencePrediction1")
            if os.path.isabs(parts[0]):
                raise ValueError("Invalid prediction file. First entry in each line must be a relative path.")
            mask = np.array(Image.open(os.path.join(os.path.dirname(path), parts[0])).convert("L")) != 0
            out.append((mask, int(float(parts[1])), float(parts[2])))
    return out


def file_tables(predictions, inst, min_instance_pixels=0):
    """`image_tables` for predictions given as masks (`read_export`) against a ground-truth instance map: the same arrays, the predictions
    in the order given (pred_kp is None).  Masks may overlap here; labels that have no instances and empty masks are skipped."""
    inst = np.asarray(inst)
    uv, n = np.unique(inst, return_counts=True)
    uv = uv.astype(np.int64)
    glab = _value_labels(uv)
    void = np.isin(inst, VOID_IDS)
    label, pix, conf, pvoid, mp, mg, mi = [], [], [], [], [], [], []
    for mask, lab, c in predictions:
        if mask.shape != inst.shape:
            raise ValueError("a mask of shape {} against an instance map of shape {}".format(mask.shape, inst.shape))
        area = int(np.count_nonzero(mask))
        if lab not in INST_LABEL_IDS or area == 0 or area < int(min_instance_pixels):
            continue
        vals, cnts = np.unique(inst[mask], return_counts=True)
        gi = np.searchsorted(uv, vals.astype(np.int64))
        own = glab[gi] == lab
        mp += [len(label)] * int(own.sum()); mg += gi[own].tolist(); mi += cnts[own].tolist()
        label.append(int(lab)); pix.append(area); conf.append(float(c)); pvoid.append(int(np.count_nonzero(void & mask)))
    i64 = lambda a: np.array(a, np.int64).reshape(-1)
    return dict(pred_kp=None, pred_label=i64(label), pred_pix=i64(pix), pred_void=i64(pvoid), pred_conf=np.array(conf, np.float64).reshape(-1),
                gt_id=uv, gt_label=glab, gt_pix=n.astype(np.int64), m_pred=i64(mp), m_gt=i64(mg), m_inter=i64(mi))


def evaluate_directory(prediction_txts, gt_instance_files, min_instance_pixels=0):
    """The host file route, the counterpart of `cityscapes_eval.evaluate_directory`: the result text files of an export (one per image)
    against the `*_gtFine_instanceIds.png` files, pairwise in the order given.  Returns `results`."""
    from PIL import Image
    prediction_txts, gt_instance_files = list(prediction_txts), list(gt_instance_files)
    if len(prediction_txts) != len(gt_instance_files):
        raise ValueError("{} prediction files against {} ground-truth files".format(len(prediction_txts), len(gt_instance_files)))
    stats = new_stats()
    for txt, gt in zip(prediction_txts, gt_instance_files):
        stats["images"].append(file_tables(read_export(txt), np.array(Image.open(gt)), min_instance_pixels))
    return results(stats)
