"""Panoptic quality of a semantic prediction against a Cityscapes instance map (fcn8s_op_panoptic_pair; the definition is in
include/fcn8s_hip.h).

IoU, iIoU, trimap IoU and the boundary F-score count pixels; a dozen "truck" pixels inside a car move them in the fifth digit.  Panoptic
quality (PQ = SQ x RQ: Kirillov et al., CVPR 2019) counts segments.  All of it is per image; train ids are those of
`cityscapes_eval.LABELS`: 0 = void, 1..11 = stuff, 12..19 = things (the labels that have instances and are evaluated).

  * Predicted segments, from the argmax a[p] and comp[p] = the connected component of p (`regions.components_numpy` /
    `fcn8s_op_regions_label`, connectivity 4 or 8): a = 0 gives no segment, kp = 0; stuff class c gives one segment per image, kp = c; a
    thing class gives one segment per component, kp = 2^31 | comp << 5 | c (images of at most 2^26 pixels).  A prediction outside 0..19
    is counted as bad and skipped.  Label ids (uint8) are mapped to train ids first.
  * Ground-truth segments, from the instance map alone, as the official conversion does.  For the value v: L = v if v < 1000 else
    v // 1000, t = trainId(L).  t = 0 (void, ignoreInEval): kg = 0; L > 33: counted as bad; stuff: kg = t; a thing with v >= 1000:
    kg = 2^31 | (v % 1000) << 5 | t; a thing with v < 1000 is a crowd region, one per class: kg = 2^30 | t.
  * The table holds every distinct (kp, kg) of the image with its pixel count, void on either side included: the counts sum to H * W minus
    the bad pixels.  Rows are int64 (kp, kg, n) in ascending (kp, kg) order.
  * Scores, float64, rows in that order, images in file order.  Segment areas are the marginals of the table.  A row with kp != 0,
    kg != 0, kg no crowd region and equal classes has iou = n / (area_p + area_g - n - count(kp, 0)); iou > 0.5 is a match: tp[c] += 1,
    iou_sum[c] += iou.  An unmatched ground-truth segment that is no crowd region: fn[c] += 1.  An unmatched predicted segment:
    fp[c] += 1, unless (count(kp, 0) + count(kp, crowd of c)) / area_p > 0.5.  Per class PQ = iou_sum / (tp + fp / 2 + fn / 2),
    SQ = iou_sum / tp (0 when tp = 0), RQ = tp / (tp + fp / 2 + fn / 2); the averages run over the classes with tp + fp + fn > 0 and are
    given for all classes, the things and the stuff.

Caveat.  Connected components are the naive way to turn a semantic map into instances: touching cars are one segment.  PQ of the things
under this rule measures the semantic model plus that rule.  PQ of the stuff classes and the fp counts (the specks) are the figures this
is for.

`pair_rows_numpy` restates the table in NumPy; `pair_rows_device` takes it on the GPU; `new_stats` / `stats_add` / `results` are the host
half for both.
"""
from __future__ import annotations

from collections import OrderedDict

import numpy as np

from . import regions
from .cityscapes_eval import IDS_TO_TRAINIDS_ARRAY, LABELS, NUM_IDS

NUM_TRAIN_IDS = 20
FIRST_THING = 12                                             # train ids 12..19 have instances
MAX_PIXELS = 1 << 26
THING_BIT = 1 << 31
CROWD_BIT = 1 << 30
DEFAULT_MAX_ROWS = 4096
TRAIN_ID_NAMES = ["void"] * NUM_TRAIN_IDS
for _n, _id, _tid, *_rest in LABELS:
    if _tid > 0:
        TRAIN_ID_NAMES[_tid] = _n


# ---- keys ------------------------------------------------------------------------------------------------------------------------------
def pred_keys(train_ids, comp):
    """kp of every pixel: int64 arrays of equal shape in; -1 where the train id is outside 0..19 (a bad pixel)."""
    a = np.asarray(train_ids).astype(np.int64); comp = np.asarray(comp).astype(np.int64)
    ok = (a >= 0) & (a < NUM_TRAIN_IDS)
    c = np.where(ok, a, 0)
    kp = np.where(c < FIRST_THING, c, THING_BIT | (comp << 5) | c)
    return np.where(ok, kp, -1)


def gt_keys(inst):
    """kg of every value of an instance map: -1 where the label is beyond 33 (a bad pixel)."""
    v = np.asarray(inst).astype(np.int64)
    lab = np.where(v < 1000, v, v // 1000)
    ok = (lab >= 0) & (lab < NUM_IDS)
    t = IDS_TO_TRAINIDS_ARRAY[np.where(ok, lab, 0)].astype(np.int64)
    kg = np.where(t < FIRST_THING, t, np.where(v < 1000, CROWD_BIT | t, THING_BIT | ((v % 1000) << 5) | t))
    return np.where(ok, kg, -1)


def key_class(k):
    """The train id of a segment key (0 for void)."""
    return np.asarray(k) & 31


def key_is_crowd(kg):
    kg = np.asarray(kg)
    return (kg & CROWD_BIT != 0) & (kg & THING_BIT == 0)


def crowd_key(c):
    return CROWD_BIT | int(c)


# ---- the NumPy restatement of the table ---------------------------------------------------------------------------------------------------
def _rows_one(pred, inst, connectivity, pred_is_train_ids):
    if pred.shape != inst.shape or pred.ndim != 2 or pred.size == 0:
        raise ValueError("a prediction of shape {} against an instance map of shape {}".format(pred.shape, inst.shape))
    if pred.size > MAX_PIXELS:
        raise ValueError("panoptic: an image has at most 2^26 pixels, got {}".format(pred.size))
    a = pred.astype(np.int64)
    if not pred_is_train_ids:
        ok = (a >= 0) & (a < NUM_IDS)
        a = np.where(ok, IDS_TO_TRAINIDS_ARRAY[np.where(ok, a, 0)].astype(np.int64), -1)
    ok = (a >= 0) & (a < NUM_TRAIN_IDS)
    comp, _area = regions.components_numpy(np.where(ok, a, 255), connectivity)
    kp = pred_keys(a, comp).ravel(); kg = gt_keys(inst).ravel()
    good = (kp >= 0) & (kg >= 0)
    both = kp[good].astype(np.uint64) << np.uint64(32) | kg[good].astype(np.uint64)
    uniq, n = np.unique(both, return_counts=True)                                # ascending (kp, kg)
    rows = np.stack([(uniq >> np.uint64(32)).astype(np.int64), (uniq & np.uint64(0xFFFFFFFF)).astype(np.int64), n.astype(np.int64)], axis=1)
    return rows.reshape(-1, 3), int(good.size - good.sum())


def pair_rows_numpy(pred, inst, connectivity=4, pred_is_train_ids=True):
    """(rows, bad) of one image [H, W], or (list of rows, list of bad) of a stack [N, H, W]: rows int64 [K, 3] = (kp, kg, pixels) in
    ascending (kp, kg), bad = the pixels that are counted nowhere.  `pred`: train ids 0..19, or label ids 0..33 with
    `pred_is_train_ids=False`; `inst`: the uint16 instance map (int16 holding its bits is taken as such)."""
    regions._check(connectivity)
    pred = np.asarray(pred); inst = np.asarray(inst)
    if inst.dtype == np.int16:
        inst = inst.view(np.uint16)
    if pred.dtype.kind not in "iu" or inst.dtype.kind not in "iu" or pred.ndim not in (2, 3):
        raise ValueError("prediction and instance map are integer arrays [H, W] or [N, H, W], got {} {} and {} {}".format(pred.dtype, pred.shape, inst.dtype, inst.shape))
    if pred.ndim == 2:
        return _rows_one(pred, inst, connectivity, pred_is_train_ids)
    if pred.shape != inst.shape:
        raise ValueError("a prediction of shape {} against an instance map of shape {}".format(pred.shape, inst.shape))
    res = [_rows_one(p, i, connectivity, pred_is_train_ids) for p, i in zip(pred, inst)]
    return [r[0] for r in res], [r[1] for r in res]


# ---- the table on the GPU ----------------------------------------------------------------------------------------------------------------
def _pow2_at_least(x):
    return 1 << max(0, int(x) - 1).bit_length()


def default_slots(H, W):
    """An eighth of the pixels, at least 256: a Cityscapes image has a few hundred pairs, a map salted at 5 % one pair per twenty pixels."""
    return _pow2_at_least(max(256, (int(H) * int(W) + 7) // 8))


def raw_pair_device(pred, inst, comp, slots_per_image, max_rows, table=None, rows=None):
    """One `fcn8s_op_panoptic_pair` call on device tensors: (rows [N, max_rows, 3] int64, counts [N, 4] int64, table) as device tensors, in
    the op's own order and with whatever it reports; nothing is downloaded.  `table` / `rows`: tensors to reuse when they are large enough."""
    import ctypes as C
    import torch
    from . import _lib as L
    kind, N, H, W = regions._kind(pred)
    if inst.element_size() != 2 or inst.is_floating_point() or tuple(inst.shape) != tuple(pred.shape) or not inst.is_contiguous() or inst.device != pred.device:
        raise ValueError("the instance map is a contiguous 16-bit integer tensor of the prediction's shape on its device")
    if comp.dtype != torch.int32 or tuple(comp.shape) != tuple(pred.shape) or not comp.is_contiguous() or comp.device != pred.device:
        raise ValueError("the components are a contiguous int32 tensor of the prediction's shape on its device")
    nbytes = int(L.lib.fcn8s_op_panoptic_work_bytes(N, int(slots_per_image)))
    if nbytes == 0:
        raise ValueError("panoptic: slots_per_image has to be a power of two in 1..2^28, got %r" % (slots_per_image,))
    if int(max_rows) < 1:
        raise ValueError("panoptic: max_rows has to be positive, got %r" % (max_rows,))
    if table is None or table.numel() < nbytes:
        table = torch.empty(nbytes, dtype=torch.uint8, device=pred.device)
    if rows is None or rows.numel() < N * int(max_rows) * 3:
        rows = torch.empty(N * int(max_rows) * 3, dtype=torch.int64, device=pred.device)
    counts = torch.empty((N, 4), dtype=torch.int64, device=pred.device)
    stream = C.c_void_p(torch.cuda.current_stream(pred.device).cuda_stream)
    L.check(L.lib.fcn8s_op_panoptic_pair(stream, C.c_void_p(inst.data_ptr()), C.c_void_p(pred.data_ptr()), kind, C.c_void_p(comp.data_ptr()), N, H, W,
                                         C.c_void_p(table.data_ptr()), int(slots_per_image), C.c_void_p(rows.data_ptr()), int(max_rows),
                                         C.c_void_p(counts.data_ptr())))
    return rows[:N * int(max_rows) * 3].view(N, int(max_rows), 3), counts, table


def sort_rows(rows):
    """Rows (kp, kg, n) in ascending (kp, kg): one sort on the 64-bit key kp << 32 | kg (both are below 2^32, and a table holds a pair once)."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 3)
    return rows[np.argsort(rows[:, 0].astype(np.uint64) << np.uint64(32) | rows[:, 1].astype(np.uint64), kind="stable")]


def pair_rows_device(pred, inst, connectivity=4, slots_per_image=None, max_rows=None, work=None):
    """The table of a device tensor `pred` (int64 train ids as `predict` returns them, or uint8 label ids; [H, W] or [N, H, W]) against the
    instance map `inst` (a 16-bit device tensor, or a NumPy uint16 map that is uploaded): `regions.label_device`, then
    `fcn8s_op_panoptic_pair`.  When the op reports a hash table that was too small or more rows than `max_rows`, the call is repeated with
    twice the slots / the reported row count; a table of 2 H W slots cannot be too small, so the repeats are bounded.  Returns
    (list of rows per image, sorted ascending as `pair_rows_numpy` gives them; int64 array of bad pixels per image; work) -- `work`: a dict
    of device scratch to hand to the next call."""
    import torch
    from .cityscapes_eval import instance_map_tensor
    regions._check(connectivity)
    kind, N, H, W = regions._kind(pred)
    if H * W > MAX_PIXELS:
        raise ValueError("panoptic: an image has at most 2^26 pixels, got {}".format(H * W))
    if not isinstance(inst, torch.Tensor):
        inst = instance_map_tensor(inst, pred.device)
    inst = inst.to(pred.device).contiguous()
    work = {} if work is None else work
    comp, _ar, work["regions"] = regions.label_device(pred, connectivity=connectivity, area=False, work=work.get("regions"))
    full = _pow2_at_least(2 * H * W)
    # without an explicit size the call starts where the last call on this `work` ended: the images of a directory are alike, and a table
    # that had to be doubled for one of them is not found too small again for each of the next
    slots = min(full, max(default_slots(H, W), work.get("slots", 0))) if slots_per_image is None else int(slots_per_image)
    rows_cap = max(DEFAULT_MAX_ROWS, work.get("max_rows", 0)) if max_rows is None else int(max_rows)
    while True:
        rows, counts, work["table"] = raw_pair_device(pred, inst, comp, slots, rows_cap, table=work.get("table"), rows=work.get("rows"))
        work["rows"] = rows.view(-1)
        cnt = counts.cpu().numpy()
        if cnt[:, 2].any():
            if slots >= full:
                raise RuntimeError("panoptic: a hash table of 2 H W slots reported an overflow")
            slots = min(full, slots * 2)
            continue
        if int(cnt[:, 0].max()) > rows_cap:
            rows_cap = int(cnt[:, 0].max())                                     # exact: the table held every pair
            continue
        break
    work["slots"], work["max_rows"] = slots, rows_cap
    if ((cnt[:, 1] + cnt[:, 3]) != H * W).any():
        raise RuntimeError("panoptic: counted and bad pixels do not add up to the image: {}".format(cnt.tolist()))
    host = rows[:, :max(int(cnt[:, 0].max()), 1)].cpu().numpy()
    return [sort_rows(host[n, :int(cnt[n, 0])]) for n in range(N)], cnt[:, 1].copy(), work


# ---- scores ------------------------------------------------------------------------------------------------------------------------------
def new_stats():
    return {"tp": np.zeros(NUM_TRAIN_IDS, np.int64), "fp": np.zeros(NUM_TRAIN_IDS, np.int64), "fn": np.zeros(NUM_TRAIN_IDS, np.int64),
            "iou_sum": np.zeros(NUM_TRAIN_IDS, np.float64)}


def stats_add(stats, rows):
    """One image's rows (kp, kg, n), ascending (kp, kg), into the running tp / fp / fn / iou_sum per train id."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 3)
    if rows.shape[0] == 0:
        return stats
    kp, kg, n = rows[:, 0], rows[:, 1], rows[:, 2]
    first = np.concatenate([[True], kp[1:] != kp[:-1]])                          # kp ascends: its segments are stretches of rows
    up, ip = kp[first], np.cumsum(first) - 1
    if (up[1:] <= up[:-1]).any():
        raise ValueError("panoptic rows have to be in ascending (kp, kg) order")
    ug, ig = np.unique(kg, return_inverse=True)
    total = lambda idx, w, size: np.bincount(idx, weights=w, minlength=size).astype(np.int64)      # (sums of at most 2^26 pixels: exact in float64)
    area_p, area_g = total(ip, n, up.size), total(ig.ravel(), n, ug.size)
    void_p = total(ip[kg == 0], n[kg == 0], up.size)
    cp, cg = key_class(kp), key_class(kg)
    own_crowd = key_is_crowd(kg) & (cp == cg)
    crowd_p = total(ip[own_crowd], n[own_crowd], up.size)
    cand = (kp != 0) & (kg != 0) & ~key_is_crowd(kg) & (cp == cg)
    matched_p = np.zeros(up.size, bool); matched_g = np.zeros(ug.size, bool)
    rc = np.nonzero(cand)[0]
    iou = n[rc].astype(np.float64) / (area_p[ip[rc]] + area_g[ig[rc]] - n[rc] - void_p[ip[rc]]).astype(np.float64)      # (all below 2^26: exact)
    hit = iou > 0.5
    for r, v in zip(rc[hit].tolist(), iou[hit].tolist()):                        # ascending rows: the order of the float sum
        c = int(cp[r])
        stats["tp"][c] += 1
        stats["iou_sum"][c] += v
        matched_p[ip[r]] = True; matched_g[ig[r]] = True
    lost = (ug != 0) & ~key_is_crowd(ug) & ~matched_g
    np.add.at(stats["fn"], key_class(ug[lost]), 1)
    spare = (up != 0) & ~matched_p & ~(2 * (void_p + crowd_p) > area_p)           # (void + crowd) / area > 0.5 in integers
    np.add.at(stats["fp"], key_class(up[spare]), 1)
    return stats


def _quality(tp, fp, fn, iou_sum):
    denom = tp + 0.5 * fp + 0.5 * fn
    if denom == 0:
        return float('nan'), float('nan'), float('nan')
    return iou_sum / denom, (iou_sum / tp if tp else 0.0), tp / denom


def results(stats):
    """The result entries: `panopticQuality` {All, Things, Stuff: {pq, sq, rq, n}} (n = the classes averaged: those with tp + fp + fn > 0),
    `panopticClassScores` {class name: {pq, sq, rq, tp, fp, fn, iouSum}} for the 19 evaluated classes, and the integer tables
    `panopticTp` / `panopticFp` / `panopticFn` (int64 [20], by train id) with the float64 `panopticIouSum`."""
    per = OrderedDict()
    for c in range(1, NUM_TRAIN_IDS):
        tp, fp, fn, s = int(stats["tp"][c]), int(stats["fp"][c]), int(stats["fn"][c]), float(stats["iou_sum"][c])
        pq, sq, rq = _quality(tp, fp, fn, s)
        per[TRAIN_ID_NAMES[c]] = OrderedDict((("pq", pq), ("sq", sq), ("rq", rq), ("tp", tp), ("fp", fp), ("fn", fn), ("iouSum", s)))

    def mean(ids):
        used = [per[TRAIN_ID_NAMES[c]] for c in ids if per[TRAIN_ID_NAMES[c]]["tp"] + per[TRAIN_ID_NAMES[c]]["fp"] + per[TRAIN_ID_NAMES[c]]["fn"] > 0]
        out = OrderedDict((k, (sum(u[k] for u in used) / len(used)) if used else float('nan')) for k in ("pq", "sq", "rq"))
        out["n"] = len(used)
        return out

    return {"panopticQuality": OrderedDict((("All", mean(range(1, NUM_TRAIN_IDS))), ("Things", mean(range(FIRST_THING, NUM_TRAIN_IDS))),
                                            ("Stuff", mean(range(1, FIRST_THING))))),
            "panopticClassScores": per,
            "panopticTp": stats["tp"].copy(), "panopticFp": stats["fp"].copy(), "panopticFn": stats["fn"].copy(),
            "panopticIouSum": stats["iou_sum"].copy()}
