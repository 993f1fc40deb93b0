#!/usr/bin/env python3
"""Generates tests/golden/instance_ap_cases.npz by RUNNING the reference's instance-level evaluator (never shipped: only arrays are
committed), under the stubs tests/golden/make_cityscapes_instances.py uses plus `np.float`.

    python tests/golden/make_instance_ap_cases.py        # needs /root/reference, scipy and Pillow

Sources exercised (reference file:line):
  cityscapesscripts/evaluation/instances2dict.py:14-53 and instance.py   the ground-truth instances of an instance-id PNG (called directly:
                                                                          the evaluator's cache file gtInstancesFile lies in the read-only tree)
  cityscapesscripts/evaluation/evalInstanceLevelSemanticLabeling.py:218-349   matchGtWithPreds / assignGt2Preds on result text files and mask PNGs
  ...:352-547   evaluateMatches: the ap array [1, 8, 10]
  ...:549-575   computeAverages

The inputs are made on a route that shares nothing with fcn8s_tensorflow_amd/instances.py, regions.py or the kernel: the predicted
instances are the components of `scipy.ndimage.label` per thing class, ordered by their first pixel; their confidences and the recorded
rows are plain Python integer sums over the pixels.

A case is a small data set: labels [N, H, W] uint8 train ids (what the pixels ended up with), softmax rows [N, H, W, 20] float32, instance
maps [N, H, W] uint16 and a connectivity.  Recorded per case: the inputs, the rows (kp, v, n, s) per image, `ap` [8, 10], the averages
(allAp, allAp50%, then ap and ap50% per class), and the match lists flattened to integers (`flatten` below) with the confidences beside
them.  Made explicit and asserted before anything is written: a ground-truth instance under 100 pixels that shields the prediction on it;
a group region; a prediction more than half on void; a caravan instance 29001 under a predicted car (not void); a class with ground truth
and no prediction (AP 0); a class with predictions and no ground truth (NaN); two touching cars predicted as one component; an IoU of
exactly 0.5 (n = 50, areas 100 and 50: no match at 0.5); equal confidences; labels >= 20; NaN, 1.0 and out-of-range probabilities; an
image without things; two squares that touch at a corner (one instance under 8-connectivity, two under 4); shapes from 1 x 1 to
2 x 48 x 80.
"""
import os
import sys
import tempfile
import types

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
C = 20
ONE = 1 << 24
ROAD, PERSON, RIDER, CAR, BUS, TRAIN, MOTORCYCLE, BICYCLE = 1, 12, 13, 14, 16, 17, 18, 19            # train ids
QS = np.array([0.9, 0.8, 0.7, 0.55, 0.95], np.float32)


def load_evaluator():
    if not hasattr(np, "bool"):
        np.bool = bool
    if not hasattr(np, "float"):
        np.float = float                                           # evalInstanceLevelSemanticLabeling.py:395 predates NumPy 1.24
    import PIL
    if not hasattr(PIL, "PILLOW_VERSION"):
        PIL.PILLOW_VERSION = PIL.__version__                      # csHelpers.py:16 predates Pillow 7
    src = open(os.path.join(REF, "cityscapesscripts/helpers/labels.py")).read().split("\n")
    lab_mod = types.ModuleType("labels")
    exec("\n".join(src[:188]), lab_mod.__dict__)                   # labels.py:191 overflows on NumPy 2; the table above it is intact
    sys.modules["labels"] = lab_mod
    sys.path.insert(0, os.path.join(REF, "cityscapesscripts", "helpers"))
    sys.path.insert(0, os.path.join(REF, "cityscapesscripts", "evaluation"))
    os.environ.setdefault("CITYSCAPES_DATASET", "/tmp")
    import evalInstanceLevelSemanticLabeling as ev
    from instances2dict import instances2dict
    ev.args.quiet = True; ev.args.JSONOutput = False
    return ev, instances2dict, lab_mod


def rect(a, y, x, h, w, value):
    a[y:y + h, x:x + w] = value


def softmax_rows(labels, q):
    """Rows in which the label's column holds q and the other columns share the rest (0.05 each where q is no number in [0, 1])."""
    H, W = labels.shape
    prob = np.empty((H, W, C), np.float32)
    with np.errstate(invalid="ignore"):
        rest = np.where((q >= 0) & (q <= 1), (np.float32(1) - q) / np.float32(C - 1), np.float32(0.05)).astype(np.float32)
    prob[:] = rest[:, :, None]
    col = np.where(labels < C, labels, 0)
    np.put_along_axis(prob, col[:, :, None].astype(np.int64), q[:, :, None], axis=2)
    return prob


def base_q(H, W):
    y, x = np.mgrid[0:H, 0:W]
    return QS[(y // 3 + x // 5) % QS.size].copy()


def scene():
    H, W = 48, 80
    lab = np.full((2, H, W), ROAD, np.uint8); inst = np.full((2, H, W), 7, np.uint16)
    q = np.stack([base_q(H, W), base_q(H, W)])
    a, g = lab[0], inst[0]
    rect(g, 2, 2, 20, 20, 26001); rect(a, 2, 4, 20, 20, CAR)                  # a car, well predicted (IoU 360 / 440)
    rect(g, 2, 30, 6, 10, 24003); rect(a, 2, 30, 6, 10, PERSON)               # a person of 60 pixels: ignored, and it shields the prediction on it
    rect(g, 10, 30, 10, 12, 26); rect(a, 10, 30, 10, 18, CAR)                 # a group of cars under a larger predicted car (120 of 180)
    rect(g, 24, 2, 10, 12, 0); rect(a, 24, 2, 10, 16, MOTORCYCLE)             # a prediction with 120 of 160 pixels on void
    rect(g, 24, 60, 12, 12, 32001); rect(a, 24, 61, 12, 12, MOTORCYCLE)
    rect(g, 24, 24, 10, 12, 29001); rect(a, 24, 24, 10, 12, CAR)              # a caravan instance under a predicted car: not void, a false positive
    rect(g, 36, 2, 12, 12, 28001)                                             # a bus that nothing predicts: AP 0
    rect(a, 38, 20, 6, 10, TRAIN)                                             # a train where none is: NaN
    rect(g, 36, 36, 10, 10, 26002); rect(g, 36, 46, 10, 10, 26003); rect(a, 36, 36, 10, 20, CAR)      # two touching cars, one component: IoU 0.5 each
    rect(g, 12, 50, 10, 10, 25001); rect(a, 12, 50, 5, 10, RIDER)             # IoU exactly 0.5: 50 / (100 + 50 - 50)
    rect(g, 0, 60, 12, 12, 33001); rect(a, 2, 62, 4, 4, BICYCLE); rect(a, 6, 66, 4, 4, BICYCLE)       # two squares that touch at a corner
    rect(a, 46, 70, 2, 10, 200); a[44, 70] = 20                               # labels >= 20
    rect(q[0], 24, 24, 10, 12, 0.625); rect(q[0], 36, 36, 10, 20, 0.625)      # equal confidences of two false positives of one class
    q[0, 5, 5] = np.nan; q[0, 5, 6] = 1.0; q[0, 5, 7] = -0.25; q[0, 5, 8] = 1.5; q[0, 5, 9] = np.inf; q[0, 5, 10] = 0.0
    a, g = lab[1], inst[1]
    rect(g, 5, 5, 20, 30, 26001); rect(a, 5, 5, 20, 26, CAR)                  # the same value 26001 in another image
    rect(g, 30, 40, 15, 10, 24001); rect(a, 30, 40, 15, 9, PERSON)
    rng = np.random.default_rng(7)
    specks = rng.random((H, W)) < 0.01
    specks[:, :52] = False
    a[specks] = PERSON                                                        # one-pixel persons on the road: what the measure is a detector of
    return lab, np.stack([softmax_rows(lab[i], q[i]) for i in range(2)]), inst


def make_cases():
    cases = []
    lab, prob, inst = scene()
    cases.append(("scene_c4", 4, lab, prob, inst))
    cases.append(("scene_c8", 8, lab, prob, inst))
    lab = np.full((1, 1, 1), RIDER, np.uint8)
    cases.append(("one_pixel", 4, lab, softmax_rows(lab[0], np.full((1, 1), 0.7, np.float32))[None], np.full((1, 1, 1), 25001, np.uint16)))
    lab = np.full((1, 16, 24), ROAD, np.uint8); inst = np.full((1, 16, 24), 7, np.uint16)
    rect(inst[0], 2, 2, 10, 12, 26001)
    cases.append(("no_things", 8, lab, softmax_rows(lab[0], base_q(16, 24))[None], inst))          # an image without predicted things
    return cases


def predicted_instances(labels, prob, connectivity):
    """[(first pixel, train id, mask, Python int sum of terms)] in the order of the first pixel -- scipy's components, plain integer sums."""
    from scipy import ndimage
    structure = np.ones((3, 3), int) if connectivity == 8 else None
    out = []
    for c in range(12, 20):
        comp, k = ndimage.label(labels == c, structure=structure)
        for i in range(1, k + 1):
            mask = comp == i
            total = 0
            for y, x in zip(*np.nonzero(mask)):
                qv = prob[y, x, c]
                if qv >= 0 and qv <= 1:
                    total += int(np.rint(np.float32(qv) * np.float32(ONE)))
            out.append((int(np.flatnonzero(mask)[0]), c, mask, total))
    return sorted(out, key=lambda r: r[0])


def rows_of(labels, prob, inst, preds):
    kp = np.zeros(labels.shape, np.int64)
    for first, c, mask, _total in preds:
        kp[mask] = (1 << 31) | (first << 5) | c
    table = {}
    H, W = labels.shape
    for y in range(H):
        for x in range(W):
            key = (int(kp[y, x]), int(inst[y, x]))
            t = 0
            if key[0]:
                qv = prob[y, x, labels[y, x]]
                if qv >= 0 and qv <= 1:
                    t = int(np.rint(np.float32(qv) * np.float32(ONE)))
            e = table.setdefault(key, [0, 0])
            e[0] += 1; e[1] += t
    return np.array([[k[0], k[1], e[0], e[1]] for k, e in sorted(table.items())], np.int64).reshape(-1, 4)


def flatten(ev, matches, keys):
    """Per image: the number of predictions, then per prediction (in the evaluator's predID order over all classes) labelID, pixelCount,
    voidIntersection, the number of matched ground-truth instances and per match (instID, its pixelCount, intersection); then the number
    of ground-truth instances of the evaluated labels and per instance (ascending instID) instID, labelID, pixelCount, the number of
    matched predictions and per match (predID, intersection).  The confidences go beside it, in prediction order."""
    ints, confs = [], []
    for key in keys:
        preds = sorted((p for lst in matches[key]["prediction"].values() for p in lst), key=lambda p: p["predID"])
        ints.append(len(preds))
        for p in preds:
            ints += [p["labelID"], p["pixelCount"], p["voidIntersection"], len(p["matchedGt"])]
            for g in p["matchedGt"]:
                ints += [g["instID"], g["pixelCount"], g["intersection"]]
            confs.append(p["confidence"])
        gts = sorted((g for lst in matches[key]["groundTruth"].values() for g in lst), key=lambda g: g["instID"])
        ints.append(len(gts))
        for g in gts:
            ints += [g["instID"], g["labelID"], g["pixelCount"], len(g["matchedPred"])]
            for p in g["matchedPred"]:
                ints += [p["predID"], p["intersection"]]
    return np.array(ints, np.int64), np.array(confs, np.float64)


def run_case(ev, instances2dict, lab_mod, name, connectivity, labels, prob, inst):
    from PIL import Image
    train2id = {t: lab_mod.trainId2label[t].id for t in range(12, 20)}
    rows = []
    with tempfile.TemporaryDirectory() as d:
        d = os.path.realpath(d)
        gt_files, txt_files = [], []
        for n in range(labels.shape[0]):
            stem = "%s_%06d_000019" % ("aachen", n)
            gf = os.path.join(d, "gt", stem + "_gtFine_instanceIds.png")
            os.makedirs(os.path.dirname(gf), exist_ok=True)
            Image.fromarray(inst[n]).save(gf)
            assert np.array_equal(np.array(Image.open(gf)), inst[n])
            preds = predicted_instances(labels[n], prob[n], connectivity)
            rows.append(rows_of(labels[n], prob[n], inst[n], preds))
            os.makedirs(os.path.join(d, "results", stem), exist_ok=True)
            lines = []
            for k, (first, c, mask, total) in enumerate(preds):
                rel = os.path.join(stem, "%04d.png" % k)
                Image.fromarray(mask.astype(np.uint8) * 255).save(os.path.join(d, "results", rel))
                lines.append("%s %d %r\n" % (rel, train2id[c], total / (int(mask.sum()) * ONE)))
            tf = os.path.join(d, "results", stem + ".txt")
            open(tf, "w").writelines(lines)
            gt_files.append(gf); txt_files.append(tf)
        ev.args.predictionPath = os.path.join(d, "results")
        ev.setInstanceLabels(ev.args)
        gt_instances = instances2dict(gt_files, False)
        matches = ev.matchGtWithPreds(txt_files, gt_files, gt_instances, ev.args)
        ap = ev.evaluateMatches(matches, ev.args)
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            avg = ev.computeAverages(ap, ev.args)
        ints, confs = flatten(ev, matches, [os.path.abspath(g) for g in gt_files])
    assert ap.shape == (1, 8, 10)
    names = list(ev.args.instLabels)
    averages = np.array([avg["allAp"], avg["allAp50%"]] + [avg["classes"][k][f] for k in names for f in ("ap", "ap50%")], np.float64)
    return dict(ap=ap[0], averages=averages, matches=ints, confidences=confs, rows=rows, names=names)


def check_scene(r4, r8):
    names = r4["names"]
    ap4, ap8 = r4["ap"], r8["ap"]
    assert names == ["person", "rider", "car", "truck", "bus", "train", "motorcycle", "bicycle"]
    assert (ap4[names.index("bus")] == 0).all()                                   # ground truth, no prediction
    assert np.isnan(ap4[names.index("train")]).all() and np.isnan(ap4[names.index("truck")]).all()      # predictions without ground truth; neither
    assert ap4[names.index("rider"), 0] == 0                                      # IoU exactly 0.5 is no match at 0.5
    assert 0 < ap4[names.index("car"), 0] < 1                                     # a match, hard false negatives (the touching cars) and false positives
    assert ap4[names.index("car"), 0] > ap4[names.index("car"), 9]
    assert ap4[names.index("motorcycle"), 0] == 1 and ap4[names.index("motorcycle"), 9] < 1           # the prediction on void is dropped below 0.75 only
    assert ap4[names.index("person"), 0] > 0                                      # the specks are false positives; the 60-pixel person is shielded
    assert len(r4["confidences"]) == len(r8["confidences"]) + 1                   # the corner-touching squares
    c = r4["confidences"]
    assert len(c) != len(np.unique(c))                                            # equal confidences
    assert np.isfinite(c).all() and (c >= 0).all() and (c <= 1).all()


def main():
    ev, instances2dict, lab_mod = load_evaluator()
    out = {}
    results = {}
    names = []
    for name, connectivity, labels, prob, inst in make_cases():
        r = run_case(ev, instances2dict, lab_mod, name, connectivity, labels, prob, inst)
        results[name] = r
        names.append(name)
        out[name + "_connectivity"] = np.int64(connectivity)
        out[name + "_labels"] = labels; out[name + "_prob"] = prob; out[name + "_inst"] = inst
        out[name + "_ap"] = r["ap"]; out[name + "_averages"] = r["averages"]
        out[name + "_matches"] = r["matches"]; out[name + "_confidences"] = r["confidences"]
        for n, rows in enumerate(r["rows"]):
            out["%s_rows%d" % (name, n)] = rows
            assert rows[:, 2].sum() == labels[n].size
    check_scene(results["scene_c4"], results["scene_c8"])
    lab = out["scene_c4_labels"]
    assert (lab >= 20).any() and np.isnan(out["scene_c4_prob"]).any() and (out["scene_c4_prob"] == 1.0).any()
    assert np.isnan(results["one_pixel"]["ap"]).all()                              # a one-pixel rider on a one-pixel instance: ignored ground truth
    assert results["no_things"]["ap"][2, 0] == 0 and len(results["no_things"]["confidences"]) == 0
    out["case_names"] = np.array(names)
    out["inst_label_names"] = np.array(results["scene_c4"]["names"])
    path = os.path.join(HERE, "instance_ap_cases.npz")
    np.savez_compressed(path, **out)
    print("written", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
