#!/usr/bin/env python3
"""Generates tests/golden/cityscapes_instances.npz by RUNNING the reference evaluator with its instance-level half switched on
(evalInstLevelScore = True, its default), under the stubs tests/golden/make_golden.py uses (never shipped: only arrays are committed).

    python tests/golden/make_cityscapes_instances.py        # needs /root/reference

Sources exercised (reference file:line):
  cityscapesscripts/evaluation/evalPixelLevelSemanticLabeling.py:184-215   generateInstanceStats
  ...:454-546  evaluateImgLists on PNG triples (prediction, *_labelIds, *_instanceIds), CSUPPORT = False
  ...:550-635  evaluatePair replayed on a fresh generateInstanceStats: the raw tp / fn / tpWeighted / fnWeighted
  ...:258-278, 332-351, 355-376  the iIoU scores and the result dictionary

Six 48 x 96 triples.  Made explicit rather than left to the seed: an image without any instance (0); a group region (an instance-class
label without instance id, value < 1000); instances of caravan / trailer (skipped, yet inside the vehicle id list); an instance with
tp = 0; an instance predicted as another label of its category (tp < cattp); two instances of one label in one image and the same v in
two images; a value of exactly 24000; predictions that contain label 0.  The script checks each of them before it writes.
"""
import json
import os
import sys
import tempfile
import types

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
H, W, NIMG = 48, 96, 6
STUFF = [0, 4, 7, 8, 11, 12, 17, 20, 21, 22, 23]                  # background labels, two of them ignored
THINGS = [24, 25, 26, 27, 28, 29, 30, 31, 32, 33]                  # labels with instances, caravan / trailer included
NAMES = ["frankfurt_000000_000294", "frankfurt_000001_007973", "lindau_000003_000019", "lindau_000010_000019", "munster_000005_000019",
         "munster_000101_000019"]


def load_evaluator():
    if not hasattr(np, "bool"):
        np.bool = bool
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
    import evalPixelLevelSemanticLabeling as ev
    ev.CSUPPORT = False
    ev.args.evalInstLevelScore = True; ev.args.evalPixelAccuracy = False; ev.args.quiet = True
    return ev, lab_mod


def rect(a, y, x, h, w, value):
    a[y:y + h, x:x + w] = value


def make_maps(lab_mod):
    rng = np.random.default_rng(2026)
    id2train = np.array([lab_mod.id2label[i].trainId for i in range(34)])
    train2id = np.array([0] + [lab_mod.trainId2label[t].id for t in range(1, 20)])
    gts = np.zeros((NIMG, H, W), np.uint8); insts = np.zeros((NIMG, H, W), np.uint16)
    for n in range(NIMG):
        bg = rng.choice(STUFF, (H // 8, W // 8))
        gts[n] = np.kron(bg, np.ones((8, 8), np.int64))
        insts[n] = gts[n]
        if n == 0:
            continue                                              # image 0: no instance at all
        for k in range(12):
            L = int(rng.choice(THINGS))
            h, w = int(rng.integers(3, 20)), int(rng.integers(3, 30))
            y, x = int(rng.integers(0, H - h)), int(rng.integers(0, W - w))
            rect(gts[n], y, x, h, w, L)
            rect(insts[n], y, x, h, w, L if rng.random() < 0.2 else L * 1000 + k + 3)
    # the explicit cases, drawn last so that nothing covers them
    rect(gts[0], 4, 4, 6, 10, 26); rect(insts[0], 4, 4, 6, 10, 26)                    # a group region (cars without ids) in the instance-free image
    rect(gts[1], 2, 2, 5, 7, 24); rect(insts[1], 2, 2, 5, 7, 24000)                   # exactly 24000
    rect(gts[1], 10, 2, 6, 9, 26); rect(insts[1], 10, 2, 6, 9, 26001)                 # two cars in one image ...
    rect(gts[1], 10, 14, 6, 9, 26); rect(insts[1], 10, 14, 6, 9, 26002)
    rect(gts[2], 30, 40, 7, 12, 26); rect(insts[2], 30, 40, 7, 12, 26001)             # ... and 26001 again in another
    rect(gts[3], 2, 60, 8, 14, 29); rect(insts[3], 2, 60, 8, 14, 29000)               # caravan and trailer instances (skipped)
    rect(gts[3], 14, 60, 8, 14, 30); rect(insts[3], 14, 60, 8, 14, 30001)
    rect(gts[3], 30, 4, 6, 6, 25); rect(insts[3], 30, 4, 6, 6, 25)                    # a rider group
    rect(gts[4], 20, 20, 9, 9, 28); rect(insts[4], 20, 20, 9, 9, 28007)               # tp = 0 (see below)
    rect(gts[5], 5, 50, 10, 16, 27); rect(insts[5], 5, 50, 10, 16, 27999)             # tp < cattp (see below)
    # predictions: the ground truth through the train ids and back (ignored labels -> 0), then 35 % of the 4 x 4 blocks damaged
    preds = train2id[id2train[gts]].astype(np.uint8)
    damaged = np.kron(rng.random((NIMG, H // 4, W // 4)) < 0.35, np.ones((4, 4), bool))
    noise = np.kron(rng.choice([0, 7, 8, 11, 21, 23, 24, 25, 26, 27, 28, 31, 32, 33], (NIMG, H // 4, W // 4)), np.ones((4, 4), np.int64))
    preds[damaged] = noise[damaged]
    rect(preds[4], 20, 20, 9, 9, 7)                               # the bus 28007 predicted as road: tp = 0, cattp = 0
    rect(preds[5], 5, 50, 10, 16, 26)                             # the truck 27999 predicted as car: tp = 0 < cattp = size
    rect(preds[5], 5, 50, 4, 16, 27)                              # ... partly right: 0 < tp < cattp
    rect(preds[3], 2, 60, 8, 14, 26)                              # the caravan predicted as car
    rect(preds[2], 0, 0, 4, 8, 0)                                 # label 0 in a prediction
    return gts, insts, preds


def check_cases(gts, insts, preds):
    assert not (insts[0] > 1000).any() and (insts[0] == 26).any()
    assert (insts[1] == 24000).any() and (insts[1] == 26001).any() and (insts[1] == 26002).any() and (insts[2] == 26001).any()
    assert (insts[3] == 29000).any() and (insts[3] == 30001).any() and (preds[3][insts[3] == 29000] == 26).all()
    m = insts[4] == 28007
    assert m.any() and not (preds[4][m] == 28).any()
    m = insts[5] == 27999
    tp, cattp = int((preds[5][m] == 27).sum()), int(np.isin(preds[5][m], range(26, 34)).sum())
    assert 0 < tp < cattp == int(m.sum())
    assert (preds == 0).any() and (preds[2][:4, :8] == 0).all()
    assert ((insts < 1000) & np.isin(insts, [24, 25, 26, 27, 28, 31, 32, 33])).any()


def main():
    from PIL import Image
    ev, lab_mod = load_evaluator()
    gts, insts, preds = make_maps(lab_mod)
    check_cases(gts, insts, preds)
    with tempfile.TemporaryDirectory() as d:
        gt_files, pred_files = [], []
        for n, nm in enumerate(NAMES):
            city = nm.split("_")[0]
            os.makedirs(os.path.join(d, "gtFine", "val", city), exist_ok=True); os.makedirs(os.path.join(d, "results"), exist_ok=True)
            gf = os.path.join(d, "gtFine", "val", city, nm + "_gtFine_labelIds.png")
            Image.fromarray(gts[n]).save(gf)
            Image.fromarray(insts[n]).save(gf.replace("labelIds", "instanceIds"))
            back = np.array(Image.open(gf.replace("labelIds", "instanceIds")))
            assert back.dtype in (np.uint16, np.int32) and np.array_equal(back, insts[n])            # the uint16 PNG survives PIL
            pf = os.path.join(d, "results", nm + "_leftImg8bit.png")
            Image.fromarray(preds[n]).save(pf)
            gt_files.append(gf); pred_files.append(pf)
        ev.args.exportFile = os.path.join(d, "out", "resultPixelLevelSemanticLabeling.json")
        res = ev.evaluateImgLists(pred_files, gt_files, ev.args)
        written = json.load(open(ev.args.exportFile))
        # the raw sums: evaluatePair replayed on fresh accumulators
        conf = ev.generateMatrix(ev.args); stats = ev.generateInstanceStats(ev.args)
        for pf, gf in zip(pred_files, gt_files):
            ev.evaluatePair(pf, gf, conf, stats, {}, ev.args)
    assert np.array_equal(conf, np.asarray(res["confMatrix"], dtype=conf.dtype))
    cls_names = list(res["classScores"]); cat_names = list(res["categoryScores"])
    fields = ["tp", "fn", "tpWeighted", "fnWeighted"]
    inst_classes = list(stats["classes"]); inst_cats = list(stats["categories"])
    out = dict(
        names=np.array(NAMES), gts=gts, insts=insts, preds=preds,
        conf=np.asarray(res["confMatrix"], dtype=np.int64),
        class_names=np.array(cls_names), cat_names=np.array(cat_names),
        class_scores=np.array([res["classScores"][k] for k in cls_names], np.float64),
        class_inst_scores=np.array([res["classInstScores"][k] for k in cls_names], np.float64),
        cat_scores=np.array([res["categoryScores"][k] for k in cat_names], np.float64),
        cat_inst_scores=np.array([res["categoryInstScores"][k] for k in cat_names], np.float64),
        averages=np.array([res["averageScoreClasses"], res["averageScoreInstClasses"], res["averageScoreCategories"],
                           res["averageScoreInstCategories"]], np.float64),
        stat_fields=np.array(fields), inst_class_names=np.array(inst_classes), inst_cat_names=np.array(inst_cats),
        inst_class_stats=np.array([[float(stats["classes"][c][f]) for f in fields] for c in inst_classes], np.float64),
        inst_cat_stats=np.array([[float(stats["categories"][c][f]) for f in fields] for c in inst_cats], np.float64),
        inst_cat_label_ids=np.array([",".join(str(i) for i in stats["categories"][c]["labelIds"]) for c in inst_cats]),
        avg_class_size_names=np.array(sorted(ev.args.avgClassSize)),
        avg_class_size=np.array([ev.args.avgClassSize[k] for k in sorted(ev.args.avgClassSize)], np.float64),
        json_keys=np.array(sorted(written)),
        prior_names=np.array(list(res["priors"])), priors=np.array([res["priors"][k] for k in res["priors"]], np.float64),
        label_names=np.array(list(res["labels"])), label_ids=np.array([res["labels"][k] for k in res["labels"]], np.int64))
    assert np.isfinite(out["class_inst_scores"]).sum() == 8 and np.isfinite(out["cat_inst_scores"]).sum() == 2
    path = os.path.join(HERE, "cityscapes_instances.npz")
    np.savez_compressed(path, **out)
    print("written", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
