#!/usr/bin/env python
"""Generates tests/golden/panoptic_cases.npz: small predictions and instance maps with the segment pair tables and the panoptic-quality counts
of the definition in include/fcn8s_hip.h at fcn8s_op_panoptic_pair, computed by a route that shares nothing with
fcn8s_tensorflow_amd/panoptic.py, regions.py or the kernels: `scipy.ndimage.label` per thing class with `ndimage.minimum` for the component
ids, the label table typed in below, and plain Python dict counting pixel by pixel.  Needs SciPy; the tests only read the file.

    python tests/golden/make_panoptic_cases.py

Layout of the file: `index` is a JSON list of cases {name, images}; arrays `<name>.pred` (uint8 train ids, [H, W] or [N, H, W]), `<name>.inst`
(uint16, the same shape), and for c in (4, 8): `<name>.c<c>.rows<k>` (int64 [K, 3] = kp, kg, pixels of image k in ascending (kp, kg)),
`<name>.c<c>.bad` (int64 [images]), `<name>.c<c>.tp` / `.fp` / `.fn` (int64 [20], by train id, over the case's images), `.iou_sum`
(float64 [20]), `.pq` (float64 [3, 3]: All / Things / Stuff x pq, sq, rq) and `.pqn` (int64 [3], the classes averaged).
"""
import json
import os

import numpy as np
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
CROSS = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], bool)
FULL = np.ones((3, 3), bool)
# label id -> train id (labels.py as the reference's author modified it): every label that is not listed is void
TRAIN = {7: 1, 8: 2, 11: 3, 12: 4, 13: 5, 17: 6, 19: 7, 20: 8, 21: 9, 22: 10, 23: 11,
         24: 12, 25: 13, 26: 14, 27: 15, 28: 16, 31: 17, 32: 18, 33: 19}
THINGS = range(12, 20)
STUFF = range(1, 12)


def table(pred, inst, conn):
    """{(kp, kg): pixels} and the bad pixels of one image."""
    H, W = pred.shape
    index = np.arange(H * W).reshape(H, W)
    comp = np.zeros((H, W), np.int64)
    for c in THINGS:
        lbl, n = ndimage.label(pred == c, structure=CROSS if conn == 4 else FULL)
        if n:
            ids = np.asarray(ndimage.minimum(index, lbl, np.arange(1, n + 1))).astype(np.int64)
            comp[lbl > 0] = ids[lbl[lbl > 0] - 1]
    counts, bad = {}, 0
    for y in range(H):
        for x in range(W):
            a, v = int(pred[y, x]), int(inst[y, x])
            lab = v if v < 1000 else v // 1000
            if not 0 <= a <= 19 or lab > 33:
                bad += 1
                continue
            kp = 0 if a == 0 else (a if a < 12 else (1 << 31) + (int(comp[y, x]) << 5) + a)
            t = TRAIN.get(lab, 0)
            if t < 12:
                kg = t
            elif v >= 1000:
                kg = (1 << 31) + ((v % 1000) << 5) + t
            else:
                kg = (1 << 30) + t
            counts[(kp, kg)] = counts.get((kp, kg), 0) + 1
    return counts, bad


def score(counts, tp, fp, fn, iou_sum):
    cls = lambda k: k % 32
    crowd = lambda k: (k >> 30) == 1
    area_p, area_g = {}, {}
    for (kp, kg), n in counts.items():
        area_p[kp] = area_p.get(kp, 0) + n
        area_g[kg] = area_g.get(kg, 0) + n
    hit_p, hit_g = set(), set()
    for (kp, kg) in sorted(counts):
        n = counts[(kp, kg)]
        if kp == 0 or kg == 0 or crowd(kg) or cls(kp) != cls(kg):
            continue
        iou = n / (area_p[kp] + area_g[kg] - n - counts.get((kp, 0), 0))
        if iou > 0.5:
            tp[cls(kp)] += 1
            iou_sum[cls(kp)] += iou
            hit_p.add(kp); hit_g.add(kg)
    for kg in area_g:
        if kg != 0 and not crowd(kg) and kg not in hit_g:
            fn[cls(kg)] += 1
    for kp in area_p:
        if kp == 0 or kp in hit_p:
            continue
        if (counts.get((kp, 0), 0) + counts.get((kp, (1 << 30) + cls(kp)), 0)) / area_p[kp] > 0.5:
            continue
        fp[cls(kp)] += 1


def averages(tp, fp, fn, iou_sum):
    out, ns = np.full((3, 3), np.nan), np.zeros(3, np.int64)
    for g, ids in enumerate((range(1, 20), THINGS, STUFF)):
        vals = []
        for c in ids:
            if tp[c] + fp[c] + fn[c] == 0:
                continue
            d = tp[c] + 0.5 * fp[c] + 0.5 * fn[c]
            vals.append((iou_sum[c] / d, iou_sum[c] / tp[c] if tp[c] else 0.0, tp[c] / d))
        ns[g] = len(vals)
        if vals:
            out[g] = np.mean(np.asarray(vals), axis=0)
    return out, ns


def scene(rng, H, W, cells, salt, shift=(1, 2)):
    """A Voronoi ground truth of stuff, instances, crowd regions, ignored labels and one value beyond label 33, and a prediction that is its
    train-id map moved by `shift` and salted with thing specks."""
    py, px = rng.integers(0, H, cells), rng.integers(0, W, cells)
    pool = [7, 7, 8, 11, 21, 23, 13, 20,                  # stuff
            26001, 26002, 26003, 24001, 24002, 25001, 27001, 28001, 33001, 33002,   # instances
            26, 24,                                       # crowd regions
            4, 9, 29001, 0]                               # ignoreInEval, with and without an instance number
    val = rng.choice(pool, cells)
    yy, xx = np.mgrid[0:H, 0:W]
    cell = np.argmin((yy[..., None] - py) ** 2 + (xx[..., None] - px) ** 2, -1)
    inst = val[cell].astype(np.uint16)
    if H * W > 40:
        inst[H // 2, W // 3:W // 3 + 3] = 40005           # label 40: no such label
    lab = np.where(inst < 1000, inst, inst // 1000)
    train = np.array([TRAIN.get(int(l), 0) for l in range(66)])[lab]
    pred = np.roll(train, shift, (0, 1)).astype(np.uint8)
    m = rng.random((H, W)) < salt
    pred[m] = rng.integers(12, 20, int(m.sum()))
    return pred, inst


def hand_cases():
    R, C, T = 1, 14, 15                                   # train ids: road, car, truck
    out = []

    def blank(H, W):
        return np.full((H, W), R, np.uint8), np.full((H, W), 7, np.uint16)

    p, i = blank(2, 4); i[0, :] = 26001; p[0, :2] = C     # 2 / (2 + 4 - 2) = 0.5 exactly
    out.append(("hand_iou_half", p, i))
    p, i = blank(3, 4); i[0, :] = 26001; i[1, :] = 0; p[:2, :] = C      # 4 / 8 without the void rule, 4 / 4 with it
    out.append(("hand_void_inside", p, i))
    p, i = blank(3, 4); i[0, :2] = 26; i[0, 2] = 0; p[0, :] = C         # 2 crowd + 1 void + 1 road: 3 / 4 > 0.5, no fp
    out.append(("hand_crowd_fp", p, i))
    p, i = blank(3, 4); i[1, 1:3] = 26                    # a crowd region predicted as road: never fn
    out.append(("hand_crowd_fn", p, i))
    p, i = blank(3, 4); i[1, 1:3] = 26001; p[1, 1:3] = T  # the same pixels, another class
    out.append(("hand_class_mismatch", p, i))
    p, i = blank(2, 5); p[0, 1:3] = 0                     # predicted void over road
    out.append(("hand_pred_void", p, i))
    p, i = blank(3, 6); i[1, 0:4] = 26001; i[2, 0:2] = 26001; i[1, 4:6] = 26002; p[1, :] = C; p[2, 0:2] = C      # 6 and 2 pixels, one component of 8
    out.append(("hand_touching", p, i))
    return out


def main():
    rng = np.random.default_rng(20190625)
    cases = hand_cases()
    cases.append(("single_1x1", np.full((1, 1), 14, np.uint8), np.full((1, 1), 26001, np.uint16)))
    cases.append(("scene_1x17",) + scene(rng, 1, 17, 4, 0.1, (0, 1)))
    cases.append(("scene_3x5",) + scene(rng, 3, 5, 3, 0.1, (0, 1)))
    cases.append(("scene_33x65",) + scene(rng, 33, 65, 14, 0.03))
    cases.append(("scene_64x128",) + scene(rng, 64, 128, 30, 0.03))
    b = [scene(rng, 48, 80, 18, 0.05), scene(rng, 48, 80, 18, 0.02, (2, 1))]
    cases.append(("batch2_48x80", np.stack([x[0] for x in b]), np.stack([x[1] for x in b])))

    arrays, index = {}, []
    for name, pred, inst in cases:
        arrays[name + ".pred"], arrays[name + ".inst"] = pred, inst
        preds, insts = (pred, inst) if pred.ndim == 3 else (pred[None], inst[None])
        for conn in (4, 8):
            tp, fp, fn, iou_sum = np.zeros(20, np.int64), np.zeros(20, np.int64), np.zeros(20, np.int64), np.zeros(20, np.float64)
            bads = []
            for k, (p, i) in enumerate(zip(preds, insts)):
                counts, bad = table(p, i, conn)
                bads.append(bad)
                arrays["%s.c%d.rows%d" % (name, conn, k)] = np.asarray([[kp, kg, counts[(kp, kg)]] for kp, kg in sorted(counts)], np.int64).reshape(-1, 3)
                score(counts, tp, fp, fn, iou_sum)
            pq, ns = averages(tp, fp, fn, iou_sum)
            key = "%s.c%d." % (name, conn)
            arrays[key + "bad"] = np.asarray(bads, np.int64)
            arrays[key + "tp"], arrays[key + "fp"], arrays[key + "fn"], arrays[key + "iou_sum"] = tp, fp, fn, iou_sum
            arrays[key + "pq"], arrays[key + "pqn"] = pq, ns
        index.append(dict(name=name, images=len(preds)))
        print(name, pred.shape)
    arrays["index"] = np.frombuffer(json.dumps(index).encode(), np.uint8)
    path = os.path.join(HERE, "panoptic_cases.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
