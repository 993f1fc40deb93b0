#!/usr/bin/env python3
"""Writes tests/golden/pseudo_label_cases.npz: inputs and expected outputs of `fcn8s_op_pseudo_label` and of the threshold fit.

The expected values come from a route that shares nothing with fcn8s_tensorflow_amd/pseudo_label.py or the kernel: plain Python loops over
the pixels, every float32 taken out of its 4 bytes with `struct` and compared as a Python float (a float32 times 1024 is exact in a double
and equals the float32 product), and `sorted()` for the portion rule -- the m_k-th largest confidence of class k, its bin rounded down; no
histogram is walked.  NumPy only makes the inputs (softmaxes of sharpened random logits) and stores the arrays.

Per case (N, P, C), prefix "<i>_":
  prob [N,P,C] float32, thr float32[C] (not bin edges, except the one class the edge rows belong to), out_ids uint8[C], base uint8 [N,P] with
  about half the pixels == base_fill, score float32 [N,P] with score_max, and
    A_*  labels / hist / counts / misc with everything given (thr, out_ids, ignore_id 250, base, score)
    B_*  the same with nothing given (thresholds NULL, out_ids NULL, ignore_id 255, no base, no score)
    fit_bins / fit_bins_pc   j_k of the portion rule on B's pixels for portion 1/5 and for the per-class portions `portions_pc` (num, den)
    C_*  labels / counts with the edge thresholds fit_bins / 1024 (and nothing else given)
Hand-made rows (cases with P >= 15, at the pixels 0..13 of image 0; HAND names them) are described where they are made.

Run from the repository root:  python tests/golden/make_pseudo_label_cases.py"""
import json
import math
import os
import struct
from fractions import Fraction

import numpy as np

M = 1024
CASES = [(1, 1, 20), (1, 15, 20), (1, 255, 20), (1, 256, 20), (1, 257, 20), (1, 513, 20), (2, 300, 20),
         (1, 257, 2), (1, 513, 2), (1, 257, 19), (2, 300, 19), (1, 257, 21), (1, 257, 64), (1, 15, 64)]
TRAIN_TO_LABEL = [0, 7, 8, 11, 12, 13, 17, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 31, 32, 33]      # labels.py: trainId -> id, 0 = void
EDGE_BIN = 700
HAND = ("tie_0", "tie_high", "on_edge", "below_edge", "one", "zeros", "negative_max", "nan_0", "nan_below_max", "inf",
        "score_on", "score_above", "score_nan", "plain")
PORTIONS_PC = [(1, 10), (1, 2), (1, 1)]


def f32(x):
    """A Python float that holds the float32 nearest to x."""
    return struct.unpack("<f", struct.pack("<f", x))[0]


def next_below(x):
    """The float32 just below the positive float32 x, by its bits."""
    return struct.unpack("<f", struct.pack("<I", struct.unpack("<I", struct.pack("<f", x))[0] - 1))[0]


def next_above(x):
    return struct.unpack("<f", struct.pack("<I", struct.unpack("<I", struct.pack("<f", x))[0] + 1))[0]


def rows_of(a):
    """[..., C] float32 array -> list of rows of Python floats, through the bytes."""
    a = np.ascontiguousarray(a, np.float32)
    Cn = a.shape[-1]
    flat = struct.unpack("<%df" % a.size, a.tobytes())
    return [flat[i:i + Cn] for i in range(0, len(flat), Cn)]


def bin_of(conf):
    if not conf > 0.0:
        return 0
    x = conf * float(M)
    return M - 1 if x >= M else int(x)


def argmax_row(row):
    best, k = row[0], 0
    for c in range(1, len(row)):
        if row[c] > best:
            best, k = row[c], c
    return best, k


def sweep(rows, Cn, thr, out_ids, ignore_id, base, base_fill, score, score_max):
    labels = []
    hist = [[0] * M for _ in range(Cn)]
    counts = [[0, 0] for _ in range(Cn)]
    misc = [0, 0, 0]
    confs = [[] for _ in range(Cn)]                       # per class, the confidences that entered the histogram
    for p, row in enumerate(rows):
        if base is not None and base[p] != base_fill:
            labels.append(base[p]); misc[1] += 1
            continue
        conf, k = argmax_row(row)
        if math.isnan(conf) or math.isinf(conf):
            labels.append(ignore_id); misc[0] += 1
            continue
        if score is not None and not (score[p] <= score_max):
            labels.append(ignore_id); misc[2] += 1; counts[k][1] += 1
            continue
        hist[k][bin_of(conf)] += 1
        confs[k].append(conf)
        if conf >= (thr[k] if thr is not None else 0.0):
            labels.append(out_ids[k] if out_ids is not None else k); counts[k][0] += 1
        else:
            labels.append(ignore_id); counts[k][1] += 1
    return labels, hist, counts, misc, confs


def portion_bins(confs, portions):
    """j_k: the bin of the m_k-th largest confidence of class k, m_k = ceil(portion_k n_k); M for a class without pixels."""
    out = []
    for k, cs in enumerate(confs):
        n = len(cs)
        if n == 0:
            out.append(M)
            continue
        need = portions[k] * n
        m = -((-need.numerator) // need.denominator)
        out.append(bin_of(sorted(cs, reverse=True)[m - 1]))
    return out


def make_inputs(N, P, Cn, rng):
    temp = rng.choice([1.0, 4.0, 12.0], (N, P, 1))
    z = rng.normal(0, 1, (N, P, Cn)) * temp
    never = Cn // 2 if Cn >= 5 else -1
    if never >= 0:
        z[..., never] = -40.0                             # a class that is never predicted
    e = np.exp(z - z.max(-1, keepdims=True))
    prob = (e / e.sum(-1, keepdims=True)).astype(np.float32)
    thr = ((np.floor((0.3 + 0.6 * rng.random(Cn)) * M) + 0.37) / M).astype(np.float32)           # 0.37 of a bin above an edge
    e_cls = Cn - 1
    thr[e_cls] = np.float32(EDGE_BIN / M)                 # the edge rows' class
    out_ids = np.array(TRAIN_TO_LABEL if Cn == 20 else [(3 * k + 5) % 256 for k in range(Cn)], np.uint8)
    base_fill = 255
    base = rng.integers(0, Cn, (N, P)).astype(np.uint8)
    base[rng.random((N, P)) < 0.5] = base_fill
    score_max = np.float32(0.05)
    score = (rng.random((N, P)) * 0.1).astype(np.float32)
    if P >= 15:
        small = np.float32(1e-3)
        h = np.full((len(HAND), Cn), small, np.float32)
        edge = np.float32(EDGE_BIN / M)
        h[0, 0] = h[0, Cn - 1] = 0.4                      # tie_0: an exact tie at the maximum, index 0 wins
        h[1, 0] = 0.1; h[1, 1] = h[1, Cn - 1] = 0.45      # tie_high: a tie between higher indices, the lower wins
        h[2, e_cls] = edge                                # on_edge: conf == 700 / 1024 against the threshold 700 / 1024: kept, bin 700
        h[3, e_cls] = next_below(float(edge))             # below_edge: the float32 below it: dropped, bin 699
        h[4] = 0.0; h[4, 0] = 1.0                         # one: conf = 1.0, bin 1023
        h[5] = 0.0                                        # zeros: k = 0, conf = 0, bin 0; kept only by a threshold of 0
        h[6] = -1.0; h[6, 1] = -0.25                      # negative_max: bin 0, below every threshold >= 0
        h[7, 0] = np.nan; h[7, 1] = 0.9                   # nan_0: NaN at index 0 is the running maximum and stays: a bad row
        hi = 2 if Cn >= 3 else 0
        h[8, 1] = np.nan; h[8, hi] = 0.8                  # nan_below_max: a NaN at a higher index never wins
        h[9, Cn - 1] = np.inf; h[9, 0] = 0.5              # inf: conf = +inf: a bad row
        for r in (10, 11, 12, 13):
            h[r, 0] = 0.97                                # clears every threshold
        prob[0, :len(HAND)] = h
        base[0, :len(HAND)] = base_fill                   # the hand-made rows are examined
        score[0, :len(HAND)] = 0.0
        score[0, 10] = score_max                          # score_on: passes
        score[0, 11] = next_above(float(score_max))       # score_above: the float32 above it fails
        score[0, 12] = np.nan                             # score_nan: fails
    return prob, thr, out_ids, base, base_fill, score, score_max


def main():
    out = {}
    for i, (N, P, Cn) in enumerate(CASES):
        rng = np.random.default_rng([2018, N, P, Cn])
        prob, thr, out_ids, base, base_fill, score, score_max = make_inputs(N, P, Cn, rng)
        rows = rows_of(prob)
        thr_l = [f32(float(v)) for v in thr]
        base_l = [int(v) for v in base.reshape(-1)]
        score_l = list(struct.unpack("<%df" % score.size, score.tobytes()))
        oid_l = [int(v) for v in out_ids]
        pre = "%d_" % i
        out[pre + "prob"] = prob; out[pre + "thr"] = thr; out[pre + "out_ids"] = out_ids; out[pre + "base"] = base
        out[pre + "score"] = score; out[pre + "score_max"] = np.float32(score_max); out[pre + "base_fill"] = np.int64(base_fill)
        lab, hist, counts, misc, _ = sweep(rows, Cn, thr_l, oid_l, 250, base_l, base_fill, score_l, f32(float(score_max)))
        out[pre + "A_labels"] = np.array(lab, np.uint8).reshape(N, P); out[pre + "A_hist"] = np.array(hist, np.int64)
        out[pre + "A_counts"] = np.array(counts, np.int64); out[pre + "A_misc"] = np.array(misc, np.int64)
        lab, hist, counts, misc, confs = sweep(rows, Cn, None, None, 255, None, None, None, None)
        out[pre + "B_labels"] = np.array(lab, np.uint8).reshape(N, P); out[pre + "B_hist"] = np.array(hist, np.int64)
        out[pre + "B_counts"] = np.array(counts, np.int64); out[pre + "B_misc"] = np.array(misc, np.int64)
        bins = portion_bins(confs, [Fraction(1, 5)] * Cn)
        pc = [Fraction(*PORTIONS_PC[k % len(PORTIONS_PC)]) for k in range(Cn)]
        out[pre + "fit_bins"] = np.array(bins, np.int64)
        out[pre + "fit_bins_pc"] = np.array(portion_bins(confs, pc), np.int64)
        out[pre + "portions_pc"] = np.array([[f.numerator, f.denominator] for f in pc], np.int64)
        lab, _, counts, _, _ = sweep(rows, Cn, [b / float(M) for b in bins], None, 255, None, None, None, None)
        out[pre + "C_labels"] = np.array(lab, np.uint8).reshape(N, P); out[pre + "C_counts"] = np.array(counts, np.int64)
    out["meta"] = np.frombuffer(json.dumps(dict(cases=CASES, hand=HAND, edge_bin=EDGE_BIN, bins=M)).encode(), np.uint8)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pseudo_label_cases.npz")
    np.savez_compressed(path, **out)
    print("%s: %d bytes, %d cases" % (path, os.path.getsize(path), len(CASES)))


if __name__ == "__main__":
    main()
