"""Writes tests/golden/focal_cases.npz: inputs and float64 results of the focal loss (fcn8s_op_focal_xent; the definition is in
include/fcn8s_hip.h), computed here with plain Python loops over pixels and classes, math.exp / math.log on Python floats (doubles) and the
modulating factor written directly as u ** gamma.  Nothing is shared with fcn8s_tensorflow_amd/loss.py or the kernel; numpy only stores the arrays.

    python tests/golden/make_focal_cases.py

A case: P = N * HW pixels, C columns of which K are logical classes (the columns >= K hold the -1e30 of a padding class and no label names
them), gamma, optional class weights (one of them 0) and optional pixel weights given as a distance code per pixel and a 256-entry table.
The logits are 3 N(0, 1) rounded to multiples of 1/128 (stored as int16, exact in float32); every 7th row from row 6 on has +40 on one class (every 28th +160), and every
other one of those rows is labelled with that class (u = 0 or tiny); the rows p % 5 == 2 have +12 on one class; every 11th row is flat; 20 %
of the labels are 255.  Weights are multiples of 1/8 and of 1/16, so that their float32 product is exact.  Every tile edge (P = 1, 15, 255,
256, 257, 513, 2 x 300), every C of the op's tests (2, 4, 19, 20, 21, 64; C = 64 up to P = 15) and every gamma (0.5, 1, 2, 5) occurs; the
full cross product would not fit the 1 MiB limit of a committed file and is held to the restatement of loss.py by the tests instead.
"""
import math
import os
import random

import numpy as np

CASES = (  # (N, HW, C, K, gamma, class weights, pixel weights)
    (1, 1, 2, 2, 2.0, 0, 0), (1, 1, 20, 20, 0.5, 1, 0), (1, 1, 64, 64, 1.0, 0, 1),
    (1, 15, 4, 4, 0.5, 0, 0), (1, 15, 19, 19, 2.0, 1, 1), (1, 15, 20, 19, 5.0, 0, 0), (1, 15, 21, 21, 1.0, 1, 0), (1, 15, 64, 64, 2.0, 1, 1),
    (1, 255, 20, 20, 2.0, 0, 0), (1, 255, 2, 2, 0.5, 1, 0),
    (1, 256, 20, 19, 0.5, 1, 1), (1, 256, 4, 4, 2.0, 0, 1),
    (1, 257, 20, 20, 1.0, 1, 1), (1, 257, 21, 21, 5.0, 0, 0),
    (1, 513, 19, 19, 0.5, 0, 1), (1, 513, 4, 4, 1.0, 1, 1), (1, 513, 2, 2, 5.0, 0, 0),
    (2, 300, 20, 19, 2.0, 1, 1), (2, 300, 4, 4, 0.5, 1, 0),
)
PAD = -1e30


def one_case(rng, N, HW, C, K, gamma, has_cw, has_pw):
    P = N * HW
    zq = [[int(round(rng.gauss(0.0, 3.0) * 128)) for _ in range(C)] for _ in range(P)]      # logits * 128
    lab = [255 if rng.random() < 0.2 else rng.randrange(K) for _ in range(P)]
    for p in range(2, P, 5):
        zq[p][rng.randrange(K)] += 128 * 12
    for p in range(3, P, 11):                                                       # flat rows
        zq[p] = [zq[p][0]] * C
    for p in range(6, P, 7):                                                        # confident rows, every other one labelled with its class
        k = rng.randrange(K)
        zq[p][k] += 128 * (160 if p % 28 == 13 else 40)                              # + 160: the others' expf is 0 in fp32, u = 0 there
        if (p // 7) % 2 == 1 and lab[p] != 255:
            lab[p] = k
    cw = [1.0] * C
    if has_cw:
        cw = [rng.randint(2, 16) / 8.0 for _ in range(C)]
        cw[1 % K] = 0.0
        for c in range(K, C):
            cw[c] = 0.0
    table = [rng.randint(0, 48) / 16.0 for _ in range(256)]
    codes = [rng.randrange(256) for _ in range(P)]
    f = [0.0] * P
    a = [0.0] * P
    d = [[0.0] * C for _ in range(P)]
    bias = [0.0] * C
    total = 0.0
    for p in range(P):
        y = lab[p]
        if y >= C:
            continue
        z = [zq[p][c] / 128.0 if c < K else PAD for c in range(C)]
        w = cw[y] * (table[codes[p]] if has_pw else 1.0)
        m = max(z)
        e = [math.exp(v - m) for v in z]
        S = 0.0
        R = 0.0
        for c in range(C):
            S += e[c]
            if c != y:
                R += e[c]
        l = m + math.log(S) - z[y]
        u = R / S
        sy = e[y] / S
        if u == 0.0:
            fp, ap = 0.0, 0.0
        else:
            fp = u ** gamma
            ap = u ** gamma + gamma * l * sy * u ** (gamma - 1.0)
        f[p], a[p] = fp, ap
        total += w * fp * l
        for c in range(C):
            g = (w / P) * ap * (e[c] / S) if c != y else -(w / P) * ap * u
            d[p][c] = g
            bias[c] += g
    out = dict(z=np.array(zq, np.int16).reshape(P, C), lab=np.array(lab, np.uint8), f=np.array(f, np.float64), a=np.array(a, np.float64),
               loss=np.float64(total / P), dlogits=np.array(d, np.float64).reshape(P, C), bias=np.array(bias, np.float64))
    if has_cw:
        out["cw"] = np.array(cw, np.float32)
    if has_pw:
        out["codes"] = np.array(codes, np.uint8)
        out["table"] = np.array(table, np.float32)
    return out


def main():
    rng = random.Random(20171)
    out = dict(params=np.array(CASES, np.float64))
    for i, case in enumerate(CASES):
        for k, v in one_case(rng, *case).items():
            out["%s_%d" % (k, i)] = v
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "focal_cases.npz")
    np.savez_compressed(path, **out)
    print("%s: %d cases, %d bytes" % (path, len(CASES), os.path.getsize(path)))


if __name__ == "__main__":
    main()
