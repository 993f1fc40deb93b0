"""Writes tests/golden/entropy_term_cases.npz: inputs and float64 results of the entropy term (fcn8s_op_entropy_term; the definition is in
include/fcn8s_hip.h), computed here with plain Python loops over pixels and classes and math.exp / math.log on Python floats (doubles).
Nothing is shared with fcn8s_tensorflow_amd/loss.py or the kernel; numpy only stores the arrays.

    python tests/golden/make_entropy_term_cases.py

A case: P pixels in N images, C columns of which K take part, a pixel set (0: label >= C, 1: label < C, 2: every pixel), first_image and a
weight that float32 holds exactly (the C ABI takes a float).  The logits are multiples of 1/128 (stored as int16, exact in float32).  Every tile edge (P = 1, 15, 255, 256, 257, 513 as one image,
2 x 300 with first_image = 1) and every (C, K) of the op's tests occurs; the full cross product would not fit the 1 MiB limit of a committed file
and is held to the restatement of loss.py by the tests instead.
"""
import math
import os
import random

import numpy as np

CASES = (  # (N, HW, C, K, pixel_set, first_image, weight)
    (1, 1, 4, 2, 2, 0, 1.0), (1, 1, 20, 19, 0, 0, 0.5), (1, 1, 20, 20, 2, 0, -1.0), (1, 1, 21, 21, 1, 0, 1.0), (1, 1, 64, 64, 2, 0, 2.0),
    (1, 15, 4, 2, 0, 0, 1.0), (1, 15, 20, 19, 1, 0, 0.5), (1, 15, 20, 20, 0, 0, 1.0), (1, 15, 21, 21, 2, 0, -0.25), (1, 15, 64, 64, 1, 0, 1.0),
    (1, 255, 20, 20, 0, 0, 1.0), (1, 255, 21, 21, 1, 0, 0.125),
    (1, 256, 20, 19, 2, 0, 1.0), (1, 256, 4, 2, 1, 0, -1.0),
    (1, 257, 20, 20, 1, 0, 0.75), (1, 257, 64, 64, 0, 0, 1.0),
    (1, 513, 21, 21, 0, 0, 1.0), (1, 513, 4, 2, 2, 0, 0.25), (1, 513, 20, 19, 0, 0, -0.5),
    (2, 300, 20, 20, 0, 1, 1.0), (2, 300, 4, 2, 2, 1, 1.0), (2, 300, 21, 21, 1, 1, -1.0), (2, 300, 20, 19, 2, 2, 1.0),
)


def one_case(rng, N, HW, C, K, pset, first, weight):
    P = N * HW
    zq = [[rng.randint(-1024, 1024) for _ in range(C)] for _ in range(P)]          # logits * 128, |z| <= 8
    for p in range(0, P, 7):                                                        # some confident rows: a large margin
        zq[p][rng.randrange(K)] += 128 * 40
    for p in range(3, P, 11):                                                       # some flat rows
        zq[p] = [zq[p][0]] * C
    lab = []
    for p in range(P):
        u = rng.random()
        lab.append(255 if u < 0.4 else (C + 1 if u < 0.45 and C + 1 < 255 else rng.randrange(C)))
    den = P * math.log(K)
    coef = weight / den
    h = [0.0] * P
    d = [[0.0] * C for _ in range(P)]
    bias = [0.0] * C
    total = 0.0
    for p in range(P):
        if p // HW < first:
            continue
        if (pset == 0 and lab[p] < C) or (pset == 1 and lab[p] >= C):
            continue
        z = [zq[p][c] / 128.0 for c in range(K)]
        m = max(z)
        b = [v - m for v in z]
        e = [math.exp(v) for v in b]
        S = 0.0
        for v in e:
            S += v
        lS = math.log(S)
        hp = 0.0
        for c in range(K):
            hp -= (e[c] / S) * (b[c] - lS)
        h[p] = hp
        total += hp
        for c in range(K):
            g = coef * (-(e[c] / S) * ((b[c] - lS) + hp))
            d[p][c] = g
            bias[c] += g
    return dict(z=np.array(zq, np.int16).reshape(P, C), lab=np.array(lab, np.uint8), h=np.array(h, np.float64), term=np.float64(total / den),
                dlogits=np.array(d, np.float64).reshape(P, C), bias=np.array(bias, np.float64))


def main():
    rng = random.Random(20051)
    out = dict(params=np.array(CASES, np.float64))
    for i, (N, HW, C, K, pset, first, weight) in enumerate(CASES):
        for k, v in one_case(rng, N, HW, C, K, pset, first, weight).items():
            out["%s_%d" % (k, i)] = v
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "entropy_term_cases.npz")
    np.savez_compressed(path, **out)
    print("%s: %d cases, %d bytes" % (path, len(CASES), os.path.getsize(path)))


if __name__ == "__main__":
    main()
